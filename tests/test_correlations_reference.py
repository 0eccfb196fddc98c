"""Validation of tests/correlations_reference.py (the float64 reference of the GPU correlation tests) and of
observables.correlations_from_sums, on the CPU: exact identities from the dense vector of all amplitudes, closed forms on a product
state, algebraic identities of the log-ratios, what the GPU tests' bound rejects and accepts at N = 80 / 50 units, and the
statistics written out again.

Rejection factors measured here (max |defective - reference| / bound at N = 80, 50 units, 48 model-drawn chains; the bound is
min(16 dev32, 2e-6 N + 2e-6) with dev32 computed on the same entries): printed by test_bound_rejects_defects_and_accepts_another_
summation_order and recorded in docs/correlations.md.
"""
import warnings

import numpy as np
import pytest

import correlations_reference as R
from conftest import all_configs
from oracle import models as M
from rnnwavefunctions_amd import params as P


def trained_like(H, seed, scale=3.0, dtype=np.float64):
    return P.randomize_biases(P.scale_kernels(P.init_gru_params([H], seed=seed, dtype=dtype), scale), seed + 1)


@pytest.mark.parametrize("N,H,seed", [(4, 6, 1), (5, 10, 2), (6, 20, 3), (6, 8, 4)])
def test_weighted_sums_over_all_configurations_equal_the_dense_vector_values(N, H, seed):
    # N = 6 stands for the rasters 2 x 3 and 3 x 2 as well: the raster model is the 1D chain in raster order
    prm = trained_like(H, seed)
    c = all_configs(N)
    lp = M.prnn_log_probability(prm, c, dtype=np.float64)
    assert abs(np.exp(lp).sum() - 1.0) < 1e-13
    z, zz, x, xx = R.exact_from_log_probs(lp, N)
    lr = R.log_ratio_all(prm, c)
    w = np.exp(lp)
    got = np.exp(lr) @ w
    pi, pj = R.pair_list(N)
    assert np.abs(got[:N] - x).max() <= 1e-12
    assert np.abs(got[N:] - xx[pi, pj]).max() <= 1e-12
    s = 2.0 * c - 1.0
    assert np.abs(w @ s - z).max() <= 1e-12 and np.abs((s * w[:, None]).T @ s - zz).max() <= 1e-12
    # not a product state: some connected xx is far from 0
    assert np.abs(xx - np.outer(x, x))[pi, pj].max() > 1e-3


def test_zero_kernels_give_a_product_state_in_closed_form():
    N, H = 6, 10
    prm = trained_like(H, 5)
    for k in prm:
        if k.endswith("kernel"):
            prm[k] = np.zeros_like(prm[k])
    c = all_configs(N)
    probs = M.prnn_site_probs(prm, c[:1], dtype=np.float64)[0]          # the same conditional at every site but the first input
    lr = R.log_ratio_all(prm, c)
    pi, pj = R.pair_list(N)
    assert np.abs(lr[N:] - (lr[pi] + lr[pj])).max() <= 1e-13            # r_ij = r_i r_j chain by chain
    lp = M.prnn_log_probability(prm, c, dtype=np.float64)
    z, zz, x, xx = R.exact_from_log_probs(lp, N)
    p1 = np.array([M.prnn_site_probs(prm, c, dtype=np.float64)[:, n, 1] @ np.exp(lp) for n in range(N)])
    assert np.abs(x - 2.0 * np.sqrt(p1 * (1.0 - p1))).max() <= 1e-13
    assert np.abs(xx - np.outer(x, x))[pi, pj].max() <= 1e-13
    assert probs.shape == (N, 2)


def test_log_ratio_identities():
    N, H = 7, 12
    prm = trained_like(H, 9)
    x = np.random.RandomState(1).randint(0, 2, size=(20, N)).astype(np.int32)
    lr = R.log_ratio_all(prm, x)
    for i, j in [(0, 1), (2, 5), (0, 6), (5, 6)]:
        xi = x.copy()
        xi[:, i] = 1 - xi[:, i]
        xij = xi.copy()
        xij[:, j] = 1 - xij[:, j]
        row = R.row_of(i, j, N)
        assert np.abs(lr[row] - (lr[i] + R.log_ratio_all(prm, xi)[j])).max() <= 1e-12
        assert np.abs(lr[row] + R.log_ratio_all(prm, xij)[row]).max() <= 1e-12
        assert np.abs(R.site_resolved(prm, x, i, j) - lr[row]).max() <= 1e-12


def test_bound_rejects_defects_and_accepts_another_summation_order():
    N, H, ns = 80, 50, 48
    prm = P.randomize_biases(P.scale_kernels(P.init_gru_params([H], seed=111, dtype=np.float32), 3.0), 112)
    u = np.random.RandomState(3).random_sample((ns, N)).astype(np.float32)
    x = M.prnn_sample(prm, N, u)[0].astype(np.int32)
    pairs = [(0, 1), (3, 40), (10, 70), (30, 34), (31, 33), (5, 78), (40, 60)]
    ref = np.stack([R.site_resolved(prm, x, i, j) for i, j in pairs])
    ch = np.repeat(np.arange(ns)[None, :], len(pairs), axis=0)
    ii = np.repeat(np.array([p[0] for p in pairs])[:, None], ns, axis=1)
    jj = np.repeat(np.array([p[1] for p in pairs])[:, None], ns, axis=1)
    direct = R.log_ratio_entries(R.scorer(prm), x, ch.ravel(), ii.ravel(), jj.ravel()).reshape(ref.shape)
    assert np.abs(direct - ref).max() <= 1e-11
    r32 = R.log_ratio_entries(R.scorer(prm, np.float32), x, ch.ravel(), ii.ravel(), jj.ravel()).reshape(ref.shape)
    dev32 = float(np.abs(r32 - direct).max())
    bound, capped = R.f32_bound(dev32, N)
    assert dev32 <= R.f32_ceiling(N)
    print("N=%d H=%d: dev32 = %.2e, bound %.3e (%s)" % (N, H, dev32, bound, "capped" if capped else "16 x dev32"))

    def factor(got):
        return float(np.abs(got - direct).max() / bound)

    single = R.log_ratio_entries(R.scorer(prm), x, ch.ravel(), ii.ravel(), np.full(ii.size, -1)).reshape(ref.shape)
    shifted = np.stack([R.site_resolved(prm, x, i, j + 1 if j + 1 < N else j - 1) for i, j in pairs])
    defects = {
        "j shifted by one": shifted,
        "only one of the two flips applied": single,
        "trunk sites i+1..j-1 taken from the base chain": np.stack([R.site_resolved(prm, x, i, j, defect="trunk_from_base") for i, j in pairs]),
        "spins of sites >= 32 read from word 0": np.stack([R.site_resolved(prm, x, i, j, defect="word0") for i, j in pairs]),
        "dropped tail": np.stack([R.site_resolved(prm, x, i, j, defect="dropped_tail") for i, j in pairs]),
    }
    for name, got in defects.items():
        f = factor(got)
        print("  rejected: %-48s %.3g x the bound" % (name, f))
        assert f > 10.0, name
    other = np.stack([R.log_ratio_other_order(prm, x, i, j) for i, j in pairs])
    f = factor(other)
    print("  accepted: float32 summed in another order              %.3g x the bound" % f)
    assert f <= 1.0


def test_correlations_from_sums_against_the_formulas_written_out_again():
    from rnnwavefunctions_amd.observables import correlations_from_sums
    N, n = 5, 200
    rng = np.random.RandomState(0)
    s = rng.randint(0, 2, size=(n, N))
    lr = 0.3 * rng.standard_normal((N + N * (N - 1) // 2, n))
    z_sums, zz_sums = R.diag_sums(s)
    x_sums, xx_sums = R.sums_from_log_ratio(lr, N)
    got = correlations_from_sums(z_sums, zz_sums, x_sums, xx_sums, n)
    ref = R.stats_from_sums(z_sums, zz_sums, x_sums, xx_sums, n)
    assert set(got) == set(ref)
    for k in ref:
        assert got[k].shape == ref[k].shape and np.allclose(got[k], ref[k], rtol=1e-12, atol=1e-14), k
    # the means are the plain sample means, the connected xx error the sample error of g = r_ij - x_j r_i - x_i r_j
    r = np.exp(lr)
    assert np.allclose(got["x"], r[:N].mean(axis=1)) and np.allclose(got["z"], (2 * s - 1).mean(axis=0))
    i, j = 1, 3
    g = r[R.row_of(i, j, N)] - got["x"][j] * r[i] - got["x"][i] * r[j]
    assert np.isclose(got["xx_c_err"][i, j], g.std() / np.sqrt(n), rtol=1e-12)
    assert np.isclose(got["xx_c"][j, i], r[R.row_of(i, j, N)].mean() - r[i].mean() * r[j].mean())
    # shards add
    h = n // 2
    a = (R.diag_sums(s[:h]), R.sums_from_log_ratio(lr[:, :h], N))
    b = (R.diag_sums(s[h:]), R.sums_from_log_ratio(lr[:, h:], N))
    both = correlations_from_sums(a[0][0] + b[0][0], a[0][1] + b[0][1], a[1][0] + b[1][0], a[1][1] + b[1][1], n)
    for k in got:
        assert np.allclose(both[k], got[k], rtol=1e-10, atol=1e-13), k


def test_correlations_from_sums_warns_and_gives_nan_on_overflow():
    from rnnwavefunctions_amd.observables import correlations_from_sums
    N, n = 3, 10
    z, zz = np.zeros(N), n * np.eye(N)
    x = np.full((N, 2), float(n))
    xx = np.zeros((N, N, 5))
    xx[np.triu_indices(N, 1)] = float(n)
    xx[0, 2, 1] = np.inf
    x[1, 1] = np.inf
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        out = correlations_from_sums(z, zz, x, xx, n)
    assert any("not finite" in str(m.message) for m in w)
    assert np.isnan(out["x"][1]) and np.isnan(out["x_err"][1]) and np.isnan(out["xx"][0, 2]) and np.isnan(out["xx"][2, 0])
    assert np.isfinite(out["x"][[0, 2]]).all() and np.isfinite(out["xx"][0, 1]) and np.isfinite(out["zz"]).all()
    with pytest.raises(ValueError):
        correlations_from_sums(z, zz, x[:, :1], xx, n)
