"""GPU tests of the second Renyi entropy of arbitrary regions for the complex RNN (rnnwf_renyi2_regions_complex, csrc/crnn_renyi.hip,
csrc/crnn_renyi_kernels.h; docs/renyi_complex.md).

Bounds, none derived from the kernels: float32 log-ratios 1e-5 N per component (the f32 row of docs/pauli_complex.md); exact enumeration
relative 2e-5 (the same row), every asserted non-zero exact value at least the floor 0.05; self pairs 2e-6 N per component; sums 1e-12
relative; statistics |z| <= 5.
"""
import ctypes as C
import math

import numpy as np
import pytest

import crnn_pauli_reference as CR
import crnn_renyi_reference as RR
from rnnwavefunctions_amd import observables as O
from rnnwavefunctions_amd import observables_complex as OC
from rnnwavefunctions_amd import params as P

pytestmark = pytest.mark.gpu

SCOPE = CR.SCOPE
NPAIRS = 19            # 38 chains: two full 16-chain blocks and a ragged one


def make_wf(N, H, prm, layers=1):
    from rnnwavefunctions_amd import _lib
    wf = _lib.NativeWavefunction(_lib.MODEL_CRNN_U1, N, 1, (H,) * layers)
    wf.set_params(prm, scope=SCOPE)
    return wf


def bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def nontrivial(m):
    return 0 < int(np.sum(m)) < len(m)


def assert_both_branches(samples, regions, npairs):
    """every non-trivial region has at least 3 and at most npairs - 3 survivors, by the NumPy rule alone; returns the counts"""
    counts = np.array([int(RR.survives(samples, m).sum()) if nontrivial(m) else npairs for m in regions])
    for m, k in zip(regions, counts):
        assert not nontrivial(m) or 3 <= k <= npairs - 3, (m, k)
    return counts


def device_reference(wf, samples, regions):
    """(R, n) complex128 log r of mixed configurations built in NumPy and scored with rnnwf_log_amp"""
    own = wf.log_amp(samples).astype(np.complex128)
    ref = np.full((len(regions), len(samples) // 2), RR.NEG, dtype=np.complex128)
    for k, m in enumerate(regions):
        ok = np.repeat(RR.survives(samples, m), 2)
        d = wf.log_amp(RR.mixed(samples, m)[ok]).astype(np.complex128) - own[ok]
        ref[k, ok[0::2]] = d[0::2] + d[1::2]
    return ref


# every NFULL row (1, 2, 3, 1 at three mask words, 4, 6, 8, 12, 16)
ROWS = [(10, 12), (12, 30), (34, 50), (70, 20), (6, 60), (6, 90), (6, 120), (6, 180), (6, 250)]


# 1. log r against explicitly swapped configurations
@pytest.mark.parametrize("N,H", ROWS)
def test_log_ratio_matches_explicit_swapped_configurations(N, H):
    prm = CR.weights(H, seed=H + N, scale=2.0 if H <= 60 else 1.0)
    wf = make_wf(N, H, prm)
    regions = RR.case_regions(N)
    seed, s = RR.pick_seed(N, NPAIRS, regions)
    counts = assert_both_branches(s, regions, NPAIRS)
    out = wf.renyi2_regions_complex(regions, NPAIRS, samples=s, log_ratio=True)
    lr = out["log_ratio"]
    assert lr.shape == (len(regions), NPAIRS) and not np.any(np.isnan(lr.real)) and not np.any(np.isnan(lr.imag))
    assert np.all(np.isfinite(out["sums"]))
    assert np.array_equal(out["in_sector"], counts)
    ref = device_reference(wf, s, regions)
    err = RR.max_abs_diff(lr, ref)                      # asserts that the (-inf, 0) entries coincide exactly
    for k, m in enumerate(regions):
        assert np.array_equal(~np.isneginf(lr[k].real), RR.popcount_rule(s, m)), k
        if not nontrivial(m):                           # the empty and the full region: exactly (0, 0), r = 1
            assert np.all(lr[k] == 0.0) and np.array_equal(out["sums"][k], [NPAIRS, 0.0, NPAIRS, 0.0])
    fin = ~np.isneginf(ref.real)
    print("[crnn renyi N=%d H=%d seed %d] %d regions, %d surviving / %d dead entries, max |d log r| %.3e, bound %.3e, max |log r| %.2f"
          % (N, H, seed, len(regions), fin.sum(), (~fin).sum(), err, CR.F32_BOUND * N, np.abs(ref[fin]).max()))
    assert np.abs(ref[fin]).max() > 0.1
    assert err <= CR.F32_BOUND * N


# 2. a chain's tail does not depend on the tile it sits in
def test_tile_independence_order_shards_and_region_lists():
    N, H = 34, 50
    wf = make_wf(N, H, CR.weights(H, seed=5, scale=2.0))
    regions = RR.case_regions(N)
    seed, s = RR.pick_seed(N, NPAIRS, regions)
    a = wf.renyi2_regions_complex(regions, NPAIRS, samples=s, log_ratio=True)
    # reversed pair order: other tiles, other lanes
    rev = np.ascontiguousarray(s.reshape(NPAIRS, 2, N)[::-1].reshape(2 * NPAIRS, N))
    b = wf.renyi2_regions_complex(regions, NPAIRS, samples=rev, log_ratio=True)
    assert bits_equal(b["log_ratio"][:, ::-1], a["log_ratio"]) and np.array_equal(a["in_sector"], b["in_sector"])
    # two shards
    cut = 10
    h1 = wf.renyi2_regions_complex(regions, cut, samples=s[:2 * cut], log_ratio=True)
    h2 = wf.renyi2_regions_complex(regions, NPAIRS - cut, samples=s[2 * cut:], log_ratio=True)
    assert bits_equal(np.concatenate([h1["log_ratio"], h2["log_ratio"]], axis=1), a["log_ratio"])
    assert np.array_equal(h1["in_sector"] + h2["in_sector"], a["in_sector"])
    assert np.allclose(h1["sums"] + h2["sums"], a["sums"], rtol=1e-12, atol=1e-300)
    # a permuted region list with duplicates: permuted rows, duplicates equal
    perm = np.array([3, 0, 0, 7, 5, 1, 2, 6, 4, 1, len(regions) - 1, len(regions) - 2])
    c = wf.renyi2_regions_complex(regions[perm], NPAIRS, samples=s, log_ratio=True)
    assert bits_equal(c["log_ratio"], a["log_ratio"][perm]) and bits_equal(c["sums"], a["sums"][perm])
    assert np.array_equal(c["in_sector"], a["in_sector"][perm])


# 3. exact enumeration over all pairs of the sector
def enumeration(N=10, H=12):
    prm = CR.weights(H)
    wf = make_wf(N, H, prm)
    cfg = CR.sector(N)
    n = len(cfg)
    ia, ib = np.repeat(np.arange(n), n), np.tile(np.arange(n), n)
    pairs = np.empty((2 * n * n, N), dtype=np.int32)
    pairs[0::2], pairs[1::2] = cfg[ia], cfg[ib]
    psi = np.zeros(2 ** N, dtype=np.complex128)
    psi[cfg @ (1 << np.arange(N - 1, -1, -1))] = np.exp(wf.log_amp(cfg).astype(np.complex128))
    psi /= np.linalg.norm(psi)
    Pc = np.exp(wf.log_prob(cfg))
    return wf, psi, pairs, Pc[ia] * Pc[ib] / Pc.sum() ** 2


def test_exact_enumeration_against_the_dense_reduced_density_matrix():
    N = 10
    wf, psi, pairs, w = enumeration(N)
    regions = np.stack([RR.sites(N, g) for g in RR.EXACT_REGIONS])
    out = wf.renyi2_regions_complex(regions, len(pairs) // 2, samples=pairs, log_ratio=True)
    r = RR.ratio(out["log_ratio"])
    for k, m in enumerate(regions):
        trace, sectors = RR.dense_renyi2(psi, N, m)
        est = np.sum(w * r[k])
        q = pairs[0::2][:, m == 1].sum(axis=1)
        worst = max(abs(np.sum(w * r[k].real * (q == c)) - t_q) for c, (p_q, t_q) in sectors.items())
        print("[crnn renyi exact] %-18s est %.8f%+.1ei dense %.8f rel %.2e, sector traces worst %.1e of total"
              % (RR.EXACT_REGIONS[k], est.real, est.imag, trace, abs(est.real - trace) / trace, worst / trace))
        assert trace >= RR.FLOOR and abs(trace - RR.EXACT_TRACE[k]) <= 1e-4
        assert abs(est.real - trace) <= 2e-5 * trace and abs(est.imag) <= 2e-5
        assert worst <= 2e-5 * trace


# 4. prefix regions and self pairs
def test_cuts_are_prefix_regions_and_self_pairs_cancel():
    N, H, n = 12, 30, 40
    wf = make_wf(N, H, CR.weights(H, seed=5, scale=2.0))
    s = CR.random_sector_samples(N, 2 * n, seed=2)
    cuts = OC.renyi2_entropy(wf, n, samples=s)
    suffix = np.stack([O.interval_region(N, l, N) for l in range(1, N)])
    same = OC.renyi2_regions(wf, suffix, n, samples=s)
    assert cuts["S2"].shape == (N - 1,)
    for k in ("S2", "err", "imag", "err_imag", "survivors"):
        assert bits_equal(cuts[k], same[k]), k
    twice = np.repeat(s[:n], 2, axis=0)                 # pairs (sigma, sigma)
    regions = RR.case_regions(N)
    out = wf.renyi2_regions_complex(regions, n, samples=twice, log_ratio=True)
    worst = max(np.abs(out["log_ratio"].real).max(), np.abs(out["log_ratio"].imag).max())
    print("[crnn renyi self pairs] max |log r| component %.3e (bound %.3e)" % (worst, 2e-6 * N))
    assert np.all(out["in_sector"] == n) and worst <= 2e-6 * N


# 5. statistics on device-drawn pairs
def test_device_drawn_entropies_within_five_standard_errors():
    N, H, n = 10, 12, 2 ** 16
    prm = CR.weights(H)
    wf = make_wf(N, H, prm)
    psi, _ = CR.dense_state(prm, N)
    regions = np.stack([RR.sites(N, g) for g in RR.EXACT_REGIONS])
    res = OC.renyi2_regions(wf, regions, n, seed=11, step=3, want_log_ratio=True)
    assert np.all(CR.in_sector(res["samples"]))
    for k, m in enumerate(regions):
        trace, sectors = RR.dense_renyi2(psi, N, m)
        match = sum(p * p for p, _ in sectors.values())              # P(equal charges) of two independent draws
        # a single site swaps equal spins only: the mixed chains are the chains themselves, r = 1 and Im r = 0 exactly, with no spread
        z_im = res["imag"][k] / res["err_imag"][k] if res["err_imag"][k] > 0.0 else 0.0
        assert res["err_imag"][k] > 0.0 or (res["imag"][k] == 0.0 and m.sum() == 1)
        z = [(res["S2"][k] + np.log(trace)) / res["err"][k], z_im,
             (res["survivors"][k] - match) / np.sqrt(match * (1.0 - match) / n)]
        print("[crnn renyi stats] %-18s S2 %.4f +- %.4f exact %.4f | Im %+.1e +- %.1e | survivors %.4f exact %.4f | z %s"
              % (RR.EXACT_REGIONS[k], res["S2"][k], res["err"][k], -np.log(trace), res["imag"][k], res["err_imag"][k], res["survivors"][k],
                 match, np.round(z, 2)))
        assert trace >= RR.FLOOR and np.all(np.abs(z) <= 5.0)
    # the symmetry-resolved entropies of the half chain from the same pairs
    m = regions[0]
    sr = OC.symmetry_resolved_renyi2(res["log_ratio"][0], res["samples"], m)
    trace, sectors = RR.dense_renyi2(psi, N, m)
    assert abs(sr["trace"].sum() - np.exp(-res["S2"][0])) <= 1e-12
    for c, (p_q, t_q) in sectors.items():
        if p_q > 0.05:
            assert abs(sr["p"][c] - p_q) <= 5.0 * sr["p_err"][c] and abs(sr["trace"][c] - t_q) <= 5.0 * sr["trace_err"][c]
            assert abs(sr["S2"][c] + np.log(t_q / p_q ** 2)) <= 5.0 * sr["S2_err"][c]
    for (a, b), want in RR.EXACT_I2:
        ta, tb, tab = (RR.dense_renyi2(psi, N, RR.sites(N, g))[0] for g in (a, b, a + b))
        exact = -np.log(ta) - np.log(tb) + np.log(tab)
        i2, err = OC.renyi2_mutual_information(wf, RR.sites(N, a), RR.sites(N, b), n, seed=12)
        print("[crnn renyi stats] I2(%s : %s) = %.4f +- %.4f, exact %.4f" % (a, b, i2, err, exact))
        assert exact >= RR.FLOOR and abs(exact - want) <= 5e-4 and abs(i2 - exact) <= 5.0 * err


# 6. call behaviour: repetition, passes, sums, work counter
def test_repeat_passes_sums_and_work(monkeypatch):
    N, H, n = 12, 30, 2000
    prm = CR.weights(H, seed=5, scale=2.0)
    wf = make_wf(N, H, prm)
    regions = np.stack([RR.sites(N, g) for g in ([4, 5, 6, 7], [6], [1, 4, 7, 10], range(0, 7), [], range(9, 12))])
    wf.timing_enable(True)
    wf.timing_reset()
    a = wf.renyi2_regions_complex(regions, n, seed=5, step=2, log_ratio=True)
    t = [wf.timing_get(i) for i in range(3)]
    s = a["samples"]
    assert np.array_equal(s, wf.sample(2 * n, seed=5, step=2)) and np.all(CR.in_sector(s))
    counts = np.array([int(RR.survives(s, m).sum()) if nontrivial(m) else n for m in regions])
    firsts = [int(np.flatnonzero(RR.normalised(m))[0]) if nontrivial(m) else 0 for m in regions]
    assert np.array_equal(a["in_sector"], counts)
    assert t[1]["cell_evals"] == sum(2 * c * (N - f) for c, f, m in zip(counts, firsts, regions) if nontrivial(m))
    # id 0: the sampling base pass, the checkpointed base pass and the site-term replay; id 1: lists and tails under one bracket
    assert t[0]["launches"] >= 3 and t[1]["launches"] == 1 and t[2]["launches"] == 1 and t[1]["mfma_flops"] > 0
    b = wf.renyi2_regions_complex(regions, n, seed=5, step=2, log_ratio=True)
    for k in ("sums", "log_ratio", "in_sector", "samples"):
        assert bits_equal(a[k], b[k]), k
    # sums against an exactly rounded re-summation of the device's own r
    r = RR.ratio(a["log_ratio"])
    resum = np.array([[math.fsum(v.real), math.fsum(v.imag), math.fsum(v.real ** 2), math.fsum(v.imag ** 2)] for v in r])
    nz = np.abs(resum) > 0
    assert np.abs(a["sums"][nz] / resum[nz] - 1.0).max() <= 1e-12 and np.all(a["sums"][~nz] == 0.0)
    # two device-drawn shards
    h1 = wf.renyi2_regions_complex(regions, 720, seed=5, step=2)
    h2 = wf.renyi2_regions_complex(regions, n - 720, seed=5, step=2, pair_offset=720)
    assert np.array_equal(h1["in_sector"] + h2["in_sector"], a["in_sector"])
    assert np.abs((h1["sums"] + h2["sums"])[nz] / a["sums"][nz] - 1.0).max() <= 1e-12
    assert np.array_equal(np.concatenate([h1["samples"], h2["samples"]]), s)
    # several passes: equal per-pair bits, additive sums and counts
    monkeypatch.setenv("RNNWF_STATE_BUDGET_MB", "1")
    wf1 = make_wf(N, H, prm)
    wf1.timing_enable(True)
    wf1.timing_reset()
    many = wf1.renyi2_regions_complex(regions, n, seed=5, step=2, log_ratio=True)
    passes = wf1.timing_get(1)["launches"]
    print("[crnn renyi passes] RNNWF_STATE_BUDGET_MB=1: %d passes" % passes)
    assert passes >= 3
    assert bits_equal(many["log_ratio"], a["log_ratio"]) and bits_equal(many["samples"], s) and np.array_equal(many["in_sector"], a["in_sector"])
    assert np.abs(many["sums"][nz] / a["sums"][nz] - 1.0).max() <= 1e-12
    assert wf1.timing_get(1)["cell_evals"] == t[1]["cell_evals"]


# 7. refusals
def test_refusals_through_the_c_call_and_the_module():
    from rnnwavefunctions_amd import _lib
    N, H, n = 6, 10, 16
    prm = CR.weights(H, seed=1)
    wf = make_wf(N, H, prm)
    reg = RR.sites(N, [2, 3])[None, :].copy()
    # a resident batch from a Pauli call, to be found intact after the refusals
    one = np.zeros((1, N), dtype=np.int32)
    x01 = RR.sites(N, [0, 1])[None, :].copy()
    ok = wf.pauli_step_complex(x01, one, [1.0], 32, seed=1)
    shapes = {"wf_dense_ampl/kernel": (H, 2)}
    mean = complex(ok["moments"][0] / 32, ok["moments"][3] / 32)
    g0 = wf.vmc_gradient(mean, 32, shapes)["wf_dense_ampl/kernel"]
    I32P, F64P = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    sums = np.zeros((1, 4))

    def call(h=None, regions=reg.ctypes.data_as(I32P), R=1, npairs=n, offset=0, out=sums.ctypes.data_as(F64P), samples=None):
        return wf.lib.rnnwf_renyi2_regions_complex(h or wf.h, regions, R, samples, npairs, 1, 0, offset, out, None, None, None)

    def last(h=None):
        return wf.lib.rnnwf_last_error(h or wf.h).decode()

    wf.timing_enable(True)
    wf.timing_reset()
    for kwargs, word in [(dict(R=0), "nregions"), (dict(R=65536), "nregions"), (dict(npairs=0), "npairs must"), (dict(regions=None), "non-null"),
                         (dict(out=None), "non-null"), (dict(offset=-1), "pair_offset")]:
        assert call(**kwargs) == -1, kwargs
        assert word in last() and "rnnwf_renyi2_regions_complex" in last(), (kwargs, last())
    bad = reg.copy()
    bad[0, 4] = 2
    assert call(regions=bad.ctypes.data_as(I32P)) == -1 and "regions[0][4] = 2" in last()
    with pytest.raises(ValueError, match="0 or 1"):
        wf.renyi2_regions_complex(bad, n)
    outside = np.array([[0, 1, 0, 1, 0, 1], [1, 1, 0, 1, 0, 1]], dtype=np.int32)
    with pytest.raises(ValueError, match=r"samples\[1\] has 4 up spins, the zero-magnetisation sector has 3"):
        wf.renyi2_regions_complex(reg, 1, samples=outside)
    with pytest.raises(ValueError, match="disjoint"):
        OC.renyi2_mutual_information(wf, RR.sites(N, [1, 2]), RR.sites(N, [2, 3]), n)
    # uncommitted parameters
    raw = _lib.NativeWavefunction(_lib.MODEL_CRNN_U1, N, 1, (H,))
    assert call(h=raw.h) == -3 and "not committed" in last(raw.h)
    # stacked layers
    st = make_wf(N, H, P.init_gru_params([H, H], seed=1, heads=CR.HEADS), layers=2)
    st.timing_enable(True)
    with pytest.raises(ValueError, match="one GRU layer only"):
        st.renyi2_regions_complex(reg, n)
    assert sum(st.timing_get(i)["launches"] for i in range(3)) == 0
    # the refused calls launched nothing and left the resident batch usable
    assert sum(wf.timing_get(i)["launches"] for i in range(3)) == 0
    assert np.array_equal(g0, wf.vmc_gradient(mean, 32, shapes)["wf_dense_ampl/kernel"])
    # every other model is refused by name, with a pointer to its own entry point
    for model, nx, ny, name in [(_lib.MODEL_GRU1D, N, 1, "GRU1D"), (_lib.MODEL_GRU1D_F64, 3, 2, "GRU1D_F64"), (_lib.MODEL_GRU1D_PARITY, N, 1, "GRU1D_PARITY"),
                                (_lib.MODEL_MDRNN2D, 3, 2, "MDRNN2D"), (_lib.MODEL_LSTM1D_F64, 3, 2, "LSTM1D_F64")]:
        w = _lib.NativeWavefunction(model, nx, ny, (H,))
        w.timing_enable(True)
        with pytest.raises(ValueError, match=r"model is %s; rnnwf_renyi2_regions serves the GRU models, rnnwf_renyi2_regions_2d the 2D RNN" % name):
            w.renyi2_regions_complex(reg, n)
        with pytest.raises(ValueError, match="CRNN_U1"):
            OC.renyi2_regions(w, reg, n)
        assert sum(w.timing_get(i)["launches"] for i in range(3)) == 0
    # the positive models' entry points still refuse the complex RNN
    with pytest.raises(ValueError, match="not implemented for the complex RNN"):
        wf.renyi2_regions(reg, n)
    with pytest.raises(ValueError, match="not implemented for the complex RNN"):
        wf.renyi2_swap(n)
    # a served call after all that
    res = OC.renyi2_regions(wf, reg, n, seed=1)
    assert res["S2"].shape == (1,) and np.isfinite(res["imag"][0]) and 0.0 <= res["survivors"][0] <= 1.0      # 16 pairs: no statistics
