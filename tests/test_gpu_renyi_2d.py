"""GPU tests of the second Renyi entropy of arbitrary lattice regions for the 2D RNN (rnnwf_renyi2_regions_2d,
mdrnn_masked_tail_kernel<..., PAIRED = true> in csrc/mdrnn_pauli_kernels.h, NativeWavefunction.renyi2_regions_2d, observables_2d).

Tolerances, the project's own for this model (tests/test_gpu_mdrnn.py, docs/renyi_regions.md): log r_A against swapped configurations
built in NumPy and scored with rnnwf_log_prob (the base kernel, independent of the tail kernel): 1e-11 N.  Exact identity over all
pairs: relative 1e-12.  Sums against math.fsum of the device's own log r: relative 1e-12.  Statistics: 5 standard errors.
"""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import pauli_2d_reference as Q
import renyi_2d_reference as R
from conftest import all_configs
from rnnwavefunctions_amd import observables_2d as O2

pytestmark = pytest.mark.gpu

SCOPE = R.SCOPE
I32P, F64P = C.POINTER(C.c_int32), C.POINTER(C.c_double)


def make_wf(Nx, Ny, H, prm):
    from rnnwavefunctions_amd import _lib
    wf = _lib.NativeWavefunction(_lib.MODEL_MDRNN2D, Nx, Ny, (H,))
    wf.set_params(prm, scope=SCOPE)
    return wf


def explicit_log_ratio(wf, pairs, masks):
    """log r_A from both swapped configurations, written out in NumPy and scored with rnnwf_log_prob (tests/renyi_2d_reference.py)."""
    return R.log_ratio_regions(lambda x: wf.log_prob(np.ascontiguousarray(x, dtype=np.int32)), pairs, masks)


def enumeration_regions(Nx, Ny):
    """row cuts, column cuts, a 2x2 corner, the bulk site, a two-piece region, a region containing lattice site 0"""
    return np.stack(R.row_cuts(Nx, Ny) + R.column_cuts(Nx, Ny) + [R.rectangle(Nx, Ny, 0, 2, 0, 2), R.mask_of(Nx, Ny, [(1, 1)]),
                    R.mask_of(Nx, Ny, [(0, 1), (Nx - 1, Ny - 1)]), R.mask_of(Nx, Ny, [(0, 0), (1, 0), (Nx - 1, Ny - 1)])])


# 1. sum over every (sigma, tau) of P(sigma) P(tau) r_A = Tr rho_A^2 from the dense vector of the base kernel's own log P
@pytest.mark.parametrize("Nx,Ny", [(3, 3), (2, 4), (4, 2)])
def test_exact_enumeration_over_all_pairs(Nx, Ny):
    N = Nx * Ny
    wf = make_wf(Nx, Ny, Q.EXACT_H, R.exact_weights())
    masks = enumeration_regions(Nx, Ny)
    c = all_configs(N).reshape(-1, Nx, Ny)
    lp = wf.log_prob(c)
    psi = np.exp(0.5 * lp)
    exact = np.array([R.purity_of_region(psi, N, m) for m in masks]) * np.exp(lp).sum() ** 2
    i, j = np.meshgrid(np.arange(2 ** N), np.arange(2 ** N), indexing="ij")
    i, j = i.ravel(), j.ravel()
    pairs = np.empty((2 * i.size, Nx, Ny), dtype=np.int32)
    pairs[0::2], pairs[1::2] = c[i], c[j]
    out = wf.renyi2_regions_2d(masks, i.size, samples=pairs, log_ratio=True)
    assert "samples" not in out and out["log_ratio"].shape == (len(masks), i.size)
    got = (np.exp(lp[i] + lp[j])[None, :] * np.exp(out["log_ratio"])).sum(axis=1)
    rel = np.abs(got / exact - 1.0)
    print("%dx%d: %d pairs, S2 = %s, max rel |sum P P r_A - Tr rho_A^2| = %.2e" % (Nx, Ny, i.size, np.round(-np.log(exact), 4), rel.max()))
    assert (-np.log(exact)).min() > 0.05
    assert rel.max() <= 1e-12


# 2. log r per pair against swapped configurations scored by the base kernel: every row of the dispatch table and every remainder
# width; lattices without a vertical neighbour, with every position a row start, with two mask words; a ragged last block
WIDTHS = [10, 17, 18, 19, 20, 36, 50, 68, 84]              # NFULL 1 (remainders 1..4 at 17..20), 2, 3, 4, 5
LATTICES = [(3, 4), (4, 3), (1, 5), (5, 1), (5, 7), (7, 5)]


@pytest.mark.parametrize("Nx,Ny", LATTICES)
@pytest.mark.parametrize("H", WIDTHS)
def test_log_ratio_matches_explicit_swapped_configurations(H, Nx, Ny):
    N, npairs = Nx * Ny, 48
    wf = make_wf(Nx, Ny, H, Q.weights(H, H + N, 1.0))
    s = np.random.RandomState(H + N).randint(0, 2, size=(2 * npairs, Nx, Ny)).astype(np.int32)
    masks = R.case_regions(Nx, Ny)
    got = wf.renyi2_regions_2d(masks, npairs, samples=s, log_ratio=True)["log_ratio"]
    ref = explicit_log_ratio(wf, s, masks)
    err = np.abs(got - ref).max()
    print("H=%d %dx%d: %d regions, max |log r - explicit| = %.2e (max |log r| %.2f)" % (H, Nx, Ny, len(masks), err, np.abs(ref).max()))
    assert got.shape == (len(masks), npairs) and np.all(np.isfinite(ref))
    assert err <= R.BOUND * N
    assert np.abs(ref).max() > 1e-3
    # 45 of the pairs: 90 chains, the last 16-chain block ragged - the same bits per pair
    ragged = wf.renyi2_regions_2d(masks, 45, samples=s[:90], log_ratio=True)["log_ratio"]
    assert np.array_equal(ragged, got[:, :45])


# 3. identities
@pytest.mark.parametrize("Nx,Ny,H", [(3, 4, 20), (5, 7, 50)])
def test_identities(Nx, Ny, H):
    N, npairs = Nx * Ny, 37
    prm = Q.weights(H, 1, 1.0)
    wf = make_wf(Nx, Ny, H, prm)
    masks = R.case_regions(Nx, Ny)
    s = np.random.RandomState(N).randint(0, 2, size=(2 * npairs, Nx, Ny)).astype(np.int32)
    a = wf.renyi2_regions_2d(masks, npairs, samples=s, log_ratio=True)
    b = wf.renyi2_regions_2d(1 - masks, npairs, samples=s, log_ratio=True)
    assert np.array_equal(a["log_ratio"], b["log_ratio"]) and np.array_equal(a["sums"], b["sums"])         # region and complement
    trivial = [k for k, m in enumerate(masks) if not m.any() or m.all()]
    assert len(trivial) == 2 and np.all(a["log_ratio"][trivial] == 0.0) and np.all(a["sums"][trivial] == float(npairs))
    assert np.abs(a["log_ratio"]).max() > 1e-3
    selfp = wf.renyi2_regions_2d(masks, npairs, samples=np.repeat(s[0::2], 2, axis=0), log_ratio=True)["log_ratio"]
    # pairs that differ only on A, region by region: the swapped configurations merely exchange
    only_a = 0.0
    for m in masks:
        if not m.any() or m.all():
            continue
        d = s.copy()
        d[1::2] = np.where(m.reshape(1, Nx, Ny).astype(bool), 1 - d[0::2], d[0::2])
        only_a = max(only_a, np.abs(wf.renyi2_regions_2d(m, npairs, samples=d, log_ratio=True)["log_ratio"]).max())
    zero = {k: np.zeros_like(v) for k, v in prm.items()}
    z = make_wf(Nx, Ny, H, zero).renyi2_regions_2d(masks, npairs, samples=s, log_ratio=True)
    print("%dx%d H=%d: self pairs max |log r| = %.2e, pairs differing only on A %.2e, zero weights %.2e"
          % (Nx, Ny, H, np.abs(selfp).max(), only_a, np.abs(z["log_ratio"]).max()))
    assert np.abs(selfp).max() <= R.BOUND * N
    assert only_a <= R.BOUND * N
    assert np.abs(z["log_ratio"]).max() <= 1e-13 and np.allclose(z["sums"], float(npairs), rtol=1e-12, atol=0)
    # duplicates are equal, a permuted region list gives permuted rows
    perm = np.random.RandomState(0).permutation(len(masks))
    perm = np.concatenate([perm, perm[:3]])
    p = wf.renyi2_regions_2d(masks[perm], npairs, samples=s, log_ratio=True)
    assert np.array_equal(p["log_ratio"], a["log_ratio"][perm]) and np.array_equal(p["sums"], a["sums"][perm])
    # (R, Nx, Ny) masks and (2 npairs, Nx Ny) samples are the same call
    q = wf.renyi2_regions_2d(masks.reshape(-1, Nx, Ny), npairs, samples=s.reshape(2 * npairs, N), log_ratio=True)
    assert np.array_equal(q["log_ratio"], a["log_ratio"])


# 4. statistics against the exact values
@functools.lru_cache(maxsize=None)
def exact_state(Nx, Ny):
    wf = make_wf(Nx, Ny, Q.EXACT_H, R.exact_weights())
    psi = np.exp(0.5 * wf.log_prob(all_configs(Nx * Ny).reshape(-1, Nx, Ny)))
    return wf, psi


@pytest.mark.parametrize("Nx,Ny", R.EXACT_LATTICES)
def test_s2_and_mutual_information_within_five_standard_errors_of_exact(Nx, Ny):
    N, npairs = Nx * Ny, 2 ** 16
    wf, psi = exact_state(Nx, Ny)
    s2_of = lambda m: -np.log(R.purity_of_region(psi, N, m))
    names, masks = zip(*R.exact_regions(Nx, Ny))
    masks = np.stack(masks)
    exact = np.array([s2_of(m) for m in masks])
    S2, err = O2.renyi2_regions(wf, masks, npairs, seed=2024)
    z = np.abs(S2 - exact) / err
    print("%dx%d: S2 = %s\n exact = %s\n err = %s\n |z| = %s" % (Nx, Ny, np.round(S2, 4), np.round(exact, 4), np.round(err, 4), np.round(z, 2)))
    assert S2.shape == err.shape == (len(masks),) and np.all(err > 0)
    assert np.abs(exact - np.array(R.EXACT_S2[(Nx, Ny)])).max() <= 5.1e-4          # the device's state is the oracle's
    assert z.max() <= 5.0
    for (a, b), listed in zip(R.i2_pairs(Nx, Ny), R.EXACT_I2[(Nx, Ny)]):
        i2_exact = s2_of(a) + s2_of(b) - s2_of(a | b)
        I2, ierr = O2.renyi2_mutual_information(wf, a, b, npairs, seed=2025)
        print(" I2(%s : %s) = %.4f +- %.4f, exact %.4f, |z| = %.2f" % (np.flatnonzero(a).tolist(), np.flatnonzero(b).tolist(), I2, ierr, i2_exact,
                                                                     abs(I2 - i2_exact) / ierr))
        assert i2_exact >= R.FLOOR and abs(i2_exact - listed) <= 5.1e-4
        assert ierr > 0 and abs(I2 - i2_exact) <= 5.0 * ierr


# 5. call behaviour
def test_device_draw_repeats_shards_sums_and_work():
    Nx, Ny, H = 5, 4, 20
    N = Nx * Ny
    wf = make_wf(Nx, Ny, H, Q.weights(H, 4, 1.0))
    masks = R.case_regions(Nx, Ny)
    npairs, k, seed, step, off = 700, 300, 123, 4, 50
    wf.timing_enable(True)
    wf.timing_reset()
    out = wf.renyi2_regions_2d(masks, npairs, seed=seed, step=step, pair_offset=off, log_ratio=True)
    firsts = [R.normalise(m)[1] for m in Q.to_visit_order(masks, Nx, Ny)]
    assert wf.timing_get(1)["cell_evals"] == 2 * npairs * sum(N - 1 - f for f in firsts if f > 0)         # work[0], exact
    for kid in (0, 1, 2):
        t = wf.timing_get(kid)
        assert t["launches"] >= 1 and t["total_ms"] > 0
    assert wf.timing_get(1)["launches"] == 1
    assert out["samples"].shape == (2 * npairs, Nx, Ny)
    assert np.array_equal(out["samples"], wf.sample(2 * npairs, seed=seed, step=step, sample_offset=2 * off))
    again = wf.renyi2_regions_2d(masks, npairs, seed=seed, step=step, pair_offset=off, log_ratio=True)
    for key in ("sums", "log_ratio", "samples"):
        assert np.array_equal(again[key], out[key]), key
    fed = wf.renyi2_regions_2d(masks, npairs, samples=out["samples"], log_ratio=True)
    assert np.array_equal(fed["log_ratio"], out["log_ratio"]) and np.array_equal(fed["sums"], out["sums"])
    lr = out["log_ratio"]
    want = np.array([[math.fsum(np.exp(row)), math.fsum(np.exp(2.0 * row))] for row in lr])
    rel = np.abs(out["sums"] / want - 1.0).max()
    print("5x4: max rel |sums - fsum of the device's own log r| = %.2e" % rel)
    assert rel <= 1e-12
    a = wf.renyi2_regions_2d(masks, k, seed=seed, step=step, pair_offset=off, log_ratio=True)
    b = wf.renyi2_regions_2d(masks, npairs - k, seed=seed, step=step, pair_offset=off + k, log_ratio=True)
    assert np.array_equal(np.concatenate([a["log_ratio"], b["log_ratio"]], axis=1), lr)
    assert np.array_equal(np.concatenate([a["samples"], b["samples"]]), out["samples"])
    assert np.allclose(a["sums"] + b["sums"], out["sums"], rtol=1e-12, atol=0)
    # nothing but empty regions: no cell evaluation, no masked-tail launch
    wf.timing_reset()
    e = wf.renyi2_regions_2d(np.stack([np.zeros(N, dtype=np.int32), np.ones(N, dtype=np.int32)]), 10, seed=1)
    assert wf.timing_get(1)["cell_evals"] == 0 and wf.timing_get(1)["launches"] == 0 and np.all(e["sums"] == 10.0)


def test_several_passes_give_the_one_pass_bits(monkeypatch):
    Nx, Ny, H, npairs = 6, 6, 20, 500
    prm = Q.weights(H, 4, 1.0)
    masks = R.case_regions(Nx, Ny)
    one = make_wf(Nx, Ny, H, prm).renyi2_regions_2d(masks, npairs, seed=5, step=2, log_ratio=True)
    monkeypatch.setenv("RNNWF_STATE_BUDGET_MB", "1")
    wf = make_wf(Nx, Ny, H, prm)
    wf.timing_enable(True)
    wf.timing_reset()
    m = wf.renyi2_regions_2d(masks, npairs, seed=5, step=2, log_ratio=True)
    passes = wf.timing_get(1)["launches"]
    print("RNNWF_STATE_BUDGET_MB=1, 6x6, 20 units, 500 pairs: %d passes" % passes)
    assert passes >= 3
    assert np.array_equal(m["samples"], one["samples"]) and np.array_equal(m["log_ratio"], one["log_ratio"])
    assert np.allclose(m["sums"], one["sums"], rtol=1e-12, atol=0)
    fed = wf.renyi2_regions_2d(masks, npairs, samples=one["samples"], log_ratio=True)          # the caller's samples through the same passes
    assert np.array_equal(fed["log_ratio"], one["log_ratio"])


# 6. refusals and the resident batch
def test_refusals_through_the_c_call_and_the_facade():
    from rnnwavefunctions_amd import _lib
    Nx, Ny, N, H, ns = 3, 2, 6, 10, 64
    wf = make_wf(Nx, Ny, H, Q.weights(H, 1, 1.0))
    shapes = {"wf_dense/kernel": (H, 2)}
    mom = wf.vmc_step(ns, seed=5, step=0, couplings=np.append(np.ones(N), 1.0))["moments"]
    g0 = wf.vmc_gradient(mom[0] / mom[2], ns, shapes)["wf_dense/kernel"]
    m = np.stack([R.mask_of(Nx, Ny, [(1, 1)]), R.mask_of(Nx, Ny, [(2, 0), (2, 1)])])
    mp = m.ctypes.data_as(I32P)
    sums = np.zeros((2, 2))
    up = sums.ctypes.data_as(F64P)

    def call(h=None, regions=mp, R_=2, npairs=4, offset=0, out=up, samples=None):
        return wf.lib.rnnwf_renyi2_regions_2d(h or wf.h, regions, R_, samples, npairs, 1, 0, offset, out, None, None)

    def last(h=None):
        return wf.lib.rnnwf_last_error(h or wf.h).decode()

    wf.timing_enable(True)
    wf.timing_reset()
    for kwargs, word in [(dict(R_=0), "nregions"), (dict(R_=-2), "nregions"), (dict(R_=65536), "nregions"), (dict(npairs=0), "npairs"),
                         (dict(npairs=-3), "npairs"), (dict(regions=None), "non-null"), (dict(out=None), "non-null"),
                         (dict(offset=-1), "pair_offset")]:
        assert call(**kwargs) == -1, kwargs
        assert word in last() and "rnnwf_renyi2_regions_2d" in last(), (kwargs, last())
    bad = m.copy()
    bad[1, 4] = 2
    assert call(regions=bad.ctypes.data_as(I32P)) == -1 and "regions[1][4] = 2" in last()
    with pytest.raises(ValueError, match=r"regions\[1\]\[4\] = 2"):
        wf.renyi2_regions_2d(bad, 4, seed=1)
    bad[1, 4] = -1
    with pytest.raises(ValueError, match="0 or 1"):
        wf.renyi2_regions_2d(bad, 4, seed=1)
    with pytest.raises(ValueError, match="npairs"):
        wf.renyi2_regions_2d(m, 0, seed=1)
    with pytest.raises(ValueError, match="pair_offset"):
        wf.renyi2_regions_2d(m, 4, seed=1, pair_offset=-1)
    for shape in [(2, N + 1), (0, N), (2, Ny, Nx)]:
        with pytest.raises(ValueError, match="shape"):
            wf.renyi2_regions_2d(np.zeros(shape, dtype=np.int32), 4)
    with pytest.raises(ValueError, match="shape"):
        wf.renyi2_regions_2d(m, 4, samples=np.zeros((7, Nx, Ny), dtype=np.int32))
    with pytest.raises(ValueError, match="disjoint"):
        O2.renyi2_mutual_information(wf, m[0], m[0], 10)
    # uncommitted parameters
    raw = _lib.NativeWavefunction(_lib.MODEL_MDRNN2D, Nx, Ny, (H,))
    assert call(h=raw.h) == -1 and "not committed" in last(raw.h)
    with pytest.raises(ValueError, match="not committed"):
        raw.renyi2_regions_2d(m, 4)
    # the refused calls launched nothing and left the resident batch of the earlier step usable
    assert sum(wf.timing_get(i)["launches"] for i in range(3)) == 0
    g1 = wf.vmc_gradient(mom[0] / mom[2], ns, shapes)["wf_dense/kernel"]
    assert np.array_equal(g0, g1)
    # with hand-fed samples pair_offset is ignored, as in rnnwf_renyi2_regions
    s = np.zeros((8, Nx, Ny), dtype=np.int32)
    assert call(samples=s.ctypes.data_as(I32P), offset=-1) == 0
    # an accepted call overwrites the states and leaves no batch
    with pytest.raises(Exception, match="vmc_step first"):
        wf.vmc_gradient(mom[0] / mom[2], ns, shapes)
    # every other model is refused by the 2D entry point, by name, with a pointer to rnnwf_renyi2_regions
    for model, nx, ny, units, name in [(_lib.MODEL_GRU1D, N, 1, (10,), "GRU1D"), (_lib.MODEL_GRU1D_F64, Nx, Ny, (10,), "GRU1D_F64"),
                                       (_lib.MODEL_GRU1D_PARITY, N, 1, (10,), "GRU1D_PARITY"), (_lib.MODEL_CRNN_U1, N, 1, (10,), "CRNN_U1"),
                                       (_lib.MODEL_LSTM1D_F64, Nx, Ny, (10,), "LSTM1D_F64")]:
        w = _lib.NativeWavefunction(model, nx, ny, units)
        w.init_params(1)
        w.timing_enable(True)
        with pytest.raises(ValueError, match=r"model is %s; rnnwf_renyi2_regions serves the GRU models" % name):
            w.renyi2_regions_2d(m, 4)
        with pytest.raises(ValueError, match="MDRNN2D"):
            O2.renyi2_regions(w, m, 4)
        with pytest.raises(ValueError, match="MDRNN2D"):
            O2.renyi2_mutual_information(w, m[0], m[1], 4)
        assert sum(w.timing_get(i)["launches"] for i in range(3)) == 0
    # the existing entry points still refuse the 2D RNN, with their old message
    from rnnwavefunctions_amd import observables as O
    for fn in (lambda: wf.renyi2_regions(m, 4, seed=1), lambda: O.renyi2_regions(wf, m, 4), lambda: wf.renyi2_swap(4, seed=1)):
        with pytest.raises(ValueError, match=r"not implemented for the 2D RNN \(MDRNN\)"):
            fn()
    assert wf.lib.rnnwf_renyi2_regions(wf.h, mp, 2, None, 4, 1, 0, 0, up, None, None) == -1
    assert last() == "rnnwf_renyi2_regions: not implemented for the 2D RNN (MDRNN)"


# 7. builders and the reference-named facade
def test_builders_and_facade():
    Nx, Ny = 3, 4
    wf, _ = exact_state(Nx, Ny)
    cuts = np.concatenate([O2.row_cut_regions(Nx, Ny), O2.column_cut_regions(Nx, Ny), O2.rectangle_region(Nx, Ny, 0, 2, 0, 2)[None, :]])
    ref = np.stack(R.row_cuts(Nx, Ny) + R.column_cuts(Nx, Ny) + [R.rectangle(Nx, Ny, 0, 2, 0, 2)])
    assert np.array_equal(cuts, ref)
    s = wf.sample(2 * 40, seed=3)
    got = wf.renyi2_regions_2d(cuts, 40, samples=s, log_ratio=True)["log_ratio"]
    err = np.abs(got - explicit_log_ratio(wf, s, ref)).max()
    print("3x4 builders: max |log r - explicit| = %.2e" % err)
    assert err <= R.BOUND * Nx * Ny
    S2, e = O2.renyi2_regions(wf, cuts[0], 2000, seed=7)                            # one mask: one region
    assert S2.shape == (1,) and np.isfinite(S2[0]) and e[0] > 0
    S2b, _ = O2.renyi2_regions(wf, cuts[0].reshape(1, Nx, Ny), 2000, seed=7)
    assert np.array_equal(S2, S2b)
    with pytest.raises(ValueError, match="shape"):
        O2.renyi2_regions(wf, np.zeros((1, Ny, Nx), dtype=np.int32), 10)
    from rnnwavefunctions_amd.TFIM2D_2DRNN.Training2DRNN_2DTFIM import MDRNNcell, RNNwavefunction
    fac = RNNwavefunction(Nx, Ny, units=[10], cell=MDRNNcell, seed=111)
    S2, e = O2.renyi2_regions(fac, O2.column_cut_regions(Nx, Ny), 500)
    assert S2.shape == (Nx - 1,) and np.all(np.isfinite(S2)) and np.all(e >= 0)
    I2, ierr = O2.renyi2_mutual_information(fac, R.mask_of(Nx, Ny, [(1, 1)]).reshape(Nx, Ny), R.mask_of(Nx, Ny, [(1, 2)]), 500)
    assert np.isfinite(I2) and ierr >= 0
