"""GPU tests of the second Renyi entropy of arbitrary regions (rnnwf_renyi2_regions, csrc/renyi_region_kernels.h,
observables.renyi2_regions / renyi2_mutual_information) on the positive GRU models: the f32 GRU1D and the f64 raster model GRU1D_F64.

Tolerances, the project's own (docs/renyi.md, tests/test_gpu_prnn.py): log r_A against swapped configurations evaluated with
rnnwf_log_prob: 1e-11 N (f64), 1e-5 N (f32).  Exact identity over all pairs: relative 1e-12 (f64), 2e-5 (f32).  Against
rnnwf_renyi2_swap on prefix regions: 1e-11 N in both precisions (the same chains are evaluated; only the f64 assembly order differs).
"""
import ctypes as C

import numpy as np
import pytest

from conftest import all_configs
from renyi_regions_reference import purity_of_region
from rnnwavefunctions_amd import params as P

pytestmark = pytest.mark.gpu

SCOPE = "RNNwavefunction"


def trained_like(H, seed, f64, scale=3.0):
    prm = P.init_gru_params([H], seed=seed, dtype=np.float64 if f64 else np.float32)
    return P.randomize_biases(P.scale_kernels(prm, scale), seed + 1)


def make_wf(f64, Nx, Ny, H, prm):
    from rnnwavefunctions_amd import _lib
    wf = _lib.NativeWavefunction(_lib.MODEL_GRU1D_F64 if f64 else _lib.MODEL_GRU1D, Nx, Ny, (H,))
    wf.set_params(prm, scope=SCOPE)
    return wf


def mask_of(N, sites):
    m = np.zeros(N, dtype=np.int32)
    m[list(sites)] = 1
    return m


def explicit_log_ratio(wf, pairs, masks):
    """log r_A from both swapped configurations, written out in NumPy and scored with rnnwf_log_prob."""
    sigma, tau = pairs[0::2], pairs[1::2]
    own = wf.log_prob(sigma) + wf.log_prob(tau)
    out = []
    for m in masks:
        in_a = m.astype(bool)[None, :]
        a, b = np.where(in_a, tau, sigma).astype(np.int32), np.where(in_a, sigma, tau).astype(np.int32)
        out.append(0.5 * (wf.log_prob(a) + wf.log_prob(b) - own))
    return np.stack(out)


def exact_regions(f64, Nx, Ny):
    """[(name, mask)] of the exact-expectation and statistical tests: a bulk interval, a two-piece region, a single site; on the
    raster also a column cut and a 2x2 corner block."""
    N = Nx * Ny
    out = [("bulk interval 3..6", mask_of(N, range(3, 6))), ("two pieces {1,2} u {6,7}", mask_of(N, [1, 2, 6, 7])), ("site 4", mask_of(N, [4]))]
    if Ny > 1:
        out.append(("columns < 1", mask_of(N, [ny * Nx for ny in range(Ny)])))
        out.append(("columns < 2", mask_of(N, [ny * Nx + nx for ny in range(Ny) for nx in range(2)])))
        out.append(("corner 2x2", mask_of(N, [0, 1, Nx, Nx + 1])))
        out.append(("far corner 2x2", mask_of(N, [N - 1, N - 2, N - 1 - Nx, N - 2 - Nx])))
    return out


# the weights of the exact and statistical tests: seed 20, chosen on the CPU with the oracle so that the mutual informations below are
# not vacuous - exact I2 (f32 N = 10 / f64 3x4): sites {3} : {5} 0.176 / 0.174; blocks {1,2} : {6,7} 0.089 (f32), {0,1,3,4} : {8,11}
# 0.111 (f64).  Required floor: 0.05.
EXACT_SEED = 20
I2_FLOOR = 0.05
EXACT_CASES = [(False, 10, 1, 10), (True, 3, 4, 10)]


def i2_regions(f64, Nx, Ny):
    N = Nx * Ny
    blocks = (mask_of(N, [0, 1, Nx, Nx + 1]), mask_of(N, [8, 11])) if Ny > 1 else (mask_of(N, [1, 2]), mask_of(N, [6, 7]))
    return [(mask_of(N, [3]), mask_of(N, [5])), blocks]


def exact_purities(wf, masks):
    psi = np.exp(0.5 * wf.log_prob(all_configs(wf.N)))
    return np.array([purity_of_region(psi, wf.N, m) for m in masks])


# 1. sum over every (sigma, tau) of P(sigma) P(tau) r_A = Tr rho_A^2 from the dense vector
@pytest.mark.parametrize("f64,Nx,Ny,H", EXACT_CASES)
def test_exact_expectation_over_all_pairs(f64, Nx, Ny, H):
    N = Nx * Ny
    wf = make_wf(f64, Nx, Ny, H, trained_like(H, EXACT_SEED, f64))
    names, masks = zip(*exact_regions(f64, Nx, Ny))
    masks = np.stack(masks)
    c = all_configs(N)
    lp = wf.log_prob(c)
    exact = exact_purities(wf, masks)
    norm2 = np.exp(lp).sum() ** 2                    # the f32 model's P sums to 1 only to ~1e-7
    purity = np.zeros(len(masks))
    rows = 2 ** N
    for i0 in range(0, rows, 64):                    # sigma in slabs of 64 configurations, tau all of them
        i, j = np.meshgrid(np.arange(i0, min(rows, i0 + 64)), np.arange(rows), indexing="ij")
        pairs = np.empty((2 * i.size, N), dtype=np.int32)
        pairs[0::2], pairs[1::2] = c[i.ravel()], c[j.ravel()]
        out = wf.renyi2_regions(masks, i.size, samples=pairs, log_ratio=True)
        assert "samples" not in out
        purity += (np.exp(lp[i.ravel()] + lp[j.ravel()])[None, :] * np.exp(out["log_ratio"])).sum(axis=1)
    rel = np.abs(purity / (exact * norm2) - 1.0)
    print("%s %dx%d H=%d: S2 = %s, max rel |sum P P r_A - Tr rho_A^2| = %.2e"
          % ("f64" if f64 else "f32", Nx, Ny, H, np.round(-np.log(exact), 4), rel.max()))
    assert (-np.log(exact)).max() > 0.05
    assert rel.max() <= (1e-12 if f64 else 2e-5)


# 2. per pair against explicit swapped configurations; every NFULL of the dispatch table, partial last blocks, remainder widths
F32_WIDTHS = [(10, 7), (30, 7), (50, 7), (60, 6), (90, 6), (120, 5), (180, 5), (250, 4),      # NFULL 1 2 3 4 6 8 12 16
              (16, 7), (20, 7), (36, 7), (64, 6), (100, 6), (128, 5), (133, 5), (256, 4)]     # other remainders of the hidden width
F64_WIDTHS = [(10, 7), (30, 7), (50, 6), (60, 6), (90, 5), (16, 7), (36, 7), (53, 6), (68, 6), (100, 5)]


def small_regions(N):
    masks = [mask_of(N, [1]), mask_of(N, [N - 1]), mask_of(N, range(2, N - 1)), mask_of(N, range(0, N, 2)), mask_of(N, [0, N - 1]),
             mask_of(N, [1, 2, N - 2]), mask_of(N, range(N // 2)), mask_of(N, range(N // 2, N)), mask_of(N, []), mask_of(N, range(N))]
    return np.stack(masks)


@pytest.mark.parametrize("f64,H,N", [(False, H, N) for H, N in F32_WIDTHS] + [(True, H, N) for H, N in F64_WIDTHS])
def test_log_ratio_matches_explicit_swapped_configurations(f64, H, N):
    npairs = 13                                      # 26 chains: the second block of 16 is partial
    wf = make_wf(f64, N, 1, H, trained_like(H, H, f64, scale=2.0 if H > 60 else 3.0))
    s = np.random.RandomState(H + N).randint(0, 2, size=(2 * npairs, N)).astype(np.int32)
    masks = small_regions(N)
    got = wf.renyi2_regions(masks, npairs, samples=s, log_ratio=True)["log_ratio"]
    ref = explicit_log_ratio(wf, s, masks)
    err = np.abs(got - ref).max()
    print("%s H=%d N=%d: max |log r - explicit| = %.2e (max |log r| %.2f)" % ("f64" if f64 else "f32", H, N, err, np.abs(ref).max()))
    assert got.shape == (len(masks), npairs)
    assert err <= (1e-11 if f64 else 1e-5) * N
    assert np.abs(ref).max() > 1e-3


@pytest.mark.parametrize("f64,Nx,Ny,H", [(True, 3, 4, 20), (False, 70, 1, 20), (True, 9, 4, 20)])
def test_raster_and_multi_word_regions_against_explicit_configurations(f64, Nx, Ny, H):
    """Raster regions on 3x4 and 9x4 (two spin words), and a 70-site chain (three words) with regions around the word boundaries."""
    from rnnwavefunctions_amd.observables import column_cut_regions, interval_region, rectangle_region
    N = Nx * Ny
    wf = make_wf(f64, Nx, Ny, H, trained_like(H, 5, f64))
    s = np.random.RandomState(7).randint(0, 2, size=(2 * 40, N)).astype(np.int32)
    masks = [interval_region(N, 1, N - 1), interval_region(N, N - 1, N), mask_of(N, range(1, N, 2))]
    if Ny > 1:
        masks += list(column_cut_regions(Nx, Ny)) + [rectangle_region(Nx, Ny, 0, 2, 0, 2), rectangle_region(Nx, Ny, Nx - 2, Nx, Ny - 2, Ny),
                                                     rectangle_region(Nx, Ny, 1, 2, 1, 3)]
    for w in range(32, N, 32):
        masks += [interval_region(N, w - 3, w), interval_region(N, w, min(N, w + 3)), interval_region(N, w - 1, w + 1), mask_of(N, [w]),
                  mask_of(N, [w - 1])]
    masks = np.stack(masks)
    got = wf.renyi2_regions(masks, 40, samples=s, log_ratio=True)["log_ratio"]
    ref = explicit_log_ratio(wf, s, masks)
    err = np.abs(got - ref).max(axis=1)
    print("%s %dx%d: %d regions, max |log r - explicit| = %.2e (max |log r| %.2f)" % ("f64" if f64 else "f32", Nx, Ny, len(masks), err.max(),
                                                                                   np.abs(ref).max()))
    assert err.max() <= (1e-11 if f64 else 1e-5) * N and np.all(np.abs(ref).max(axis=1) > 1e-3)


# 3. cross-check with the existing pass
@pytest.mark.parametrize("f64,H,N", [(False, 50, 40), (False, 20, 70), (True, 50, 12), (True, 20, 36), (False, 10, 2), (True, 10, 3)])
def test_prefix_regions_equal_the_swap_pass(f64, H, N):
    npairs = 45
    wf = make_wf(f64, N, 1, H, trained_like(H, 7, f64))
    s = np.random.RandomState(N).randint(0, 2, size=(2 * npairs, N)).astype(np.int32)
    swap = wf.renyi2_swap(npairs, samples=s, want_log_ratio=True)["log_ratio"]
    prefix = (np.arange(N)[None, :] < np.arange(1, N)[:, None]).astype(np.int32)
    a = wf.renyi2_regions(prefix, npairs, samples=s, log_ratio=True)
    b = wf.renyi2_regions(1 - prefix, npairs, samples=s, log_ratio=True)
    d = np.abs(a["log_ratio"] - swap[1:N]).max()
    print("%s H=%d N=%d: prefix regions vs renyi2_swap max |d log r| = %.2e (max |log r| %.2f)"
          % ("f64" if f64 else "f32", H, N, d, np.abs(swap).max()))
    assert d <= 1e-11 * N
    assert np.array_equal(a["log_ratio"], b["log_ratio"]) and np.array_equal(a["sums"], b["sums"])
    assert np.abs(swap[1:N]).max() > 1e-3


# 4. a chain paired with itself, and all-zero weights
@pytest.mark.parametrize("f64,H,N", [(False, 50, 20), (False, 10, 9), (False, 20, 40), (True, 50, 12), (True, 90, 8)])
def test_self_pairs_and_zero_weights_give_log_r_zero(f64, H, N):
    wf = make_wf(f64, N, 1, H, trained_like(H, 1, f64))
    s = np.random.RandomState(N).randint(0, 2, size=(37, N)).astype(np.int32)
    masks = small_regions(N)
    lr = wf.renyi2_regions(masks, 37, samples=np.repeat(s, 2, axis=0), log_ratio=True)["log_ratio"]
    print("%s H=%d N=%d: self pairs max |log r| = %.2e" % ("f64" if f64 else "f32", H, N, np.abs(lr).max()))
    assert np.abs(lr).max() <= (1e-11 if f64 else 2e-6) * N
    zero = {k: np.zeros_like(v) for k, v in trained_like(H, 1, f64).items()}
    wz = make_wf(f64, N, 1, H, zero)
    t = np.random.RandomState(N + 1).randint(0, 2, size=(2 * 37, N)).astype(np.int32)
    out = wz.renyi2_regions(masks, 37, samples=t, log_ratio=True)
    assert np.abs(out["log_ratio"]).max() <= 1e-13
    assert np.allclose(out["sums"], 37.0, rtol=1e-12, atol=0)


# 5. statistics against the exact values
@pytest.mark.parametrize("f64,Nx,Ny,H", EXACT_CASES)
def test_s2_and_mutual_information_within_five_standard_errors_of_exact(f64, Nx, Ny, H):
    from rnnwavefunctions_amd.observables import renyi2_mutual_information, renyi2_regions
    N, npairs = Nx * Ny, 2 ** 16
    wf = make_wf(f64, Nx, Ny, H, trained_like(H, EXACT_SEED, f64))
    names, masks = zip(*exact_regions(f64, Nx, Ny))
    masks = np.stack(masks)
    exact = -np.log(exact_purities(wf, masks))
    S2, err = renyi2_regions(wf, masks, npairs, seed=2024)
    print("%s %dx%d: S2 = %s\n exact = %s\n err = %s" % ("f64" if f64 else "f32", Nx, Ny, np.round(S2, 4), np.round(exact, 4), np.round(err, 4)))
    assert S2.shape == err.shape == (len(masks),)
    assert exact.max() > 0.05 and np.all(err > 0)
    assert np.all(np.abs(S2 - exact) <= 5 * err + 1e-6)
    for a, b in i2_regions(f64, Nx, Ny):
        ea, eb, eab = -np.log(exact_purities(wf, np.stack([a, b, a | b])))
        i2_exact = ea + eb - eab
        I2, ierr = renyi2_mutual_information(wf, a, b, npairs, seed=2025)
        print(" I2(%s : %s) = %.4f +- %.4f, exact %.4f" % (np.flatnonzero(a).tolist(), np.flatnonzero(b).tolist(), I2, ierr, i2_exact))
        assert i2_exact > I2_FLOOR
        assert 0 < ierr < i2_exact / 3                             # resolved (CPU reference at 2^16 pairs: errors 0.005 .. 0.011, I2 0.09 .. 0.18)
        assert abs(I2 - i2_exact) <= 5 * ierr + 1e-6
    with pytest.raises(ValueError, match="disjoint"):
        renyi2_mutual_information(wf, masks[0], masks[0], 10)


# 6. call behaviour
@pytest.mark.parametrize("f64,H,N", [(False, 50, 16), (False, 10, 40), (True, 20, 12)])
def test_device_draw_repeats_shards_and_passes(f64, H, N, monkeypatch):
    prm = trained_like(H, 9, f64)
    wf = make_wf(f64, N, 1, H, prm)
    masks = small_regions(N)
    masks = np.concatenate([masks, masks[2:4]])                   # duplicates
    npairs, k, seed, step, off = 700, 300, 123, 4, 50
    out = wf.renyi2_regions(masks, npairs, seed=seed, step=step, pair_offset=off, log_ratio=True)
    assert np.array_equal(out["samples"], wf.sample(2 * npairs, seed, step, 2 * off).reshape(2 * npairs, N))
    again = wf.renyi2_regions(masks, npairs, seed=seed, step=step, pair_offset=off, log_ratio=True)
    assert np.array_equal(again["log_ratio"], out["log_ratio"]) and np.array_equal(again["sums"], out["sums"])
    fed = wf.renyi2_regions(masks, npairs, samples=out["samples"], log_ratio=True)
    assert np.array_equal(fed["log_ratio"], out["log_ratio"]) and np.array_equal(fed["sums"], out["sums"])
    lr = out["log_ratio"]
    assert np.all(lr[8] == 0.0) and np.all(lr[9] == 0.0) and np.all(out["sums"][8:10] == float(npairs))      # empty and full: exactly 0
    assert np.array_equal(lr[10:12], lr[2:4]) and np.array_equal(out["sums"][10:12], out["sums"][2:4])      # duplicates
    assert np.abs(lr[:8]).max() > 1e-3
    # the order of the regions in the call does not matter
    perm = np.random.RandomState(0).permutation(len(masks))
    shuffled = wf.renyi2_regions(masks[perm], npairs, samples=out["samples"], log_ratio=True)
    assert np.array_equal(shuffled["log_ratio"], lr[perm]) and np.array_equal(shuffled["sums"], out["sums"][perm])
    a = wf.renyi2_regions(masks, k, seed=seed, step=step, pair_offset=off, log_ratio=True)
    b = wf.renyi2_regions(masks, npairs - k, seed=seed, step=step, pair_offset=off + k, log_ratio=True)
    assert np.array_equal(np.concatenate([a["log_ratio"], b["log_ratio"]], axis=1), lr)
    assert np.allclose(a["sums"] + b["sums"], out["sums"], rtol=1e-13, atol=0)
    monkeypatch.setenv("RNNWF_STATE_BUDGET_MB", "1")             # several passes (whole 16-chain blocks each)
    many = make_wf(f64, N, 1, H, prm)
    many.timing_enable(True)
    m = many.renyi2_regions(masks, npairs, seed=seed, step=step, pair_offset=off, log_ratio=True)
    assert many.timing_get(2)["launches"] >= 2
    assert np.array_equal(m["samples"], out["samples"]) and np.array_equal(m["log_ratio"], lr)
    assert np.allclose(m["sums"], out["sums"], rtol=1e-13, atol=0)


@pytest.mark.parametrize("f64,N", [(False, 2), (False, 3), (True, 2), (True, 3)])
def test_smallest_chains(f64, N):
    H = 10
    wf = make_wf(f64, N, 1, H, trained_like(H, 4, f64))
    masks = np.array([[(k >> n) & 1 for n in range(N)] for k in range(2 ** N)], dtype=np.int32)        # every subset
    c = all_configs(N)
    i, j = np.meshgrid(np.arange(2 ** N), np.arange(2 ** N), indexing="ij")
    pairs = np.empty((2 * i.size, N), dtype=np.int32)
    pairs[0::2], pairs[1::2] = c[i.ravel()], c[j.ravel()]
    got = wf.renyi2_regions(masks, i.size, samples=pairs, log_ratio=True)["log_ratio"]
    assert np.abs(got - explicit_log_ratio(wf, pairs, masks)).max() <= (1e-11 if f64 else 1e-5) * N
    assert np.all(got[0] == 0.0) and np.all(got[-1] == 0.0)


def test_timing_ids_and_work_counter():
    N, H, npairs = 12, 20, 100
    wf = make_wf(False, N, 1, H, trained_like(H, 2, False))
    masks = np.stack([mask_of(N, [3, 7]), mask_of(N, range(0, 5)), mask_of(N, [N - 1]), mask_of(N, []), mask_of(N, range(N)),
                      mask_of(N, [0, 1, 2, 11]), mask_of(N, [1])])
    first = [3, 5, 11, None, None, 3, 1]                          # after normalisation; None: empty
    wf.timing_enable(True)
    wf.renyi2_regions(masks, npairs, seed=3)
    for kid in (0, 1, 2):
        t = wf.timing_get(kid)
        assert t["launches"] >= 1 and t["total_ms"] > 0
    assert wf.timing_get(1)["cell_evals"] == 2 * npairs * sum(N - f for f in first if f is not None)
    wf.timing_reset()
    wf.renyi2_regions(masks[3:5], npairs, seed=3)                 # nothing but empty regions: no cell evaluation
    assert wf.timing_get(1)["cell_evals"] == 0 and wf.timing_get(1)["launches"] == 0


# 7. refusals and the resident batch
def test_refused_models_and_arguments():
    from rnnwavefunctions_amd import _lib
    from rnnwavefunctions_amd import compat as tf
    from rnnwavefunctions_amd.observables import renyi2_mutual_information, renyi2_regions
    from rnnwavefunctions_amd.TFIM2D_1DRNN.RNNwavefunction import RNNwavefunction as RNN2D
    cases = [(_lib.MODEL_GRU1D_PARITY, 6, 1, (10,), "parity"), (_lib.MODEL_CRNN_U1, 6, 1, (10,), "complex RNN"),
             (_lib.MODEL_MDRNN2D, 3, 3, (10,), "MDRNN"), (_lib.MODEL_LSTM1D_F64, 3, 3, (10,), "LSTM"),
             (_lib.MODEL_GRU1D, 6, 1, (10, 10), "stacked layers"), (_lib.MODEL_GRU1D_F64, 3, 2, (10, 10), "stacked layers")]
    i32p, f64p = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    for model, nx, ny, units, why in cases:
        wf = _lib.NativeWavefunction(model, nx, ny, units)
        wf.init_params(1)
        m = mask_of(nx * ny, [1])
        with pytest.raises(ValueError, match=why):
            wf.renyi2_regions(m, 4, seed=1)
        with pytest.raises(ValueError, match=why):
            renyi2_regions(wf, m, 4)
        with pytest.raises(ValueError, match=why):                # the existing pass refuses as before
            wf.renyi2_swap(4, seed=1)
        sums = np.empty((1, 2))
        assert wf.lib.rnnwf_renyi2_regions(wf.h, m.ctypes.data_as(i32p), 1, None, 4, 1, 0, 0, sums.ctypes.data_as(f64p), None, None) == -1
        assert b"rnnwf_renyi2_regions" in wf.lib.rnnwf_last_error(wf.h)
    lstm = RNN2D(3, 3, cell=tf.contrib.rnn.LSTMCell, units=[10])
    with pytest.raises(ValueError, match="LSTM"):
        renyi2_regions(lstm, mask_of(9, [4]), 100)
    with pytest.raises(ValueError, match="LSTM"):
        renyi2_mutual_information(lstm, mask_of(9, [4]), mask_of(9, [6]), 100)

    N = 6
    wf = make_wf(False, N, 1, 10, trained_like(10, 1, False))
    m = np.stack([mask_of(N, [1]), mask_of(N, [2, 3])])
    mp, sums = m.ctypes.data_as(i32p), np.empty((2, 2))
    sp = sums.ctypes.data_as(f64p)
    call = wf.lib.rnnwf_renyi2_regions
    with pytest.raises(ValueError, match="npairs"):
        wf.renyi2_regions(m, 0, seed=1)
    with pytest.raises(ValueError, match="pair_offset"):
        wf.renyi2_regions(m, 4, seed=1, pair_offset=-1)
    bad = m.copy()
    bad[1, 4] = 2
    with pytest.raises(ValueError, match=r"regions\[1\]\[4\] = 2"):
        wf.renyi2_regions(bad, 4, seed=1)
    bad[1, 4] = -1
    with pytest.raises(ValueError, match="0 or 1"):
        wf.renyi2_regions(bad, 4, seed=1)
    with pytest.raises(ValueError, match="shape"):
        wf.renyi2_regions(np.zeros((2, N + 1), dtype=np.int32), 4)
    with pytest.raises(ValueError, match="shape"):
        wf.renyi2_regions(np.zeros((0, N), dtype=np.int32), 4)
    with pytest.raises(ValueError, match="shape"):
        wf.renyi2_regions(m, 4, samples=np.zeros((7, N), dtype=np.int32))
    assert call(wf.h, mp, 0, None, 4, 1, 0, 0, sp, None, None) == -1 and b"nregions" in wf.lib.rnnwf_last_error(wf.h)
    assert call(wf.h, mp, -2, None, 4, 1, 0, 0, sp, None, None) == -1 and b"nregions" in wf.lib.rnnwf_last_error(wf.h)
    assert call(wf.h, mp, 2, None, -3, 1, 0, 0, sp, None, None) == -1 and b"npairs" in wf.lib.rnnwf_last_error(wf.h)
    assert call(wf.h, None, 2, None, 4, 1, 0, 0, sp, None, None) == -1 and b"regions" in wf.lib.rnnwf_last_error(wf.h)
    assert call(wf.h, mp, 2, None, 4, 1, 0, 0, None, None, None) == -1 and b"sums" in wf.lib.rnnwf_last_error(wf.h)
    assert call(wf.h, mp, 2, None, 4, 1, 0, -1, sp, None, None) == -1 and b"pair_offset" in wf.lib.rnnwf_last_error(wf.h)
    # with hand-fed samples pair_offset is ignored, as in rnnwf_renyi2_swap
    s = np.zeros((8, N), dtype=np.int32)
    assert call(wf.h, mp, 2, s.ctypes.data_as(i32p), 4, 1, 0, -1, sp, None, None) == 0
    # the existing pass's refusals of arguments are as they were
    with pytest.raises(ValueError, match="npairs"):
        wf.renyi2_swap(0, seed=1)
    with pytest.raises(ValueError, match="pair_offset"):
        wf.renyi2_swap(4, seed=1, pair_offset=-1)


def test_resident_batch_rule():
    from rnnwavefunctions_amd import _lib
    N, H, ns = 8, 20, 256
    wf = make_wf(False, N, 1, H, trained_like(H, 2, False))
    shapes = {"wf_dense/kernel": (H, 2)}
    m = wf.vmc_step(ns, seed=5, step=0, couplings=np.append(np.ones(N), 1.0))["moments"]
    g0 = wf.vmc_gradient(m[0] / m[2], ns, shapes)["wf_dense/kernel"]
    mask = mask_of(N, [2, 5])
    bad = mask.copy()
    bad[3] = 7
    for refused in (lambda: wf.renyi2_regions(mask, 0, seed=1), lambda: wf.renyi2_regions(bad, 10, seed=1),
                    lambda: wf.renyi2_regions(mask, 10, seed=1, pair_offset=-1)):
        with pytest.raises(ValueError):                          # refused: the batch stays resident
            refused()
        g1 = wf.vmc_gradient(m[0] / m[2], ns, shapes)["wf_dense/kernel"]
        assert np.array_equal(g0, g1)
    wf.renyi2_regions(mask, 100, seed=1)                          # overwrites the states: the gradient refuses
    with pytest.raises(_lib.RnnwfError, match="vmc_step first"):
        wf.vmc_gradient(m[0] / m[2], ns, shapes)


# 8. the reference-named facades
def test_facades():
    from rnnwavefunctions_amd.observables import column_cut_regions, interval_region, renyi2_mutual_information, renyi2_regions
    from rnnwavefunctions_amd.TFIM1D.RNNwavefunction import RNNwavefunction as RNN1D
    from rnnwavefunctions_amd.TFIM2D_1DRNN.RNNwavefunction import RNNwavefunction as RNN2D
    S2, err = renyi2_regions(RNN2D(3, 3, units=[10]), column_cut_regions(3, 3), 2000, seed=7)
    assert S2.shape == err.shape == (2,) and np.all(np.isfinite(S2)) and np.all(err >= 0)
    wf = RNN1D(8, units=[10])
    S2, err = renyi2_regions(wf, interval_region(8, 2, 5), 2000, seed=7)          # one mask: one region
    assert S2.shape == (1,) and np.isfinite(S2[0])
    I2, ierr = renyi2_mutual_information(wf, interval_region(8, 1, 3), interval_region(8, 5, 7), 2000, seed=7)
    assert np.isfinite(I2) and ierr >= 0
