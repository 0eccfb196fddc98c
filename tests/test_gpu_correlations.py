"""GPU tests of the correlation functions (rnnwf_correlations, csrc/corr_kernels.h, observables.correlations) on the positive GRU
models: the f32 GRU1D and the f64 raster model GRU1D_F64.

Tolerances: log r against flipped configurations evaluated with rnnwf_log_prob: 1e-11 N (f64), 1e-5 N (f32 - the project's parity
bound; rnnwf_log_prob may run another base-pass kernel).  log r_i against the flip pass's log-prob queue: half the difference of
two log-probabilities, each within 2e-6 N + 2e-6 (f32, either engine: tests/test_gpu_prnn.py) or 1e-11 N (f64).  Exact identity
over all configurations: relative 1e-12 (f64), 2e-5 (f32), as tests/test_gpu_renyi.py.
"""
import numpy as np
import pytest

import correlations_reference as R
from conftest import all_configs
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


def explicit_log_ratio(wf, s):
    """(N + N(N-1)/2, ns) through rnnwf_log_prob on NumPy-flipped configurations."""
    N = wf.N
    base = wf.log_prob(s)
    rows = []
    for i in range(N):
        x = s.copy()
        x[:, i] = 1 - x[:, i]
        rows.append(0.5 * (wf.log_prob(x) - base))
    for i, j in zip(*R.pair_list(N)):
        x = s.copy()
        x[:, i] = 1 - x[:, i]
        x[:, j] = 1 - x[:, j]
        rows.append(0.5 * (wf.log_prob(x) - base))
    return np.stack(rows)


# 1. sum over every sigma of P(sigma) r = <psi| sx_i sx_j |psi>
@pytest.mark.parametrize("f64,Nx,Ny,H,seed", [(False, 10, 1, 10, 10), (False, 10, 1, 20, 20), (True, 3, 4, 10, 10), (True, 4, 3, 20, 20)])
def test_exact_identity_over_all_configurations(f64, Nx, Ny, H, seed):
    N = Nx * Ny
    wf = make_wf(f64, Nx, Ny, H, trained_like(H, seed, f64))
    c = all_configs(N)
    lp = wf.log_prob(c)
    out = wf.correlations(len(c), samples=c, want_log_ratio=True)
    w = np.exp(lp)
    got = np.exp(out["log_ratio"]) @ w
    z, zz, x, xx = R.exact_from_log_probs(lp, N)
    pi, pj = R.pair_list(N)
    target = np.concatenate([x, xx[pi, pj]]) * w.sum()        # unnormalised: the f32 model's P sums to 1 only to ~1e-7
    rel = np.abs(got / target - 1.0)
    print("%s %dx%d H=%d: max rel |sum P r - <sx sx>| = %.2e; max |xx_c| = %.3f" % ("f64" if f64 else "f32", Nx, Ny, H, rel.max(),
                                                                                  np.abs(xx - np.outer(x, x))[pi, pj].max()))
    assert np.abs(xx - np.outer(x, x))[pi, pj].max() > 1e-3
    assert rel.max() <= (1e-12 if f64 else 2e-5)
    zs, zzs = R.diag_sums(c)
    assert np.array_equal(out["z_sums"], zs) and np.array_equal(out["zz_sums"], zzs)


# 2. per chain: singles against the flip pass's queue, everything against explicit flipped configurations
F32_WIDTHS = [(10, 7), (30, 7), (50, 7), (60, 6), (90, 6), (120, 5), (180, 5), (250, 4),      # NFULL 1 2 3 4 6 8 12 16
              (17, 6), (34, 6), (51, 6), (36, 6), (52, 6), (68, 5), (100, 5)]                 # remainder units 1, 2, 3, 4 (x 4)
F64_WIDTHS = [(10, 7), (30, 7), (50, 6), (60, 6), (90, 5), (53, 5), (68, 5), (100, 5)]      # NFULL 1 2 3 4 6; 4-wave rows; widest


@pytest.mark.parametrize("f64,H,N", [(False, H, N) for H, N in F32_WIDTHS] + [(True, H, N) for H, N in F64_WIDTHS])
def test_log_ratio_matches_flip_queue_and_explicit_configurations(f64, H, N):
    ns = 27                                          # the second block of 16 is partial
    wf = make_wf(f64, N, 1, H, trained_like(H, H, f64, scale=2.0 if H > 60 else 3.0))
    s = np.random.RandomState(H + N).randint(0, 2, size=(ns, N)).astype(np.int32)
    got = wf.correlations(ns, samples=s, want_log_ratio=True)["log_ratio"]
    lpq = np.zeros((N + 1, ns))
    wf.tfim_eloc(s, np.ones(N), 1.0, log_probs=lpq)
    err1 = np.abs(got[:N] - 0.5 * (lpq[1:] - lpq[0])).max()
    ref = explicit_log_ratio(wf, s)
    err = np.abs(got - ref).max()
    print("%s H=%d N=%d: max |log r_i - queue| = %.2e, max |log r - explicit| = %.2e (max |log r| %.2f)"
          % ("f64" if f64 else "f32", H, N, err1, err, np.abs(ref).max()))
    assert err1 <= (1e-11 * N if f64 else 2e-6 * N + 2e-6)
    assert err <= (1e-11 if f64 else 1e-5) * N
    assert np.abs(ref[N:]).max() > 1e-3


def test_raster_model_sites_are_in_raster_order():
    Nx, Ny, H = 3, 4, 20
    wf = make_wf(True, Nx, Ny, H, trained_like(H, 5, True))
    s = np.random.RandomState(7).randint(0, 2, size=(40, Nx * Ny)).astype(np.int32)
    got = wf.correlations(40, samples=s, want_log_ratio=True)["log_ratio"]
    assert np.abs(got - explicit_log_ratio(wf, s)).max() <= 1e-11 * Nx * Ny


# 3. all-zero weights
@pytest.mark.parametrize("f64,H,N", [(False, 50, 20), (False, 10, 9), (True, 50, 12), (True, 90, 8)])
def test_zero_weights_give_log_r_zero_and_exact_diagonal_sums(f64, H, N):
    zero = {k: np.zeros_like(v) for k, v in trained_like(H, 1, f64).items()}
    wz = make_wf(f64, N, 1, H, zero)
    t = np.random.RandomState(N + 1).randint(0, 2, size=(75, N)).astype(np.int32)
    out = wz.correlations(75, samples=t, want_log_ratio=True)
    assert np.abs(out["log_ratio"]).max() <= 1e-13
    zs, zzs = R.diag_sums(t)
    assert np.array_equal(out["z_sums"], zs) and np.array_equal(out["zz_sums"], zzs)
    assert np.allclose(out["x_sums"], 75.0, rtol=1e-12, atol=0)
    iu = np.triu_indices(N, 1)
    assert np.allclose(out["xx_sums"][iu], 75.0, rtol=1e-12, atol=0)
    il = np.tril_indices(N)
    assert np.all(out["xx_sums"][il] == 0.0)


# 4. statistics against the exact values
@pytest.mark.parametrize("f64,Nx,Ny,H,seed", [(False, 10, 1, 10, 10), (True, 3, 4, 10, 10)])
def test_means_within_five_standard_errors_of_exact(f64, Nx, Ny, H, seed):
    from rnnwavefunctions_amd.observables import correlations
    N = Nx * Ny
    wf = make_wf(f64, Nx, Ny, H, trained_like(H, seed, f64))
    z, zz, x, xx = R.exact_from_log_probs(wf.log_prob(all_configs(N)), N)
    c = correlations(wf, 2 ** 16, seed=2024)
    pi, pj = R.pair_list(N)
    worst = {}
    for k, exact in (("z", z), ("zz", zz), ("x", x), ("xx", xx), ("zz_c", zz - np.outer(z, z)), ("xx_c", xx - np.outer(x, x))):
        with np.errstate(invalid="ignore", divide="ignore"):
            t = np.abs(c[k] - exact) / c[k + "_err"]
        t = t[np.isfinite(t)]
        worst[k] = float(t.max())
        assert np.all(np.abs(c[k] - exact) <= 5 * c[k + "_err"] + 1e-6), k
    xx_c = np.abs(xx - np.outer(x, x))[pi, pj].max()
    print("%s %dx%d: worst |mean - exact| / err = %s; exact max |xx_c| = %.4f, largest xx_c err = %.4f"
          % ("f64" if f64 else "f32", Nx, Ny, {k: round(v, 2) for k, v in worst.items()}, xx_c, c["xx_c_err"][pi, pj].max()))
    # Non-triviality floor 0.02: on the CPU reference (oracle GRU in float64, these weights) the largest exact connected xx is 0.0499
    # (10 x 1, 10 units, seed 10) and 0.0567 (3 x 4); a product state has 0 everywhere.  With errors below 0.004 at 2^16 samples a
    # product-state estimate (xx = x x^T) would miss such a pair by more than 5 standard errors.
    assert xx_c > 0.02 and 5 * c["xx_c_err"][pi, pj].max() < 0.02
    assert np.all(np.diag(c["xx"]) == 1.0) and np.all(np.diag(c["zz"]) == 1.0)


# 5. device draw: rnnwf_sample's chains, repeated calls, shards, passes
@pytest.mark.parametrize("f64,H,N", [(False, 50, 16), (False, 10, 11), (True, 20, 12)])
def test_device_draw_repeats_shards_and_passes(f64, H, N, monkeypatch):
    prm = trained_like(H, 9, f64)
    wf = make_wf(f64, N, 1, H, prm)
    ns, k, seed, step, off = 1403, 592, 123, 4, 50
    keys = ("z_sums", "zz_sums", "x_sums", "xx_sums")
    out = wf.correlations(ns, seed=seed, step=step, sample_offset=off, want_log_ratio=True, want_samples=True)
    assert np.array_equal(out["samples"], wf.sample(ns, seed, step, off).reshape(ns, N))
    again = wf.correlations(ns, seed=seed, step=step, sample_offset=off, want_log_ratio=True)
    assert np.array_equal(again["log_ratio"], out["log_ratio"]) and all(np.array_equal(again[q], out[q]) for q in keys)
    fed = wf.correlations(ns, samples=out["samples"], want_log_ratio=True)
    assert np.array_equal(fed["log_ratio"], out["log_ratio"]) and all(np.array_equal(fed[q], out[q]) for q in keys)
    a = wf.correlations(k, seed=seed, step=step, sample_offset=off, want_log_ratio=True)
    b = wf.correlations(ns - k, seed=seed, step=step, sample_offset=off + k, want_log_ratio=True)
    assert np.array_equal(np.concatenate([a["log_ratio"], b["log_ratio"]], axis=1), out["log_ratio"])
    for q in keys:
        assert np.allclose(a[q] + b[q], out[q], rtol=1e-12, atol=0), q
    assert np.array_equal(a["z_sums"] + b["z_sums"], out["z_sums"]) and np.array_equal(a["zz_sums"] + b["zz_sums"], out["zz_sums"])
    monkeypatch.setenv("RNNWF_STATE_BUDGET_MB", "1")             # several passes (whole 16-chain blocks each)
    many = make_wf(f64, N, 1, H, prm)
    many.timing_enable(True)
    m = many.correlations(ns, seed=seed, step=step, sample_offset=off, want_log_ratio=True, want_samples=True)
    assert many.timing_get(2)["launches"] >= 3
    assert np.array_equal(m["samples"], out["samples"]) and np.array_equal(m["log_ratio"], out["log_ratio"])
    for q in keys:
        assert np.allclose(m[q], out[q], rtol=1e-12, atol=0), q
    assert np.array_equal(m["zz_sums"], out["zz_sums"])
    # the sums are those of the log-ratios
    xs, xxs = R.sums_from_log_ratio(out["log_ratio"], N)
    assert np.allclose(out["x_sums"], xs, rtol=1e-12, atol=0) and np.allclose(out["xx_sums"], xxs, rtol=1e-12, atol=0)


# 6. refusals and the resident batch
def test_refused_models_and_arguments():
    import ctypes as C
    from rnnwavefunctions_amd import _lib
    cases = [(_lib.MODEL_GRU1D_PARITY, 6, 1, (10,), "parity"), (_lib.MODEL_CRNN_U1, 6, 1, (10,), "complex RNN"),
             (_lib.MODEL_MDRNN2D, 3, 3, (10,), "MDRNN"), (_lib.MODEL_LSTM1D_F64, 3, 3, (10,), "LSTM"),
             (_lib.MODEL_GRU1D, 6, 1, (10, 10), "stacked layers"), (_lib.MODEL_GRU1D_F64, 3, 2, (10, 10), "stacked layers")]
    for model, nx, ny, units, why in cases:
        wf = _lib.NativeWavefunction(model, nx, ny, units)
        wf.init_params(1)
        with pytest.raises(ValueError, match=why):
            wf.correlations(4, seed=1)
    wf = make_wf(False, 6, 1, 10, trained_like(10, 1, False))
    with pytest.raises(ValueError, match="ns must be"):
        wf.correlations(0, seed=1)
    with pytest.raises(ValueError, match="sample_offset"):
        wf.correlations(4, seed=1, sample_offset=-1)
    f64p = C.POINTER(C.c_double)
    bufs = [np.empty(6), np.empty((6, 6)), np.empty((6, 2)), np.empty((6, 6, 5))]
    ptrs = [b.ctypes.data_as(f64p) for b in bufs]
    for missing in range(4):
        args = [None if k == missing else p for k, p in enumerate(ptrs)]
        assert wf.lib.rnnwf_correlations(wf.h, None, 4, 1, 0, 0, *args, None, None) == -1
        assert b"sums" in wf.lib.rnnwf_last_error(wf.h)
    assert wf.lib.rnnwf_correlations(wf.h, None, -3, 1, 0, 0, *ptrs, None, None) == -1
    assert wf.lib.rnnwf_correlations(wf.h, None, 4, 1, 0, 0, *ptrs, None, None) == 0
    with pytest.raises(ValueError, match="shape"):
        wf.correlations(4, samples=np.zeros((7, 6), dtype=np.int32))


def test_resident_batch_rule():
    from rnnwavefunctions_amd import _lib
    N, H, ns = 8, 20, 256
    wf = make_wf(False, N, 1, H, trained_like(H, 2, False))
    shapes = {"wf_dense/kernel": (H, 2)}
    m = wf.vmc_step(ns, seed=5, step=0, couplings=np.append(np.ones(N), 1.0))["moments"]
    g0 = wf.vmc_gradient(m[0] / m[2], ns, shapes)["wf_dense/kernel"]
    with pytest.raises(ValueError):                              # refused: the batch stays resident
        wf.correlations(0, seed=1)
    g1 = wf.vmc_gradient(m[0] / m[2], ns, shapes)["wf_dense/kernel"]
    assert np.array_equal(g0, g1)
    wf.correlations(100, seed=1)                                 # overwrites the states: the gradient refuses
    with pytest.raises(_lib.RnnwfError, match="vmc_step first"):
        wf.vmc_gradient(m[0] / m[2], ns, shapes)


def test_timing_ids_and_work_counter():
    N, H, ns = 12, 20, 100
    wf = make_wf(False, N, 1, H, trained_like(H, 2, False))
    wf.timing_enable(True)
    wf.correlations(ns, seed=3)
    for kid in (0, 1, 2):
        t = wf.timing_get(kid)
        assert t["launches"] >= 1 and t["total_ms"] > 0
    assert wf.timing_get(1)["launches"] == 2                     # trunk + branch
    assert wf.timing_get(1)["cell_evals"] == ns * (N * (N - 1) // 2 + N * (N - 1) * (N - 2) // 6)


def test_short_chains():
    for N in (1, 2, 3):
        wf = make_wf(False, N, 1, 10, trained_like(10, 3, False))
        s = all_configs(N)
        s = np.concatenate([s] * 5)
        got = wf.correlations(len(s), samples=s, want_log_ratio=True)
        assert np.abs(got["log_ratio"] - explicit_log_ratio(wf, s)).max() <= 1e-5 * N
        zs, zzs = R.diag_sums(s)
        assert np.array_equal(got["z_sums"], zs) and np.array_equal(got["zz_sums"], zzs)


# 7. the reference-named facades
def test_facades():
    from rnnwavefunctions_amd import compat as tf
    from rnnwavefunctions_amd.observables import correlations
    from rnnwavefunctions_amd.TFIM1D.RNNwavefunction import RNNwavefunction as RNN1D
    from rnnwavefunctions_amd.TFIM2D_1DRNN.RNNwavefunction import RNNwavefunction as RNN2D
    for wf, N in ((RNN2D(3, 3, units=[10]), 9), (RNN1D(8, units=[10]), 8)):
        c = correlations(wf, 2000, seed=7)
        assert c["z"].shape == (N,) and c["xx"].shape == (N, N) and c["xx_c_err"].shape == (N, N)
        assert all(np.all(np.isfinite(v)) for v in c.values())
        assert np.array_equal(c["xx"], c["xx"].T) and np.array_equal(c["zz"], c["zz"].T)
    lstm = RNN2D(3, 3, cell=tf.contrib.rnn.LSTMCell, units=[10])
    with pytest.raises(ValueError, match="LSTM"):
        correlations(lstm, 100)
