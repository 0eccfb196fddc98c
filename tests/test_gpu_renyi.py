"""GPU tests of the second Renyi entropy by the swap trick (rnnwf_renyi2_swap, csrc/renyi_kernels.h, observables.renyi2_entropy)
on the positive GRU models: the f32 GRU1D and the f64 raster model GRU1D_F64.

Tolerances: log r_l against swapped configurations evaluated with rnnwf_log_prob: 1e-11 N (f64), 1e-5 N (f32 - the project's
parity bound; rnnwf_log_prob may run another base-pass kernel).  Exact identity over all pairs: relative 1e-12 (f64), 2e-5 (f32).
"""
import numpy as np
import pytest

from conftest import all_configs
from rnnwavefunctions_amd import params as P
from test_renyi_host import exact_renyi2, swap_log_ratio

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


def exact_from_wf(wf):
    return exact_renyi2(np.exp(0.5 * wf.log_prob(all_configs(wf.N))), wf.N)


def explicit_log_ratio(wf, pairs):
    sigma, tau = pairs[0::2], pairs[1::2]
    return np.stack([swap_log_ratio(wf.log_prob, sigma, tau, l) if 0 < l < wf.N else np.zeros(len(sigma))
                     for l in range(wf.N + 1)])


# 1. sum over every (sigma, tau) of P(sigma) P(tau) r_l = Tr rho_A^2
@pytest.mark.parametrize("f64,Nx,Ny,H,seed", [(False, 6, 1, 10, 3), (False, 6, 1, 20, 20), (True, 2, 3, 10, 3), (True, 3, 2, 20, 20)])
def test_exact_identity_over_all_pairs(f64, Nx, Ny, H, seed):
    N = Nx * Ny
    wf = make_wf(f64, Nx, Ny, H, trained_like(H, seed, f64))
    c = all_configs(N)
    lp = wf.log_prob(c)
    i, j = np.meshgrid(np.arange(2 ** N), np.arange(2 ** N), indexing="ij")
    pairs = np.empty((2 * i.size, N), dtype=np.int32)
    pairs[0::2], pairs[1::2] = c[i.ravel()], c[j.ravel()]
    out = wf.renyi2_swap(i.size, samples=pairs, want_log_ratio=True)
    w = np.exp(lp[i.ravel()] + lp[j.ravel()])
    purity = (w[None, :] * np.exp(out["log_ratio"])).sum(axis=1)
    exact = exact_renyi2(np.exp(0.5 * lp), N)
    # unnormalised exact purity (sum P)^2 Tr rho_A^2: the f32 model's P sums to 1 only to ~1e-7
    target = np.exp(-exact) * np.exp(lp).sum() ** 2
    rel = np.abs(purity / target - 1.0)
    print("%s %dx%d H=%d: S2 = %s, max rel |sum P P r - Tr rho_A^2| = %.2e"
          % ("f64" if f64 else "f32", Nx, Ny, H, np.round(exact, 4), rel.max()))
    assert exact[1:N].max() > 0.05
    assert rel.max() <= (1e-12 if f64 else 2e-5)
    assert np.all(out["log_ratio"][[0, N]] == 0.0)


# 2. per pair against explicit swapped configurations; every NFULL of the dispatch table, partial last blocks
F32_WIDTHS = [(10, 7), (30, 7), (50, 7), (60, 6), (90, 6), (120, 5), (180, 5), (250, 4)]      # NFULL 1 2 3 4 6 8 12 16
F64_WIDTHS = [(10, 7), (30, 7), (50, 6), (60, 6), (90, 5)]                                  # NFULL 1 2 3 4 6


@pytest.mark.parametrize("f64,H,N", [(False, H, N) for H, N in F32_WIDTHS] + [(True, H, N) for H, N in F64_WIDTHS])
def test_log_ratio_matches_explicit_swapped_configurations(f64, H, N):
    npairs = 13                                      # 26 chains: the second block of 16 is partial
    Nx, Ny = (N, 1) if not f64 else (N, 1)
    wf = make_wf(f64, Nx, Ny, H, trained_like(H, H, f64, scale=2.0 if H > 60 else 3.0))
    s = np.random.RandomState(H + N).randint(0, 2, size=(2 * npairs, N)).astype(np.int32)
    got = wf.renyi2_swap(npairs, samples=s, want_log_ratio=True)["log_ratio"]
    ref = explicit_log_ratio(wf, s)
    err = np.abs(got - ref).max()
    print("%s H=%d N=%d: max |log r - explicit| = %.2e (max |log r| %.2f)" % ("f64" if f64 else "f32", H, N, err, np.abs(ref).max()))
    assert err <= (1e-11 if f64 else 1e-5) * N
    assert np.abs(ref).max() > 1e-3


def test_raster_model_cuts_count_raster_sites():
    Nx, Ny, H = 3, 4, 20
    wf = make_wf(True, Nx, Ny, H, trained_like(H, 5, True))
    s = np.random.RandomState(7).randint(0, 2, size=(2 * 40, Nx * Ny)).astype(np.int32)
    got = wf.renyi2_swap(40, samples=s, want_log_ratio=True)["log_ratio"]
    assert np.abs(got - explicit_log_ratio(wf, s)).max() <= 1e-11 * Nx * Ny


# 3. a chain paired with itself, and all-zero weights
@pytest.mark.parametrize("f64,H,N", [(False, 50, 20), (False, 10, 9), (True, 50, 12), (True, 90, 8)])
def test_self_pairs_and_zero_weights_give_log_r_zero(f64, H, N):
    wf = make_wf(f64, N, 1, H, trained_like(H, 1, f64))
    s = np.random.RandomState(N).randint(0, 2, size=(37, N)).astype(np.int32)
    lr = wf.renyi2_swap(37, samples=np.repeat(s, 2, axis=0), want_log_ratio=True)["log_ratio"]
    print("%s H=%d N=%d: self pairs max |log r| = %.2e" % ("f64" if f64 else "f32", H, N, np.abs(lr).max()))
    assert np.abs(lr).max() <= (1e-11 if f64 else 2e-6) * N
    zero = {k: np.zeros_like(v) for k, v in trained_like(H, 1, f64).items()}
    wz = make_wf(f64, N, 1, H, zero)
    t = np.random.RandomState(N + 1).randint(0, 2, size=(2 * 37, N)).astype(np.int32)
    out = wz.renyi2_swap(37, samples=t, want_log_ratio=True)
    assert np.abs(out["log_ratio"]).max() <= 1e-13
    assert np.allclose(out["sums"], 37.0, rtol=1e-13, atol=0)


# 4. device draw: rnnwf_sample's chains, shards, passes
@pytest.mark.parametrize("f64,H,N", [(False, 50, 16), (False, 10, 11), (True, 20, 12)])
def test_device_draw_shards_and_passes(f64, H, N, monkeypatch):
    prm = trained_like(H, 9, f64)
    wf = make_wf(f64, N, 1, H, prm)
    npairs, k, seed, step, off = 700, 300, 123, 4, 50
    out = wf.renyi2_swap(npairs, seed=seed, step=step, pair_offset=off, want_log_ratio=True, want_samples=True)
    assert np.array_equal(out["samples"], wf.sample(2 * npairs, seed, step, 2 * off))
    again = wf.renyi2_swap(npairs, seed=seed, step=step, pair_offset=off, want_log_ratio=True)
    assert np.array_equal(again["log_ratio"], out["log_ratio"]) and np.array_equal(again["sums"], out["sums"])
    # explicit samples give the same per-pair values as the device draw
    fed = wf.renyi2_swap(npairs, samples=out["samples"], want_log_ratio=True)
    assert np.array_equal(fed["log_ratio"], out["log_ratio"])
    a = wf.renyi2_swap(k, seed=seed, step=step, pair_offset=off, want_log_ratio=True)
    b = wf.renyi2_swap(npairs - k, seed=seed, step=step, pair_offset=off + k, want_log_ratio=True)
    assert np.array_equal(np.concatenate([a["log_ratio"], b["log_ratio"]], axis=1), out["log_ratio"])
    assert np.allclose(a["sums"] + b["sums"], out["sums"], rtol=1e-13, atol=0)
    monkeypatch.setenv("RNNWF_STATE_BUDGET_MB", "1")             # several passes (whole 16-chain blocks each)
    many = make_wf(f64, N, 1, H, prm)
    m = many.renyi2_swap(npairs, seed=seed, step=step, pair_offset=off, want_log_ratio=True, want_samples=True)
    assert np.array_equal(m["samples"], out["samples"]) and np.array_equal(m["log_ratio"], out["log_ratio"])
    assert np.allclose(m["sums"], out["sums"], rtol=1e-13, atol=0)


# 5. statistics against the exact value
@pytest.mark.parametrize("f64,Nx,Ny,H,seed", [(False, 10, 1, 10, 10), (True, 3, 4, 10, 10)])
def test_s2_within_five_standard_errors_of_exact(f64, Nx, Ny, H, seed):
    from rnnwavefunctions_amd.observables import renyi2_entropy
    N = Nx * Ny
    wf = make_wf(f64, Nx, Ny, H, trained_like(H, seed, f64))
    exact = exact_from_wf(wf)
    S2, err = renyi2_entropy(wf, 2 ** 16, seed=2024)
    print("%s %dx%d: S2 = %s\n exact = %s\n err = %s" % ("f64" if f64 else "f32", Nx, Ny, np.round(S2, 4), np.round(exact, 4),
                                                      np.round(err, 4)))
    assert exact[1:N].max() > 0.05
    assert np.all(np.abs(S2 - exact) <= 5 * err + 1e-6)
    assert S2[0] == 0.0 and S2[N] == 0.0


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
            wf.renyi2_swap(4, seed=1)
    wf = make_wf(False, 6, 1, 10, trained_like(10, 1, False))
    with pytest.raises(ValueError, match="npairs"):
        wf.renyi2_swap(0, seed=1)
    with pytest.raises(ValueError, match="pair_offset"):
        wf.renyi2_swap(4, seed=1, pair_offset=-1)
    sums = np.empty((7, 2))
    assert wf.lib.rnnwf_renyi2_swap(wf.h, None, 4, 1, 0, 0, None, None, None) == -1
    assert b"sums" in wf.lib.rnnwf_last_error(wf.h)
    assert wf.lib.rnnwf_renyi2_swap(wf.h, None, -3, 1, 0, 0, sums.ctypes.data_as(C.POINTER(C.c_double)), None, None) == -1
    with pytest.raises(ValueError, match="shape"):
        wf.renyi2_swap(4, samples=np.zeros((7, 6), dtype=np.int32))


def test_resident_batch_rule():
    from rnnwavefunctions_amd import _lib
    N, H, ns = 8, 20, 256
    wf = make_wf(False, N, 1, H, trained_like(H, 2, False))
    shapes = {"wf_dense/kernel": (H, 2)}
    m = wf.vmc_step(ns, seed=5, step=0, couplings=np.append(np.ones(N), 1.0))["moments"]
    g0 = wf.vmc_gradient(m[0] / m[2], ns, shapes)["wf_dense/kernel"]
    with pytest.raises(ValueError):                              # refused: the batch stays resident
        wf.renyi2_swap(0, seed=1)
    g1 = wf.vmc_gradient(m[0] / m[2], ns, shapes)["wf_dense/kernel"]
    assert np.array_equal(g0, g1)
    wf.renyi2_swap(100, seed=1)                                  # overwrites the states: the gradient refuses
    with pytest.raises(_lib.RnnwfError, match="vmc_step first"):
        wf.vmc_gradient(m[0] / m[2], ns, shapes)


def test_timing_ids_and_work_counter():
    N, H, npairs = 12, 20, 100
    wf = make_wf(False, N, 1, H, trained_like(H, 2, False))
    wf.timing_enable(True)
    wf.renyi2_swap(npairs, seed=3)
    for kid in (0, 1, 2):
        t = wf.timing_get(kid)
        assert t["launches"] >= 1 and t["total_ms"] > 0
    assert wf.timing_get(1)["cell_evals"] == npairs * N * (N - 1)


# 7. the reference-named facades
def test_facades():
    from rnnwavefunctions_amd import compat as tf
    from rnnwavefunctions_amd.observables import renyi2_entropy
    from rnnwavefunctions_amd.TFIM1D.RNNwavefunction import RNNwavefunction as RNN1D
    from rnnwavefunctions_amd.TFIM2D_1DRNN.RNNwavefunction import RNNwavefunction as RNN2D
    for wf, N in ((RNN2D(3, 3, units=[10]), 9), (RNN1D(8, units=[10]), 8)):
        S2, err = renyi2_entropy(wf, 2000, seed=7)
        assert S2.shape == (N + 1,) and err.shape == (N + 1,)
        assert S2[0] == 0.0 and S2[N] == 0.0 and np.all(np.isfinite(S2))
    lstm = RNN2D(3, 3, cell=tf.contrib.rnn.LSTMCell, units=[10])
    with pytest.raises(ValueError, match="LSTM"):
        renyi2_entropy(lstm, 100)
