"""Corners of the ping-pong kernels' tile walk (csrc/pp_kernels.h: PPWalk, the lock-step count, the staging slot): fewer tiles than the
eight waves of a workgroup - idle waves execute barriers only - a single tile, a single step per chain, batches that are no multiple
of the 32-chain tile, chains past one spin word, and every kernel of the layer pipeline (first, middle, top).  Each case pins the
bf16x3 engine and compares the local energies with the float64 oracle at the tolerances of the both-engines tests of
test_gpu_prnn.py / test_gpu_crnn.py (one layer: test_both_*_engines_agree_with_the_f64_oracle; stacks: test_stacked_layers_on_both_engines)."""
import numpy as np
import pytest

from oracle import estimators as E
from oracle import models as M
from rnnwavefunctions_amd import params as P

pytestmark = pytest.mark.gpu


def params_like(H, L, seed, heads):
    # the weight scales of trained_like (one layer) and stacked_like (stacks) in test_gpu_prnn.py / test_gpu_crnn.py
    return P.randomize_biases(P.scale_kernels(P.init_gru_params([H] * L, seed=seed, heads=heads), 2.0 if L == 1 else 1.6), seed + 1)


def pinned_bf16x3(monkeypatch, model, N, H, L, prm):
    from rnnwavefunctions_amd import _lib
    monkeypatch.setenv("RNNWF_ENGINE", "bf16x3")                 # read once, at rnnwf_create
    wf = _lib.NativeWavefunction(model, N, 1, (H,) * L)
    wf.set_params(prm, scope="RNNwavefunction")
    return wf


@pytest.mark.parametrize("N,H,L,ns", [(2, 37, 1, 1), (3, 50, 1, 33), (3, 44, 2, 33), (5, 50, 3, 40), (34, 50, 2, 9)])
def test_prnn_flip_walk_corners(N, H, L, ns, monkeypatch):
    from rnnwavefunctions_amd import _lib
    prm = params_like(H, L, seed=N + H + L, heads=("wf_dense",))
    prm64 = {k: v.astype(np.float64) for k, v in prm.items()}
    rng = np.random.RandomState(N + ns)
    s = rng.randint(0, 2, (ns, N)).astype(np.int32)
    Jz = 1.0 + 0.1 * rng.standard_normal(N)
    e64 = E.ising_local_energies(Jz, 1.1, s, lambda x: M.prnn_log_probability(prm64, x, dtype=np.float64))
    wf = pinned_bf16x3(monkeypatch, _lib.MODEL_GRU1D, N, H, L, prm)
    e = wf.tfim_eloc(s, Jz, 1.1)
    assert wf.engine_name() == "bf16x3"
    err = np.abs(e / e64 - 1).max()
    print("pRNN N=%d H=%d L=%d ns=%d: max rel E_loc err = %.2e" % (N, H, L, ns, err))
    if L == 1:
        assert err <= 2e-5
    else:
        assert np.allclose(e, e64, rtol=3e-5)


@pytest.mark.parametrize("N,H,L,ns", [(4, 37, 1, 2), (6, 50, 3, 33), (34, 44, 2, 5)])
def test_crnn_swap_walk_corners(N, H, L, ns, monkeypatch):
    from rnnwavefunctions_amd import _lib
    prm = params_like(H, L, seed=N + H + L, heads=("wf_dense_ampl", "wf_dense_phase"))
    prm64 = {k: v.astype(np.float64) for k, v in prm.items()}
    rng = np.random.RandomState(N + ns)
    s = np.stack([rng.permutation(np.repeat([0, 1], N // 2)) for _ in range(ns)]).astype(np.int32)
    J1, J2, Bz = 1.0 + 0.1 * rng.standard_normal(N), 0.4 * np.ones(N), np.zeros(N)
    e64 = E.j1j2_local_energies(J1, J2, Bz, s, lambda x: M.crnn_log_amplitude(prm64, x, dtype=np.float64), False, False)
    wf = pinned_bf16x3(monkeypatch, _lib.MODEL_CRNN_U1, N, H, L, prm)
    e, _ = wf.j1j2_eloc(s, J1, J2, Bz, False, False)
    assert wf.engine_name() == "bf16x3"
    err = np.abs(e - e64).max() / max(1.0, np.abs(e64).max())
    print("cRNN N=%d H=%d L=%d ns=%d: max |E_loc - f64| / max|E| = %.2e" % (N, H, L, ns, err))
    if L == 1:
        assert err < 3e-5
    else:
        assert np.allclose(e, e64, rtol=1e-4, atol=1e-4)
