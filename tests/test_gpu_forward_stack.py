"""The one-wave forward kernels of the f32/f64-input MFMA engine across the single-layer / stack boundary.

One layer and stacks run the same four pass bodies (csrc/gru_kernels.h: prnn_base_pass, prnn_flip_pass; csrc/crnn_kernels.h:
crnn_base_pass, crnn_swap_pass) over one layer-stack core (csrc/gru_core.h: GruStack).  What differs between them at compile time -
the first layer's step variant, the checkpoint row (NL * KT values, all N sites for a stack, N - 1 for one layer), the waves per
workgroup of the stack's base pass - is what these cases exercise: two spin words, a ragged second 16-chain block, RNNWF_ENGINE=f32
and RNNWF_NO_COOP=1 so that exactly these kernels run, against the float64 oracle.

Tolerances (those of the stack tests of test_gpu_prnn.py): log-probabilities and the log-probability queue 2e-6 N L + 2e-6 in
float32, 1e-11 N in float64; local energies rtol 3e-5 (float64 model: 1e-9).

The complex RNN runs N = 34, not 33: its U(1) mask allows N // 2 spins of either kind, so a chain of odd length has no configuration
of non-zero amplitude (every log-amplitude is -inf and there is nothing to compare); 34 is the next length with two spin words.
"""
import functools

import numpy as np
import pytest

from oracle import estimators as E
from oracle import models as M
from oracle import philox
from rnnwavefunctions_amd import params as P

pytestmark = pytest.mark.gpu

SCOPE = "RNNwavefunction"
N, NS = 33, 17
NX, NY = 11, 3             # the float64 model lives on a lattice: 33 sites in raster order
NC = 34                    # complex RNN (module docstring)
CHEADS = ("wf_dense_ampl", "wf_dense_phase")
PRNN = [("f32", 20, 1), ("f32", 20, 2), ("f32", 68, 3), ("f64", 20, 1), ("f64", 36, 2)]
CRNN = [(20, 1), (50, 2)]


def f64(prm):
    return {k: v.astype(np.float64) for k, v in prm.items()}


def tol(dt, L, n=N):
    return 1e-11 * n if dt == "f64" else 2e-6 * n * L + 2e-6


@pytest.fixture(autouse=True)
def one_wave_f32_kernels(monkeypatch):
    monkeypatch.setenv("RNNWF_ENGINE", "f32")
    monkeypatch.setenv("RNNWF_NO_COOP", "1")


def prnn_wf(dt, H, L, prm):
    from rnnwavefunctions_amd import _lib
    if dt == "f64":
        wf = _lib.NativeWavefunction(_lib.MODEL_GRU1D_F64, NX, NY, (H,) * L)
    else:
        wf = _lib.NativeWavefunction(_lib.MODEL_GRU1D, N, 1, (H,) * L)
    wf.set_params(prm, scope=SCOPE)
    return wf


@functools.lru_cache(maxsize=None)
def prnn_case(dt, H, L, ns=NS):
    """Parameters, teacher-forced spins and the float64 references of one case (computed once, read-only)."""
    prm = P.randomize_biases(P.scale_kernels(P.init_gru_params([H] * L, seed=H + L, dtype=np.float64 if dt == "f64" else np.float32), 1.6), H)
    prm64 = f64(prm)
    rng = np.random.RandomState(H + 7 * L)
    s = rng.randint(0, 2, (ns, N)).astype(np.int32)
    logp = lambda x: M.prnn_log_probability(prm64, x, dtype=np.float64)
    if dt == "f64":
        Jz = 1.0 + 0.1 * rng.standard_normal((NX, NY))
        e_ref, q_ref = E.ising2d_local_energies(Jz, 0.9, NX, NY, s, logp, return_log_probs=True)
    else:
        Jz = 1.0 + 0.1 * rng.standard_normal(N)
        e_ref, q_ref = E.ising_local_energies(Jz, 0.9, s, logp, return_log_probs=True)
    for a in (s, Jz, e_ref, q_ref):
        a.setflags(write=False)
    return prm, prm64, s, Jz, logp(s), e_ref, q_ref


@pytest.mark.parametrize("dt,H,L", PRNN)
def test_prnn_sampling(dt, H, L):
    prm, prm64 = prnn_case(dt, H, L)[:2]
    wf = prnn_wf(dt, H, L, prm)
    s, lg = wf.sample(NS, seed=21, step=3, return_log=True)
    s = s.reshape(NS, N)
    s_ref, _ = M.prnn_sample(prm64, N, philox.uniforms(21, 3, 0, NS, N), dtype=np.float64)
    # a draw can leave the oracle's only where u is within float rounding of p0: ~N * 1e-6 per chain, so one chain at the very most
    same = ~(s != s_ref).any(axis=1)
    assert same.sum() >= NS - 1
    err = np.abs(lg - M.prnn_log_probability(prm64, s, dtype=np.float64)).max()
    print("pRNN %s H=%d L=%d sampling: max |log P - oracle64| = %.2e" % (dt, H, L, err))
    assert err <= tol(dt, L)


@pytest.mark.parametrize("dt,H,L", PRNN)
def test_prnn_log_probability(dt, H, L):
    prm, _, s, _, lp_ref = prnn_case(dt, H, L)[:5]
    err = np.abs(prnn_wf(dt, H, L, prm).log_prob(s) - lp_ref).max()
    print("pRNN %s H=%d L=%d: max |log P - oracle64| = %.2e" % (dt, H, L, err))
    assert err <= tol(dt, L)


def check_prnn_energies(dt, H, L, wf, case):
    _, _, s, Jz, _, e_ref, q_ref = case
    q = np.zeros(q_ref.size)
    e = wf.tfim_eloc(s, Jz, 0.9, log_probs=q)
    print("pRNN %s H=%d L=%d ns=%d: max |queue - oracle64| = %.2e, max rel dE = %.2e" %
          (dt, H, L, len(s), np.abs(q - q_ref.ravel()).max(), np.abs(e / e_ref - 1).max()))
    assert np.abs(q - q_ref.ravel()).max() <= tol(dt, L)
    assert np.allclose(e, e_ref, rtol=1e-9 if dt == "f64" else 3e-5)
    return e, q


@pytest.mark.parametrize("dt,H,L", PRNN)
def test_prnn_local_energies(dt, H, L):
    case = prnn_case(dt, H, L)
    check_prnn_energies(dt, H, L, prnn_wf(dt, H, L, case[0]), case)


def test_prnn_stack_in_three_passes(monkeypatch):
    """68 units x 3 layers keep 33 sites x 51 values x 64 lanes x 4 B = 421 KB per 16 chains: a budget of 1 MB holds two blocks, so 81
    chains run as 32 + 32 + 17 - every pass writes and reads its checkpoints from row 0 with the stack's stride and site count."""
    dt, H, L, ns = "f32", 68, 3, 81
    case = prnn_case(dt, H, L, ns)
    e1, q1 = check_prnn_energies(dt, H, L, prnn_wf(dt, H, L, case[0]), case)
    monkeypatch.setenv("RNNWF_STATE_BUDGET_MB", "1")
    e3, q3 = check_prnn_energies(dt, H, L, prnn_wf(dt, H, L, case[0]), case)
    assert np.array_equal(e1, e3) and np.array_equal(q1, q3)


# ---- complex RNN --------------------------------------------------------------------------------------------------------------

def crnn_wf(H, L, prm):
    from rnnwavefunctions_amd import _lib
    wf = _lib.NativeWavefunction(_lib.MODEL_CRNN_U1, NC, 1, (H,) * L)
    wf.set_params(prm, scope=SCOPE)
    return wf


@functools.lru_cache(maxsize=None)
def crnn_case(H, L, ns=NS):
    prm = P.randomize_biases(P.scale_kernels(P.init_gru_params([H] * L, seed=H + L, heads=CHEADS), 1.6), H)
    prm64 = f64(prm)
    rng = np.random.RandomState(H + 7 * L)
    s = np.stack([rng.permutation(np.repeat([0, 1], NC // 2)) for _ in range(ns)]).astype(np.int32)
    J1, J2, Bz = 1.0 + 0.1 * rng.standard_normal(NC), 0.5 + 0.1 * rng.standard_normal(NC), 0.1 * rng.standard_normal(NC)
    amp = lambda x: M.crnn_log_amplitude(prm64, x, dtype=np.float64)
    e_ref = E.j1j2_local_energies(J1, J2, Bz, s, amp, True, False)        # periodic couplings
    for a in (s, J1, J2, Bz, e_ref):
        a.setflags(write=False)
    return prm, prm64, s, (J1, J2, Bz), amp(s), e_ref


@pytest.mark.parametrize("H,L", CRNN)
def test_crnn_sampling(H, L):
    prm, prm64 = crnn_case(H, L)[:2]
    wf = crnn_wf(H, L, prm)
    s, lg = wf.sample(NS, seed=21, step=3, return_log=True)
    assert np.all(s.sum(axis=1) == NC // 2)
    s_ref = M.crnn_sample(prm, NC, philox.uniforms(21, 3, 0, NS, NC))
    assert (~(s != s_ref).any(axis=1)).sum() >= NS - 1                     # as test_prnn_sampling
    err = np.abs(lg - 2.0 * M.crnn_log_amplitude(prm64, s, dtype=np.float64).real).max()
    print("cRNN H=%d L=%d sampling: max |log P - oracle64| = %.2e" % (H, L, err))
    assert err <= tol("f32", L, NC)


@pytest.mark.parametrize("H,L", CRNN)
def test_crnn_log_probability(H, L):
    prm, _, s, _, a_ref = crnn_case(H, L)[:5]
    wf = crnn_wf(H, L, prm)
    err = np.abs(wf.log_prob(s) - 2.0 * a_ref.real).max()
    got = wf.log_amp(s)
    print("cRNN H=%d L=%d: max |log P - oracle64| = %.2e, |d re| = %.2e, |d im| = %.2e" %
          (H, L, err, np.abs(got.real - a_ref.real).max(), np.abs(got.imag - a_ref.imag).max()))
    assert err <= tol("f32", L, NC)


def check_crnn_energies(H, L, wf, case):
    _, _, s, (J1, J2, Bz), _, e_ref = case
    e, ncon = wf.j1j2_eloc(s, J1, J2, Bz, periodic=True, marshall=False)
    print("cRNN H=%d L=%d ns=%d: max rel |dE| = %.2e" % (H, L, len(s), np.abs(e / e_ref - 1).max()))
    assert np.allclose(e, e_ref, rtol=3e-5)
    return e, ncon


@pytest.mark.parametrize("H,L", CRNN)
def test_crnn_local_energies(H, L):
    case = crnn_case(H, L)
    check_crnn_energies(H, L, crnn_wf(H, L, case[0]), case)


def test_crnn_stack_in_three_passes(monkeypatch):
    """50 units x 2 layers keep 34 sites x 26 values x 64 lanes x 4 B = 221 KB per 16 chains: a budget of 1 MB holds four blocks, so
    150 chains run as 64 + 64 + 22."""
    H, L, ns = 50, 2, 150
    case = crnn_case(H, L, ns)
    e1, n1 = check_crnn_energies(H, L, crnn_wf(H, L, case[0]), case)
    monkeypatch.setenv("RNNWF_STATE_BUDGET_MB", "1")
    e3, n3 = check_crnn_energies(H, L, crnn_wf(H, L, case[0]), case)
    assert n1 == n3 and np.allclose(e1, e3, rtol=1e-6, atol=1e-6)       # as test_multi_pass_estimators_equal_the_single_pass
