"""CPU tests of the complex RNN's stochastic-reconfiguration yardstick (tests/crnn_sr_reference.py) and of the host side of
rnnwavefunctions_amd/sr.py for it.  N = 6, every sample in the zero-magnetisation sector."""
import numpy as np
import pytest

import autograd_reference as A
import crnn_pauli_reference as CP
import crnn_sr_reference as C
import sr_reference as R
from rnnwavefunctions_amd import params as P
from rnnwavefunctions_amd import sr

EPS64 = 2.0 ** -53
PHASE = A.SCOPE + "/wf_dense_phase/"


@pytest.fixture(scope="module")
def case():
    N, H, ns = 6, 7, 19
    rng = np.random.RandomState(5)
    prm = {k: np.asarray(v, dtype=np.float64) for k, v in CP.weights(H, seed=3).items()}
    s = CP.random_sector_samples(N, ns, 11)
    e = rng.standard_normal(ns) + 1j * rng.standard_normal(ns)
    return prm, s, e, C.jacobian(prm, s)


def phase_columns(prm):
    """mask over the flat parameter vector: the phase head's own kernel and bias"""
    return np.concatenate([np.full(int(np.size(prm[k])), k.startswith(PHASE)) for k in C.names(prm)])


def test_twice_the_force_is_the_gradient_of_the_complex_cost(case):
    prm, s, e, o = case
    assert o.shape == (len(s), P.count_params(prm)) and np.abs(o.imag).max() > 0
    g = C.flatten({k: v[None] for k, v in A.gradient("crnn", prm, s, e).items()})[0]
    assert np.abs(2.0 * C.force(o, e) - g).max() <= 1e-12 * np.abs(g).max()
    # the same as Re(dO^H eps) / ns written with complex numbers
    d, eps = o - o.mean(axis=0), e - e.mean()
    assert np.abs(2.0 * np.real(d.conj().T @ eps) / len(s) - g).max() <= 1e-12 * np.abs(g).max()
    assert np.allclose(C.qgt(o), np.real(d.conj().T @ d) / len(s), rtol=0, atol=1e-14 * np.abs(C.qgt(o)).max())


def test_push_through_identity(case):
    """Obar^T (Obar Obar^T + ns lam)^-1 ebar = (S + lam)^-1 F.  Both sides come out of one LU solve, backward stable: a relative
    error of at most ~ order x 2^-53 x condition number each.  S and Obar Obar^T / ns share their non-zero spectrum, so both shifted
    matrices have condition number (|S|_2 + lam) / lam; the orders are nparams and 2 ns; factor 16 as everywhere."""
    prm, s, e, o = case
    for lam in (1e-3, 1e-1):
        a, b = C.minsr_direction(o, e, lam), C.sr_direction(o, e, lam)
        kappa = (np.linalg.norm(C.qgt(o), 2) + lam) / lam
        bound = 16 * (o.shape[1] + 2 * o.shape[0]) * EPS64 * kappa
        err = np.linalg.norm(a - b) / np.linalg.norm(b)
        print("lambda %g: |a - b| / |b| %.3e, bound %.3e (condition number %.3e)" % (lam, err, bound, kappa))
        assert err <= bound


def test_zero_phase_head_and_real_energies_reduce_to_the_positive_form(case):
    """Phase head at zero (kernel and bias) and real E_loc.  phi = pi softsign(z) with z = 0 everywhere, d phi / dz = pi: Im O is
    pi x (the selected column's hidden state, summed over the sites) on the phase head's kernel, pi N / 2 on its bias (the same for
    every sample of the sector: centred away), and EXACTLY zero on every other parameter (the chain rule multiplies by the zero
    kernel); Re O is exactly zero on the phase head.  So Im eps = 0, F = force of sqrt(P) (zero on the phase head), S is block
    diagonal - the QGT of sqrt(P) on the other parameters, Im dO^T Im dO / ns on the phase head - and delta is the positive model's
    direction on the other parameters and zero on the phase head."""
    prm, s, e, _ = case
    prm0 = dict(prm)
    for k in prm0:
        if k.startswith(PHASE):
            prm0[k] = np.zeros_like(prm0[k])
    o = C.jacobian(prm0, s)
    er = e.real
    ph = phase_columns(prm0)
    assert ph.sum() == 2 * 7 + 2
    assert np.array_equal(o.imag[:, ~ph], np.zeros_like(o.imag[:, ~ph])) and np.array_equal(o.real[:, ph], np.zeros_like(o.real[:, ph]))
    assert np.abs(o.imag[:, ph]).max() > 1.0
    bias = C.unflatten(o.imag, prm0)[PHASE + "bias"]
    assert np.abs(bias - np.pi * 3).max() <= 1e-14 * np.pi * 3          # N / 2 sites select either column
    assert np.array_equal(C.epsilon(er)[len(s):], np.zeros(len(s)))
    lam = 1e-2
    S, F, delta = C.qgt(o), C.force(o, er), C.sr_direction(o, er, lam)
    Sp, Fp = R.qgt(o.real), R.force(o.real, er)                          # sr_reference's forms on the log-derivatives of sqrt(P)
    scale = np.abs(S).max()
    assert np.abs(S[np.ix_(~ph, ~ph)] - Sp[np.ix_(~ph, ~ph)]).max() <= 1e-14 * scale
    assert np.array_equal(S[np.ix_(ph, ~ph)], np.zeros((ph.sum(), (~ph).sum())))
    dim = R.centred(o.imag[:, ph])
    assert np.abs(S[np.ix_(ph, ph)] - dim.T @ dim / len(s)).max() <= 1e-14 * scale
    assert np.abs(F - Fp).max() <= 1e-14 * np.abs(Fp).max() and np.array_equal(F[ph], np.zeros(ph.sum()))
    ref = R.sr_direction(o.real[:, ~ph], er, lam)
    assert np.linalg.norm(delta[~ph] - ref) <= 1e-10 * np.linalg.norm(ref) and np.array_equal(delta[ph], np.zeros(ph.sum()))
    mdir = C.minsr_direction(o, er, lam)
    assert np.linalg.norm(mdir - delta) <= 1e-9 * np.linalg.norm(delta)


def test_sites_fixed_by_the_mask_contribute_nothing_to_the_amplitude(case):
    """(1, 1, 1, 0, 0, 0): after three up spins the last three sites are forced, their conditional amplitude is 1 whatever the
    weights.  Dropping those sites' terms (site_weight 0) leaves d Re log psi unchanged to rounding; the phase is not masked, so
    d Im log psi changes."""
    prm = case[0]
    s = np.array([[1, 1, 1, 0, 0, 0], [0, 0, 0, 1, 1, 1], [1, 0, 1, 0, 1, 0]], dtype=np.int32)
    full = C.jacobian(prm, s)
    head = C.jacobian(prm, s, site_weight=[1.0, 1.0, 1.0, 0.0, 0.0, 0.0])
    scale = np.abs(full.real).max()
    assert np.abs(full.real[:2] - head.real[:2]).max() <= 1e-14 * scale
    assert np.abs(full.real[2] - head.real[2]).max() > 1e-3 * scale          # (1,0,1,0,1,0): only the last site is forced
    assert np.abs(full.imag[:2] - head.imag[:2]).max() > 1e-3 * np.abs(full.imag).max()


# ---- host side of sr.py: no device ------------------------------------------------------------------------------------------

class _Fake:
    """what sr.py needs of a complex NativeWavefunction, computed from the reference Jacobian: no device"""

    def __init__(self, prm, o, e):
        self.N, self.o, self.e, self.prm = 6, o, e, prm

    def _layout(self):
        return [(k[len(A.SCOPE) + 1:], int(self.prm[k].size)) for k in C.names(self.prm)]

    def log_derivatives_complex(self):
        return self.o

    def sr_gram_complex(self):
        return C.gram(self.o), C.epsilon(self.e)

    def sr_apply_complex(self, y):
        return C.stacked(self.o).T @ y


def test_minsr_direction_and_qgt_through_the_facade(case):
    prm, s, e, o = case
    wf = _Fake(prm, o, e)
    ref = C.minsr_direction(o, e, 1e-2)
    assert np.linalg.norm(sr.minsr_direction_complex(wf, 1e-2) - ref) <= 1e-10 * np.linalg.norm(ref)
    assert np.allclose(sr.qgt_complex(wf), C.qgt(o), rtol=0, atol=1e-15 * np.abs(C.qgt(o)).max())


def test_host_side_argument_refusals(case):
    prm, s, e, o = case
    wf = _Fake(prm, o, e)
    for bad in (0.0, -1e-3, np.inf, np.nan):
        with pytest.raises(ValueError, match="diag_shift"):
            sr.minsr_direction_complex(wf, bad)
        with pytest.raises(ValueError, match="diag_shift"):
            sr.train_j1j2(wf, 1.0, 0.2, 0.0, prm, 1, 10, 1e-2, bad, 1)
    with pytest.raises(ValueError, match="solver"):
        sr.minsr_direction_complex(wf, 1e-3, solver="gpu")
    with pytest.raises(ValueError, match="numsamples"):
        sr.train_j1j2(wf, 1.0, 0.2, 0.0, prm, 1, 1, 1e-2, 1e-3, 1)
