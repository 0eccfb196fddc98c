"""CPU tests of the 2D RNN's stochastic-reconfiguration yardstick (tests/mdrnn_sr_reference.py) and of the host side of
rnnwavefunctions_amd/sr.py for it.  3 x 2 lattice, 7 units."""
import numpy as np
import pytest

import autograd_reference as A
import mdrnn_sr_reference as R
from rnnwavefunctions_amd import params as P
from rnnwavefunctions_amd import sr

EPS64 = 2.0 ** -53


@pytest.fixture(scope="module")
def case():
    Nx, Ny, H, ns = 3, 2, 7, 19
    rng = np.random.RandomState(5)
    prm = P.randomize_biases(P.scale_kernels(P.init_mdrnn_params(H, seed=3), 1.25), 4)
    prm = {k: np.asarray(v, dtype=np.float64) for k, v in prm.items()}
    s = rng.randint(0, 2, size=(ns, Nx, Ny)).astype(np.int32)
    e = rng.standard_normal(ns) * 2.0 - 3.0
    return prm, s, e, R.jacobian(prm, s)


def test_weighted_sum_is_the_gradient_of_the_cost(case):
    """sum_s 2 w_s O_s with w_s = (E_s - mean E) / ns, which is 2 F, is autograd's gradient of the reference's cost"""
    prm, s, e, o = case
    assert o.shape == (len(s), P.count_params(prm)) and np.abs(o).max() > 0
    g = R.flatten({k: v[None] for k, v in A.gradient("mdrnn", prm, s, e).items()})[0]
    w = (e - e.mean()) / len(s)
    assert np.abs(2.0 * w @ o - g).max() <= 1e-12 * np.abs(g).max()
    assert np.abs(2.0 * R.force(o, e) - g).max() <= 1e-12 * np.abs(g).max()


def test_push_through_identity(case):
    """dO^T (dO dO^T + ns lam)^-1 eps = (S + lam)^-1 F; both sides one backward-stable LU solve with condition number
    (|S|_2 + lam) / lam, of orders ns and nparams; factor 16 as everywhere."""
    prm, s, e, o = case
    for lam in (1e-3, 1e-1):
        a, b = R.minsr_direction(o, e, lam), R.sr_direction(o, e, lam)
        kappa = (np.linalg.norm(R.qgt(o), 2) + lam) / lam
        bound = 16 * (o.shape[1] + o.shape[0]) * EPS64 * kappa
        err = np.linalg.norm(a - b) / np.linalg.norm(b)
        print("lambda %g: |a - b| / |b| %.3e, bound %.3e (condition number %.3e)" % (lam, err, bound, kappa))
        assert err <= bound


def test_rows_of_the_centred_jacobian_sum_to_zero(case):
    prm, s, e, o = case
    d = R.centred(o)
    assert np.abs(d.sum(axis=0)).max() <= len(s) * 4 * EPS64 * np.abs(o).max()
    assert np.abs(R.gram(o).sum(axis=1)).max() <= len(s) * o.shape[1] * 8 * EPS64 * np.abs(o).max() ** 2


def test_lattice_axes_are_not_interchangeable(case):
    """the 3 x 2 and the 2 x 3 lattice walk different zig-zag paths: the same spins reshaped give another Jacobian"""
    prm, s, e, o = case
    o2 = R.jacobian(prm, s.reshape(len(s), 2, 3))
    assert np.abs(o2 - o).max() > 1e-3 * np.abs(o).max()


# ---- host side of sr.py: no device ------------------------------------------------------------------------------------------

class _Fake:
    """what sr.py needs of a 2D NativeWavefunction, computed from the reference Jacobian: no device"""

    def __init__(self, prm, o, e):
        self.N, self.o, self.e, self.prm = 6, o, e, prm

    def _layout(self):
        return [(k[len(A.SCOPE) + 1:], int(self.prm[k].size)) for k in R.names(self.prm)]

    def log_derivatives_2d(self):
        return self.o

    def sr_gram_2d(self):
        return R.gram(self.o), R.epsilon(self.e)

    def sr_apply_2d(self, y):
        return R.centred(self.o).T @ y


def test_minsr_direction_and_qgt_through_the_facade(case):
    prm, s, e, o = case
    wf = _Fake(prm, o, e)
    ref = R.minsr_direction(o, e, 1e-2)
    assert np.linalg.norm(sr.minsr_direction_2d(wf, 1e-2) - ref) <= 1e-10 * np.linalg.norm(ref)
    assert np.allclose(sr.qgt_2d(wf), R.qgt(o), rtol=0, atol=1e-15 * np.abs(R.qgt(o)).max())


def test_host_side_argument_refusals(case):
    prm, s, e, o = case
    wf = _Fake(prm, o, e)
    for bad in (0.0, -1e-3, np.inf, np.nan):
        with pytest.raises(ValueError, match="diag_shift"):
            sr.minsr_direction_2d(wf, bad)
        with pytest.raises(ValueError, match="diag_shift"):
            sr.train_tfim2d(wf, 1.0, 3.0, prm, 1, 10, 1e-2, bad, 1)
    with pytest.raises(ValueError, match="solver"):
        sr.minsr_direction_2d(wf, 1e-3, solver="gpu")
    with pytest.raises(ValueError, match="numsamples"):
        sr.train_tfim2d(wf, 1.0, 3.0, prm, 1, 1, 1e-2, 1e-3, 1)
    with pytest.raises(ValueError, match="Jz"):
        sr.train_tfim2d(wf, np.ones(5), 3.0, prm, 1, 10, 1e-2, 1e-3, 1)
