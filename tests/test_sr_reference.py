"""CPU tests of the stochastic-reconfiguration yardstick (tests/sr_reference.py) and of the host side of rnnwavefunctions_amd/sr.py."""
import os
import re

import numpy as np
import pytest
import torch

import autograd_reference as A
import sr_reference as R
from rnnwavefunctions_amd import params as P
from rnnwavefunctions_amd import sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def case():
    N, H, ns = 6, 7, 19
    rng = np.random.RandomState(5)
    prm = P.randomize_biases(P.scale_kernels(P.init_gru_params([H], seed=3, dtype=np.float64), 2.0), 4)
    s = rng.randint(0, 2, size=(ns, N)).astype(np.int32)
    e = rng.standard_normal(ns)
    return prm, s, e, R.jacobian(prm, s)


def test_jacobian_ties_to_the_gradient_of_the_cost(case):
    prm, s, e, o = case
    assert o.shape == (len(s), P.count_params(prm))
    g = R.flatten({k: v[None] for k, v in A.gradient("gru", prm, s, e).items()})[0]
    mine = 2.0 * (R.epsilon(e)[:, None] * o).mean(axis=0)
    assert np.abs(mine - g).max() <= 1e-12 * np.abs(g).max()
    assert np.abs(2.0 * R.force(o, e) - g).max() <= 1e-12 * np.abs(g).max()


def test_jacobian_row_is_half_the_gradient_of_one_log_probability(case):
    prm, s, e, o = case
    leaves = A.to_torch(prm, torch.float64, requires_grad=True)
    A.prnn_log_probability(leaves, s[3:4])[0].backward()
    row = np.concatenate([0.5 * leaves[k].grad.numpy().ravel() for k in R.names(prm)])
    assert np.abs(row - o[3]).max() <= 1e-14 * np.abs(row).max()


def test_push_through_identity(case):
    prm, s, e, o = case
    for lam in (1e-3, 1e-1):
        a, b = R.minsr_direction(o, e, lam), R.sr_direction(o, e, lam)
        assert np.linalg.norm(a - b) <= 1e-9 / lam * 1e-3 * np.linalg.norm(b)      # (S + lam)^-1 amplifies rounding by <= |S| / lam


def test_centred_gram_rows_and_columns_sum_to_zero(case):
    o = case[3]
    g = R.gram(o)
    assert np.array_equal(g, g.T)
    scale = np.abs(g).sum(axis=1).max()
    assert np.abs(g.sum(axis=0)).max() <= 1e-13 * scale and np.abs(g.sum(axis=1)).max() <= 1e-13 * scale


def test_flatten_round_trip(case):
    prm, s, e, o = case
    d = R.unflatten(o, prm)
    assert all(d[k].shape == (len(s),) + prm[k].shape for k in prm)
    assert np.array_equal(R.flatten(d), o)


# ---- host side of sr.py: no device ------------------------------------------------------------------------------------------

def test_solve_shifted_is_the_cholesky_solution(case):
    prm, s, e, o = case
    g, eps = R.gram(o), R.epsilon(e)
    y = sr.solve_shifted(g, eps, 1e-3)
    assert np.abs((g + len(eps) * 1e-3 * np.eye(len(eps))) @ y - eps).max() <= 1e-10 * np.abs(eps).max()
    assert np.linalg.norm(R.centred(o).T @ y - R.minsr_direction(o, e, 1e-3)) <= 1e-10 * np.linalg.norm(R.minsr_direction(o, e, 1e-3))


class _Fake:
    """what sr.py needs of a NativeWavefunction, computed from the reference Jacobian: no device"""

    def __init__(self, prm, o, e):
        self.N, self.o, self.e, self.prm = 6, o, e, prm

    def _layout(self):
        return [(k[len(A.SCOPE) + 1:], int(self.prm[k].size)) for k in R.names(self.prm)]

    def log_derivatives(self):
        return self.o

    def sr_gram(self):
        return R.gram(self.o), R.epsilon(self.e)

    def sr_apply(self, y):
        return R.centred(self.o).T @ y


def test_minsr_direction_and_qgt_through_the_facade(case):
    prm, s, e, o = case
    wf = _Fake(prm, o, e)
    ref = R.minsr_direction(o, e, 1e-2)
    assert np.linalg.norm(sr.minsr_direction(wf, 1e-2) - ref) <= 1e-10 * np.linalg.norm(ref)
    assert np.allclose(sr.qgt(wf), R.qgt(o), rtol=0, atol=1e-15 * np.abs(R.qgt(o)).max())
    flat = sr.flatten_params(wf, prm)
    back = sr.unflatten_params(wf, flat, prm)
    assert all(np.array_equal(back[k], prm[k]) and back[k].dtype == prm[k].dtype for k in prm)


def test_host_side_argument_refusals(case):
    prm, s, e, o = case
    wf = _Fake(prm, o, e)
    for bad in (0.0, -1e-3, np.inf, np.nan):
        with pytest.raises(ValueError, match="diag_shift"):
            sr.minsr_direction(wf, bad)
        with pytest.raises(ValueError, match="diag_shift"):
            sr.train_tfim(wf, np.ones(6), 1.0, prm, 1, 10, 1e-2, bad, 1)
    with pytest.raises(ValueError, match="gram must be"):
        sr.solve_shifted(np.eye(3), np.ones(4), 1e-3)
    with pytest.raises(ValueError, match="Jz must have"):
        sr.train_tfim(wf, np.ones(5), 1.0, prm, 1, 10, 1e-2, 1e-3, 1)
    with pytest.raises(ValueError, match="numsamples"):
        sr.train_tfim(wf, np.ones(6), 1.0, prm, 1, 1, 1e-2, 1e-3, 1)


def test_header_binding_and_build_list_agree():
    from rnnwavefunctions_amd import _lib, build
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rnnwf.h")).read(), flags=re.S)
    for name, nargs in (("rnnwf_log_derivatives", 4), ("rnnwf_sr_gram", 3), ("rnnwf_sr_apply", 3), ("rnnwf_resident_samples", 1)):
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, header)
        assert m and len(m.group(1).split(",")) == nargs == len(_lib.PROTOTYPES[name][1]), name
    assert "sr.hip" in build.SOURCES and build.compile_flags("sr.hip") == build.compile_flags("grad.hip")
    for m in ("log_derivatives", "sr_gram", "sr_apply", "set_params_flat", "resident_samples"):
        assert callable(getattr(_lib.NativeWavefunction, m))
