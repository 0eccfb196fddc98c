"""CPU tests of the LSTM wave function's stochastic-reconfiguration yardstick (tests/lstm_sr_reference.py): what it computes, and
what the Jacobian bound of tests/test_gpu_lstm_sr.py rejects and accepts.  3 x 2 lattice, 7 units, 37 samples (two 16-chain blocks
and a ragged one)."""
import numpy as np
import pytest
import torch

import lstm_grad_reference as G
import lstm_sr_reference as R
from rnnwavefunctions_amd import params as P

EPS64 = 2.0 ** -53
SCOPE = G.SCOPE


@pytest.fixture(scope="module")
def case():
    nx, ny, H, ns = 3, 2, 7, 37
    rng = np.random.RandomState(5)
    prm = {k: np.asarray(v, dtype=np.float64) for k, v in G.parameters(H, seed=3).items()}
    s = rng.randint(0, 2, size=(ns, nx, ny)).astype(np.int32)
    e = rng.standard_normal(ns) * 2.0 - 3.0
    return prm, s, e, R.jacobian(prm, s)


def jacobian_bound_ratio(O, ref, N):
    """tests/test_gpu_lstm_sr.py: check_jacobian's figure - the worst row error over the row's largest element, over 1e-10 N"""
    return (np.abs(O - ref).max(axis=1) / np.abs(ref).max(axis=1)).max() / (1e-10 * N)


def test_weighted_sum_is_the_gradient(case):
    """sum_s 2 w_s O_s is lstm_grad_reference.gradient for the weights w; with w_s = (E_s - mean E) / ns it is 2 F"""
    prm, s, e, o = case
    assert o.shape == (len(s), P.count_params(prm)) and np.abs(o).max() > 0
    w = (e - e.mean()) / len(s)
    g = R.flatten({k: v[None] for k, v in G.gradient(prm, s, w).items()})[0]
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


def test_bound_rejects_head_rows_summed_over_a_block(case):
    """what the backward kernel's weighted mode does with the head row - one sum over the 16 chains of a wave - in place of the
    chain's own row: the tensors of wf_dense of every sample replaced by their sum over the sample's 16-chain block"""
    prm, s, e, o = case
    jd = R.unflatten(o, prm)
    bad = {k: v.copy() for k, v in jd.items()}
    for k in bad:
        if "wf_dense" in k:
            for b0 in range(0, len(s), 16):
                bad[k][b0:b0 + 16] = jd[k][b0:b0 + 16].sum(axis=0, keepdims=True)
    ratio = jacobian_bound_ratio(R.flatten(bad), o, s.shape[1] * s.shape[2])
    print("head rows summed per block: error / bound %.3e" % ratio)
    assert ratio > 1e6


def test_bound_rejects_a_missing_forget_bias(case):
    prm, s, e, o = case
    ratio = jacobian_bound_ratio(R.jacobian(prm, s, forget_bias=0.0), o, s.shape[1] * s.shape[2])
    print("forget_bias = 0: error / bound %.3e" % ratio)
    assert ratio > 1e6


def test_bound_accepts_another_summation_order_over_sites(case):
    """log P is a sum over sites, and so is O: the per-site Jacobians (site_weight = a unit vector) added from the last site to the
    first, the order of the backward kernel's walk, against the one reverse pass over the whole sum"""
    prm, s, e, o = case
    N = s.shape[1] * s.shape[2]
    total = np.zeros_like(o)
    for n in reversed(range(N)):
        total = total + R.jacobian(prm, s, site_weight=torch.eye(N, dtype=torch.float64)[n])
    ratio = jacobian_bound_ratio(total, o, N)
    print("sites summed in reverse: error / bound %.3e" % ratio)
    assert ratio <= 1.0
