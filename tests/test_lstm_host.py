"""Host-side tests of the LSTM wave function (model LSTM1D_F64): parameter initialisation, the TF sentinels of compat, the C
header, and exact identities that pin the NumPy restatement (tests/lstm_reference.py) the GPU tests compare against."""
import itertools
import os
import re

import numpy as np
import pytest

from conftest import ROOT, all_configs
from lstm_reference import LSTM, lstm_log_probability, lstm_sample
from oracle import philox
from rnnwavefunctions_amd import compat as tf
from rnnwavefunctions_amd import params as P

SCOPE = "RNNwavefunction"


@pytest.mark.parametrize("H,count", [(10, 542), (50, 10702)])
def test_init_lstm_params_names_shapes_and_count(H, count):
    p = P.init_lstm_params([H], seed=111)
    assert list(p) == [SCOPE + "/" + P.LSTM_PREFIX + "kernel", SCOPE + "/" + P.LSTM_PREFIX + "bias",
                       SCOPE + "/wf_dense/kernel", SCOPE + "/wf_dense/bias"]
    assert P.LSTM_PREFIX == LSTM == "multi_rnn_cell/cell_0/lstm_cell/"
    assert p[SCOPE + "/" + LSTM + "kernel"].shape == (2 + H, 4 * H)
    assert p[SCOPE + "/" + LSTM + "bias"].shape == (4 * H,)
    assert p[SCOPE + "/wf_dense/kernel"].shape == (H, 2)
    assert all(v.dtype == np.float64 for v in p.values())
    assert not p[SCOPE + "/" + LSTM + "bias"].any() and not p[SCOPE + "/wf_dense/bias"].any()
    assert P.count_params(p) == count
    k = p[SCOPE + "/" + LSTM + "kernel"]
    lim = np.sqrt(6.0 / (2 + H + 4 * H))                    # glorot: fan_in 2 + H, fan_out 4H
    assert np.abs(k).max() <= lim and np.abs(k).max() > 0.9 * lim


def test_init_lstm_params_is_deterministic_and_draws_in_tensor_order():
    a, b = P.init_lstm_params([7], seed=5), P.init_lstm_params([7], seed=5)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    assert not np.array_equal(a[SCOPE + "/" + LSTM + "kernel"], P.init_lstm_params([7], seed=6)[SCOPE + "/" + LSTM + "kernel"])
    rng = np.random.RandomState(5)
    lk = np.sqrt(6.0 / (9 + 28))
    assert np.array_equal(a[SCOPE + "/" + LSTM + "kernel"], rng.uniform(-lk, lk, size=(9, 28)))
    ld = np.sqrt(6.0 / (7 + 2))
    assert np.array_equal(a[SCOPE + "/wf_dense/kernel"], rng.uniform(-ld, ld, size=(7, 2)))
    c = P.init_lstm_params([7], seed=5, scope="other")
    assert all(k.startswith("other/") for k in c)


def test_init_lstm_params_refuses_stacked_layers():
    with pytest.raises(ValueError, match="one layer"):
        P.init_lstm_params([10, 10])


def test_compat_lstm_sentinels():
    assert tf.contrib.rnn.LSTMCell is tf.LSTMCell
    assert tf.nn.rnn_cell.LSTMCell is tf.LSTMCell
    assert callable(tf.nn.relu)
    assert tf.is_lstm_cell(tf.contrib.rnn.LSTMCell) and tf.is_lstm_cell(tf.nn.rnn_cell.LSTMCell)
    assert tf.is_lstm_cell(tf.LSTMCell(10)) and tf.is_lstm_cell("LSTMCell")
    assert not tf.is_lstm_cell(None) and not tf.is_lstm_cell(tf.contrib.cudnn_rnn.CudnnCompatibleGRUCell)
    assert not tf.is_lstm_cell("CudnnCompatibleGRUCell")
    assert not tf.is_gru_cell(tf.contrib.rnn.LSTMCell) and not tf.is_gru_cell("LSTMCell")
    assert tf.is_gru_cell(None)


def test_header_declares_the_lstm_model():
    with open(os.path.join(ROOT, "include", "rnnwf.h")) as f:
        h = f.read()
    assert re.search(r"RNNWF_MODEL_LSTM1D_F64\s*=\s*5\b", h)
    assert re.search(r"#define RNNWF_ABI_VERSION 1\b", h)
    from rnnwavefunctions_amd import _lib
    assert _lib.MODEL_LSTM1D_F64 == 5 and _lib.ABI_VERSION == 1


def _trained_like(H, seed):
    return P.randomize_biases(P.scale_kernels(P.init_lstm_params([H], seed=seed), 1.8), seed + 1)


def test_reference_is_normalised_on_3x3():
    prm = _trained_like(6, 3)
    lp = lstm_log_probability(prm, all_configs(9), 3, 3)
    assert abs(np.exp(lp).sum() - 1.0) < 1e-13


def test_reference_zero_weights_give_the_uniform_distribution():
    prm = {k: np.zeros_like(v) for k, v in P.init_lstm_params([5], seed=1).items()}
    s = all_configs(6)
    assert np.allclose(lstm_log_probability(prm, s, 2, 3), -6 * np.log(2.0), rtol=0, atol=1e-15)


def test_reference_zero_kernel_matches_the_constant_recursion():
    """K = 0: the gates see the bias only, c_n = s(b_f + 1) c_{n-1} + s(b_i) tanh(b_j), h_n = s(b_o) tanh(c_n), identical
    for every configuration; log P = sum_n log softmax(h_n Wd + bd)[s_n]."""
    H, Nx, Ny = 4, 2, 3
    rng = np.random.RandomState(7)
    prm = P.init_lstm_params([H], seed=2)
    prm[SCOPE + "/" + LSTM + "kernel"][:] = 0.0
    prm[SCOPE + "/" + LSTM + "bias"][:] = rng.standard_normal(4 * H)
    prm[SCOPE + "/wf_dense/bias"][:] = rng.standard_normal(2)
    b = prm[SCOPE + "/" + LSTM + "bias"]
    sig = lambda x: 1.0 / (1.0 + np.exp(-x))                       # noqa: E731
    c = np.zeros(H)
    z = []
    for _ in range(Nx * Ny):
        c = sig(b[2 * H:3 * H] + 1.0) * c + sig(b[:H]) * np.tanh(b[H:2 * H])
        h = sig(b[3 * H:]) * np.tanh(c)
        z.append(h @ prm[SCOPE + "/wf_dense/kernel"] + prm[SCOPE + "/wf_dense/bias"])
    z = np.array(z)
    ls = z - np.log(np.exp(z).sum(axis=1, keepdims=True))
    s = all_configs(Nx * Ny)
    want = ls[np.arange(Nx * Ny)[None, :], s].sum(axis=1)
    assert np.allclose(lstm_log_probability(prm, s, Nx, Ny), want, rtol=0, atol=1e-13)


def test_reference_sampler_agrees_with_its_log_probability():
    prm = _trained_like(8, 4)
    u = philox.uniforms(111, 0, 0, 200, 12)
    s, lp, p0 = lstm_sample(prm, 3, 4, u)
    assert np.allclose(lp, lstm_log_probability(prm, s, 3, 4), rtol=0, atol=1e-12)
    assert set(np.unique(s)) <= {0, 1} and p0.shape == (200, 12)
    # the draws follow u < p0 -> spin 0 away from ties
    clear = np.abs(u - p0) > 1e-12
    assert np.array_equal((s == 0)[clear], (u < p0)[clear])


def test_reference_matches_a_site_by_site_enumeration_on_2x2():
    """Chain rule: P(s) from the reference equals the product of its own conditionals obtained by summing P over the
    later sites (enumeration over 2^4 configurations)."""
    prm = _trained_like(3, 9)
    allc = all_configs(4)
    P_all = np.exp(lstm_log_probability(prm, allc, 2, 2))
    for s in itertools.islice(allc, 0, 16, 5):
        prob = 1.0
        for n in range(4):
            pre = (allc[:, :n] == s[:n]).all(axis=1)
            prob *= P_all[pre & (allc[:, n] == s[n])].sum() / P_all[pre].sum()
        assert abs(prob - P_all[(allc == s).all(axis=1)][0]) < 1e-13
