"""NumPy float64 restatement of the LSTM wave function over the raster path (the default cell of
2DTFIM_1DRNN/RNNwavefunction.py:9,37: tf.nn.rnn_cell.LSTMCell with TF 1.x defaults - forget_bias 1.0, tanh, no
peepholes, no projection, no clipping - followed by Dense(2) + softmax), the yardstick of tests/test_gpu_lstm.py.

One step:  z = [x, h] K + b;  i, j, f, o = split(z, 4);  c' = sigmoid(f + 1) c + sigmoid(i) tanh(j);  h' = sigmoid(o) tanh(c').
The state starts at (c, h) = (0, 0), x = 0 at the first site and the one-hot of the previous spin afterwards; the sites
are visited in raster order n = ny * Nx + nx (:74-80, :118-123), i.e. along the flat index of a (ns, Nx * Ny) sample.
"""
import numpy as np

from oracle import models as M

LSTM = "multi_rnn_cell/cell_0/lstm_cell/"


def _get(params, scope, name):
    return np.asarray(params[scope + "/" + name] if scope + "/" + name in params else params[name], dtype=np.float64)


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def lstm_step(x, c, h, K, b):
    """One LSTMCell step on a batch: returns (c', h')."""
    H = h.shape[1]
    z = np.concatenate([x, h], axis=1) @ K + b
    i, j, f, o = z[:, :H], z[:, H:2 * H], z[:, 2 * H:3 * H], z[:, 3 * H:]
    c = _sigmoid(f + 1.0) * c + _sigmoid(i) * np.tanh(j)
    return c, _sigmoid(o) * np.tanh(c)


def _unpack(params, scope):
    return (_get(params, scope, LSTM + "kernel"), _get(params, scope, LSTM + "bias"),
            _get(params, scope, "wf_dense/kernel"), _get(params, scope, "wf_dense/bias"))


def _log_softmax(z):
    m = z.max(axis=1, keepdims=True)
    return z - m - np.log(np.exp(z - m).sum(axis=1, keepdims=True))


def lstm_log_probability(params, samples, Nx, Ny, scope="RNNwavefunction"):
    """log P of (B, Nx * Ny) configurations (2DTFIM_1DRNN/RNNwavefunction.py:84-130), float64 (B,)."""
    K, b, Wd, bd = _unpack(params, scope)
    s = np.asarray(samples).reshape(len(samples), -1).astype(np.int64)
    B, N = s.shape
    assert N == Nx * Ny
    H = b.size // 4
    x = np.zeros((B, 2))
    c = np.zeros((B, H))
    h = np.zeros((B, H))
    lp = np.zeros(B)
    for n in range(N):
        c, h = lstm_step(x, c, h, K, b)
        lp += _log_softmax(h @ Wd + bd)[np.arange(B), s[:, n]]
        x = np.eye(2)[s[:, n]]
    return lp


def lstm_site_probs(params, samples, Nx, Ny, scope="RNNwavefunction", dtype=np.float64):
    """Teacher-forced conditional of spin 0 at every site of (B, Nx * Ny) configurations, (B, N) in the arithmetic `dtype`
    (float64: the restatement above; float32: the same formulas on parameters rounded to float32 - the yardstick of the
    sampler check's near-tie band, tests/sampler_reference.py).  p0 = exp(log_softmax(h Wd + bd))[:, 0], as lstm_sample records it."""
    dt = np.dtype(dtype).type
    K, b, Wd, bd = (a.astype(dt) for a in _unpack(params, scope))
    s = np.asarray(samples).reshape(len(samples), -1).astype(np.int64)
    B, N = s.shape
    assert N == Nx * Ny
    H = b.size // 4
    eye = np.eye(2, dtype=dt)
    x = np.zeros((B, 2), dtype=dt)
    c = np.zeros((B, H), dtype=dt)
    h = np.zeros((B, H), dtype=dt)
    p0 = np.empty((B, N), dtype=dt)
    for n in range(N):
        z = np.concatenate([x, h], axis=1) @ K + b
        i, j, f, o = z[:, :H], z[:, H:2 * H], z[:, 2 * H:3 * H], z[:, 3 * H:]
        one = dt(1)
        c = (one / (one + np.exp(-(f + one)))) * c + (one / (one + np.exp(-i))) * np.tanh(j)
        h = (one / (one + np.exp(-o))) * np.tanh(c)
        p0[:, n] = np.exp(_log_softmax(h @ Wd + bd)[:, 0])
        x = eye[s[:, n]]
    return p0


def lstm_sample(params, Nx, Ny, u, scope="RNNwavefunction"):
    """Ancestral sampling (:35-82) with explicit uniforms u (ns, Nx * Ny) - oracle.philox.uniforms, the stream of the
    native sampler - and tf.multinomial's decision rule (oracle.models.multinomial_2).  Returns (samples int64,
    log P float64, p0 (ns, N): the probability of spin 0 at every drawn site, for near-tie accounting)."""
    K, b, Wd, bd = _unpack(params, scope)
    ns, N = u.shape
    assert N == Nx * Ny
    H = b.size // 4
    x = np.zeros((ns, 2))
    c = np.zeros((ns, H))
    h = np.zeros((ns, H))
    samples = np.empty((ns, N), dtype=np.int64)
    lp = np.zeros(ns)
    p0 = np.empty((ns, N))
    for n in range(N):
        c, h = lstm_step(x, c, h, K, b)
        ls = _log_softmax(h @ Wd + bd)
        s = M.multinomial_2(ls, u[:, n])
        samples[:, n] = s
        p0[:, n] = np.exp(ls[:, 0])
        lp += ls[np.arange(ns), s]
        x = np.eye(2)[s]
    return samples, lp, p0
