"""torch-CPU float64 restatement of the LSTM wave function's FORWARD (tests/lstm_reference.py's arithmetic: tf.nn.rnn_cell.LSTMCell
with TF 1.x defaults, forget_bias 1, then Dense(2) + softmax over the raster path), so that one reverse-mode pass gives every element
of   d/dtheta sum_s w_s log P(s)   exactly: the yardstick of tests/test_gpu_lstm_grad.py.  TEST INFRASTRUCTURE ONLY.

Written from tests/lstm_reference.py, not from the HIP code.  The bound (judge) is the float64 families' of
tests/test_gpu_gradient_classes.py: autograd_reference.verdict with unit_roundoff_ratio 2^-29, FACTOR 16 and the rounding floor of
tests/gradient_classes_reference.py (N x 2^-53 x max_k sum_s |w_s d log P_s / d theta_k| / max |g_ref|); no other constant.

lstm_log_probability takes switches that make it deliberately WRONG, for tests/test_lstm_grad_reference.py to show what the bound
rejects; nothing else uses them.
"""
import collections
import time

import numpy as np
import torch

import autograd_reference as A
import lstm_reference as LR
from rnnwavefunctions_amd import params as P

SCOPE = A.SCOPE
LSTM = LR.LSTM
NS = 40                    # two full 16-chain blocks and a ragged one of 8
# every NFULL (<= 20, 36, 52, 68 units), full tiles (16), a full and a partial mixed tile (20, 36, 52, 68 / 17, 21, 33, 37, 53)
WIDTHS = (10, 16, 17, 20, 21, 33, 36, 37, 50, 52, 53, 67, 68)
LATTICES = ((11, 3), (17, 2), (7, 5), (2, 1))      # 33 to 35 sites: the spin-word boundary is crossed; 2 x 1: a single checkpoint
SHARP = 3.0
# one to five spin words: where lstm_bwd_kernel's word walk (wcur, wlow, spin_in) swaps, refetches and hands a spin over
BIG_LATTICES = (
    (8, 4),       # 32 sites: one full word; wlow never loaded
    (16, 4),      # 64 sites: two full words; the swap at 32, no refetch
    (13, 5),      # 65 sites: one site in the third word; the refetch at n = 64 reads word 0
    (12, 8),      # 96 sites: three full words
    (10, 10),     # 100 sites: the benchmarked size
    (12, 12),     # 144 sites: five words; refetches at 128, 96 and 64
)
BIG_NFULL_LATTICES = ((13, 5), (10, 10), (12, 12))       # each of these also at one width of every NFULL
BIG_NFULL_WIDTHS = (20, 36, 52, 68)
# (lattice, units): sharp where it is not SHARP.  17 units with kernels x 3 is nearly polarised (float64 sampler, 400 draws: 92 to 98 %
# ones at sites 31 and 63 on 13 x 5 and 10 x 10, 90 % at x 2, 84 % at x 1.5), so 40 rows would often hold one spin value at a word
# boundary; with the kernels as initialised it is 70 to 75 %.  No other case is above 87 % at either site.  13 x 5 / 17 is a GPU case
# (big_cases), 10 x 10 / 17 the second fixture of tests/test_lstm_grad_reference.py.
BIG_SHARP = {((13, 5), 17): 1.0, ((10, 10), 17): 1.0}
WIDE = dict(shape=(10, 10), ns=1000, configs=NS, widths=(21, 50, 68))      # 62 full blocks and a ragged one of 8


def big_cases():
    """[(lattice, units)]: every width on BIG_LATTICES in rotation, then BIG_NFULL_WIDTHS on each of BIG_NFULL_LATTICES"""
    return [(BIG_LATTICES[k % len(BIG_LATTICES)], u) for k, u in enumerate(WIDTHS)] + \
           [(s, u) for s in BIG_NFULL_LATTICES for u in BIG_NFULL_WIDTHS]


def big_sharp(shape, units):
    return BIG_SHARP.get((tuple(shape), units), SHARP)


def word_boundaries_mixed(samples, w):
    """both spin values at site 63, and at site 31 where the lattice has them, among the rows with non-zero weight: the spins the word
    walk hands over from bit 31 of the word below"""
    s = np.asarray(samples).reshape(len(samples), -1)[np.asarray(w) != 0.0]
    return all(len(np.unique(s[:, n])) == 2 for n in (31, 63) if n < s.shape[1])


def wide_batch(configs, ns):
    """(ns, N) rows repeating the distinct configurations, and the index of each row's configuration: row r holds configuration
    (7 r + 3 (r // 16)) mod m, so the 16 rows of a block differ from one another and the blocks from their neighbours"""
    c = np.asarray(configs).reshape(len(configs), -1)
    m = len(c)
    assert m >= 16 and m % 7 and len(np.unique(c, axis=0)) == m
    r = np.arange(ns)
    idx = (7 * r + 3 * (r // 16)) % m
    for b in range(0, ns, 16):
        assert len(set(idx[b:b + 16])) == len(idx[b:b + 16])
    return np.ascontiguousarray(c[idx]), idx


def nfull(units):
    return next(nf for nf in (1, 2, 3, 4) if 16 * nf + 4 >= units)


def parameters(units, seed=111, sharp=SHARP):
    """kernels x sharp and every bias randomised, as gradient_classes_reference.parameters"""
    return P.randomize_biases(P.scale_kernels(P.init_lstm_params([units], seed=seed), sharp), seed + 1)


def weights(ns, seed=7):
    """one weight per sample with both signs and exact zeros (the first chain of the second block, the one before the last)"""
    w = np.random.RandomState(seed).standard_normal(ns) / ns
    w[min(16, ns - 1)] = 0.0
    if ns > 2:
        w[ns - 2] = 0.0
    return w


def lstm_log_probability(params, samples, scope=SCOPE, inputs=None, site_weight=None, forget_bias=1.0, carry_without_f=False):
    """float64 (B,).  inputs / site_weight: as autograd_reference.prnn_log_probability.  forget_bias: what is added to f before its
    sigmoid.  carry_without_f: the path c -> c' differentiates as 1 instead of sigmoid(f + 1) (values unchanged)."""
    s = torch.as_tensor(np.ascontiguousarray(samples), dtype=torch.int64).reshape(len(samples), -1)
    fed = s if inputs is None else torch.as_tensor(np.ascontiguousarray(inputs), dtype=torch.int64).reshape(len(samples), -1)
    B, N = s.shape
    K, b = params[scope + "/" + LSTM + "kernel"], params[scope + "/" + LSTM + "bias"]
    Wd, bd = params[scope + "/wf_dense/kernel"], params[scope + "/wf_dense/bias"]
    dtype = K.dtype
    H = b.shape[0] // 4
    x = torch.zeros((B, 2), dtype=dtype)
    c = torch.zeros((B, H), dtype=dtype)
    h = torch.zeros((B, H), dtype=dtype)
    lp = torch.zeros(B, dtype=torch.float64)
    eye = torch.eye(2, dtype=dtype)
    for n in range(N):
        z = torch.cat([x, h], dim=1) @ K + b
        i, j, f, o = z[:, :H], z[:, H:2 * H], z[:, 2 * H:3 * H], z[:, 3 * H:]
        fg = torch.sigmoid(f + forget_bias)
        kept = fg * c.detach() + (c - c.detach()) if carry_without_f else fg * c
        c = kept + torch.sigmoid(i) * torch.tanh(j)
        h = torch.sigmoid(o) * torch.tanh(c)
        term = torch.log_softmax((h @ Wd + bd).to(torch.float64), dim=1).gather(1, s[:, n:n + 1])[:, 0]
        lp = lp + (term if site_weight is None else site_weight[n] * term)
        x = eye[fed[:, n]]
    return lp


def gradient(params, samples, w, dtype=torch.float64, **kw):
    """{scoped tf name: float64 ndarray}: d/dtheta sum_s w_s log P(s), every element, from one backward()"""
    leaves = A.to_torch(params, dtype, requires_grad=True)
    (lstm_log_probability(leaves, samples, **kw) * torch.as_tensor(np.asarray(w, dtype=np.float64))).sum().backward()
    return {k: v.grad.detach().to(torch.float64).numpy().reshape(np.shape(params[k])) for k, v in leaves.items()}


def per_sample_terms(params, samples, w):
    """{name: (ns,) + shape float64}: w_s d log P_s / d tensor (gradient_classes_reference.per_sample_gradients)"""
    leaves = A.to_torch(params, torch.float64, requires_grad=True)
    L = lstm_log_probability(leaves, samples) * torch.as_tensor(np.asarray(w, dtype=np.float64))
    order = sorted(leaves)
    g = torch.autograd.grad(L, [leaves[k] for k in order], grad_outputs=torch.eye(len(L), dtype=L.dtype), is_grads_batched=True)
    return {k: v.detach().numpy().reshape((len(L),) + np.shape(params[k])) for k, v in zip(order, g)}


def abs_term_sums(params, samples, w):
    """{name: sum_s |w_s d log P_s / d tensor|} for a long batch on a small lattice, whose terms do not fit at once: d log P_s depends
    on the configuration alone, so the derivatives are taken once per distinct configuration and weighted with its sum of |w_s|"""
    s = np.asarray(samples).reshape(len(samples), -1)
    configs, inverse = np.unique(s, axis=0, return_inverse=True)
    mass = np.bincount(np.ravel(inverse), weights=np.abs(np.asarray(w, dtype=np.float64)), minlength=len(configs))
    t = per_sample_terms(params, configs, np.ones(len(configs)))
    return {k: np.tensordot(mass, np.abs(v), axes=(0, 0)) for k, v in t.items()}


Reference = collections.namedtuple("Reference", "g64 g32 terms floor seconds")


def rounding_floor(N, abs_sums, g64):
    """gradient_classes_reference.rounding_floor for a float64 family, from the terms' absolute sums over the samples"""
    out = {}
    for k, t in abs_sums.items():
        ref_max = np.abs(g64[k]).max()
        out[k] = N * 2.0 ** -53 * t.max() / ref_max if ref_max > 0 else 0.0
    return out


def reference(params, samples, w, keep_terms=True):
    """float64 and float32 autograd gradients, the float64 per-sample terms (keep_terms) and the floor they give"""
    t0 = time.time()
    N = int(np.prod(np.shape(samples)[1:]))
    g64 = gradient(params, samples, w, dtype=torch.float64)
    g32 = gradient(params, samples, w, dtype=torch.float32)
    terms = per_sample_terms(params, samples, w) if keep_terms else None
    sums = {k: np.abs(t).sum(axis=0) for k, t in terms.items()} if keep_terms else abs_term_sums(params, samples, w)
    return Reference(g64, g32, terms, rounding_floor(N, sums, g64), time.time() - t0)


def judge(label, grads, ref, echo=print):
    """(worst deviation / bound, failures) under the float64 families' bound"""
    return A.verdict(grads, ref.g64, ref.g32, unit_roundoff_ratio=A.F64_OVER_F32, factor=A.FACTOR, label=label, floor=ref.floor, echo=echo)


def unscoped(grads, scope=SCOPE):
    return {k[len(scope) + 1:]: v for k, v in grads.items()}


def scoped(grads, scope=SCOPE):
    return {scope + "/" + k: v for k, v in grads.items()}


def shapes(params, scope=SCOPE):
    return {k[len(scope) + 1:]: v.shape for k, v in params.items()}
