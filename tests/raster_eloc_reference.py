"""Float64 reference, bounds and defect models of the raster-lattice local-energy (flip) pass.  TEST INFRASTRUCTURE ONLY.

The two float64 models on the 2D raster path - the GRU (MODEL_GRU1D_F64, one layer or a stack) and the LSTM (MODEL_LSTM1D_F64) -
return the whole log-probability queue from tfim_eloc(..., log_probs=lp): row 0 is log P(s), row k + 1 is log P(s with flat site k
flipped).  `reference` scores that queue from site 0 in float64 (oracle.estimators.ising2d_local_energies on the oracle's
log-probability of the family); `judge` compares a queue and its energies with it under three bounds, none taken from a kernel:

  rows   |lp - lp_ref| <= 1e-11 N on every entry          the log P tolerance of test_gpu_lstm.py / test_gpu_prnn.py for these models
  row 0  equals wf.log_prob(s) bit for bit                the same base kernel (docs/lstm.md; the f64 GRU likewise)
  E_loc  |e - e_ref| <= Bx sum_k r_k 1e-11 N + 1e-13 (|diag| + Bx sum_k r_k),   r_k = exp((lp_ref[k + 1] - lp_ref[0]) / 2)
         first term: what the row bound lets through (exp(D / 2) has relative error |dD| / 2, |dD| <= 2e-11 N); second: a few
         float64 roundings of the sum.  r_k comes from the reference alone.

and asserts that the weights are sharp: the ratios r_k of the batch spread, r.std() > 0.2 r.mean() (test_gpu_sharpened.check_tfim asks
the same of its ratio sums; glorot weights give r_k ~ 1 throughout).

`queue_rows` evaluates the same queue a second way - one pass over the sites that shares every flipped chain's prefix with the
unflipped chain, as the kernels do - in any NumPy float type.  In numpy.longdouble (64-bit mantissa on x86) it is the yardstick
that shows the float64 reference's own error (test_raster_eloc_reference.py); in float64 with a knob turned it is a defect model.
The cells are restated here from the formulas (oracle/models.py: gru_cell; tests/lstm_reference.py: lstm_step), not called.
"""
import time

import numpy as np

import lstm_reference as L
import sampler_reference as R
from oracle import estimators as E
from oracle import models as M

SCOPE = R.SCOPE
BX = 3.0
ROW_TOL = 1e-11                    # per site, on every queue entry
SUM_TOL = 1e-13                    # a few float64 roundings, relative to |diag| + Bx sum_k r_k
CHAINS = 16                        # chains per block of both flip kernels
CUS = 256                          # compute units of the MI355X: sizes the grid-stride case where no device is asked

# id, family, units, Nx, Ny, samples (None: from the CU count, grid_stride_ns), kernel scale, what it is for.  Kernel scale 3
# (sampler_reference.build_params) everywhere: the longdouble yardstick stays below a tenth of the row bound at every case
# (test_raster_eloc_reference.py::test_float64_reference_against_longdouble lists the figures).
CASES = [
    ("lstm-20-8x4", "lstm", (20,), 8, 4, 33, 3.0, "N = 32: last site is bit 31, no second word"),
    ("lstm-10-3x11", "lstm", (10,), 3, 11, 37, 3.0, "N = 33: second word holds one spin; NFULL 1; ragged"),
    ("lstm-21-5x13", "lstm", (21,), 5, 13, 40, 3.0, "N = 65, 3 words; NFULL 2 with remainder 1"),
    ("lstm-36-8x8", "lstm", (36,), 8, 8, 48, 3.0, "N = 64: two full words; NFULL 2 full"),
    ("lstm-37-11x3", "lstm", (37,), 11, 3, 21, 3.0, "N = 33; NFULL 3; Nx > Ny"),
    ("lstm-50-10x10", "lstm", (50,), 10, 10, 64, 3.0, "N = 100, 4 words: the size docs/lstm.md times"),
    ("lstm-53-9x11", "lstm", (53,), 9, 11, 17, 3.0, "N = 99; NFULL 4; one block plus one lane"),
    ("lstm-68-12x12", "lstm", (68,), 12, 12, 48, 3.0, "N = 144, 5 words; widest image; 8-wave flip, 4-wave base pass"),
    ("lstm-50-5x13-stride", "lstm", (50,), 5, 13, None, 3.0, "more tiles than waves: the grid-stride loop"),
    ("gru64-20-3x11", "gru64", (20,), 3, 11, 37, 3.0, "NFULL 1"),
    ("gru64-36-5x13", "gru64", (36,), 5, 13, 40, 3.0, "NFULL 2"),
    ("gru64-50-10x10", "gru64", (50,), 10, 10, 64, 3.0, "NFULL 3"),
    ("gru64-68-9x7", "gru64", (68,), 9, 7, 33, 3.0, "N = 63: last site is bit 30; NFULL 4"),
    ("gru64-100-12x12", "gru64", (100,), 12, 12, 32, 3.0, "NFULL 6"),
    ("gru64-69-11x3", "gru64", (69,), 11, 3, 21, 3.0, "first width of NFULL 6"),
    ("gru64-20x2-5x13", "gru64", (20, 20), 5, 13, 40, 3.0, "stack, 2 layers"),
    ("gru64-50x2-12x12", "gru64", (50, 50), 12, 12, 32, 3.0, "stack at the gradient test's size"),
    ("gru64-36x3-3x11", "gru64", (36, 36, 36), 3, 11, 37, 3.0, "3 layers"),
    ("gru64-20x4-3x11", "gru64", (20, 20, 20, 20), 3, 11, 21, 3.0, "4 layers"),
]
CASE_IDS = [c[0] for c in CASES]


def case(cid):
    return CASES[CASE_IDS.index(cid)]


def grid_stride_ns(cus):
    """Chains of the grid-stride case: launch_shrinking starts at most 8 waves on each CU (one workgroup per CU from 37 units,
    docs/lstm.md), so 16 (8 cus // 64 + 2) chains give 64 (8 cus // 64 + 2) > 8 cus tiles on the 65-site lattice."""
    return CHAINS * (8 * cus // 64 + 2)


def couplings(Nx, Ny):
    """Random bonds, so that a transposed bond index shows."""
    return np.random.RandomState(Nx * Ny).uniform(0.5, 1.5, (Nx, Ny))


def log_prob_fn(family, prm, Nx, Ny):
    if family == "lstm":
        return lambda x: L.lstm_log_probability(prm, x, Nx, Ny)
    prm64 = R.cast(prm, np.float64)
    return lambda x: M.prnn_log_probability(prm64, x, dtype=np.float64)


def reference(family, prm, s, Jz, Bx, Nx, Ny, chunk=None):
    """(e_ref (ns,), lp_ref (N + 1, ns)): every chain of the queue scored from site 0 in float64.  chunk: rows per call of the
    log-probability (memory and BLAS blocking only)."""
    fn = log_prob_fn(family, prm, Nx, Ny)
    if chunk is not None:
        whole = fn
        fn = lambda x: np.concatenate([whole(x[k:k + chunk]) for k in range(0, len(x), chunk)])
    s = np.asarray(s).reshape(len(s), Nx * Ny)
    with np.errstate(over="ignore"):
        return E.ising2d_local_energies(Jz, Bx, Nx, Ny, s, fn, return_log_probs=True)


def diagonal(s, Jz, Nx, Ny):
    """-sum over bonds of Jz sz sz' on the C-order (Nx, Ny) reshape, bond (i, j)-(i + 1, j) with Jz[i, j] and (i, j)-(i, j + 1)
    with Jz[i, j] (2DTFIM_1DRNN/Training1DRNN_2DTFIM.py:27-49)."""
    sz = 2.0 * np.asarray(s).reshape(len(s), Nx, Ny) - 1.0
    Jz = np.asarray(Jz).reshape(Nx, Ny)
    return -((sz[:, :-1, :] * sz[:, 1:, :] * Jz[:-1, :]).sum(axis=(1, 2)) + (sz[:, :, :-1] * sz[:, :, 1:] * Jz[:, :-1]).sum(axis=(1, 2)))


def measure(lp, e, lp_ref, e_ref, s, Jz, Bx, Nx, Ny, log_prob=None):
    """The figures `judge` asserts on.  lp may be flat ((N + 1) ns,) as tfim_eloc fills it."""
    N = Nx * Ny
    ns = len(e_ref)
    lp = np.asarray(lp).reshape(N + 1, ns)
    with np.errstate(over="ignore"):
        r = np.exp(0.5 * (lp_ref[1:] - lp_ref[0]))
    rsum = r.sum(axis=0)
    diag = diagonal(s, Jz, Nx, Ny)
    row_err = np.abs(lp - lp_ref)
    e_err = np.abs(np.asarray(e) - e_ref)
    e_bound = Bx * rsum * ROW_TOL * N + SUM_TOL * (np.abs(diag) + Bx * rsum)
    wr = np.unravel_index(int(np.argmax(np.where(np.isfinite(row_err), row_err, np.inf))), row_err.shape)
    we = int(np.argmax(np.where(np.isfinite(e_err), e_err / e_bound, np.inf)))
    return dict(N=N, ns=ns, finite=bool(np.all(np.isfinite(lp)) and np.all(np.isfinite(e))),
                row_over=float(row_err[wr] / (ROW_TOL * N)), worst_row=(int(wr[0]), int(wr[1])), row_err=float(row_err[wr]),
                e_over=float(e_err[we] / e_bound[we]), worst_e=we, e_err=float(e_err[we]), e_bound=float(e_bound[we]),
                ratio_min=float(r.min()), ratio_max=float(r.max()), sharp=bool(r.std() > 0.2 * r.mean()),
                spread=float(r.std() / r.mean()),
                row0_equal=None if log_prob is None else bool(np.array_equal(lp[0], log_prob)))


def line(label, m, seconds=None):
    return ("%s N %d ns %d: max row error / bound %.3e (%.2e at row %d chain %d)  max E error / bound %.3e (%.2e of %.2e, chain %d)  "
            "ratios %.2e .. %.2e (std / mean %.2f)%s" %
            (label, m["N"], m["ns"], m["row_over"], m["row_err"], m["worst_row"][0], m["worst_row"][1], m["e_over"], m["e_err"],
             m["e_bound"], m["worst_e"], m["ratio_min"], m["ratio_max"], m["spread"],
             "" if seconds is None else "  reference %.1f s" % seconds))


def judge(lp, e, lp_ref, e_ref, s, Jz, Bx, Nx, Ny, log_prob=None, label=""):
    """Asserts the three bounds and the sharpness; log_prob: wf.log_prob(s) for the bit-for-bit comparison of row 0 (None: not
    asked, for queues that come from no device).  Returns the figures of `measure`."""
    m = measure(lp, e, lp_ref, e_ref, s, Jz, Bx, Nx, Ny, log_prob)
    assert m["finite"], "%s non-finite values" % label
    assert m["row_over"] <= 1.0, ("%s queue row %d (flipped site %d), chain %d (block %d): |lp - ref| = %.3e > %.3e" %
                                  (label, m["worst_row"][0], m["worst_row"][0] - 1, m["worst_row"][1], m["worst_row"][1] // CHAINS,
                                   m["row_err"], ROW_TOL * m["N"]))
    assert m["row0_equal"] is not False, "%s row 0 of the queue differs from log_prob(s)" % label
    assert m["e_over"] <= 1.0, "%s chain %d: |E - ref| = %.3e > %.3e" % (label, m["worst_e"], m["e_err"], m["e_bound"])
    assert m["sharp"], "%s the ratios do not spread (std / mean = %.3f): the weights are not sharp" % (label, m["spread"])
    return m


# ---- the queue evaluated with shared prefixes, in any float type ---------------------------------------------------------------------

def _sigmoid(x):
    one = x.dtype.type(1)
    return one / (one + np.exp(-x))


def _log_softmax(z):
    m = z.max(axis=1, keepdims=True)
    return z - m - np.log(np.exp(z - m).sum(axis=1, keepdims=True))


class _Cells:
    """step(x (B, 2), state) -> (state', log p (B, 2)); state: a list of (B, H) arrays ([c, h] for the LSTM, one h per GRU layer)."""

    def __init__(self, family, prm, dtype, scope=SCOPE):
        get = lambda name: np.asarray(prm[scope + "/" + name]).astype(dtype)
        self.dtype, self.lstm = dtype, family == "lstm"
        self.Wd, self.bd = get("wf_dense/kernel"), get("wf_dense/bias")
        if self.lstm:
            self.K, self.b = get(L.LSTM + "kernel"), get(L.LSTM + "bias")
            self.widths = [self.b.size // 4] * 2
        else:
            names = ("gates/kernel", "gates/bias", "candidate/input_projection/kernel", "candidate/input_projection/bias",
                     "candidate/hidden_projection/kernel", "candidate/hidden_projection/bias")
            self.layers = [[get(M.GRU % l + n) for n in names] for l in range(M.num_gru_layers(prm, scope))]
            self.widths = [w[4].shape[0] for w in self.layers]

    def step(self, x, state):
        one = self.dtype(1)
        if self.lstm:
            c, h = state
            H = h.shape[1]
            z = np.concatenate([x, h], axis=1) @ self.K + self.b
            c = _sigmoid(z[:, 2 * H:3 * H] + one) * c + _sigmoid(z[:, :H]) * np.tanh(z[:, H:2 * H])
            h = _sigmoid(z[:, 3 * H:]) * np.tanh(c)
            new = [c, h]
        else:
            new = []
            for (Wg, bg, Wci, bci, Wch, bch), h in zip(self.layers, state):
                H = h.shape[1]
                g = _sigmoid(np.concatenate([x, h], axis=1) @ Wg + bg)
                cand = np.tanh((x @ Wci + bci) + g[:, :H] * (h @ Wch + bch))
                x = (one - g[:, H:]) * cand + g[:, H:] * h
                new.append(x)
        return new, _log_softmax(new[-1] @ self.Wd + self.bd)


def queue_rows(family, prm, s, dtype=np.float64, checkpoint_shift=0, word0=False):
    """(lpq (N + 1, B), base (N, B), own (N, B)) in `dtype`: the log-probability queue of the (B, N) configurations, the flip base of
    every flipped chain (the terms of sites 0 .. k with site k flipped, before its continuation k + 1 .. N - 1 is added) and the
    unflipped chain's own terms of sites 0 .. k.  One pass over the
    sites: at site n the unflipped chains advance, the chains flipped at k < n advance with their own inputs, and the chain
    flipped at n starts from the unflipped state after site n with the flipped spin as its next input.

    The knobs turn it into a defect model (float64 only makes sense there):
      checkpoint_shift = 1  the continuation of flipped site k starts from the state after site k - 1 (zero state for k = 0)
      word0                 the flip pass reads the spin of site n >= 32 from word 0 of the packed spins, bit n & 31: site n - 32
                            up to 63 sites; the base pass (row 0 and every flip base) reads the right spins"""
    dt = np.dtype(dtype).type
    s = np.asarray(s).reshape(len(s), -1).astype(np.int64)
    B, N = s.shape
    cells = _Cells(family, prm, dt)
    eye = np.eye(2, dtype=dt)
    ar = np.arange(B)
    seen = s[:, np.arange(N) & 31] if word0 else s           # what the flip pass reads
    x = np.zeros((B, 2), dtype=dt)
    state = [np.zeros((B, w), dtype=dt) for w in cells.widths]
    fstate = [np.zeros((N, B, w), dtype=dt) for w in cells.widths]
    fx = np.zeros((N, B, 2), dtype=dt)
    flp = np.zeros((N, B), dtype=dt)
    base = np.zeros((N, B), dtype=dt)
    own = np.zeros((N, B), dtype=dt)
    prefix = np.zeros(B, dtype=dt)
    with np.errstate(over="ignore"):
        for n in range(N):
            before = state
            state, lg = cells.step(x, state)
            if n:
                new, flg = cells.step(fx[:n].reshape(n * B, 2), [f[:n].reshape(n * B, -1) for f in fstate])
                for f, v in zip(fstate, new):
                    f[:n] = v.reshape(n, B, -1)
                flp[:n] += flg.reshape(n, B, 2)[:, ar, seen[:, n]]
                fx[:n] = eye[seen[:, n]]
            base[n] = prefix + lg[ar, 1 - s[:, n]]
            flp[n] = base[n]
            for f, v in zip(fstate, before if checkpoint_shift else state):
                f[n] = v
            fx[n] = eye[1 - seen[:, n]]
            prefix = prefix + lg[ar, s[:, n]]
            own[n] = prefix
            x = eye[s[:, n]]
    return np.concatenate([prefix[None], flp]), base, own


def yardstick(family, prm, s):
    """The queue in numpy.longdouble."""
    return queue_rows(family, prm, s, np.longdouble)[0]


# ---- defect models: each returns a defective (lp, e) from the reference's, for test_raster_eloc_reference.py only ---------------------

def energies(lp, s, Jz, Bx, Nx, Ny):
    """E_loc assembled from a queue."""
    with np.errstate(over="ignore"):
        return diagonal(s, Jz, Nx, Ny) - Bx * np.exp(0.5 * (lp[1:] - lp[0])).sum(axis=0)


def inject_word0(family, prm, s, lp_ref):
    """(a) the flip pass reads sites >= 32 from word 0."""
    lp = lp_ref.copy()
    lp[1:] = queue_rows(family, prm, s, word0=True)[0][1:]
    return lp


def inject_checkpoint(family, prm, s, lp_ref):
    """(b) every continuation starts from the checkpoint one site early."""
    lp = lp_ref.copy()
    lp[1:] = queue_rows(family, prm, s, checkpoint_shift=1)[0][1:]
    return lp


def inject_ragged(lp_ref):
    """(c) the chains of the last 16-chain block all take chain ns - 1's rows."""
    lp = lp_ref.copy()
    ns = lp.shape[1]
    lp[:, (ns - 1) // CHAINS * CHAINS:] = lp[:, ns - 1:]
    return lp


def inject_one_stride(family, prm, s, lp_ref, waves):
    """(d) only the first `waves` tiles run: tile t = k nsb + block (flipped site k < N - 1) beyond them keeps its flip base."""
    lp = lp_ref.copy()
    base = queue_rows(family, prm, s)[1]
    N, ns = base.shape
    nsb = (ns + CHAINS - 1) // CHAINS
    tile = np.arange(N - 1)[:, None] * nsb + np.arange(ns)[None, :] // CHAINS
    lp[1:N] = np.where(tile >= waves, base[:N - 1], lp[1:N])
    return lp


def inject_transposed_bonds(e_ref, s, Jz, Nx, Ny):
    """(e) the bonds taken on the (Ny, Nx) reshape of the spins and of Jz."""
    return e_ref - diagonal(s, Jz, Nx, Ny) + diagonal(s, np.asarray(Jz).reshape(Ny, Nx), Ny, Nx)


def inject_small_ratio(family, prm, s, lp_ref):
    """(f) a wrong SMALL ratio: the flipped chain with the smallest true ratio of the case (flipped site k < N - 1) stops its
    continuation one site short, so its row lacks the term of site N - 1.  The ratio stays of its order of magnitude; E_loc moves
    by Bx |r' - r|.  (Putting the unflipped chain's log P into the row instead would make the ratio 1 and move E_loc by Bx, which
    the energy does see.)  Returns (lp, (row, chain), true ratio, defective ratio)."""
    sites = np.asarray(s).reshape(len(s), -1)
    N = sites.shape[1]
    gap = lp_ref[1:N] - lp_ref[0]
    k, b = np.unravel_index(int(np.argmin(gap)), gap.shape)
    flipped = sites[b:b + 1].copy()
    flipped[0, k] ^= 1
    lp = lp_ref.copy()
    lp[k + 1, b] = queue_rows(family, prm, flipped)[2][N - 2, 0]
    return lp, (int(k) + 1, int(b)), float(np.exp(0.5 * gap[k, b])), float(np.exp(0.5 * (lp[k + 1, b] - lp_ref[0, b])))


def timed_reference(family, prm, s, Jz, Bx, Nx, Ny):
    t0 = time.time()
    e_ref, lp_ref = reference(family, prm, s, Jz, Bx, Nx, Ny)
    return e_ref, lp_ref, time.time() - t0
