"""Float64 reference, bounds, cases and defect models of the 2D RNN's local-energy (flip) pass: mdrnn_flip_kernel of
csrc/mdrnn_kernels.h, driven by eloc_on_device of csrc/mdrnn.hip.  TEST INFRASTRUCTURE ONLY.

tfim_eloc(s, Jz, Bx, log_probs=lp) of the 2D RNN returns the whole log-probability queue, (N + 1, chains): row 0 is log P(s), row
nx Ny + ny + 1 is log P(s with the spin at (nx, ny) flipped).  Three evaluations of that queue live here:

  `queue`         THE REFERENCE.  Written from the model's definition - h' = elu(x_h Uh + h_h Wh + x_v Uv + h_v Wv + b) on the snake
                  path (oracle.models.zigzag_order), the neighbours being the previous site of the row and the site above, looked up
                  by LATTICE COORDINATES - for all N + 1 configurations of a chain at once.  The only economy: a configuration whose
                  flipped site is not yet visited is, so far, the unflipped one, so its state and inputs are the unflipped chain's
                  (shared prefixes).  Any NumPy float type; the four products of a step are ONE product over the stacked operand
                  [x_h | h_h | x_v | h_v], and `order` renumbers the hidden units: other summation orders than the oracle's.
  `oracle_queue`  every configuration scored from site 0 by oracle.estimators.ising2d_local_energies on
                  oracle.models.mdrnn_log_probability: the second honest float64 realisation.
  `kernel_form`   the kernel's bookkeeping restated - positions along the path, pv = p - 2 j - 1, one slot per lattice column for the
                  states a chain produced itself, the `pv <= i` switch between base-pass states and slots, the row turn - with one
                  switch per defect.  Without a switch it must reproduce `queue` (test_mdrnn_flip_reference.py); it is never a
                  reference.

Bounds (`judge`), none taken from a kernel:

  rows    |lp - lp_ref| <= 1e-11 N on every entry: the family's documented bound (tests/test_gpu_mdrnn.py, docs/pauli_2d.md).  It
          counts only where the reference earns it: on the checked chains of every case both float64 realisations stay within
          LICENCE = 1/16 of it of the numpy.longdouble `queue` (test_mdrnn_flip_reference.py prints the table).
  E_loc   |e - e_ref| <= Bx sum_k r_k 1e-11 N + 1e-13 (|diag| + Bx sum_k r_k), r_k = exp((lp_ref[k + 1] - lp_ref[0]) / 2) from the
          reference alone (raster_eloc_reference.measure builds it; the bonds are those of oracle.estimators.ising2d_local_energies)
  finite  every checked reference row is finite: no row is excused
  sharp   the ratios of the checked chains spread, r.std() > 0.2 r.mean() (flip_rows_reference's and raster_eloc_reference's criterion)
  row 0   within the row bound of wf.log_prob(s) (whether it is bit-equal is printed)

Defect models (test_mdrnn_flip_reference.py shows each refused, and bit-invisible where that is what justifies a case):
switches of `kernel_form` -
  (a) switch="le_plus" / "lt"  the switch between base-pass and own states read as pv <= i + 1 / as pv < i
  (b) mirror=False             the column slot not mirrored on odd rows (nx = j)
  (c) turn="zero"              at a row turn the vertical operand is not the state just computed (h_n already cleared)
  (e) vword="p"                the vertical neighbour's spin bit read from the word of p, bit pv & 31
  (f) flip_word0=True          the flipped bit applied in word 0 whatever i >> 5 is
  (g) store_short=True         states stored only up to row Ny - 3: row Ny - 1 reads stale slots
  (h) drop_last_unit=True      the last remainder unit of the flip pass is dropped
  (j) stale_first=True         a column slot holds another chain's own state where this chain's first state belongs
and edits of a clean queue -
  (d) inject_row_map           the queue row of (nx, ny) taken as ny Nx + nx + 1 (transposed), or as nx Nx + ny + 1 (Nx for Ny)
  (i) inject_ragged            lanes of the invalid chains of a ragged block add their continuation into chain ns - 1's rows
"""
import os
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import flip_rows_reference as F
import raster_eloc_reference as Q
import sampler_reference as R
from oracle import estimators as E
from oracle import models as M
from oracle import philox

SCOPE = R.SCOPE
BX = 3.0
SEED = 111
ROW_TOL = Q.ROW_TOL                # per site, on every queue entry
CHAINS = Q.CHAINS                  # chains per block (tile column) of mdrnn_flip_kernel
LICENCE = 1.0 / 16.0               # share of the row bound the float64 realisations may use against longdouble

# id, Nx, Ny, units, samples, kernel scale, checked 16-chain blocks (None: all), what it is for.
#
# Scales: x 1.25 throughout, confirmed on the checked chains themselves by test_mdrnn_flip_reference.py (finite on every row,
# sharp, both float64 realisations within 1/16 of the bound).  The elu cell is unbounded, so narrow layers saturate early: at x 1.5
# the own draws of 9x11 with 17 units reach log r = -1.2e7 (the float64 realisations then differ from longdouble by 71 row bounds
# and the from-site-0 oracle, which takes log(softmax), returns -inf), those of 1x40 with 20 units -4 410 (-inf from the oracle),
# and of the width sweep on 7x5 the widths 9, 10, 19, 33 and 36 give -inf from the oracle, 36 units also 0.077 of the bound against
# longdouble.  At x 1.25 all of these are finite and within 0.01 of the bound, except 10 units on 7x5 (log r down to -2 216, -inf
# from the oracle): that width runs at x 1.0 (log r -26 .. 1.9).
# Samples: 2 008 on the non-square lattices = 125 full blocks and one of 8 chains; with N - 1 >= 32 tile rows that is more tiles
# than the 32 wave slots of 256 CUs hold, so the later blocks' tiles are second and later tiles of their waves at any occupancy.
CASES = [
    ("cfg4", 12, 12, 50, 10000, 1.25, 4, "config 4 as benchmarked: 143 x 625 tiles, laps of the persistent grid"),
    ("cfg4-ragged", 12, 12, 50, 10007, 1.25, 4, "config 4 with a ragged last block of 7 chains"),
    ("13x5-50", 13, 5, 50, 2008, 1.25, 4, "Nx > Ny, 3 words; 3 full tiles, rem 2"),
    ("5x13-68", 5, 13, 68, 2008, 1.25, 4, "Nx < Ny, 3 words; 4 full tiles, rem 4"),
    ("7x9-84", 7, 9, 84, 2008, 1.25, 4, "2 words; 5 full tiles, rem 4: one workgroup per CU"),
    ("9x11-17", 9, 11, 17, 2008, 1.25, 4, "4 words; 1 full tile, rem 1"),
    ("11x3-35", 11, 3, 35, 2008, 1.25, 4, "33 sites: word 1 holds one position; 2 full tiles, rem 3"),
    ("3x33-50", 3, 33, 50, 2008, 1.25, 4, "32 row turns; an own-state slot is read one step after it is written"),
    ("33x3-50", 33, 3, 50, 2008, 1.25, 4, "the longest rows: 33 column slots"),
    ("16x16-50", 16, 16, 50, 528, 1.25, 3, "256 sites, 8 spin words: the limit of the word array"),
    ("1x40-20", 1, 40, 20, 72, 1.25, None, "every site a row turn"),
    ("40x1-20", 40, 1, 20, 72, 1.25, None, "no site has a vertical neighbour"),
]
CASE_IDS = [c[0] for c in CASES]

# every width class on one small non-square two-word lattice: 16 f + r for f = 1..5, r = 1..4, and the widths at or below 16 the
# suite uses elsewhere (no remainder unit there: rem <= 0)
WIDTH_LATTICE = (7, 5)
WIDTH_NS = 40                      # two full blocks and a ragged one of 8; every chain is judged
WIDTHS = [6, 9, 10, 16] + [16 * f + r for f in range(1, 6) for r in range(1, 5)]


def width_scale(H):
    return 1.0 if H == 10 else 1.25


def case(cid):
    return CASES[CASE_IDS.index(cid)]


def build_params(H, scale):
    """Sharpened as sampler_reference.build_params: kernels x scale, every bias randomised."""
    return R.build_params("mdrnn", (H,), seed=SEED, sharp=scale)


def couplings(Nx, Ny):
    """Random bonds, so that a transposed bond index shows."""
    return Q.couplings(Nx, Ny)


def checked_chains(ns, blocks):
    """Global indices of the chains of the checked blocks: whole 16-chain blocks at fixed positions - the first, the last (ragged
    where ns is), the others evenly between; all chains where blocks is None."""
    return np.arange(ns) if blocks is None else F.checked_chains(ns, CHAINS, blocks)


def oracle_draws(prm, Nx, Ny, chains):
    """The model's own draws sample(ns, seed=111, step=0) of the chains `chains`, by the CPU oracle's sampler on the same uniforms
    (chain b consumes the uniforms of global index b): what the CPU tests judge in place of the device's draws."""
    chains = np.asarray(chains)
    out = np.empty((len(chains), Nx, Ny), dtype=np.int64)
    cuts = np.flatnonzero(np.diff(chains) != 1) + 1
    for run in np.split(np.arange(len(chains)), cuts):
        u = philox.uniforms(SEED, 0, int(chains[run[0]]), len(run), Nx * Ny)
        out[run] = M.mdrnn_sample(prm, Nx, Ny, u, SCOPE)[0]
    return out


# ---- the reference: the model's definition with shared prefixes, in any float type ---------------------------------------------------

THREADS = min(8, os.cpu_count() or 1)
_POOL = []


def _pool():
    if not _POOL:
        _POOL.append(ThreadPoolExecutor(THREADS))
    return _POOL[0]


class _Cell:
    """step(x_h, h_h, x_v, h_v) -> h' and log_p(h) -> (.., 2), in `dtype`.  order > 0: the hidden units renumbered by a fixed
    permutation (seed `order`) - the same function, every product over the units summed in another order."""

    def __init__(self, prm, dtype, order=0):
        get = lambda name: np.asarray(prm[SCOPE + "/" + name]).astype(dtype)
        self.dtype = dtype
        self.H = H = get("b_rnn_0").shape[0]
        u = np.random.RandomState(order).permutation(H) if order else np.arange(H)
        self.W = np.ascontiguousarray(np.concatenate([get("Uh_rnn_0")[:, u], get("Wh_rnn_0")[u][:, u],
                                                      get("Uv_rnn_0")[:, u], get("Wv_rnn_0")[u][:, u]]))
        self.b = get("b_rnn_0")[u]
        self.Wd, self.bd = np.ascontiguousarray(get("wf_dense/kernel")[u]), get("wf_dense/bias")

    def _by_rows(self, fn, a):
        """fn of the rows of a (rows, K).  numpy.longdouble has no BLAS: there the rows go to a few threads in blocks (NumPy's
        loops release the interpreter lock); every row is computed as it would be alone, so the result does not depend on it."""
        if self.dtype is not np.longdouble or len(a) < 4096:
            return fn(a)
        return np.concatenate(list(_pool().map(fn, np.array_split(a, 4 * THREADS))))

    def _elu_of(self, op):
        pre = op @ self.W + self.b
        zero = self.dtype(0)
        return np.where(pre > zero, pre, np.expm1(np.minimum(pre, zero)))

    def _log_softmax_of(self, h):
        z = h @ self.Wd + self.bd
        m = z.max(axis=1, keepdims=True)
        return z - m - np.log(np.exp(z - m).sum(axis=1, keepdims=True))

    def step(self, xh, hh, xv, hv):
        """Operands (.., 2), (.., H), (.., 2), (.., H) with equal leading shape."""
        op = np.concatenate([xh, hh, xv, hv], axis=-1).reshape(-1, 2 * self.H + 4)
        return self._by_rows(self._elu_of, op).reshape(hh.shape[:-1] + (self.H,))

    def log_p(self, h):
        return self._by_rows(self._log_softmax_of, h.reshape(-1, self.H)).reshape(h.shape[:-1] + (2,))


def queue(prm, s, dtype=np.float64, order=0):
    """(lpq (N + 1, B), baseq (N + 1, B)) in `dtype` for configurations s (B, Nx, Ny): lpq is the queue (row 0 log P(s), row
    nx Ny + ny + 1 the flip at (nx, ny)); baseq[row] is the part of that row up to and including the flipped site itself (row 0:
    log P(s)), which on the device the base pass writes and the flip pass adds to.

    Configuration 0 is s, configuration k + 1 is s with the k-th visited site flipped.  At the k-th visited site the configurations
    0 .. k are evaluated; k + 1 .. N have seen no flipped spin yet and take configuration 0's state."""
    dt = np.dtype(dtype).type
    s = np.asarray(s).astype(np.int64)
    B, Nx, Ny = s.shape
    N = Nx * Ny
    cell = _Cell(prm, dt, order)
    H = cell.H
    eye = np.eye(2, dtype=dt)
    ar = np.arange(B)
    zeros_h, zeros_x = np.zeros((N + 1, B, H), dtype=dt), np.zeros((N + 1, B, 2), dtype=dt)
    h, x = {}, {}                                            # (nx, ny) -> states (N + 1, B, H) / one-hot spins (N + 1, B, 2)
    lp = np.zeros((N + 1, B), dtype=dt)
    base = np.zeros((N + 1, B), dtype=dt)
    rows = np.zeros(N + 1, dtype=np.int64)
    with np.errstate(over="ignore"):
        for k, (nx, ny, nxh) in enumerate(M.zigzag_order(Nx, Ny)):
            n = k + 1
            hh, xh = h.get((nxh, ny), zeros_h)[:n], x.get((nxh, ny), zeros_x)[:n]
            hv, xv = h.get((nx, ny - 1), zeros_h)[:n], x.get((nx, ny - 1), zeros_x)[:n]
            new = cell.step(xh, hh, xv, hv)
            lg = cell.log_p(new)
            sk = s[:, nx, ny]
            base[n] = lp[0] + lg[0, ar, 1 - sk]              # the configuration flipped here: the shared state, the other spin
            lp[:n] += lg[:, ar, sk]
            lp[n] = base[n]
            lp[n + 1:] = lp[0]
            full = np.empty((N + 1, B, H), dtype=dt)
            full[:n] = new
            full[n:] = new[0]
            xs = np.empty((N + 1, B, 2), dtype=dt)
            xs[:] = eye[sk]
            xs[n] = eye[1 - sk]
            h[(nx, ny)], x[(nx, ny)] = full, xs
            rows[n] = nx * Ny + ny + 1
            for key in [key for key in h if key[1] < ny - 1]:   # rows above the previous one have no reader left
                del h[key], x[key]
    base[0] = lp[0]
    lpq, baseq = np.empty_like(lp), np.empty_like(base)
    lpq[rows], baseq[rows] = lp, base
    return lpq, baseq


def oracle_queue(prm, s, Jz, Bx=BX):
    """(e (B,), lp (N + 1, B)): every configuration of the queue scored from site 0 in float64 by the oracle."""
    s = np.asarray(s)
    _, Nx, Ny = s.shape
    with np.errstate(over="ignore"):
        return E.ising2d_local_energies(Jz, Bx, Nx, Ny, s, lambda c: M.mdrnn_log_probability(prm, c, SCOPE), return_log_probs=True)


def energies(lp, s, Jz, Bx=BX):
    """E_loc assembled in float64 from a queue (N + 1, B)."""
    s = np.asarray(s)
    B, Nx, Ny = s.shape
    return Q.energies(np.asarray(lp, dtype=np.float64), s.reshape(B, Nx * Ny), Jz, Bx, Nx, Ny)


class Reference:
    """The float64 reference of a set of checked chains: their global indices `chains` in a batch of `ns`, configurations s
    (B, Nx, Ny), queue lp and its base part (N + 1, B), energies e, seconds."""

    def __init__(self, prm, s, Jz, Bx=BX, chains=None, ns=None):
        t0 = time.time()
        self.s = np.asarray(s).astype(np.int64)
        self.B, self.Nx, self.Ny = self.s.shape
        self.N = self.Nx * self.Ny
        self.Jz, self.Bx = np.asarray(Jz, dtype=np.float64), float(Bx)
        self.chains = np.arange(self.B) if chains is None else np.asarray(chains)
        self.ns = int(self.chains.max()) + 1 if ns is None else ns
        self.lp, self.base = queue(prm, self.s)
        self.e = energies(self.lp, self.s, self.Jz, self.Bx)
        self.distinct = len({c.tobytes() for c in self.s})
        self.seconds = time.time() - t0


def measure(lp, e, ref, log_prob=None):
    """raster_eloc_reference.measure on the checked chains; the worst entries named by their GLOBAL chain index."""
    m = Q.measure(lp, e, ref.lp, ref.e, ref.s.reshape(ref.B, ref.N), ref.Jz, ref.Bx, ref.Nx, ref.Ny)
    m["ref_finite"] = bool(np.all(np.isfinite(ref.lp)) and np.all(np.isfinite(ref.e)))
    m["worst_row"] = (m["worst_row"][0], int(ref.chains[m["worst_row"][1]]))
    m["worst_e"] = int(ref.chains[m["worst_e"]])
    m["log_share"] = float((np.abs(ref.lp[1:] - ref.lp[0]) > 2.0).mean())       # |log r| > 1
    m["distinct"] = ref.distinct
    if log_prob is not None:
        d = np.abs(np.asarray(lp)[0] - np.asarray(log_prob))
        m["row0_over"] = float(np.where(np.isfinite(d), d, np.inf).max() / (ROW_TOL * ref.N))
        m["row0_equal"] = bool(np.array_equal(np.asarray(lp)[0], log_prob))
    return m


def where(ref, row, chain):
    """Coordinates of a queue entry for a failure message: the lattice site, its position on the path, the tile of the walk."""
    nsb = (ref.ns + CHAINS - 1) // CHAINS
    if row == 0:
        return "queue row 0 (log P(s)), chain %d (block %d of %d)" % (chain, chain // CHAINS, nsb)
    nx, ny = divmod(row - 1, ref.Ny)
    p = ny * ref.Nx + (nx if ny % 2 == 0 else ref.Nx - 1 - nx)
    return ("queue row %d: flipped site (%d, %d) = position %d of the path (spin word %d, bit %d), chain %d, block %d of %d = tile %d" %
            (row, nx, ny, p, p >> 5, p & 31, chain, chain // CHAINS, nsb, p * nsb + chain // CHAINS))


def line(label, m, seconds=None):
    text = Q.line(label, m, seconds)
    text += "  |log r| > 1 on %.0f %% of the rows, %d distinct of %d" % (100 * m["log_share"], m["distinct"], m["ns"])
    if "row0_over" in m:
        text += "  row 0 vs log_prob / bound %.3e (%s)" % (m["row0_over"], "bit-equal" if m["row0_equal"] else "not bit-equal")
    return text


def judge(lp, e, ref, log_prob=None, label=""):
    """Asserts: the reference finite on every checked row (no row is excused), lp and e finite, the row bound on every entry, the
    E_loc bound, row 0 within the row bound of log_prob, the sharpness of the checked chains.  Returns the figures of `measure`."""
    m = measure(lp, e, ref, log_prob)
    assert m["ref_finite"], "%s the float64 reference is not finite on %d of its entries" % (label, int((~np.isfinite(ref.lp)).sum()))
    assert m["finite"], "%s non-finite values" % label
    assert m["row_over"] <= 1.0, "%s %s: |lp - ref| = %.3e > %.3e" % (label, where(ref, *m["worst_row"]), m["row_err"], ROW_TOL * ref.N)
    assert m["e_over"] <= 1.0, ("%s chain %d (block %d): |E - ref| = %.3e > %.3e" %
                                (label, m["worst_e"], m["worst_e"] // CHAINS, m["e_err"], m["e_bound"]))
    if log_prob is not None:
        assert m["row0_over"] <= 1.0, "%s row 0 of the queue is %.3f row bounds from log_prob(s)" % (label, m["row0_over"])
    assert m["sharp"], "%s the ratios do not spread (std / mean = %.3f): the weights are not sharp" % (label, m["spread"])
    return m


# ---- the kernel's bookkeeping, with one switch per defect --------------------------------------------------------------------------

def kernel_form(prm, s, switch="le", mirror=True, turn="state", vword="pv", flip_word0=False, store_short=False,
                drop_last_unit=False, stale_first=False):
    """The queue (N + 1, B) in float64 as mdrnn_base_kernel and mdrnn_flip_kernel compute it: spins in visit order, positions
    p = ny Nx + j, column nx = j on even rows and Nx - 1 - j on odd ones, vertical neighbour at position pv = p - 2 j - 1.  The base
    pass leaves the state after every position (hs) and every row up to its flipped position.  Tile i of the flip pass - the chain
    flipped at position i - starts from hs[i] and walks i + 1 .. N - 1; its vertical operand is zero on the first row, the state just
    computed at a row turn (pv = p - 1), hs[pv] where pv <= i, else its own column slot; it stores every state but the last row's
    into the slot of its column.  All tiles advance together here (axis 0 of the arrays below is i).  The switches are the defect
    models of the module docstring; they act on the flip pass alone."""
    s = np.asarray(s).astype(np.int64)
    B, Nx, Ny = s.shape
    N = Nx * Ny
    cell = _Cell(prm, np.float64)
    H = cell.H
    eye = np.eye(2)
    ar = np.arange(B)
    sp = np.stack([s[:, nx, ny] for nx, ny, _ in M.zigzag_order(Nx, Ny)], axis=1)          # (B, N) in visit order
    zh, zx = np.zeros((B, H)), np.zeros((B, 2))
    hs = np.zeros((N, B, H))
    base = np.zeros((N, B))
    cum = np.zeros(B)
    with np.errstate(over="ignore"):
        for p in range(N):
            ny, j = divmod(p, Nx)
            pv = p - 2 * j - 1 if ny > 0 else -1
            hh, xh = (zh, zx) if j == 0 else (hs[p - 1], eye[sp[:, p - 1]])
            hv, xv = (zh, zx) if pv < 0 else (hs[pv], eye[sp[:, pv]])
            hs[p] = cell.step(xh, hh, xv, hv)
            lg = cell.log_p(hs[p])
            base[p] = cum + lg[ar, 1 - sp[:, p]]
            cum = cum + lg[ar, sp[:, p]]
        # the flipped configurations' spin words, one set per tile, padded to whole words as the device's are
        seen = np.zeros((N, B, 32 * ((N + 31) // 32)), dtype=np.int64)
        seen[:, :, :N] = sp[None]
        i_all = np.arange(N)
        seen[i_all, :, np.where(i_all >= 32, i_all & 31, i_all) if flip_word0 else i_all] ^= 1
        hn = hs.copy()                                       # tile i: the state after position i
        slot = np.zeros((N, B, Nx, H))
        tail = np.zeros((N, B))
        last_stored = N - 2 * Nx if store_short else N - Nx
        for p in range(1, N):
            n = p                                            # tiles 0 .. p - 1 are on their way
            ny, j = divmod(p, Nx)
            pv = p - 2 * j - 1 if ny > 0 else -1
            nx = Nx - 1 - j if (ny & 1) and mirror else j
            i = np.arange(n)
            if j == 0:
                hh, xh = np.zeros((n, B, H)), np.zeros((n, B, 2))
            else:
                hh, xh = hn[:n], eye[seen[:n, :, p - 1]]
            if pv < 0:
                hv, xv = np.zeros((n, B, H)), np.zeros((n, B, 2))
            else:
                xv = eye[seen[:n, :, (p & ~31) | (pv & 31) if vword == "p" else pv]]
                if pv == p - 1:
                    hv = np.zeros((n, B, H)) if turn == "zero" else hn[:n]
                else:
                    from_base = {"le": pv <= i, "le_plus": pv <= i + 1, "lt": pv < i}[switch]
                    hv = np.where(from_base[:, None, None], hs[pv][None], slot[:n, :, nx])
            new = cell.step(xh, hh, xv, hv)
            if drop_last_unit:
                new[..., H - 1] = 0.0
            lg = cell.log_p(new)
            so = seen[:n, :, p]
            tail[:n] += np.where(so == 1, lg[..., 1], lg[..., 0])
            if p < last_stored:
                slot[:n, :, nx] = new
                if stale_first:                              # tile p - 1's first state: another chain's stands in its slot
                    slot[p - 1, :, nx] = np.roll(new[p - 1], 1, axis=0)
            hn[:n] = new
    lpq = np.empty((N + 1, B))
    lpq[0] = cum
    for p in range(N):
        ny, j = divmod(p, Nx)
        nx = Nx - 1 - j if ny & 1 else j
        lpq[nx * Ny + ny + 1] = base[p] + tail[p]
    return lpq


# ---- defect models that edit a clean queue -----------------------------------------------------------------------------------------

def inject_row_map(lp, Nx, Ny, how):
    """(d) the flip at (nx, ny) lands in queue row ny Nx + nx + 1 (how = "transposed") or nx Nx + ny + 1 (how = "stride": Nx taken
    for Ny; rows that then collide or fall outside keep what the base pass left, row 0's value standing in)."""
    out = np.empty_like(lp)
    out[:] = lp[0]
    for nx in range(Nx):
        for ny in range(Ny):
            row = ny * Nx + nx + 1 if how == "transposed" else nx * Nx + ny + 1
            if row <= Nx * Ny:
                out[row] = lp[nx * Ny + ny + 1]
    out[0] = lp[0]
    return out


def inject_ragged(ref, lp):
    """(i) every lane of an invalid chain of the ragged last block (it computes chain ns - 1's continuation, clamped) adds it into
    chain ns - 1's rows: the row holds base + (1 + invalid lanes) x continuation.  None where the checked chains end on no ragged
    block."""
    invalid = -ref.ns % CHAINS
    if invalid == 0 or ref.chains[-1] != ref.ns - 1:
        return None
    out = lp.copy()
    out[1:, -1] += invalid * (ref.lp[1:, -1] - ref.base[1:, -1])
    return out
