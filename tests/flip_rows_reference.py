"""Float64 reference, float32 yardstick, bounds and defect models of the f32-family TFIM local-energy (flip) pass of the positive 1D
GRU - one layer, stacks and the parity-symmetric class; the bf16x3 and the f32-input-MFMA engines.  TEST INFRASTRUCTURE ONLY.

tfim_eloc(..., log_probs=lp) returns the whole log-probability queue: row 0 is log P(s), row k + 1 is log P(s with site k flipped)
(for the parity class the symmetrised log(0.5 (P(x) + P(reversed x))) of every row: prnn.hip combines the two directions' queues
before the energies are assembled).  `reference` scores the queue of the checked chains twice with `queue` - a one-pass evaluation
that shares every flipped chain's prefix with the unflipped chain, as the kernels do - in float64 (the reference) and in float32 (the
yardstick).  tests/test_flip_rows_reference.py validates `queue` against the from-site-0 oracle (`oracle_reference`:
oracle.estimators.ising_local_energies on oracle.models.prnn_log_probability / prnn_paritysym_log_probability) at every case's shape.
The cells are restated from the formulas of oracle/models.py (gru_cell, multi_gru, prnn_site_probs), not called; as there, the cell
and the softmax run in the arithmetic `dtype`, the selected probabilities are cast to float64 before the log and the sum over sites.

Bounds, none taken from a kernel (`judge`):

  yardstick   y_b = max over the checked rows k and over FOUR float32 realisations of |lp32_ref[k, b] - lp64_ref[k, b]|, per chain b
              (single rows of that difference pass through zero), at least one float32 rounding of the value itself,
              2^-24 max_k |lp64_ref[k, b]|.  The realisations are the same float32 restatement with the hidden units renumbered
              (ORDERS: the model's numbering and three fixed permutations): every product over the units is summed in another order.
              One realisation is not enough where the chain amplifies rounding (x 3 kernels over 200 steps): a chain's single
              float32 error can come out a tenth of its typical size by chance, and an honest float32 evaluation then misses 16 x
              that.  Measured on 384 chains of the 200-site case, f32 C oracle, worst deviation / bound: 1.87 with one realisation,
              0.67 with two or three, 0.40 with four (test_flip_rows_reference.py).  A chain with a non-finite float32
              realisation has no yardstick: `judge` refuses it, it is never excused.
  rows        |lp[k, b] - lp64_ref[k, b]| <= FACTOR y_b on every entry of chain b, FACTOR = 16 as tests/autograd_reference.py: the
              yardstick is ONE realisation of float32 rounding, the kernels sum in other orders and restart from checkpoints that a
              different base kernel wrote.  Stacks: the same construction - the float32 restatement runs the same layers.
  row 0       |lp[0, b] - wf.log_prob(s)[b]| <= FACTOR y_b (not bit for bit: test_gpu_prnn.py - the base pass and the flip pass may
              associate their float32 sums differently)
  E_loc       |e_b - e_ref_b| <= Bx sum_k r_k FACTOR y_b + N 2^-53 (|diag_b| + Bx sum_k r_k),  r_k = exp((lp64_ref[k + 1] - lp64_ref[0]) / 2)
              first term: what the row bound lets through to first order (exp(D / 2) has relative error |dD| / 2, |dD| <= 2 FACTOR y_b);
              second: the sum.  util_kernels.h: tfim_eloc_kernel adds the bond terms and one float64 exp per site in float64 (eight
              partial sums joined in fixed order), so the summation term carries 2^-53, not 2^-24.
  sharpness   the ratios of the checked chains spread, r.std() > 0.2 r.mean() (test_gpu_sharpened.check_tfim)

Where a case checks a fixed SUBSET of flipped sites (N = 200, 100 units: the whole queue of whole tiles is too slow to score), the rows
of those sites are judged as above; the energy has no full reference there, so it is judged against the energy assembled in float64
from the queue under test itself, under the summation term alone - the decomposition  E error = row errors + assembly error.

A failure names the queue row, the chain, the flipped site, its 32-bit spin word, the 16- or 32-chain tile of the engine and the
tile's index in the walk (site x tiles per site + tile column: prnn_flip_pp_kernel's t, the f32 kernel's likewise with 16 chains).

Defect models (test_flip_rows_reference.py shows each refused): knobs of `queue` in float64, or edits of a clean queue -
  (a) weights16        the flip pass multiplies by weights cut to the sum of two bf16 terms (16 significant bits)
  (b) state16          the same cut applied to the hidden state after every step of the flip pass
  (c) word0            the flip pass reads the spins of sites >= 32 from word 0 of the packed spins
  (d) checkpoint_shift a flipped chain restarted from the checkpoint one site early (+1) or one site late (-1)
  (e) inject_ragged    in a ragged last tile the last valid chain takes its neighbour's rows
  (f) inject_unwritten one (site, tile) left unwritten: its rows equal row 0
  (g) lagged           stacks: an upper layer reads the lower layer's record of the previous site
  (h) inject_neighbour one row carries the value of the neighbouring flipped site
The knobs (a), (b), (c), (g) act on the flip pass alone - the continuation of a flipped chain after its restart - because the base
pass (row 0, every flip base, every checkpoint) is another kernel on another engine.
"""
import time

import numpy as np

import sampler_reference as R
from oracle import estimators as E
from oracle import models as M

SCOPE = R.SCOPE
FACTOR = 16.0                      # tests/autograd_reference.py: FACTOR
EPS32 = 2.0 ** -24
EPS64 = 2.0 ** -53
BX = 1.0
SEED = 111
SHARP = 3.0
ORDERS = (0, 1, 2, 3)              # numberings of the hidden units of the yardstick's float32 realisations (Reference)

# Sites of the cases that check a subset of the flipped sites (N = 200): both sides of every word boundary a 7-word chain has on its
# way, the first and the last site, and every 24th site between them
SITES_200 = tuple(sorted(set((0, 31, 32, 63, 64, 191, 192, 199)) | set(range(0, 200, 24))))

# id, family, N, units, samples, RNNWF_ENGINE while the handle is created (None: unset, "default"), the engine the flip pass must
# report, further environment of the handle, checked tiles, flipped sites (None: all), what it is for.
#
# Engine and kernel of every case, read from the sources (prnn.hip: use_split, pack_image; split.hip: with_layout, riders,
# stack_split_available, base_bf_pack; rnnwf_api.hip: pick_nfull):
#   * a batch runs bf16x3 by default when (N - 1) ceil(ns / 32) >= 8 CUs (2 048 on 256 CUs) and the width has a bf16x3 kernel: every
#     default case below except the 20-site one does (24 727, 25 472, 24 727 tiles), so each reaches the kernel named as listed; no N
#     or ns had to be moved.
#   * widths: <= 36 units flat (NFULL 1, 2) | 37..50 aligned (NFULL 3, K-packed) | 51..52 padded (NFULL 3) | 53..68 riders (NFULL 4)
#     | 69..100 streamed (NFULL 6) | above 100 (NFULL 8, 12, 16) the f32-input MFMA with the image through L2, whatever the switch.
#   * stacks: 37..50 units of equal width run the bf16x3 layer pipeline, every other stack ((64, 20): NFULL 4) the f32 stack kernels.
#   * 20 sites, 500 samples: 304 32-chain tiles < 8 CUs -> f32mfma; its base pass is the cooperative bf16 kernel (50 units: NFULL 3),
#     under RNNWF_NO_COOP=1 the one-wave kernel.  Under RNNWF_ENGINE=f32 the base pass is the cooperative f32 kernel (626 blocks <= 4 CUs).
#   * laps: the ping-pong kernels (37..50 units, the layer pipeline, the parity class at 50 units) hold 8 waves on a CU - one
#     workgroup - so tiles from 8 CUs on are walked in a second lap: for them 8 CUs is exact.  The grids of the 4-wave flat, padded,
#     riders and streamed kernels and of the f32 kernels come from the occupancy query (handle.h: persistent_grid) and may hold more,
#     at most the hardware's 32 waves on a CU: for them 8 CUs is a LOWER bound of the lap, and the GPU test prints which checked
#     tiles also lie beyond 32 CUs (the two config-2 cases, the 200-site case, 128 units, (64, 20), the parity class do; flat-36
#     with 8 192 and padded-52 with 8 064 tiles in all cannot).  Every checked tile column is checked at every flipped site, so its last
#     tile has index >= (N - 2) x tiles per site: beyond 8 CUs in every case that HAS more than 8 CUs tiles.
#   * four layers: as listed (2 048 samples on 33 sites) the case has 32 x 64 = 2 048 tiles, exactly one lap of 256 CUs; 2 080 samples,
#     one more tile column, are the nearest shape that reaches a second lap (2 080 tiles), so the case runs 2 080.
#   * two cases have fewer tiles than 8 CUs as the issue lists them (406 samples at 256 units: 1 014 tiles of 16; 500 samples on 20
#     sites: 608) and cannot lap at any nearby shape: they are here for their kernels (image through L2 at NFULL 16; the run script's
#     base passes), not for the walk.
# Checked tiles (fractions of the tile columns, never chosen by outcome): the first, the last (ragged where the case is) and fixed
# positions between.  Their number is fixed by the cost of the reference alone - the float64 queue and the four float32 realisations of
# a case take up to about 3 s on 16 threads - and the 200-site case checks as many whole tiles as config 2 does.
CASES = [
    ("cfg2-ragged", "gru", 80, (50,), 10007, None, "bf16x3", {}, 12, None, "config 2, ragged: 313 tiles of 32, the last holds 23"),
    ("cfg2-ragged-f32", "gru", 80, (50,), 10007, "f32", "f32mfma", {}, 24, None, "the same on the f32 engine (bench's f32 leg): 626 tiles of 16, the last holds 7"),
    ("flat-36", "gru", 65, (36,), 4096, "bf16x3", "bf16x3", {}, 12, None, "flat class, 3 spin words"),
    ("aligned-37", "gru", 33, (37,), 4096, "bf16x3", "bf16x3", {}, 18, None, "first width of the aligned class; bit 31 and word 1"),
    ("padded-52", "gru", 64, (52,), 4096, "bf16x3", "bf16x3", {}, 12, None, "padded class, two full words"),
    ("riders-53", "gru", 40, (53,), 4096, "bf16x3", "bf16x3", {}, 18, None, "riders, LDS-resident: first width"),
    ("riders-68", "gru", 40, (68,), 4096, "bf16x3", "bf16x3", {}, 18, None, "riders, LDS-resident: last width"),
    ("streamed-69", "gru", 40, (69,), 4096, "bf16x3", "bf16x3", {}, 18, None, "streamed class: first width"),
    ("cfg5-shape", "gru", 200, (100,), 4096, None, "bf16x3", {}, 12, SITES_200, "config 5's shape, 7 spin words"),
    ("wide-128", "gru", 40, (128,), 4096, None, "f32mfma", {}, 18, None, "above 100 units: image through L2 (NFULL 8)"),
    ("wide-256", "gru", 40, (256,), 406, None, "f32mfma", {}, 9, None, "NFULL 16; 25 tiles of 16 and a ragged one of 6"),
    ("cfg2-l2", "gru", 80, (50, 50), 10000, None, "bf16x3", {}, 9, None, "config 2 with two layers: the layer pipeline; ragged (312 tiles of 32 and one of 16)"),
    ("stack-3", "gru", 40, (50, 50, 50), 4096, "bf16x3", "bf16x3", {}, 12, None, "three layers: first, middle and top kernel"),
    ("stack-4", "gru", 33, (44, 44, 44, 44), 2080, "bf16x3", "bf16x3", {}, 12, None, "four layers; 65 tile columns: a second lap"),
    ("stack-64-20", "gru", 40, (64, 20), 4096, None, "f32mfma", {}, 24, None, "unequal widths (padding inside the library)"),
    ("parity-40", "parity", 40, (50,), 9008, "bf16x3", "bf16x3", {}, 12, None, "parity-symmetric, both directions; ragged (16 in the last tile)"),
    ("script-20", "gru", 20, (50,), 500, None, "f32mfma", {}, 16, None, "run-script size: cooperative base pass; 31 tiles of 16 and a ragged one of 4"),
    ("script-20-nocoop", "gru", 20, (50,), 500, None, "f32mfma", {"RNNWF_NO_COOP": "1"}, 16, None, "the same on the one-wave base kernel"),
]
CASE_IDS = [c[0] for c in CASES]


def case(cid):
    return CASES[CASE_IDS.index(cid)]


def tile_of_engine(engine):
    """Chains per flip tile: 32 on the bf16x3 engine (split_kernels.h), 16 on the f32-input MFMA (gru_kernels.h)."""
    return 32 if engine == "bf16x3" else 16


def build_params(family, units):
    return R.build_params(family, units, seed=SEED, sharp=SHARP)


def couplings(N):
    """Random bonds, so that a shifted bond index shows."""
    return np.random.RandomState(N).uniform(0.5, 1.5, N)


def checked_tiles(ns, tile, count, shift=0):
    """`count` tile columns of the batch at fixed positions: the first, the last, the others evenly between.  shift: every column
    moved on by `shift` (cyclically) - another fixed set, for the CPU study of the bound."""
    ntile = (ns + tile - 1) // tile
    count = min(count, ntile)
    if count == 1:
        return np.array([0])
    return np.unique((np.round(np.linspace(0, ntile - 1, count)).astype(np.int64) + shift) % ntile)


def checked_chains(ns, tile, count, per_tile=None, shift=0):
    """Global indices of the chains of the checked tiles, whole tiles (per_tile: the CPU study's cut - the first per_tile chains of
    each tile, of the last tile its last per_tile valid ones, so that the ragged edge stays in)."""
    out = []
    tiles = checked_tiles(ns, tile, count, shift)
    for t in tiles:
        lo, hi = t * tile, min(ns, (t + 1) * tile)
        if per_tile is not None:
            lo, hi = (max(lo, hi - per_tile), hi) if t == tiles[-1] else (lo, min(hi, lo + per_tile))
        out.append(np.arange(lo, hi))
    return np.concatenate(out)


# ---- the from-site-0 oracle ----------------------------------------------------------------------------------------------------------

def log_prob_fn(family, prm, dtype=np.float64):
    p = R.cast(prm, dtype)
    fn = M.prnn_paritysym_log_probability if family == "parity" else M.prnn_log_probability
    return lambda x: fn(p, x, SCOPE, dtype)


def oracle_reference(family, prm, s, Jz, Bx=BX):
    """(e (B,), lp (N + 1, B)): every chain of the queue scored from site 0 in float64 by the oracle's estimator."""
    with np.errstate(over="ignore"):
        return E.ising_local_energies(Jz, Bx, np.asarray(s), log_prob_fn(family, prm), return_log_probs=True)


# ---- the queue with shared prefixes, in any float type, with the defect knobs -----------------------------------------------------------

def two_bf16_terms(a):
    """Every element rounded to 16 significant bits: what the sum of two bf16 terms (8 bits each) holds."""
    m, e = np.frexp(np.asarray(a, dtype=np.float64))
    return np.ldexp(np.round(m * 65536.0) / 65536.0, e).astype(a.dtype)


class _Cells:
    """step(x (B, 2), states) -> (states', p (B, 2)): the GRU stack and the softmax head in the arithmetic `dtype`."""
    NAMES = ("gates/kernel", "gates/bias", "candidate/input_projection/kernel", "candidate/input_projection/bias",
             "candidate/hidden_projection/kernel", "candidate/hidden_projection/bias")

    def __init__(self, prm, dtype, weights16=False, order=0):
        """order > 0: the hidden units of every layer renumbered by a fixed permutation (seed `order`) - the same function, every
        product over the units summed in another order: another realisation of the rounding."""
        cut = two_bf16_terms if weights16 else (lambda a: a)
        get = lambda name: np.asarray(prm[SCOPE + "/" + name]).astype(dtype)
        rng = np.random.RandomState(order)
        self.dtype = dtype
        self.layers = []
        q = np.arange(2)                                     # numbering of the layer's input: the one-hot spin, then the layer below
        for l in range(M.num_gru_layers(prm, SCOPE)):
            Wg, bg, Wci, bci, Wch, bch = [get(M.GRU % l + n) for n in self.NAMES]
            H = Wch.shape[0]
            u = rng.permutation(H) if order else np.arange(H)
            rows, cols = np.concatenate([q, len(q) + u]), np.concatenate([u, H + u])
            self.layers.append(tuple(np.ascontiguousarray(a) for a in
                                     (cut(Wg)[rows][:, cols], bg[cols], cut(Wci)[q][:, u], bci[u], cut(Wch)[u][:, u], bch[u])))
            q = u
        self.Wd, self.bd = np.ascontiguousarray(get("wf_dense/kernel")[q]), get("wf_dense/bias")
        self.widths = [w[4].shape[0] for w in self.layers]

    def step(self, x, states, lagged=False):
        one = self.dtype(1)
        new = []
        for l, ((Wg, bg, Wci, bci, Wch, bch), h) in enumerate(zip(self.layers, states)):
            if lagged and l:
                x = states[l - 1]                     # the lower layer's output of the previous site
            H = h.shape[1]
            g = one / (one + np.exp(-(np.concatenate([x, h], axis=1) @ Wg + bg)))
            cand = np.tanh((x @ Wci + bci) + g[:, :H] * (h @ Wch + bch))
            x = (one - g[:, H:]) * cand + g[:, H:] * h
            new.append(x)
        z = new[-1] @ self.Wd + self.bd
        e = np.exp(z - z.max(axis=1, keepdims=True))
        return new, e / e.sum(axis=1, keepdims=True)


def queue_rows(prm, s, dtype=np.float64, sites=None, weights16=False, state16=False, word0=False, checkpoint_shift=0, lagged=False,
               order=0):
    """(1 + len(sites), B) float64: log P of the (B, N) configurations and of each with one of `sites` (ascending; default all) flipped,
    cells and softmax in `dtype`.  One pass over the sites: at site n the unflipped chains advance, the chains flipped at k < n
    advance with their own inputs, and the chain flipped at n starts from the unflipped state after site n with the flipped spin as
    its next input.  The knobs are the defect models of the module docstring; they leave row 0 and every flip base alone.  order: the
    numbering of the hidden units (_Cells): 0 is the model's, others give further realisations of the rounding."""
    dt = np.dtype(dtype).type
    s = np.asarray(s).reshape(len(s), -1).astype(np.int64)
    B, N = s.shape
    sites = np.arange(N) if sites is None else np.asarray(sites, dtype=np.int64)
    assert np.all(np.diff(sites) > 0) and sites[0] >= 0 and sites[-1] < N
    K = len(sites)
    cells = _Cells(prm, dt, order=order)
    fcells = _Cells(prm, dt, weights16=True, order=order) if weights16 else cells
    eye = np.eye(2, dtype=dt)
    ar = np.arange(B)
    seen = s[:, np.arange(N) & 31] if word0 else s           # what the flip pass reads
    x = np.zeros((B, 2), dtype=dt)
    state = [np.zeros((B, w), dtype=dt) for w in cells.widths]
    fstate = [np.zeros((K, B, w), dtype=dt) for w in cells.widths]
    fx = np.zeros((K, B, 2), dtype=dt)
    flp = np.zeros((K, B))
    base = np.zeros((K, B))
    prefix = np.zeros(B)
    m = 0                                                    # flipped chains started so far: slots 0 .. m - 1
    with np.errstate(over="ignore", divide="ignore"):
        for n in range(N):
            before = state
            state, p = cells.step(x, state)
            lg = np.log(p.astype(np.float64))
            if m:
                new, fp = fcells.step(fx[:m].reshape(m * B, 2), [f[:m].reshape(m * B, -1) for f in fstate], lagged)
                for f, v in zip(fstate, new):
                    f[:m] = (two_bf16_terms(v) if state16 else v).reshape(m, B, -1)
                flp[:m] += np.log(fp.astype(np.float64)).reshape(m, B, 2)[:, ar, seen[:, n]]
                fx[:m] = eye[seen[:, n]]
                if checkpoint_shift < 0 and sites[m - 1] == n - 1:
                    # one site late: the chain flipped at n - 1 takes the unflipped state after site n; its flipped spin never entered
                    for f, v in zip(fstate, state):
                        f[m - 1] = v
                    flp[m - 1] = base[m - 1] + lg[ar, s[:, n]]
            if m < K and sites[m] == n:
                base[m] = prefix + lg[ar, 1 - s[:, n]]
                flp[m] = base[m]
                for f, v in zip(fstate, before if checkpoint_shift > 0 else state):
                    f[m] = v
                fx[m] = eye[1 - seen[:, n]]
                m += 1
            prefix = prefix + lg[ar, s[:, n]]
            x = eye[s[:, n]]
    return np.concatenate([prefix[None], flp])


def queue(family, prm, s, dtype=np.float64, sites=None, **knobs):
    """`queue_rows` of the family: the parity class symmetrises row by row - the reversed chain of (s flipped at k) is (reversed s)
    flipped at N - 1 - k, so the second direction is one more pass over the reversed configurations."""
    s = np.asarray(s).reshape(len(s), -1)
    if family != "parity":
        return queue_rows(prm, s, dtype, sites, **knobs)
    N = s.shape[1]
    sites = np.arange(N) if sites is None else np.asarray(sites, dtype=np.int64)
    f = queue_rows(prm, s, dtype, sites, **knobs)
    r = queue_rows(prm, s[:, ::-1], dtype, (N - 1 - sites)[::-1], **knobs)
    r = np.concatenate([r[:1], r[1:][::-1]])
    return np.logaddexp(f, r) - np.log(2.0)


# ---- reference and yardstick of a set of checked chains ------------------------------------------------------------------------------------

class Reference:
    """What `judge` needs of a case: the checked chains (global indices `chains` of a batch of `ns`, configurations `s`), the flipped
    sites, the float64 queue rows lp64 ((1 + sites, B)), the float32 realisations lp32 (a list of such, one per ORDERS), the yardstick y and the energies e64 (None
    where the sites are a subset)."""

    def __init__(self, family, prm, s, Jz, Bx=BX, sites=None, chains=None, ns=None, tile=32):
        t0 = time.time()
        self.family, self.Jz, self.Bx, self.tile = family, np.asarray(Jz, dtype=np.float64), float(Bx), tile
        self.s = np.asarray(s).reshape(len(s), -1).astype(np.int64)
        self.B, self.N = self.s.shape
        self.full = sites is None
        self.sites = np.arange(self.N) if sites is None else np.asarray(sites, dtype=np.int64)
        self.rows = np.concatenate([[0], self.sites + 1])
        self.chains = np.arange(self.B) if chains is None else np.asarray(chains)
        self.ns = int(self.chains.max()) + 1 if ns is None else ns
        self.lp64 = queue(family, prm, self.s, np.float64, None if self.full else self.sites)
        self.lp32 = [queue(family, prm, self.s, np.float32, None if self.full else self.sites, order=o) for o in ORDERS]
        with np.errstate(invalid="ignore"):
            d = np.max([np.abs(lp - self.lp64) for lp in self.lp32], axis=0)
        self.y = np.maximum(d.max(axis=0), EPS32 * np.abs(self.lp64).max(axis=0))      # nan where a float32 run is not finite
        self.bound = FACTOR * self.y
        with np.errstate(over="ignore"):
            self.r = np.exp(0.5 * (self.lp64[1:] - self.lp64[0]))
        self.diag = diagonal(self.s, self.Jz)
        self.e64 = self.diag - self.Bx * self.r.sum(axis=0) if self.full else None
        self.seconds = time.time() - t0


def diagonal(s, Jz):
    """-sum_i Jz[i] sz_i sz_{i+1} of the open chain (1DTFIM/TrainingRNN_1DTFIM.py:31-38)."""
    sz = 2.0 * np.asarray(s) - 1.0
    return -(sz[:, :-1] * sz[:, 1:] * np.asarray(Jz)[:-1]).sum(axis=1)


def energies(lp, s, Jz, Bx=BX):
    """E_loc assembled in float64 from a whole queue (N + 1, B)."""
    with np.errstate(over="ignore"):
        return diagonal(s, Jz) - Bx * np.exp(0.5 * (lp[1:] - lp[0])).sum(axis=0)


def measure(lp, e, ref, log_prob=None, assembled=None):
    """The figures `judge` asserts on.  lp (1 + sites, B): the rows ref.rows of the checked chains' queue; e (B,) their energies or
    None (not judged); log_prob: wf.log_prob of the checked chains; assembled: where ref checks a subset of the sites, (E_loc
    assembled in float64 from the whole queue under test, the sum of its ratios) - what e is judged against there."""
    lp = np.asarray(lp)
    assert lp.shape == ref.lp64.shape, (lp.shape, ref.lp64.shape)
    with np.errstate(invalid="ignore"):
        over = np.abs(lp - ref.lp64) / ref.bound
    over = np.where(np.isfinite(over), over, np.inf)
    wr = np.unravel_index(int(np.argmax(over)), over.shape)
    m = dict(N=ref.N, B=ref.B, rows=over.size, finite=bool(np.all(np.isfinite(lp)) and (e is None or np.all(np.isfinite(e)))),
             row_over=float(over[wr]), worst_row=(int(ref.rows[wr[0]]), int(ref.chains[wr[1]])),
             row_err=float(np.abs(lp - ref.lp64)[wr]), row_bound=float(ref.bound[wr[1]]),
             ratio_min=float(ref.r.min()), ratio_max=float(ref.r.max()), spread=float(ref.r.std() / ref.r.mean()),
             sharp=bool(ref.r.std() > 0.2 * ref.r.mean()), y_min=float(ref.y.min()), y_max=float(ref.y.max()),
             e_over=None, row0_over=None)
    if e is not None:
        e = np.asarray(e)
        if ref.full:
            rsum = ref.r.sum(axis=0)
            e_bound = ref.Bx * rsum * ref.bound + ref.N * EPS64 * (np.abs(ref.diag) + ref.Bx * rsum)
            e_err = np.abs(e - ref.e64)
        else:
            e_own, rsum = assembled
            e_bound = ref.N * EPS64 * (np.abs(ref.diag) + ref.Bx * rsum)
            e_err = np.abs(e - e_own)
        with np.errstate(invalid="ignore"):
            eo = np.where(np.isfinite(e_err), e_err / e_bound, np.inf)
        we = int(np.argmax(eo))
        m.update(e_over=float(eo[we]), worst_e=int(ref.chains[we]), e_err=float(e_err[we]), e_bound=float(e_bound[we]))
    if log_prob is not None:
        with np.errstate(invalid="ignore"):
            o = np.abs(lp[0] - np.asarray(log_prob)) / ref.bound
        o = np.where(np.isfinite(o), o, np.inf)
        m.update(row0_over=float(o.max()), worst_row0=int(ref.chains[int(np.argmax(o))]))
    return m


def where(ref, row, chain):
    """Coordinates of a queue entry for a failure message."""
    tiles = (ref.ns + ref.tile - 1) // ref.tile
    if row == 0:
        return "queue row 0 (log P(s)), chain %d (tile %d of %d chains)" % (chain, chain // ref.tile, ref.tile)
    k = row - 1
    return ("queue row %d: flipped site %d (spin word %d, bit %d), chain %d, tile column %d of %d chains = tile %d of the walk (%d per site)" %
            (row, k, k // 32, k % 32, chain, chain // ref.tile, ref.tile, k * tiles + chain // ref.tile, tiles))


def line(label, m, seconds=None):
    text = ("%s N %d: %d rows of %d chains checked; max row error / bound %.3f (%.2e of %.2e at row %d chain %d)" %
            (label, m["N"], m["rows"], m["B"], m["row_over"], m["row_err"], m["row_bound"], m["worst_row"][0], m["worst_row"][1]))
    if m["e_over"] is not None:
        text += "  max E error / bound %.3f (%.2e of %.2e, chain %d)" % (m["e_over"], m["e_err"], m["e_bound"], m["worst_e"])
    if m["row0_over"] is not None:
        text += "  row 0 vs log_prob / bound %.3f" % m["row0_over"]
    text += "  yardstick %.1e .. %.1e  ratios %.2e .. %.2e (std / mean %.2f)" % (m["y_min"], m["y_max"], m["ratio_min"], m["ratio_max"],
                                                                                m["spread"])
    return text + ("" if seconds is None else "  reference %.1f s" % seconds)


def judge(lp, e, ref, log_prob=None, assembled=None, label=""):
    """Asserts finiteness, the row bound on every entry, the E_loc bound, row 0 against log_prob within the row bound, and the
    sharpness of the checked chains.  Returns the figures of `measure`."""
    m = measure(lp, e, ref, log_prob, assembled)
    assert m["finite"], "%s non-finite values" % label
    assert np.all(np.isfinite(ref.y)), ("%s chains %s have no yardstick: a float32 realisation of the reference is not finite there" %
                                        (label, ref.chains[~np.isfinite(ref.y)].tolist()))
    assert m["row_over"] <= 1.0, ("%s %s: |lp - ref| = %.3e > %.3e = %g x yardstick" %
                                  (label, where(ref, *m["worst_row"]), m["row_err"], m["row_bound"], FACTOR))
    if m["e_over"] is not None:
        assert m["e_over"] <= 1.0, ("%s chain %d (tile column %d of %d chains): |E - ref| = %.3e > %.3e" %
                                    (label, m["worst_e"], m["worst_e"] // ref.tile, ref.tile, m["e_err"], m["e_bound"]))
    if m["row0_over"] is not None:
        assert m["row0_over"] <= 1.0, ("%s %s: row 0 of the queue is %.3f row bounds from log_prob(s)" %
                                       (label, where(ref, 0, m["worst_row0"]), m["row0_over"]))
    assert m["sharp"], "%s the ratios do not spread (std / mean = %.3f): the weights are not sharp" % (label, m["spread"])
    return m


# ---- defect models that edit a clean queue (rows ref.rows of the checked chains); the others are knobs of `queue` -------------------------

def inject_ragged(ref, lp):
    """(e) the last valid chain of a ragged last tile takes its neighbour's rows.  None where the checked chains hold no such pair."""
    if ref.ns % ref.tile < 2 or ref.chains[-1] != ref.ns - 1 or ref.chains[-2] != ref.ns - 2:
        return None
    out = lp.copy()
    out[:, -1] = lp[:, -2]
    return out


def inject_unwritten(ref, lp):
    """(f) one (site, tile) left unwritten: the rows of the LAST checked site that has a tile of its own (site N - 1's row is completed
    by the base pass) equal row 0 in the last checked tile column - the tile a walk that stops after its first lap never reaches."""
    j = int(np.flatnonzero(ref.sites < ref.N - 1)[-1]) + 1
    cols = ref.chains // ref.tile == ref.chains[-1] // ref.tile
    out = lp.copy()
    out[j, cols] = lp[0, cols]
    return out


def inject_neighbour(ref, lp):
    """(h) one row carries the value of the neighbouring flipped site: of the first checked chain, the middle checked site takes the
    next checked one's."""
    j = 1 + len(ref.sites) // 2
    out = lp.copy()
    out[j, 0] = lp[j + 1, 0]
    return out
