"""Float64 reference, float32 yardstick, bounds and defect models of the J1-J2 local-energy (swap) pass of the complex U(1) RNN - one
layer, stacks; the bf16x3 and the f32-input-MFMA engines.  TEST INFRASTRUCTURE ONLY.

j1j2_eloc(s, J1, J2, Bz, periodic, marshall) returns complex64 E_loc = diag + sum_k H_k exp(log psi(s'_k) - log psi(s)) over the
anti-aligned bonds k of s (s'_k: the two spins of bond k exchanged, H_k = +-J_k / 2) and the number of scored configurations.  The
enumerate kernel makes no item for a bond whose coupling is exactly 0, so with J = 1 on ONE bond and 0 elsewhere the output is
diag + 1/2 exp(d_k): every connected amplitude ratio can be read through the public call (the probe of test_gpu_crnn_swap_full.py).

`connected` lists the bonds (slot, lo, hi, coefficient), which of them are anti-aligned in each sample, the diagonal and the count,
as oracle.estimators.j1j2_slices does (validated against it by tests/test_crnn_swap_reference.py).  Bond slot: J1 bond of site a ->
a, J2 bond of site a -> N + a (the order of the reference's rows); lo < hi are the two sites, lo the first changed one.

`log_ratios` returns d = log psi(s') - log psi(s) of every (bond, chain) in one pass over the sites that shares each swapped chain's
prefix with the chain itself, as the kernels do: the state after site lo is the chain's own, the term of site lo is the own head's
value for the other spin, the up-count restarts from the own prefix, sites lo + 1 .. N - 1 are re-evaluated with site hi flipped.  The
cell, the masked amplitude (sqrt softmax, U(1) mask from site N/2 on, l2 normalisation) and the phase pi softsign are restated from
the formulas of oracle/models.py (gru_cell, multi_gru, _crnn_masked_ampl, crnn_log_amplitude), not called; they run in the arithmetic
`dtype`, the per-site terms are cast to float64 before they are summed (crnn_kernels.h sums them in double).  The test validates it
against M.crnn_log_amplitude(dtype=float64) on fully written-out swapped rows.

Bounds, none taken from a kernel (FACTOR = 16 as tests/autograd_reference.py):

  yardstick   y_b = max over the checked anti-aligned bonds k and over FOUR float32 realisations (the float32 restatement with the
              hidden units renumbered: ORDERS of flip_rows_reference, whose docstring says why one realisation is not enough) of
              |d32[k, b] - d64[k, b]| (complex modulus), at least 2^-24 max_k |d64[k, b]|.  A chain with a non-finite realisation
              has no yardstick: the judges refuse it, it is never excused.
  probe       J = 1 on one bond (SwapItem.coef = 1/2 exactly), all else 0: v = 2 (E - diag_ref) against v_ref = exp(d64),
              |v - v_ref| <= |v_ref| FACTOR y_b + 2 2^-24 (|Re E_ref| + |Im E_ref|); the second term is the float32 rounding of the
              complex64 output per component (E = diag + v / 2, so v carries twice E's rounding).  A chain whose bond is aligned
              must return exactly diag_ref (+-1/4) with zero imaginary part.
  E_loc       |e - e_ref| <= sum_k |H_k| |r_k| (FACTOR y_b + 2^-24) + 2^-24 |e_ref| + N 2^-53 (|diag| + sum_k |H_k| |r_k|),
              r_k = exp(d64[k]).  First term: what the ratio bound lets through to first order, and `coef` cast to float; second:
              the complex64 output; third: the sum.  FOUND in the sources: every swap kernel's store (crnn_swap_kernel,
              crnn_ml_swap_kernel, crnn_split_kernels.h) forms exp(dre) * coef, cos and sin in double and writes a double2;
              j1j2_eloc_kernel adds diag and the 2 N slots in double in bond order and casts once to float2; the enumerate kernel
              sums the diagonal in double.  So the summation term carries 2^-53 as stated (it is 2^-24 of the second term and
              decides nothing).
  ncon        equals the reference count exactly
  sharpness   the largest |r| over the checked chains is above 3 (test_gpu_sharpened.test_config3_sharpened)

A failure names the sample, the bond (slot, lo, hi), the spin words of lo and hi, the up-count at lo, and the tile: (lo, rank of the
sample among the chains that have this bond // tile size) - 32 items on bf16x3, 16 on f32mfma.  The rank is the item's index where one
bond fills the list and the enumerate kernel's blocks arrive in order; with several bonds per lo the list interleaves them.

Defect models (test_crnn_swap_reference.py shows each refused) - knobs of `log_ratios` in float64, of `connected`, or edits of a clean
result:
  (a) weights16       the continuation multiplies by weights cut to the sum of two bf16 terms (16 significant bits)
  (b) state16         the same cut applied to the hidden state after every step of the continuation
  (c) word0           the continuation reads the spins of sites >= 32 from word 0 of the packed spins
  (d) keep_hi         site hi is not flipped
  (e) restart_shift   the continuation starts from the state one site early (+1) or late (-1)
  (f) count_shift     the up-count at the restart is off by one.  The count only enters the U(1) mask, so this shows only from site
                      N/2 on - but every swapped chain passes through there, so every bond shows it
  (g) inject_neighbour one contribution carries the neighbouring bond's value (the item read from the next slot).  A contribution
                      merely STORED under the neighbouring slot cannot be seen from outside: j1j2_eloc_kernel adds all 2 N slots
  (h) inject_zero     one contribution left at zero
  (i) marshall_j2     the Marshall sign applied to the J2 bonds too (knob of `connected`)
  (j) unwrapped       a wrap bond's (lo, hi) taken as (site, site + dist) without the modulus: hi >= N is never reached.  A wrap bond
                      exchanges site 0 or 1 with the far end; at some cases (config 3's shape among them) every such exchange of the
                      model's own samples is suppressed to |r| < 1e-8, below the float32 rounding of the output, and neither this
                      defect nor anything else about the wrap bonds can show there.  At the other cases (w37, w53, w68, 128 units,
                      the stacks: |r| up to 9) it does; test_crnn_swap_reference.py prints the largest wrap ratio of every case
  (k) inject_ragged   in a ragged last tile the last valid item takes its neighbour's value
  (l) lagged          stacks: an upper layer of the continuation reads the lower layer's output of the previous site
The knobs (a), (b), (c), (l) act on the continuation alone: the base pass (log psi(s), the swap bases, every checkpoint) is another
kernel.
"""
import time

import numpy as np

import flip_rows_reference as F
import sampler_reference as R
from autograd_reference import FACTOR
from oracle import models as M

SCOPE = R.SCOPE
EPS32 = 2.0 ** -24
EPS64 = 2.0 ** -53
SEED = 111
SHARP = 3.0
ORDERS = F.ORDERS
checked_chains = F.checked_chains
two_bf16_terms = F.two_bf16_terms


def probe_slots(N):
    """The fixed set of probed bond slots of a long chain: the first and the last bond, both sides of every 32-site word boundary for
    dist 1 and 2, the bonds straddling N/2, every wrap bond."""
    j1 = {0, N - 2, N - 1, N // 2 - 2, N // 2 - 1, N // 2}
    j2 = {0, N - 3, N - 2, N - 1, N // 2 - 3, N // 2 - 2, N // 2 - 1, N // 2}
    for w in range(32, N, 32):
        j1 |= {w - 2, w - 1, w}
        j2 |= {w - 3, w - 2, w - 1, w}
    return tuple(sorted(a for a in j1 if 0 <= a < N)) + tuple(sorted(N + a for a in j2 if 0 <= a < N))


# id, N, units, samples, RNNWF_ENGINE while the handle is created (None: unset, "default"), the engine the pass must report, checked
# 16-chain blocks, probed slots (None: every J1 and J2 bond, wrap bonds included), what it is for.
#
# Engine and kernel of every case, read from the sources (crnn.hip: pack_image, with_launch, j1j2_on_device; split.hip: with_layout,
# riders, stack_split_available; rnnwf_api.hip: pick_nfull).  Unlike the positive GRU's flip pass the complex model chooses by width
# alone, whatever the batch: engine_split = not RNNWF_ENGINE=f32 and (one layer: NFULL <= 6, i.e. <= 100 units | stack:
# stack_split_available: NFULL 3 and <= 50 units).
#   * 50 units (cfg3-ragged, n66): NFULL 3, K-packed layout -> crnn_swap_pp_kernel, the ping-pong kernel, tiles of 32 items, 8 waves =
#     one workgroup on a CU, so tiles from 8 CUs on are walked in a second lap (test_gpu_crnn_swap_full.py says on which batch)
#   * cfg3-f32: crnn_swap_kernel<3, 4>, tiles of 16 items
#   * w36: NFULL 2, flat (crnn_swap_split_kernel MODE 1) | w37: NFULL 3 aligned, the ping-pong kernel | w52: NFULL 3 padded
#     (crnn_swap_split_kernel MODE 0) | w53, w68: NFULL 4, riders with the image in LDS (crnn_split_swap_stream) | w69, w100: NFULL 6,
#     riders streamed
#   * wide-128: NFULL 8 > 6 -> f32mfma, crnn_swap_kernel<8, 4> with the image read through L2 (GruLayout::SPILL)
#   * n258: 20 units, NFULL 1, flat crnn_swap_split_kernel; N > 256: the enumerate kernel's diagonal from global memory, 9 spin words,
#     j1j2_eloc_kernel does not clear the counters (the memset does, every call)
#   * cfg3-l2, stack-3: crnn_stack_swap - crnn_swap_pp_kernel<STACK> below, crnn_swap_pp_upper_kernel middle (three layers only) and top
#   * stack-64-20: H = 64, NFULL 4, no layer pipeline -> f32mfma, crnn_ml_swap_kernel<4, 2, 4>; the 20-unit layer padded to 64
# N = 34: bit 31 is the last of word 0, sites 32 and 33 lie in word 1; the mask starts at site 17.
# Checked blocks: fixed by the cost of the reference alone (float64 and four float32 realisations of every bond of the checked chains).
CASES = [
    ("cfg3-ragged", 40, (50,), 10007, None, "bf16x3", 24, None, "the benchmarked shape; ragged (its own samples fill 1 574 tiles of 32: the GPU test reaches the second lap on a further batch)"),
    ("cfg3-f32", 40, (50,), 10007, "f32", "f32mfma", 24, None, "crnn_swap_kernel, tiles of 16"),
    ("w36", 34, (36,), 2055, "bf16x3", "bf16x3", 12, None, "flat class: last width"),
    ("w37", 34, (37,), 2055, "bf16x3", "bf16x3", 12, None, "aligned class: first width"),
    ("w52", 34, (52,), 2055, "bf16x3", "bf16x3", 12, None, "padded class: last width"),
    ("w53", 34, (53,), 2055, "bf16x3", "bf16x3", 12, None, "riders, LDS-resident: first width"),
    ("w68", 34, (68,), 2055, "bf16x3", "bf16x3", 12, None, "riders, LDS-resident: last width"),
    ("w69", 34, (69,), 2055, "bf16x3", "bf16x3", 12, None, "riders, streamed: first width"),
    ("w100", 34, (100,), 2055, "bf16x3", "bf16x3", 12, None, "riders, streamed: last width"),
    ("wide-128", 34, (128,), 1030, None, "f32mfma", 12, None, "f32mfma, image through L2"),
    ("n66", 66, (50,), 1031, None, "bf16x3", 8, probe_slots(66), "third spin word; the tile scan's second 64-site chunk (lo = 64)"),
    ("n258", 258, (20,), 70, None, "bf16x3", 2, probe_slots(258), "diagonal from global memory, 9 words, counters cleared by memset"),
    ("cfg3-l2", 40, (50, 50), 10000, None, "bf16x3", 8, None, "layer pipeline (crnn_stack_swap), rec_start"),
    ("stack-3", 34, (50, 50, 50), 2055, "bf16x3", "bf16x3", 8, None, "first, middle and top kernel"),
    ("stack-64-20", 34, (64, 20), 2055, None, "f32mfma", 8, None, "f32 stack kernels, padded layer"),
]
CASE_IDS = [c[0] for c in CASES]
BLOCK = 16                         # checked chains are whole blocks of the base pass


def case(cid):
    return CASES[CASE_IDS.index(cid)]


def tile_of_engine(engine):
    """Items per swap tile: 32 on the bf16x3 engine (crnn_split_kernels.h), 16 on the f32-input MFMA (crnn_kernels.h)."""
    return 32 if engine == "bf16x3" else 16


def build_params(units, sharp=SHARP):
    return R.build_params("crnn", units, seed=SEED, sharp=sharp)


def wrap_slots(N):
    """The three bonds that exist only on the periodic chain: J1 of site N - 1, J2 of sites N - 2 and N - 1."""
    return np.array([N - 1, 2 * N - 2, 2 * N - 1])



def random_couplings(N):
    """J1 = 1 + 0.1 randn, J2 = 0.5 + 0.1 randn, Bz = 0.05 randn: no two bonds alike, so that a shifted bond index shows."""
    rng = np.random.RandomState(N)
    return 1.0 + 0.1 * rng.randn(N), 0.5 + 0.1 * rng.randn(N), 0.05 * rng.randn(N)


def one_hot_couplings(N, slot):
    """J = 1 on the bond of `slot`, everything else and Bz zero."""
    J = np.zeros(2 * N)
    J[slot] = 1.0
    return J[:N], J[N:], np.zeros(N)


# ---- connected configurations ------------------------------------------------------------------------------------------------------

class Connected:
    """The bonds with a non-zero coupling: slot, site, dist, lo, hi, coef (K,), in the reference's row order (J1 by site, then J2 by
    site); active (K, B): the bond is anti-aligned in the sample; diag (B,); count (B,) = 1 + anti-aligned bonds."""

    def __init__(self, slot, site, dist, lo, hi, coef, active, diag):
        self.slot, self.site, self.dist, self.lo, self.hi, self.coef, self.active, self.diag = slot, site, dist, lo, hi, coef, active, diag
        self.count = 1 + active.sum(axis=0)

    def of(self, b):
        """The bond list of sample b: (slot, lo, hi, coefficient) of its anti-aligned bonds."""
        return [(int(self.slot[k]), int(self.lo[k]), int(self.hi[k]), float(self.coef[k])) for k in np.flatnonzero(self.active[:, b])]


def connected(s, J1, J2, Bz, periodic=False, marshall=False, marshall_j2=False):
    """J1J2MatrixElements for every row of s (B, N), restated from oracle.estimators.j1j2_matrix_elements.  marshall_j2: defect (i)."""
    s = np.asarray(s).astype(np.int64)
    B, N = s.shape
    J1, J2, Bz = (np.asarray(a, dtype=np.float64) for a in (J1, J2, Bz))
    diag = (s - 0.5) @ Bz
    rows = []
    for dist, J in ((1, J1), (2, J2)):
        lim = N if periodic else N - dist
        for a in range(lim):
            t = (a + dist) % N
            if dist == 2 and J[a] == 0.0:
                continue                                     # (the reference skips a zero J2 in the diagonal too; a zero J1 adds 0)
            diag = diag + 0.25 * J[a] * np.where(s[:, a] == s[:, t], 1.0, -1.0)
            if J[a] != 0.0:
                sign = -1.0 if marshall and (dist == 1 or marshall_j2) else 1.0
                rows.append(((dist - 1) * N + a, a, dist, min(a, t), max(a, t), sign * J[a] / 2))
    if rows:
        slot, site, dist, lo, hi = (np.array([r[i] for r in rows], dtype=np.int64) for i in range(5))
        coef = np.array([r[5] for r in rows])
    else:
        slot = site = dist = lo = hi = np.zeros(0, dtype=np.int64)
        coef = np.zeros(0)
    return Connected(slot, site, dist, lo, hi, coef, s[:, lo].T != s[:, hi].T, diag)


def all_bonds(N):
    """(lo, hi) of the 2 N bond slots of the periodic chain."""
    a = np.arange(N)
    t1, t2 = (a + 1) % N, (a + 2) % N
    return np.concatenate([np.minimum(a, t1), np.minimum(a, t2)]), np.concatenate([np.maximum(a, t1), np.maximum(a, t2)])


def unwrapped(N):
    """Defect (j): `all_bonds` with (lo, hi) = (site, site + dist), no modulus; differs on the three wrap bonds."""
    a = np.arange(N)
    return np.concatenate([a, a]), np.concatenate([a + 1, a + 2])


def swapped_rows(s, lo, hi):
    """(K, B, N): s with the spins of sites lo[k], hi[k] exchanged - written out in full, for the from-site-0 oracle."""
    s = np.asarray(s)
    out = np.repeat(s[None], len(lo), axis=0)
    k = np.arange(len(lo))
    out[k, :, lo] = s[:, hi].T
    out[k, :, hi] = s[:, lo].T
    return out


# ---- log psi(s') - log psi(s) with shared prefixes, in any float type, with the defect knobs ---------------------------------------------

class _Cells:
    """step(x (B, 2), states) -> states': the GRU stack in the arithmetic `dtype`; site(out, n, N, num_up) -> (la, ph) (B, 2): log of
    the masked, normalised amplitudes and the phases of both spin values."""
    NAMES = F._Cells.NAMES

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
        self.Wa, self.ba = np.ascontiguousarray(cut(get("wf_dense_ampl/kernel"))[q]), get("wf_dense_ampl/bias")
        self.Wp, self.bp = np.ascontiguousarray(cut(get("wf_dense_phase/kernel"))[q]), get("wf_dense_phase/bias")
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
        return new

    def site(self, out, n, N, num_up):
        dt = self.dtype
        z = out @ self.Wa + self.ba
        e = np.exp(z - z.max(axis=1, keepdims=True))
        ampl = np.sqrt(e / e.sum(axis=1, keepdims=True))
        if n >= N / 2:
            up = num_up.astype(dt)
            base = dt(N // 2 - 1)
            act_up = (base - up >= 0).astype(dt)
            act_down = (base - (dt(n) - up) >= 0).astype(dt)
            ampl = ampl * np.stack([act_down, act_up], axis=1)
            ampl = ampl / np.sqrt(np.maximum((ampl * ampl).sum(axis=1, keepdims=True), dt(1e-30)))
        zp = out @ self.Wp + self.bp
        return np.log(ampl), dt(np.pi) * (zp / (dt(1) + np.abs(zp)))


def log_ratios(prm, s, bonds, dtype=np.float64, order=0, only=None, weights16=False, state16=False, word0=False, keep_hi=False,
               restart_shift=0, count_shift=0, lagged=False, return_own=False):
    """(K, B) complex128 d[k, b] = log psi(s_b with the spins of sites lo[k] < hi[k] flipped) - log psi(s_b), bonds = (lo, hi), for the
    (bond, chain) pairs of the mask `only` (K, B) (default: the anti-aligned ones, where flipping both is the exchange); nan elsewhere.
    One pass over the sites: at site n the own chains advance, the continuations started at lo < n advance with their own inputs, and
    those with lo = n start from the own state after site n with the other spin as their next input and the own head's term for it.
    hi >= N is never reached (defect (j)).  The knobs are the defect models of the module docstring.  return_own: also log psi(s) (B,)
    complex128."""
    dt = np.dtype(dtype).type
    s = np.asarray(s).astype(np.int64)
    B, N = s.shape
    lo, hi = (np.asarray(a, dtype=np.int64) for a in bonds)
    assert np.all(lo < hi) and np.all(lo >= 0) and np.all(lo < N)
    if only is None:
        only = s[:, lo].T != s[:, np.minimum(hi, N - 1)].T
    perm = np.argsort(lo, kind="stable")
    pk, pb = np.nonzero(np.asarray(only)[perm])              # the continuations, sorted by lo: bond perm[pk] of chain pb
    plo, phi = lo[perm][pk], hi[perm][pk]
    P = len(pk)
    cells = _Cells(prm, dt, order=order)
    fcells = _Cells(prm, dt, weights16=True, order=order) if weights16 else cells
    eye = np.eye(2, dtype=dt)
    ar = np.arange(B)
    seen = s[:, np.arange(N) & 31] if word0 else s           # what the continuation reads
    x = np.zeros((B, 2), dtype=dt)
    state = [np.zeros((B, w), dtype=dt) for w in cells.widths]
    fstate = [np.zeros((P, w), dtype=dt) for w in cells.widths]
    fx = np.zeros((P, 2), dtype=dt)
    fre, fim, bre, bim = np.zeros(P), np.zeros(P), np.zeros(P), np.zeros(P)
    fup = np.zeros(P, dtype=np.int64)
    pre, pim = np.zeros(B), np.zeros(B)
    own_up = np.zeros(B, dtype=np.int64)
    m = 0                                                    # continuations started so far: 0 .. m - 1
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        for n in range(N):
            before = state
            state = cells.step(x, state)
            la, ph = cells.site(state[-1], n, N, own_up)
            la, ph = la.astype(np.float64), ph.astype(np.float64)
            if m:
                new = fcells.step(fx[:m], [f[:m] for f in fstate], lagged)
                for f, v in zip(fstate, new):
                    f[:m] = two_bf16_terms(v) if state16 else v
                fla, fph = fcells.site(fstate[-1][:m], n, N, fup[:m])
                sig = seen[pb[:m], n] ^ ((phi[:m] == n) & (not keep_hi)).astype(np.int64)
                am = np.arange(m)
                fre[:m] += fla[am, sig].astype(np.float64)
                fim[:m] += fph[am, sig].astype(np.float64)
                fup[:m] += sig
                fx[:m] = eye[sig]
                if restart_shift < 0:
                    # one site late: the continuations of lo = n - 1 take the own state after site n; their flipped spin never entered
                    j = np.flatnonzero(plo[:m] == n - 1)
                    for f, v in zip(fstate, state):
                        f[j] = v[pb[j]]
                    fre[j] = bre[j] + la[pb[j], sig[j]]
                    fim[j] = bim[j] + ph[pb[j], sig[j]]
            new_m = int(np.searchsorted(plo, n, side="right"))
            if new_m > m:
                c = pb[m:new_m]
                other = 1 - s[c, n]                          # the swap base is the base pass's: the chain's own spins
                fed = 1 - seen[c, n]
                bre[m:new_m] = pre[c] + la[c, other]
                bim[m:new_m] = pim[c] + ph[c, other]
                fre[m:new_m], fim[m:new_m] = bre[m:new_m], bim[m:new_m]
                for f, v in zip(fstate, before if restart_shift > 0 else state):
                    f[m:new_m] = v[c]
                fx[m:new_m] = eye[fed]
                fup[m:new_m] = own_up[c] + fed + count_shift
                m = new_m
            pre = pre + la[ar, s[:, n]]
            pim = pim + ph[ar, s[:, n]]
            own_up = own_up + s[:, n]
            x = eye[s[:, n]]
        d = np.full((len(lo), B), complex(np.nan, np.nan))
        d[perm[pk], pb] = (fre - pre[pb]) + 1j * (fim - pim[pb])
    return (d, pre + 1j * pim) if return_own else d


def oracle_log_ratios(prm, s, lo, hi, dtype=np.float64):
    """(K, B) complex128 from site 0: M.crnn_log_amplitude on the written-out exchanged rows of the anti-aligned (bond, chain) pairs
    minus on the rows themselves; nan elsewhere."""
    p = R.cast(prm, dtype)
    s = np.asarray(s)
    anti = s[:, lo].T != s[:, hi].T
    rows = swapped_rows(s, lo, hi)[anti]
    out = np.full(anti.shape, complex(np.nan, np.nan))
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        own = M.crnn_log_amplitude(p, s, SCOPE, dtype=dtype).astype(np.complex128)
        out[anti] = M.crnn_log_amplitude(p, rows, SCOPE, dtype=dtype).astype(np.complex128)
    return out - own[None]


# ---- reference and yardstick of a set of checked chains ----------------------------------------------------------------------------------

class Reference:
    """What the judges need of a case: the checked chains (global indices `chains` of a batch of `ns`, configurations `s`), of all 2 N
    bond slots of the periodic chain lo, hi, anti (2 N, B) (the bond is anti-aligned), d64 (2 N, B), dev (2 N, B) = max over the four
    float32 realisations of |d32 - d64| (nan where one is not finite), r = exp(d64) (0 where aligned)."""

    def __init__(self, prm, s, chains=None, ns=None, tile=32):
        t0 = time.time()
        self.s = np.asarray(s).astype(np.int64)
        self.B, self.N = self.s.shape
        self.tile = tile
        self.chains = np.arange(self.B) if chains is None else np.asarray(chains)
        self.ns = int(self.chains.max()) + 1 if ns is None else ns
        self.lo, self.hi = all_bonds(self.N)
        self.anti = self.s[:, self.lo].T != self.s[:, self.hi].T
        self.d64 = log_ratios(prm, self.s, (self.lo, self.hi), np.float64)
        self.d32 = [log_ratios(prm, self.s, (self.lo, self.hi), np.float32, order=o) for o in ORDERS]
        with np.errstate(invalid="ignore"):
            self.dev = np.max([np.abs(d - self.d64) for d in self.d32], axis=0)
            self.r = np.where(self.anti, np.exp(np.where(self.anti, self.d64, 0.0)), 0.0)
        self.up_lo = np.concatenate([np.zeros((self.B, 1), dtype=np.int64), np.cumsum(self.s, axis=1)], axis=1)[:, self.lo].T      # (2 N, B) ups below lo
        self.seconds = time.time() - t0

    def yardstick(self, slots):
        """y (B,) over the anti-aligned bonds among `slots`; nan where a float32 realisation is not finite."""
        slots = np.asarray(slots)
        a = self.anti[slots]
        dev = np.where(a, self.dev[slots], 0.0)
        big = np.where(a, np.abs(self.d64[slots]), 0.0)
        return np.maximum(dev.max(axis=0), EPS32 * big.max(axis=0))      # np.maximum and max propagate nan

    def energies(self, con):
        """(e_ref (B,) complex128, sum_k |H_k| |r_k| (B,)) of the couplings behind `con` = connected(self.s, ...)."""
        assert np.array_equal(con.active, self.anti[con.slot])
        hr = con.coef[:, None] * self.r[con.slot]
        return con.diag + hr.sum(axis=0), np.abs(hr).sum(axis=0)


def where(ref, slot, b):
    """Coordinates of a (bond, checked chain) for a failure message."""
    N, lo, hi = ref.N, int(ref.lo[slot]), int(ref.hi[slot])
    rank = int(ref.anti[slot, :b].sum())                     # among the CHECKED chains only where the batch holds more: a lower bound
    first = int(ref.chains[0]) == 0 and np.array_equal(ref.chains[:b + 1], np.arange(b + 1))
    return ("sample %d, bond slot %d (J%d bond of site %d: lo %d in spin word %d, hi %d in spin word %d), %d ups below lo, tile (lo %d, "
            "item %s%d // %d = %s%d)" % (ref.chains[b], slot, 1 if slot < N else 2, slot % N, lo, lo // 32, hi, hi // 32, ref.up_lo[slot, b],
                                         lo, "" if first else ">= ", rank, ref.tile, "" if first else ">= ", rank // ref.tile))


def measure_probes(E, ref, slots):
    """E (P, B) complex: the energies the one-hot probe of each of `slots` returned on the checked chains.  The figures judge_probes
    asserts on."""
    slots = np.asarray(slots)
    E = np.asarray(E).astype(np.complex128)
    N = ref.N
    y = ref.yardstick(slots)
    a = ref.anti[slots]
    diag = np.where(a, -0.25, 0.25)                          # J = 1 on the one bond, Bz = 0
    v_ref = ref.r[slots]
    e_ref = diag + 0.5 * v_ref
    v = 2.0 * (E - diag)
    bound = np.abs(v_ref) * FACTOR * y[None, :] + 2.0 * EPS32 * (np.abs(e_ref.real) + np.abs(e_ref.imag))
    err = np.abs(v - v_ref)
    with np.errstate(invalid="ignore", divide="ignore"):
        over = np.where(a, err / bound, 0.0)
    over = np.where(np.isfinite(over), over, np.inf)
    w = np.unravel_index(int(np.argmax(over)), over.shape)
    exact = ~a & ((E.real != diag) | (E.imag != 0.0))
    return dict(N=N, B=ref.B, probes=len(slots), ratios=int(a.sum()), finite=bool(np.all(np.isfinite(E))), over=float(over[w]),
                worst=(int(slots[w[0]]), int(w[1])), err=float(err[w]), bound=float(bound[w]), inexact=np.argwhere(exact),
                y_min=float(np.nanmin(y)), y_max=float(np.max(y)), r_max=float(np.abs(v_ref).max()), slots=slots)


def judge_probes(E, ref, slots, label=""):
    m = measure_probes(E, ref, slots)
    assert m["finite"], "%s non-finite values" % label
    y = ref.yardstick(slots)
    assert np.all(np.isfinite(y)), ("%s chains %s have no yardstick: a float32 realisation of the reference is not finite there" %
                                    (label, ref.chains[~np.isfinite(y)].tolist()))
    assert m["over"] <= 1.0, ("%s %s: |v - v_ref| = %.3e > %.3e" % (label, where(ref, *m["worst"]), m["err"], m["bound"]))
    if len(m["inexact"]):
        p, b = m["inexact"][0]
        raise AssertionError("%s %s: the bond is aligned, yet E = %r is not exactly the diagonal" % (label, where(ref, int(m["slots"][p]), int(b)), E[p][b]))
    return m


def measure_energies(e, ref, con):
    """e (B,) complex: j1j2_eloc of the checked chains under the couplings behind `con`."""
    e = np.asarray(e).astype(np.complex128)
    e_ref, mag = ref.energies(con)
    y = ref.yardstick(con.slot)
    bound = mag * (FACTOR * y + EPS32) + EPS32 * np.abs(e_ref) + ref.N * EPS64 * (np.abs(con.diag) + mag)
    err = np.abs(e - e_ref)
    with np.errstate(invalid="ignore"):
        over = err / bound
    over = np.where(np.isfinite(over), over, np.inf)
    w = int(np.argmax(over))
    return dict(N=ref.N, B=ref.B, finite=bool(np.all(np.isfinite(e))), over=float(over[w]), worst=w, err=float(err[w]), bound=float(bound[w]),
                y=y, r_max=float(np.abs(ref.r[con.slot]).max()), ncon=int(con.count.sum()))


def judge_energies(e, ref, con, label=""):
    m = measure_energies(e, ref, con)
    assert m["finite"], "%s non-finite values" % label
    assert np.all(np.isfinite(m["y"])), ("%s chains %s have no yardstick: a float32 realisation of the reference is not finite there" %
                                         (label, ref.chains[~np.isfinite(m["y"])].tolist()))
    b = m["worst"]
    assert m["over"] <= 1.0, ("%s sample %d (bonds (slot, lo, hi, coef) %s): |E - ref| = %.3e > %.3e" %
                              (label, ref.chains[b], con.of(b), m["err"], m["bound"]))
    return m


def assert_sharp(ref, label=""):
    r = float(np.abs(ref.r).max())
    assert r > 3.0, "%s the largest amplitude ratio of the checked chains is %.3g <= 3: the weights are not sharp" % (label, r)
    return r


def probe_line(label, m, seconds=None):
    return ("%s N %d: %d probes, %d ratios of %d chains; max ratio error / bound %.3f (%.2e of %.2e, slot %d chain %d)  yardstick %.1e .. "
            "%.1e  max |r| %.3g%s" % (label, m["N"], m["probes"], m["ratios"], m["B"], m["over"], m["err"], m["bound"], m["worst"][0],
                                      m["worst"][1], m["y_min"], m["y_max"], m["r_max"], "" if seconds is None else "  reference %.1f s" % seconds))


def energy_line(label, m):
    return "%s max E error / bound %.3f (%.2e of %.2e, chain %d)" % (label, m["over"], m["err"], m["bound"], m["worst"])


# ---- probes and energies assembled from a matrix of log-ratios: what an evaluation (honest or defective) would have returned ----------

def probes_from(d, ref, slots, output32=True):
    """(P, B) the one-hot probes' E = diag + 1/2 exp(d) (the diagonal alone where the bond is aligned), rounded to complex64."""
    slots = np.asarray(slots)
    a = ref.anti[slots]
    with np.errstate(invalid="ignore", over="ignore"):
        E = np.where(a, -0.25 + 0.5 * np.exp(np.where(a, d[slots], 0.0)), 0.25 + 0.0j)
    return E.astype(np.complex64).astype(np.complex128) if output32 else E


def energies_from(d, ref, con, output32=True):
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.where(con.active, np.exp(np.where(con.active, d[con.slot], 0.0)), 0.0)
    e = con.diag + (con.coef.astype(np.float32).astype(np.float64)[:, None] * r).sum(axis=0)
    return e.astype(np.complex64).astype(np.complex128) if output32 else e


# ---- defect models that edit a clean matrix d (2 N, B); the others are knobs of `log_ratios` and `connected` -----------------------------

def _middle_pair(ref, slots):
    """(slot, its successor among `slots`, chain): the middle one of the pairs of consecutive probed slots both anti-aligned in a chain."""
    slots = np.asarray(slots)
    both = np.argwhere(ref.anti[slots[:-1]] & ref.anti[slots[1:]])
    p, b = both[len(both) // 2]
    return int(slots[p]), int(slots[p + 1]), int(b)


def inject_neighbour(ref, d, slots):
    """(g) one contribution carries the value of the next probed bond."""
    k, k1, b = _middle_pair(ref, slots)
    out = d.copy()
    out[k, b] = d[k1, b]
    return out


def inject_zero(ref, d, slots):
    """(h) one contribution left at zero: exp(d) = 0."""
    k, _, b = _middle_pair(ref, slots)
    out = d.copy()
    out[k, b] = complex(-np.inf, 0.0)
    return out


def inject_ragged(ref, d):
    """(k) in a ragged last tile the last valid item takes its neighbour's value: the last checked chain the one before's, on the bonds
    both have.  None where the checked chains do not end in the batch's last two chains of a ragged block."""
    if ref.ns % BLOCK < 2 or ref.chains[-1] != ref.ns - 1 or ref.chains[-2] != ref.ns - 2:
        return None
    both = ref.anti[:, -1] & ref.anti[:, -2]
    out = d.copy()
    out[both, -1] = d[both, -2]
    return out
