"""One case per STACK ROW of the kernel table for the Pauli and the region-Renyi passes of stacked GRU layers (rnnwf_pauli_step_stack,
rnnwf_renyi2_regions_stack: csrc/stack_chain_kernels.h).  TEST INFRASTRUCTURE ONLY; validated by tests/test_stack_rows_reference.py,
used by tests/test_gpu_stack_rows.py.

The rows.  csrc/shapes.h instantiates the stack kernels once per row KR<T, NL, NFULL, WAVES> with NL >= 2 of `GruKernels` (the lines
`KR<double, 2, 1, 4> ... KR<double, 4, 4, 4>` and `KR<float, 2, 1, 4> ... KR<float, 4, 6, 4>`): 12 float64 and 15 float32 rows.
ROW_WAVES restates their waves per workgroup; test_stack_rows_reference.py reads shapes.h and asserts that CASES reaches every row with
the waves written here.  spill_of restates csrc/layout.h's `MlSpill<NFULL, NL, T>::pick()` from the byte sizes of the lines
`struct GruLayout` (OFF_AVEC .. BYTES) and `struct UpperLayout` (SZ_AVEC .. BYTES): how many of the upper layers' weight images stay
out of the 160 KB of LDS and are read through L2.  0 < spill < NL - 1 is a partial spill: one kernel body addresses both kinds of layer.

CASES: per row one stack of equal widths, gradient_classes_reference.CLASS_WIDTHS[NFULL][(NL + j) % 2] (first and last width of the
class alternating over the rows, so both ends of every class occur for each element type), and two stacks of unequal widths per
element type.  Shapes are the smallest at which these kernels can still go wrong, not the workload's: N = 40 (40 x 1 float32, 8 x 5
raster float64: two words of packed spins with room for restarts well inside the second), 37 samples for the Pauli pass and 19 pairs
for the Renyi pass (two full 16-chain blocks and a ragged one).  The 38 chains of a case are sample(38, seed=111, step=0); the Pauli
pass takes the first 37 (the same chains as sample(37, ...): the uniforms are indexed by chain).

Operators: hamiltonian(40) = pauli_stack_reference.hamiltonian("mixed", 40) and strings whose first flipped site lies inside the second
word (X on 35 and 38, on 33 and 37, on 36 and 39) and exactly on site 32; regions(shape) = renyi_stack_reference.boundary_regions(40),
small_regions(shape) and two regions that start inside the second word.

Bounds, none from a kernel under test: float64 1e-11 N; float32, BOTH passes, renyi_reference.f32_bound(dev32, N) with dev32 the
float32 NumPy oracle's deviation from the float64 brute force on the same chains and masks; E_loc, per-term sums and Renyi sums as
pauli_stack_reference.judge and renyi_stack_reference.judge_sums derive them from that.  The weight seeds (sharp = 3) are chosen on
the CPU from oracle-drawn chains (oracle.philox + the oracle's sampler) so that every case meets the judges' non-triviality
conditions - ratios spread (std > 0.2 mean), max |log r| > 0.1 and a share >= 1/4 above 0.01 - and never by the outcome of a GPU run.

Also here: the site-resolved form the kernels use, for both passes (tail_form: every layer restarted from the chain's own states
before the mask's first site f), with the defects of renyi_stack_reference.DEFECTS and two more (DEFECTS below), a float32 stack in
another summation order (other_order_scorer) and the restart through float32-rounded states (round_restart=True).
"""
import collections
import re

import numpy as np

import gradient_classes_reference as GC
import pauli_stack_reference as SR
import renyi_regions_reference as G
import renyi_stack_reference as S
from oracle import models as M
from oracle import philox
from rnnwavefunctions_amd import observables as O

SCOPE = S.SCOPE
N = 40
SHAPE = {False: (40, 1), True: (8, 5)}
NS, NPAIRS = 37, 19
SEED = 111                       # of the chains: sample(38, seed=SEED, step=0)
LDS = 160 * 1024

# waves per workgroup of the stack rows, restated from shapes.h: 4 unless listed
ROW_WAVES = {("float", 2, 3): 8, ("float", 3, 2): 8, ("float", 3, 3): 8, ("double", 2, 2): 8}
NFULLS = {"float": (1, 2, 3, 4, 6), "double": (1, 2, 3, 4)}

Case = collections.namedtuple("Case", "f64 shape units T NL NFULL WAVES spill seed")


# ---- layout.h restated ---------------------------------------------------------------------------------------------------------------

def gru_layout_bytes(size, nfull, nout=1):
    """GruLayout<T, NFULL, NOUT>::BYTES, sizeof(T) = size"""
    kt, nt, vw = 4 * nfull + 1, 3 * nfull + 1, 16 // size
    ng = (kt - 1) // vw
    off_arem = nt * ng * 64 * 16
    off_binit = off_arem + nt * 64 * size
    off_xc = off_binit + 3 * (nt * 16 + 4) * size
    wd_q = ((nout * kt + 3) // 4) * 4
    off_wd = off_xc + 3 * ((nfull + 1) * 16 + 4) * size
    off_bd = off_wd + 4 * wd_q * size
    return ((off_bd + 32 + 15) // 16) * 16


def upper_layout_bytes(size, nfull):
    """UpperLayout<NFULL, T>::BYTES"""
    kt, nt, nt2, vw = 4 * nfull + 1, 3 * nfull + 1, 4 * nfull + 1, 16 // size
    ng = (kt - 1) // vw
    off_b = 2 * (nt * ng * 64 * 16 + nt * 64 * size)
    return ((off_b + nt2 * 16 * size + 15) // 16) * 16


def spill_of(T, NL, nfull):
    """MlSpill<NFULL, NL, T>::value: the number of top layers whose image is read through L2"""
    size = 8 if T == "double" else 4
    l0, up = gru_layout_bytes(size, nfull), upper_layout_bytes(size, nfull)
    assert l0 <= LDS
    for s in range(NL):
        if l0 + (NL - 1 - s) * up <= LDS:
            return s
    return NL - 1


def nfull_of(T, units):
    return next(nf for nf in NFULLS[T] if 16 * nf + 4 >= max(units))


def shapes_h_stack_rows(text):
    """{(T, NL, NFULL): WAVES} of the rows with NL >= 2 of `using GruKernels = KernelTable<...>;` in the text of csrc/shapes.h"""
    block = re.search(r"using GruKernels = KernelTable<(.*?)>>;", text, re.S).group(1)
    rows = {}
    for T, nl, nf, w in re.findall(r"KR<(\w+), (\d+), (\d+), (\d+)", block):
        if int(nl) >= 2:
            assert (T, int(nl), int(nf)) not in rows
            rows[T, int(nl), int(nf)] = int(w)
    return rows


# ---- the case table ------------------------------------------------------------------------------------------------------------------
# weight seeds: the first of 111, 112, ... at which the case meets the non-triviality conditions of both judges on oracle-drawn chains
# with a margin (std > 0.3 mean, max |log r| > 0.2, share >= 0.3) and the honest float32 evaluations stay below half the float32 bound
# (test_stack_rows_reference.py asserts the conditions themselves); (float64, units) -> seed, 111 unless listed
WSEED = {(False, (69, 69)): 112, (False, (53, 53, 53)): 112, (False, (100, 100, 100)): 112, (False, (17, 17, 17, 17)): 112,
         (False, (36, 36, 36, 36)): 112, (False, (69, 69, 69, 69)): 113, (True, (53, 53, 53)): 112}
UNEQUAL = [(37, 20, 53), (68, 21)]


def row_case(f64, units):
    T = "double" if f64 else "float"
    NL, nf = len(units), nfull_of(T, units)
    return Case(f64, SHAPE[f64], tuple(units), T, NL, nf, ROW_WAVES.get((T, NL, nf), 4), spill_of(T, NL, nf), WSEED.get((f64, tuple(units)), 111))


def _cases():
    out = []
    for f64 in (False, True):
        T = "double" if f64 else "float"
        for NL in (2, 3, 4):
            for j, nf in enumerate(NFULLS[T]):
                out.append(row_case(f64, (GC.CLASS_WIDTHS[nf][(NL + j) % 2],) * NL))
        out += [row_case(f64, u) for u in UNEQUAL]
    return out


CASES = _cases()


def case_id(c):
    return "%s-%s" % ("f64" if c.f64 else "f32", "x".join(str(u) for u in c.units))


def row_label(c):
    return "[%s] row (%s, %d, %d) %d waves, spill %d of %d upper" % (case_id(c), c.T, c.NL, c.NFULL, c.WAVES, c.spill, c.NL - 1)


def case_of(f64, NL, nfull, equal=True):
    return next(c for c in CASES if (c.f64, c.NL, c.NFULL) == (f64, NL, nfull) and (len(set(c.units)) == 1) == equal)


def weights(c, seed=None):
    return S.weights(c.f64, c.units, seed=c.seed if seed is None else seed)


def oracle_chains(c, prm, n=2 * NPAIRS, seed=SEED, step=0):
    """the chains sample(n, seed, step) draws, from the oracle's own sampler on the same uniforms"""
    u = philox.uniforms(seed, step, 0, n, N)
    return M.prnn_sample(prm, N, u, SCOPE, dtype=np.float64 if c.f64 else np.float32)[0].astype(np.int32)


# ---- operators -----------------------------------------------------------------------------------------------------------------------

def hamiltonian(n=N):
    terms = SR.hamiltonian("mixed", n).terms + [(0.3, [("X", 35), ("X", 38)]), (0.22, [("X", 32)]), (-0.27, [("X", 33), ("Z", 20), ("X", 37)]),
                                               (0.18, [("X", 36), ("X", 39)])]
    return O.Hamiltonian(n, terms)


def flip_masks(ham):
    return O.group_by_mask(ham.flip)[0]


def regions(shape):
    """(names, masks (R, N))"""
    n = shape[0] * shape[1]
    both = S.boundary_regions(n) + S.small_regions(*shape) + [("interval 33..36", S.mask_of(n, range(33, 36))), ("sites 36 and 38", S.mask_of(n, [36, 38]))]
    names, masks = zip(*both)
    return list(names), np.stack(masks)


def first_sites(masks, paired):
    """the first site f of every mask as the kernels see it (PAIRED: of the mask normalised so that site 0 is not in it)"""
    return [G.normalise(m)[1] if paired else int(np.flatnonzero(m)[0]) for m in np.asarray(masks)]


# ---- brute force in any scorer ---------------------------------------------------------------------------------------------------------

def scorer(prm, dtype=np.float64):
    return SR.scorer(prm, dtype)


def pauli_log_ratio(log_p, samples, masks):
    """(M, ns) 1/2 [log P(sigma ^ F) - log P(sigma)]: every flipped configuration written out and scored from site 0, in one batch"""
    samples, masks = np.asarray(samples), np.asarray(masks)
    flipped = (samples[None, :, :] ^ masks[:, None, :].astype(samples.dtype)).reshape(-1, samples.shape[1])
    return 0.5 * (log_p(flipped).reshape(len(masks), len(samples)) - log_p(samples)[None, :])


def renyi_log_ratio(log_p, pairs, masks):
    return G.log_ratio_regions(log_p, np.asarray(pairs), np.asarray(masks))


def other_order_scorer(prm, dtype=np.float32, parts=3):
    """log P of the stack with every gate and candidate sum of every layer accumulated in ANOTHER order than oracle.models.gru_cell:
    input and hidden products separately, the hidden one in `parts` slices of the hidden index added last to first, sigmoid as
    1/2 (1 + tanh(x/2)), log-softmax as z - logaddexp.  The same function of the parameters; in float32 a second, differently rounded
    evaluation (renyi_reference.log_prob_other_order is the one-layer form)."""
    p = {k: np.asarray(v, dtype=dtype) for k, v in prm.items()}
    NL = M.num_gru_layers(p, SCOPE)
    Wd, bd = p[SCOPE + "/wf_dense/kernel"], p[SCOPE + "/wf_dense/bias"]
    half, one = dtype(0.5), dtype(1)

    def cell(x, h, layer):
        pre = SCOPE + "/" + M.GRU % layer
        Wg, bg = p[pre + "gates/kernel"], p[pre + "gates/bias"]
        Wci, bci = p[pre + "candidate/input_projection/kernel"], p[pre + "candidate/input_projection/bias"]
        Wch, bch = p[pre + "candidate/hidden_projection/kernel"], p[pre + "candidate/hidden_projection/bias"]
        H, nin = h.shape[1], x.shape[1]
        cuts = np.linspace(0, H, parts + 1).astype(int)

        def hidden(W):
            acc = np.zeros((len(h), W.shape[1]), dtype=dtype)
            for k in range(parts - 1, -1, -1):
                acc = acc + h[:, cuts[k]:cuts[k + 1]] @ W[cuts[k]:cuts[k + 1]]
            return acc
        g = (bg + hidden(Wg[nin:])) + x @ Wg[:nin]
        g = half * (one + np.tanh(half * g))
        r, u = g[:, :H], g[:, H:]
        c = np.tanh(r * (bch + hidden(Wch)) + (x @ Wci + bci))
        return u * h + (one - u) * c

    def log_p(x):
        x = np.asarray(x)
        B, n = x.shape
        states = M._zero_states(p, SCOPE, B, dtype)
        inp = np.zeros((B, 2), dtype=dtype)
        lp = np.zeros(B)
        for k in range(n):
            for layer in range(NL):
                states[layer] = cell(inp if layer == 0 else states[layer - 1], states[layer], layer)
            z = (states[-1] @ Wd + bd).astype(np.float64)
            lp += z[np.arange(B), x[:, k]] - np.logaddexp(z[:, 0], z[:, 1])
            inp = np.eye(2, dtype=dtype)[x[:, k]]
        return lp
    return log_p


# ---- the site-resolved form of the stack kernels, both passes, with defects --------------------------------------------------------------

DEFECTS = dict(S.DEFECTS, layer_image_swapped="layer l >= 1 runs on another upper layer's weight image", restart_one_row_late="states restored from row f, not f - 1")
PAULI_DEFECTS = ("layer_below", "mask_word_0", "mask_shifted", "layer_image_swapped", "restart_one_row_late")      # the others need a partner


def swapped_images(prm):
    """the upper layers' parameters rotated among themselves: layer l >= 1 takes those of layer l + 1 (the top one: layer 1's)"""
    NL = M.num_gru_layers(prm, SCOPE)
    assert NL >= 3, "two layers have one upper image: nothing to swap"
    out = dict(prm)
    for l in range(1, NL):
        src = l + 1 if l + 1 < NL else 1
        for k in prm:
            if k.startswith(SCOPE + "/" + M.GRU % l):
                out[k] = prm[SCOPE + "/" + M.GRU % src + k[len(SCOPE + "/" + M.GRU % l):]]
                assert out[k].shape == prm[k].shape, "layer_image_swapped needs layers of equal width"
    return out


def tail_form(prm, chains, masks, paired, defect=None, dtype=np.float64, round_restart=False):
    """log r of every mask as stack_chain_kernels.h computes it.  f = the mask's first site (PAIRED: of the normalised mask); f >= 1:
    EVERY layer's state restored from the chain's own states before site f (row f - 1), the chain's own spin f - 1 fed, the changed
    chain (own ^ mask; PAIRED: the partner's spin on the mask) teacher-forced over f..N-1; f = 0 (Pauli only): all N sites from the zero
    states.  log r = 1/2 (tail - suffix) (PAIRED: summed over both chains of the pair), suffix = the chain's own terms from f.
    Returns (M, ns) or, PAIRED, (R, npairs).  defect: one of DEFECTS; round_restart: the restored states rounded through float32."""
    chains = np.asarray(chains)
    n = chains.shape[1]
    prm = S.R.to64(prm) if dtype == np.float64 else S.R.to32(prm)
    tail_prm = swapped_images(prm) if defect == "layer_image_swapped" else prm
    own, st = S.run_stack(prm, chains, dtype)
    partner = chains.reshape(-1, 2, n)[:, ::-1].reshape(-1, n) if paired else None
    # rows of the partner's states: chain 2p <-> 2p + 1
    swap = np.arange(len(chains)) ^ 1
    out = np.zeros((len(masks), len(chains)))
    for k, mask in enumerate(np.asarray(masks)):
        if paired:
            m, f = G.normalise(mask)
            if f == 0:
                continue
        else:
            m, f = np.asarray(mask).astype(np.int64), int(np.flatnonzero(mask)[0])
        if defect == "mask_shifted":
            m = np.concatenate([[0], m[:-1]])
        elif defect == "mask_word_0":
            m = m[np.arange(n) & 31]
        elif defect == "own_on_A":
            m = np.zeros(n, dtype=np.int64)
        in_m = m.astype(bool)[None, :]
        changed = np.where(in_m, partner, chains) if paired else chains ^ m[None, :].astype(chains.dtype)
        if f == 0:
            out[k] = 0.5 * (S.run_stack(tail_prm, changed, dtype)[0].sum(axis=1) - own.sum(axis=1))
            continue
        start = st[f if defect == "restart_one_row_late" else f - 1]
        if defect == "partner_checkpoint":
            start = [h[swap] for h in start]
        if defect == "layer_below":
            start = [start[0]] + [start[l - 1] for l in range(1, len(start))]
        if round_restart:
            start = [h.astype(np.float32).astype(dtype) for h in start]
        tail = S.run_stack(tail_prm, changed, dtype, states=start, spin_in=chains[:, f - 1], n0=f)[0].sum(axis=1)
        out[k] = 0.5 * (tail - own[:, f:].sum(axis=1))
    return out[:, 0::2] + out[:, 1::2] if paired else out


# ---- a case's references ---------------------------------------------------------------------------------------------------------------

def pauli_tol(c, ref_lr, lr32):
    """(tol, dev32, how): the log-ratio bound of the case's element type"""
    if c.f64:
        return S.f64_bound(N), 0.0, "1e-11 N"
    dev32 = float(np.abs(np.asarray(lr32) - ref_lr).max())
    bound, capped = S.f32_bound(dev32, N)
    return bound, dev32, "capped" if capped else "16 x dev32 %.2e" % dev32


def spread(ref_lr):
    """std / mean of the ratios r = exp(log r): the Pauli cases require > 0.2"""
    with np.errstate(over="ignore"):
        r = np.exp(ref_lr)
    return float(r.std() / r.mean())


def judge_renyi(label, got, ref, ref32, c, names, echo=print):
    """renyi_stack_reference.judge, its failure naming region, pair, chains and 16-chain block"""
    got, ref = np.asarray(got), np.asarray(ref)
    bound = S.f64_bound(N) if c.f64 else S.f32_bound(float(np.abs(np.asarray(ref32) - ref).max()), N)[0]
    d = np.abs(got - ref)
    r, p = np.unravel_index(int(np.argmax(d)), d.shape)
    assert np.all(np.isfinite(got)) and d[r, p] <= bound, "%s: region %d (%s), pair %d (chains %d, %d; block %d): |log r - ref| = %.3e > %.3e" % (
        label, r, names[r], p, 2 * p, 2 * p + 1, p // 8, d[r, p], bound)
    res = S.judge(label, got, ref, ref32, c.f64, N, echo=echo)
    res.update(region=int(r), pair=int(p))
    return res
