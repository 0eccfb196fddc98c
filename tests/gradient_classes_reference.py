"""Case table and reference helpers of tests/test_gpu_gradient_classes.py and tests/test_gradient_classes_reference.py: one case at
least for EVERY gradient kernel class, at the smallest shapes at which those kernels can still go wrong.  TEST INFRASTRUCTURE ONLY.

The classes, read from the code (this file restates the few integer expressions it needs and names where each stands):

  rnnwf_api.hip: pick_nfull     NFULL = the smallest of 1, 2, 3, 4, (5: 2D RNN only), 6, 8, 12, 16 with 16 NFULL + 4 >= widest layer;
                                float64 GRU <= 6 (100 units), 2D RNN <= 5 (84 units), f32 GRU <= 16 (260 units)
  rnnwf_api.hip: rnnwf_create   stacks: 2..4 layers, GRU families only, f32 <= 100 units, float64 <= 68 units
  grad.hip: gru_widths          NFULL 1, 2, 3, 4: every family and layer count; 6: f32 any layer count, float64 one layer;
                                8, 12, 16: f32, one layer.  (Its own refusal is unreachable: rnnwf_create refuses those stacks first.)
  grad.hip: GLaunch::WIDE       the kernels of grad_wide.hip: f32 NFULL 8, 12, 16 and the float64 GRU's NFULL 6
  grad.hip: GLaunch::PAIR_OK    not WIDE, float, GradPair<T, NFULL, NOUT>::FITS - see pair_fits() below: NFULL 1, 2, 3 of the three f32
                                families, one layer or layer 0 of a stack; taken while ceil(ns / 16) <= 2 x CUs and not RNNWF_NO_COOP
  mdrnn.hip: with_md_width      NFULL 1..5 (to 20, 36, 52, 68, 84 units), remainder H - 16 NFULL
  the parity-symmetric model    is MODEL_GRU1D_PARITY on the positive GRU's classes, each run twice per gradient (grad.hip: launch)

A width class NFULL covers 16 (previous NFULL) + 5 .. 16 NFULL + 4 units: CLASS_WIDTHS has its first and last width.  Class 1 spans
1 .. 20: its "first" width here is 17, the smallest with a full 16-row tile AND a remainder unit; 6 units (no full tile) is a case too.

Shapes: 33 sites (the second spin word holds one spin), 34 for the complex model (U(1) needs an even length), 11 x 3 / 17 x 2 rasters
for the float64 GRU, 7 x 5 for the 2D RNN (zig-zag path, two words); 40 samples = two full 16-chain blocks and a ragged one of 8.
The chain-length cases (N = 1, 2, 4, 33, 65 on the 20-unit class) share 37 samples: with 40 every N x ns is a multiple of 4, and the
weight-gradient product (tn_gemm.h) pads the last k-group of four rows only where it is not - 37 x 4 = 148 rows is the multiple,
37, 74, 1221 and 2405 rows are not.

The bound is autograd_reference.verdict's, 16 x the float32-vs-float64 autograd deviation per tensor in both norms (x 2^-29 for the
float64 families), with ONE floor under the yardstick (rounding_floor): at 40 samples the float32 autograd deviation of a small tensor
can collapse far below one ulp of what is summed.  The floor is the expression of tests/test_gpu_sr.py's tie bound,
N x unit round-off of the model's type x max_k sum_s |w_s d log psi_s / d theta_k| over the tensor, relative to the tensor's
reference maximum, from the float64 reference's per-sample derivatives.  It is used for both norms as it stands (for the l2 norm that
is the tighter reading: ||d||_2 / ||g||_2 of an error of that size per element can reach sqrt(elements) x it).
"""
import collections
import time

import numpy as np
import torch

import autograd_reference as A
from rnnwavefunctions_amd import params as P

SCOPE = A.SCOPE
HEADS = ("wf_dense_ampl", "wf_dense_phase")
NS = 40                    # two full 16-chain blocks and a ragged one of 8
NS_LENGTHS = 37            # the chain-length cases (see the module docstring)
F64_FAMILIES = ("gru64", "mdrnn")
GRU_FAMILIES = ("gru", "parity", "crnn", "gru64")

# first and last width of every width class (pick_nfull); 5 exists for the 2D RNN only, which has no 6
CLASS_WIDTHS = {1: (17, 20), 2: (21, 36), 3: (37, 52), 4: (53, 68), 5: (69, 84), 6: (69, 100), 8: (101, 132), 12: (133, 196), 16: (197, 260)}

Case = collections.namedtuple("Case", "family shape units ns sharp")


# ---- the dispatch code's integer facts -----------------------------------------------------------------------------------------

def nfull(family, units):
    """rnnwf_api.hip: pick_nfull on the widest layer; None: rnnwf_create refuses the width."""
    H = max(units)
    for nf in (1, 2, 3, 4, 5, 6, 8, 12, 16):
        if nf == 5 and family != "mdrnn":
            continue
        if 16 * nf + 4 < H:
            continue
        if (family == "mdrnn" and nf > 5) or (family == "gru64" and nf > 6):
            return None
        return nf
    return None


def refusal(family, units):
    """None where the code admits (family, units), else the message rnnwf_create raises (checked in its order)."""
    if len(units) > 1:
        if family == "mdrnn":
            return "rnnwf_create: the 2D RNN has one layer"
        if family == "gru64" and max(units) > 68:
            return "rnnwf_create: stacked float64 layers: num_units <= 68"
        if family != "gru64" and max(units) > 100:
            return "rnnwf_create: stacked layers: num_units <= 100"
    if nfull(family, units) is None:
        return "rnnwf_create: num_units too large (f32 GRU: <= 260, f64 GRU: <= 100, 2D RNN: <= 84)"
    return None


# classes the issue's prose could be read to include and the code refuses: (family, units, message)
REFUSED = [
    ("gru64", (69, 69), refusal("gru64", (69, 69))),          # float64 stacks stop at NFULL 4
    ("gru64", (100, 100, 100), refusal("gru64", (100, 100, 100))),
    ("gru", (101, 101), refusal("gru", (101, 101))),          # f32 stacks stop at NFULL 6
    ("crnn", (132, 20), refusal("crnn", (132, 20))),
    ("gru64", (101,), refusal("gru64", (101,))),              # one layer: float64 stops at NFULL 6, f32 at 16, the 2D RNN at 5
    ("gru", (261,), refusal("gru", (261,))),
    ("crnn", (261,), refusal("crnn", (261,))),
    ("mdrnn", (85,), refusal("mdrnn", (85,))),
    ("mdrnn", (20, 20), refusal("mdrnn", (20, 20))),
]


def _gru_layout_bytes(nf, nout, es):
    """layout.h: GruLayout<T, NFULL, NOUT>::BYTES, es = sizeof(T)."""
    kt, nt, vw = 4 * nf + 1, 3 * nf + 1, 16 // es
    ng = (kt - 1) // vw
    off = nt * ng * 64 * 16                          # OFF_AREM
    off += nt * 64 * es                              # OFF_BINIT
    off += 3 * (nt * 16 + 4) * es                    # OFF_XC
    off += 3 * ((nf + 1) * 16 + 4) * es              # OFF_WD
    off += 4 * ((nout * kt + 3) // 4 * 4) * es       # OFF_BD
    return (off + 32 + 15) // 16 * 16


def _bwd_bytes(nf, es):
    """grad_kernels.h: GradLayout<NFULL, T>::BWD_BYTES."""
    kt, vw = 4 * nf + 1, 16 // es
    return (nf + 1) * ((3 * kt + vw - 1) // vw) * 64 * 16


def pair_fits(family, nf):
    """grad.hip: GLaunch::PAIR_OK = not WIDE and T = float and GradPair<T, NFULL, NOUT>::FITS, where (grad_kernels.h)
    FITS = not GruLayout::SPILL and GruLayout::BYTES + BWD_BYTES + 2 x SLOT <= 160 KiB, SLOT = (6 KT + NOUT) x 64 x 4 B rounded to 16."""
    if family in F64_FAMILIES or nf in (8, 12, 16):
        return False
    nout, kt = (3 if family == "crnn" else 1), 4 * nf + 1
    img = _gru_layout_bytes(nf, nout, 4)
    slot = ((6 * kt + nout) * 64 * 4 + 15) // 16 * 16
    return img <= 160 * 1024 and img + _bwd_bytes(nf, 4) + 2 * slot <= 160 * 1024


def engine(case):
    """What engine_name() reports after the case's vmc_step (rnnwf_api.hip: rnnwf_engine_name).  float64 families: f64mfma.  Positive and
    parity GRU: the engine of the last flip pass, and 40 samples are far too few tiles for the bf16x3 one (prnn.hip: use_split) -
    f32mfma; with ONE site no flip pass runs and the name is the handle's configured engine, bf16x3 for one layer up to 100 units.
    Complex: the configured engine - bf16x3 for one layer up to NFULL 6 and for stacks of 37..50 units (split.hip: stack_split_available)."""
    nf, N = nfull(case.family, case.units), case.shape[0] * case.shape[1]
    if case.family in F64_FAMILIES:
        return "f64mfma"
    configured = nf <= 6 if len(case.units) == 1 else (nf == 3 and max(case.units) <= 50)
    if case.family == "crnn" or N == 1:
        return "bf16x3" if configured else "f32mfma"
    return "f32mfma"


def passes(case):
    """backward passes = weight-gradient products per gradient (timers 3 and 4)"""
    return len(case.units) * (2 if case.family == "parity" else 1)


# ---- the table --------------------------------------------------------------------------------------------------------------------

def _shape(family, k=0):
    return {"gru": (33, 1), "parity": (33, 1), "crnn": (34, 1), "gru64": ((11, 3), (17, 2))[k % 2], "mdrnn": (7, 5)}[family]


def _sharp(family):
    return 1.25 if family == "mdrnn" else 3.0        # test_gpu_gradient_full.py states why the 2D RNN cannot take x 3


def _cases():
    out = []

    def add(family, units, shape=None, ns=NS):
        units = tuple(units)
        assert refusal(family, units) is None, (family, units)
        out.append(Case(family, shape or _shape(family, len(out)), units, ns, _sharp(family)))

    # one layer: 6 units and both ends of every class the family has
    for family in ("gru", "crnn", "gru64"):
        for nf in (1, 2, 3, 4, 6, 8, 12, 16):
            if nfull(family, (CLASS_WIDTHS[nf][1],)) != nf:
                continue
            for H in ((6, 20) if nf == 1 else CLASS_WIDTHS[nf]):
                add(family, (H,))
    # stacks: first / last width alternating over the (layers, NFULL) cells - both occur for every NFULL and every layer count
    for family in ("gru", "crnn", "gru64"):
        for NL in (2, 3, 4):
            for j, nf in enumerate((1, 2, 3, 4, 6)):
                H = CLASS_WIDTHS[nf][(NL + j) % 2]
                if refusal(family, (H,) * NL) is None:
                    add(family, (H,) * NL)
    # unequal widths: the narrower layers are padded to the widest; (20, 36, 52) and (20, 36) have the widest layer on top
    add("gru", (64, 20))
    add("gru", (20, 36, 52))
    add("crnn", (50, 20, 36))
    add("gru64", (36, 20))
    # parity-symmetric: one case per one-layer class, ends alternating, and two stacks (one of unequal widths, widest on top)
    for j, nf in enumerate((1, 2, 3, 4, 6, 8, 12, 16)):
        add("parity", (CLASS_WIDTHS[nf][(j + 1) % 2],))
    add("parity", (21, 21))
    add("parity", (20, 36, 52))
    # the 2D RNN: 6 units and both ends of its five classes
    for nf in (1, 2, 3, 4, 5):
        for H in ((6, 20) if nf == 1 else CLASS_WIDTHS[nf]):
            add("mdrnn", (H,))
    # chain lengths on the narrowest class, all with 37 samples: one site, two, rows a multiple of 4 (148), not one (1221), 65 sites
    for N in (1, 2, 4, 33, 65):
        add("gru", (20,), shape=(N, 1), ns=NS_LENGTHS)
    return out


CASES = _cases()


def case_id(c):
    return "%s-%dx%d-%s-%d" % (c.family, c.shape[0], c.shape[1], "x".join(map(str, c.units)), c.ns)


IDS = [case_id(c) for c in CASES]


def gradient_class(c):
    """(family's kernel family, layers, NFULL): the key with_gru_grad / the 2D RNN's width switch dispatch on"""
    return ("gru" if c.family == "parity" else c.family, len(c.units), nfull(c.family, c.units))


def admitted_classes():
    """every class the dispatch code admits, from refusal() and nfull() alone"""
    out = set()
    for family in ("gru", "crnn", "gru64"):
        for NL in (1, 2, 3, 4):
            for nf in (1, 2, 3, 4, 6, 8, 12, 16):
                H = CLASS_WIDTHS[nf][1]
                if refusal(family, (H,) * NL) is None and nfull(family, (H,) * NL) == nf:
                    out.add((family, NL, nf))
    out |= {("mdrnn", 1, nf) for nf in (1, 2, 3, 4, 5)}
    return out


# one case per class that has the pair kernel (the first of the table), for the pair / four-wave comparison
def _pair_cases():
    seen, out = set(), []
    for c in CASES:
        key = (c.family, len(c.units), nfull(c.family, c.units))
        if c.ns == NS and pair_fits(c.family, key[2]) and key not in seen:
            seen.add(key)
            out.append(c)
    return out


PAIR_CASES = _pair_cases()


# ---- parameters, batches, references -------------------------------------------------------------------------------------------

def parameters(c, seed=111):
    """kernels x sharp and every bias randomised, as test_gpu_gradient_full.py: build"""
    def sharpened(prm):
        return P.randomize_biases(P.scale_kernels(prm, c.sharp), seed + 1)
    if c.family == "mdrnn":
        return sharpened(P.init_mdrnn_params(c.units[0], seed=seed))
    if c.family == "crnn":
        return sharpened(P.init_gru_params(list(c.units), seed=seed, heads=HEADS))
    return sharpened(P.init_gru_params(list(c.units), seed=seed, dtype=np.float64 if c.family == "gru64" else np.float32))


def couplings(c):
    N = c.shape[0] * c.shape[1]
    if c.family == "crnn":
        return np.concatenate([np.ones(N), 0.5 * np.ones(N), np.zeros(N), [0.0, 0.0]])
    return np.append(np.ones(N), 3.0 if c.family in F64_FAMILIES else 1.0)


def model_id(c):
    from rnnwavefunctions_amd import _lib
    return {"gru": _lib.MODEL_GRU1D, "parity": _lib.MODEL_GRU1D_PARITY, "crnn": _lib.MODEL_CRNN_U1, "gru64": _lib.MODEL_GRU1D_F64,
            "mdrnn": _lib.MODEL_MDRNN2D}[c.family]


def autograd_family(family):
    return "gru" if family == "gru64" else family


def unit_roundoff(family):
    return 2.0 ** -53 if family in F64_FAMILIES else 2.0 ** -24


def sample_costs(family, leaves, s, e, **kw):
    """(ns,) float64 tensor L with cost = sum_s L_s: both costs are linear in the per-sample log psi.
    real: w_s log P_s, w_s = (E_s - <E>) / ns; complex: (2 / ns) (Re l_s Re(E_s - <E>) + Im l_s Im(E_s - <E>))."""
    lp = A.FORWARD[autograd_family(family)](leaves, s, SCOPE, **kw)
    e = np.asarray(e)
    d = torch.as_tensor((e - e.mean()) / len(e))
    if family == "crnn":
        return 2.0 * (lp.real * d.real + lp.imag * d.imag)
    return lp * d


def per_sample_gradients(family, prm, s, e, dtype=torch.float64, **kw):
    """{name: (ns,) + shape float64}: d L_s / d tensor, one batched reverse pass (row s of the identity as grad_outputs)"""
    leaves = A.to_torch(prm, dtype, requires_grad=True)
    L = sample_costs(family, leaves, s, e, **kw)
    order = sorted(leaves)
    g = torch.autograd.grad(L, [leaves[k] for k in order], grad_outputs=torch.eye(len(L), dtype=L.dtype), is_grads_batched=True,
                            allow_unused=True)
    return {k: (torch.zeros((len(L),) + leaves[k].shape) if v is None else v).detach().to(torch.float64).numpy()
               .reshape((len(L),) + np.shape(prm[k])) for k, v in zip(order, g)}


def rounding_floor(c, terms, g64):
    """{name: N x unit round-off x max_k sum_s |term_sk| / max |g64|} (0 where the reference tensor is exactly zero: nothing is
    summed there and the kernel must give zero)"""
    N, u = c.shape[0] * c.shape[1], unit_roundoff(c.family)
    out = {}
    for k, t in terms.items():
        ref_max = np.abs(g64[k]).max()
        out[k] = N * u * np.abs(t).sum(axis=0).max() / ref_max if ref_max > 0 else 0.0
    return out


Reference = collections.namedtuple("Reference", "g64 g32 terms floor seconds")


def reference(c, prm, s, e):
    """float64 and float32 autograd gradients, the float64 per-sample terms and the floor they give"""
    t0 = time.time()
    fam = autograd_family(c.family)
    g64 = A.gradient(fam, prm, s, e, dtype=torch.float64)
    g32 = A.gradient(fam, prm, s, e, dtype=torch.float32)
    terms = per_sample_gradients(c.family, prm, s, e)
    return Reference(g64, g32, terms, rounding_floor(c, terms, g64), time.time() - t0)


def judge(label, c, grads, ref, echo=print):
    """verdict under the bound of the module docstring: (worst ratio, failures)"""
    scale = A.F64_OVER_F32 if c.family in F64_FAMILIES else 1.0
    return A.verdict(grads, ref.g64, ref.g32, unit_roundoff_ratio=scale, label=label, floor=ref.floor, echo=echo)
