"""Float64 restatement of TF-1 Adam and the case table of tests/test_gpu_train_images.py (device-resident training: rnnwf_train_steps /
rnnwf_adam_step of csrc/train.hip, whose update re-packs every weight image from packer tables recorded once per handle).  TEST
INFRASTRUCTURE ONLY.

`AdamReference` is written from the formula of tf.train.AdamOptimizer (TF 1.x), not imported from rnnwavefunctions_amd.training:

    lr_t  = lr sqrt(1 - beta2^t) / (1 - beta1^t)
    m     = beta1 m + (1 - beta1) g
    v     = beta2 v + (1 - beta2) g^2
    theta = theta - lr_t m / (sqrt(v) + epsilon)          float32 models: theta rounded to float32 after each step

in float64, one IEEE operation per operator, left to right as written above (g^2 enters as ((1 - beta2) g) g).  The learning rate is
an argument of every step.  tests/test_train_reference.py checks it against torch.optim.Adam, against closed forms, and checks that
training.Adam - the optimizer the drivers' host path uses - equals it bit for bit.

CASES: one row per packer table row of train.hip (`switch` on the width class NFULL) that device training can reach.

  id, family, (Nx, Ny), units, samples, environment while the handles are created, the engine_name() the trained handle must report
  after its local-energy pass, why the row is there.

Width classes (rnnwf_api.hip: pick_nfull): NFULL = the smallest of 1, 2, 3, 4, (5: 2D RNN only), 6, 8, 12, 16 with 16 NFULL + 4 >= the
widest layer - 20 | 36 | 52 | 68 | (84) | 100 | 132 | 196 | 260 units.  Tables of train.hip and the rows of this table that replay them:

  wimg_table<NOUT>     f32 forward image, NFULL 1, 2, 3, 4, 6, 8, 12, 16: every one-layer gru / parity / crnn row (read by the base
                       pass, the sampler, log_prob and - on the f32-input MFMA - the flip / swap pass).  At NFULL 3 the positive
                       GRU's base pass reads wbasebf instead: the RNNWF_BASE=f32 rows make it read wimg.
  wsplit_table<NOUT>   bf16x3 image: NFULL 1 (20), 2 (36), 3 aligned (37, 50), 3 padded (51, 52), 4 riders (53, 68), 6 streamed
                       (69, 100).  The positive GRU's flip pass reads it only on the bf16x3 engine, which 48 chains do not choose
                       (prnn.hip: use_split wants (N - 1) ceil(ns / 32) >= 8 CUs tiles): the RNNWF_ENGINE=bf16x3 rows pin it.  With the
                       engine pinned use_split takes no small-batch fallback, so 48 chains on 6 sites DO run the bf16x3 flip kernel
                       and no row needed more samples or sites.  The complex RNN's swap pass runs bf16x3 at every batch size up to
                       100 units (crnn.hip: engine_split), so its default rows already read wsplit; its RNNWF_ENGINE=bf16x3 rows
                       are the same kernels with the engine pinned and are kept because the pinned handle is a configuration of
                       its own (rnnwf_api.hip: knobs).
  wsplit16             beside wsplit at 69..100 units, positive GRU, bf16x3: gru-69-bf16x3, gru-100-bf16x3.
  wimg_table_f64       NFULL 1, 2, 3, 4, 6: gru64 36, 52, 68, 69, 100 (NFULL 1 is test_gpu_training.py's).
  wbasebf_table        NFULL 3, one layer, default engine: gru 37, 50, 51, 52, parity-52, crnn 50, 52.
  mdrnn_pack_table     NFULL 2, 4, 5: mdrnn 36, 68, 84 (1 and 3: test_gpu_training.py's 10, 16 and 50 units).
  grad_stack_forward_table   stacks; wsplit + wsplit_up[] of the layer pipeline: the two RNNWF_ENGINE=bf16x3 stacks (NFULL 3, <= 50
                       units - split.hip: stack_split_available looks at the widest layer, so (50, 44, 37) runs the pipeline).
  backward image       added by ensure_bwd_image in the first iteration of every row; wide backward images (grad_wide.hip) at
                       f32 NFULL 8, 12, 16 and float64 NFULL 6.
  dW -> flat gather    grad_flat_probe's table: every row (assertion (a) of the GPU test).

Every width the table lists is admitted by rnnwf_create (gradient_classes_reference.refusal is None for each: checked by
tests/test_train_reference.py), so no row had to be replaced.
"""
import math

import numpy as np

SCOPE = "RNNwavefunction"
HEADS = ("wf_dense_ampl", "wf_dense_phase")
F64_FAMILIES = ("gru64", "mdrnn")

LEARNING_RATES = (1e-2, 5e-3, 2e-3)      # one per device iteration of a case
NS = 48                                  # three 16-chain blocks, or one 32-chain tile and a half
SEED = 111


class AdamReference:
    """TF-1 Adam in float64 on {name: float64 array}.  model_dtype np.float32: theta is rounded to float32 after every step (and
    returned as float64 holding those values); m, v stay float64.  m, v: {name: array}, t: steps taken."""

    def __init__(self, model_dtype=np.float64, beta1=0.9, beta2=0.999, epsilon=1e-8):
        self.model_dtype = np.dtype(model_dtype)
        self.beta1, self.beta2, self.epsilon = float(beta1), float(beta2), float(epsilon)
        self.t = 0
        self.m, self.v = {}, {}

    def step(self, theta, grads, lr):
        self.t += 1
        b1, b2 = self.beta1, self.beta2
        lr_t = float(lr) * math.sqrt(1.0 - b2 ** self.t) / (1.0 - b1 ** self.t)
        out = {}
        for k, p in theta.items():
            p = np.asarray(p, dtype=np.float64)
            g = np.asarray(grads[k], dtype=np.float64)
            m = self.m.get(k, np.zeros_like(g))
            v = self.v.get(k, np.zeros_like(g))
            m = b1 * m + (1.0 - b1) * g
            v = b2 * v + ((1.0 - b2) * g) * g
            p = p - (lr_t * m) / (np.sqrt(v) + self.epsilon)
            if self.model_dtype == np.float32:
                p = p.astype(np.float32).astype(np.float64)
            self.m[k], self.v[k], out[k] = m, v, p
        return out

    def flat(self, names):
        """(m, v) concatenated in the order of `names` (the library's flat order: NativeWavefunction._layout, scoped)"""
        return (np.concatenate([self.m[k].ravel() for k in names]), np.concatenate([self.v[k].ravel() for k in names]))


# ---- the dispatch code's integer facts --------------------------------------------------------------------------------------------------

def nfull(family, units):
    """rnnwf_api.hip: pick_nfull on the widest layer"""
    H = max(units)
    for nf in (1, 2, 3, 4, 5, 6, 8, 12, 16):
        if nf == 5 and family != "mdrnn":
            continue
        if 16 * nf + 4 >= H:
            return nf
    return None


def engine_split(family, units, env):
    """prnn.hip / crnn.hip: pack_image - the handle holds bf16x3 images: an f32 family, not RNNWF_ENGINE=f32, and one layer of
    NFULL <= 6 or a stack of NFULL 3 and <= 50 units (split.hip: stack_split_available)"""
    nf = nfull(family, units)
    return (family not in F64_FAMILIES and env.get("RNNWF_ENGINE") != "f32" and
            (nf <= 6 if len(units) == 1 else (nf == 3 and max(units) <= 50)))


def expected_engine(family, units, env):
    """rnnwf_api.hip: rnnwf_engine_name after a local-energy pass of NS chains on 6 sites.  float64 families: f64mfma.  Complex: the
    configured engine (engine_split).  Positive / parity: the engine of the last flip pass - bf16x3 only where engine_split and the
    engine is pinned, since 5 x 2 tiles of 32 chains are far fewer than 8 CUs (prnn.hip: use_split)."""
    if family in F64_FAMILIES:
        return "f64mfma"
    split = engine_split(family, units, env)
    if family == "crnn":
        return "bf16x3" if split else "f32mfma"
    return "bf16x3" if split and env.get("RNNWF_ENGINE") == "bf16x3" else "f32mfma"


# ---- the table --------------------------------------------------------------------------------------------------------------------------

BF = {"RNNWF_ENGINE": "bf16x3"}
BASE32 = {"RNNWF_BASE": "f32"}

_GRU_WHY = {20: "NFULL 1, flat", 36: "NFULL 2, flat: last width", 37: "NFULL 3, aligned (K-packed): first width; wbasebf",
            50: "NFULL 3, aligned: last width; wbasebf", 51: "NFULL 3, padded split layout: first width; wbasebf",
            52: "NFULL 3, padded: last width; wbasebf", 53: "NFULL 4, riders: first width", 68: "NFULL 4, riders: last width",
            69: "NFULL 6, streamed: first width; backward operand through L2", 100: "NFULL 6: last width",
            101: "NFULL 8: first width; forward image through L2, wide backward image", 132: "NFULL 8: last width",
            196: "NFULL 12: last width, wide backward image", 260: "NFULL 16: last width, wide backward image"}


def _cases():
    out = []

    def add(cid, family, units, env, why, shape=None):
        shape = shape or ((3, 2) if family in F64_FAMILIES else (6, 1))
        out.append((cid, family, shape, tuple(units), NS, dict(env), expected_engine(family, units, env), why))

    for H in (20, 36, 37, 50, 51, 52, 53, 68, 69, 100, 101, 132, 196, 260):
        add("gru-%d" % H, "gru", (H,), {}, "wimg " + _GRU_WHY[H])
    for H in (20, 36, 37, 50, 51, 52, 53, 68, 69, 100):
        add("gru-%d-bf16x3" % H, "gru", (H,), BF, "the flip pass reads the re-packed wsplit%s: %s" %
            (" / wsplit16" if H > 68 else "", _GRU_WHY[H]))
    for H in (37, 50, 52):
        add("gru-%d-base-f32" % H, "gru", (H,), BASE32, "the base pass reads wimg, not wbasebf: " + _GRU_WHY[H])
    add("parity-52", "parity", (52,), {}, "parity-symmetric, both directions: NFULL 3 padded; wbasebf")
    add("parity-68", "parity", (68,), {}, "parity-symmetric: NFULL 4")
    for H in (20, 36, 50, 52, 53, 68, 69, 100, 132, 196, 260):
        add("crnn-%d" % H, "crnn", (H,), {}, "complex, three head rows (NOUT 3); the swap pass reads wsplit up to 100 units: NFULL %d" %
            nfull("crnn", (H,)))
    for H in (20, 36, 50, 52, 53, 68, 69, 100):
        add("crnn-%d-bf16x3" % H, "crnn", (H,), BF, "the same kernels on the pinned engine: NFULL %d" % nfull("crnn", (H,)))
    for H in (36, 52, 68, 69, 100):
        add("gru64-%d" % H, "gru64", (H,), {}, "wimg_table_f64 NFULL %d%s" % (nfull("gru64", (H,)), ", wide backward image" if H > 68 else ""))
    for H in (36, 68, 84):
        add("mdrnn-%d" % H, "mdrnn", (H,), {}, "mdrnn_pack_table NFULL %d" % nfull("mdrnn", (H,)))
    add("stack-64-20", "gru", (64, 20), {}, "unequal widths, NFULL 4: the narrower layer padded inside the library")
    add("stack-20-50-36", "gru", (20, 50, 36), {}, "three layers, the widest in the middle, NFULL 3: cooperative multi-layer base pass")
    add("stack-100-100", "gru", (100, 100), {}, "stack at NFULL 6")
    add("stack-50-44-37-bf16x3", "gru", (50, 44, 37), BF, "the layer pipeline: wsplit and wsplit_up[0], wsplit_up[1] (top)")
    add("crnn-stack-68-20", "crnn", (68, 20), {}, "complex stack of unequal widths, NFULL 4")
    add("crnn-stack-50-50-bf16x3", "crnn", (50, 50), BF, "complex layer pipeline: wsplit and wsplit_up[0] with three head rows")
    add("gru64-stack-36-36", "gru64", (36, 36), {}, "float64 stack, NFULL 2")
    add("gru64-stack-68-52-20", "gru64", (68, 52, 20), {}, "float64 stack of unequal widths, NFULL 4 (the widest a float64 stack has)")
    return out


CASES = _cases()
CASE_IDS = [c[0] for c in CASES]


def case(cid):
    return CASES[CASE_IDS.index(cid)]


# What the table must reach: (family, units, environment) of every row the issue lists ...
def _required():
    req = [("gru", (H,), {}) for H in (20, 36, 37, 50, 51, 52, 53, 68, 69, 100, 101, 132, 196, 260)]
    req += [("gru", (H,), BF) for H in (20, 36, 37, 50, 51, 52, 53, 68, 69, 100)]
    req += [("gru", (H,), BASE32) for H in (37, 50, 52)]
    req += [("parity", (52,), {}), ("parity", (68,), {})]
    req += [("crnn", (H,), {}) for H in (20, 36, 50, 52, 53, 68, 69, 100, 132, 196, 260)]
    req += [("crnn", (H,), BF) for H in (20, 36, 50, 52, 53, 68, 69, 100)]
    req += [("gru64", (H,), {}) for H in (36, 52, 68, 69, 100)]
    req += [("mdrnn", (H,), {}) for H in (36, 68, 84)]
    req += [("gru", (64, 20), {}), ("gru", (20, 50, 36), {}), ("gru", (100, 100), {}), ("gru", (50, 44, 37), BF),
            ("crnn", (68, 20), {}), ("crnn", (50, 50), BF), ("gru64", (36, 36), {}), ("gru64", (68, 52, 20), {})]
    return req


REQUIRED = _required()

# ... and the (table, row) pairs of train.hip's switches the suite did not run before (tests/test_train_reference.py: table_rows)
REQUIRED_TABLE_ROWS = (
    {("wimg<1>", nf) for nf in (1, 2, 3, 4, 6, 8, 12, 16)} | {("wimg<3>", nf) for nf in (1, 2, 3, 4, 6, 8, 12, 16)} |
    {("wsplit<1>", r) for r in ("1", "2", "3a", "3p", "4", "6")} | {("wsplit<3>", r) for r in ("1", "2", "3a", "3p", "4", "6")} |
    {("wsplit16", 6)} | {("wimg_f64", nf) for nf in (2, 3, 4, 6)} | {("wbasebf", 3)} | {("mdrnn", nf) for nf in (2, 4, 5)} |
    {("stack", "gru", 3), ("stack", "gru", 4), ("stack", "gru", 6), ("stack", "crnn", 3), ("stack", "crnn", 4), ("stack", "gru64", 2),
     ("stack", "gru64", 4), ("wsplit_up<1>", 3), ("wsplit_up<3>", 3)})


def table_rows(family, units, env):
    """The (table, row) pairs train.hip: build replays for a handle - its `if` ladder restated."""
    nf = nfull(family, units)
    split = engine_split(family, units, env)
    nout = 3 if family == "crnn" else 1
    rows = set()
    if family == "mdrnn":
        return {("mdrnn", nf)}
    if len(units) > 1:
        rows.add(("stack", "gru" if family == "parity" else family, nf))
        if split:
            rows |= {("wsplit<%d>" % nout, "3a"), ("wsplit_up<%d>" % nout, 3)}
        return rows
    rows.add(("wimg_f64", nf) if family == "gru64" else ("wimg<%d>" % nout, nf))
    if split:
        rows.add(("wsplit<%d>" % nout, {3: "3a" if max(units) <= 50 else "3p"}.get(nf, str(nf))))
        if nf == 6 and family != "crnn":
            rows.add(("wsplit16", 6))
    if family != "gru64" and nf == 3 and "RNNWF_BASE" not in env and env.get("RNNWF_ENGINE") != "f32":
        rows.add(("wbasebf", 3))                        # split.hip: base_bf_pack
    return rows


# ---- parameters, couplings, configurations ----------------------------------------------------------------------------------------------

def parameters(family, units, seed=SEED):
    """P.init_*_params with the kernels x 1.5 and every bias randomised, as tests/test_gpu_fuzz.py"""
    from rnnwavefunctions_amd import params as P
    if family == "mdrnn":
        prm = P.init_mdrnn_params(units[0], seed=seed)
    elif family == "crnn":
        prm = P.init_gru_params(list(units), seed=seed, heads=HEADS)
    else:
        prm = P.init_gru_params(list(units), seed=seed, dtype=np.float64 if family == "gru64" else np.float32)
    return P.randomize_biases(P.scale_kernels(prm, 1.5), seed + 1)


def model_dtype(family):
    return np.float64 if family in F64_FAMILIES else np.float32


def hamiltonian(family, N):
    """Random couplings around 1 with a transverse field, so that the flip pass runs and a shifted bond index shows; complex: J2 = 0.4."""
    rng = np.random.RandomState(N + 17)
    if family == "crnn":
        return dict(J1=1 + 0.1 * rng.standard_normal(N), J2=0.4 * np.ones(N), Bz=0.05 * rng.standard_normal(N))
    return dict(Jz=1 + 0.1 * rng.standard_normal(N), Bx=2.0 if family in F64_FAMILIES else 0.8)


def couplings(family, ham):
    """the vector rnnwf_vmc_step / rnnwf_train_steps take"""
    if family == "crnn":
        return np.concatenate([ham["J1"], ham["J2"], ham["Bz"], [0.0, 0.0]])
    return np.append(ham["Jz"], ham["Bx"])


def configurations(family, shape, count=NS, seed=5):
    """fixed configurations: random spins; complex: of the zero-magnetisation sector; 2D RNN: (count, Nx, Ny)"""
    rng = np.random.RandomState(seed)
    N = shape[0] * shape[1]
    if family == "crnn":
        return np.stack([rng.permutation(np.repeat([0, 1], N // 2)) for _ in range(count)]).astype(np.int32)
    s = rng.randint(0, 2, (count, N)).astype(np.int32)
    return s.reshape(count, shape[0], shape[1]) if family == "mdrnn" else s


def oracle_value(family, prm64, s):
    """log P (complex: log psi) of the float64 oracle"""
    from oracle import models as M
    if family == "mdrnn":
        return M.mdrnn_log_probability(prm64, s)
    if family == "crnn":
        return M.crnn_log_amplitude(prm64, s, dtype=np.float64)
    if family == "parity":
        return M.prnn_paritysym_log_probability(prm64, s, dtype=np.float64)
    return M.prnn_log_probability(prm64, np.asarray(s).reshape(len(s), -1), dtype=np.float64)


def oracle_bound(family, N, layers):
    """the bounds the suite uses for these entry points (test_gpu_crnn.py, test_gpu_prnn.py, test_gpu_mdrnn.py)"""
    return 1e-11 * N if family in F64_FAMILIES else 3e-6 * N * layers + 3e-6
