"""Float64 reference of the SAMPLER: one decision per draw.  TEST INFRASTRUCTURE ONLY.

A sample matrix s (ns, N) drawn with (seed, step, sample_offset) consumed the uniforms u = oracle.philox.uniforms(seed, step,
sample_offset, ns, N).  For every row the conditional p0[b, n] = p(spin 0 at draw n | the row's own earlier spins) is evaluated
teacher-forced in float64, and the decision the kernel must have made is

    s[b, n] == (u[b, n] >= p0[b, n])          (tf.multinomial over two classes: oracle.models.multinomial_2, gru_kernels.h)

Because the row's own prefix is fed, EVERY one of the ns * N draws is checked - also those after a near-tie - and nothing is sampled
sequentially.  The conditionals are restated here from the formulas of oracle/models.py and tests/lstm_reference.py:

    gru      positive GRU, one layer or a stack, float32 or float64 parameters (M.prnn_site_probs); the float64 GRU on the 2D raster
             is this on the flat (ns, Nx * Ny) samples.  Draw n = site n.
    parity   the parity-symmetric class DRAWS from the forward chain alone (prnn.hip: the reversed chains only enter log P_sym
             afterwards, as 1DTFIM/RNNwavefunction_paritysym.py samples), so its conditionals are the GRU's.
    crnn     complex U(1) GRU: p0 = a0^2 / (a0^2 + a1^2) of the MASKED amplitude (M._crnn_masked_ampl).  Where the mask forces the
             spin p0 is exactly 0 or 1: the decision admits no band there and u is irrelevant.
    mdrnn    2D RNN on the zig-zag path.  Its uniforms are indexed by PATH POSITION, not by site index: column k of u belongs to
             the k-th visited site (mdrnn_kernels.h draws with `p`, M.mdrnn_sample with `k`).  p0 and the decisions are therefore
             returned in path order; `path_spins` puts a (ns, Nx, Ny) sample matrix into that order.
    lstm     LSTM over the raster path (lstm_reference.lstm_site_probs).  Draw n = flat site n.

Near-tie band, from the reference alone: y[b, n] = max over draws <= n of |p0_f32 - p0_f64| along row b (rounding accumulates along
the chain; p0_f32 is the same restatement in float32 arithmetic), band = FACTOR * max(y, 2^-24), scaled by F64_OVER_F32 for the
float64 families (the rule of test_gpu_gradient_full.py).  A draw with |u - p0_f64| < band is excused, every other one must match
exactly.  The cap is a condition on the case, not a measurement: at most CAP_DRAWS of a case's draws may lie in the band and at most
CAP_ROWS of its rows may hold such a draw.
"""
import time

import numpy as np

import autograd_reference as A
import lstm_reference as L
from oracle import models as M
from oracle import philox

SCOPE = "RNNwavefunction"
FACTOR = A.FACTOR
F64_OVER_F32 = A.F64_OVER_F32
FLOOR = 2.0 ** -24                 # one float32 unit round-off, and the spacing of the uniforms
CAP_DRAWS = 1e-3
CAP_ROWS = 0.05
FLOAT64_FAMILIES = ("gru64", "mdrnn", "lstm")
CHUNK = 4096                       # rows per pass of a restatement (memory only; the result does not depend on it)


def cast(params, dtype):
    return {k: np.asarray(v).astype(dtype) for k, v in params.items()}


# ---- conditionals of spin 0, teacher-forced, (B, N) in the arithmetic `dtype` ------------------------------------------------------

def gru_p0(params, samples, dtype, scope=SCOPE):
    s = np.asarray(samples).reshape(len(samples), -1)
    return M.prnn_site_probs(cast(params, dtype), s, scope, dtype)[:, :, 0]


def crnn_p0(params, samples, dtype, scope=SCOPE, mask_delay=0):
    """(p0, forced): p0 = a0^2 / (a0^2 + a1^2) of M._crnn_masked_ampl; forced marks the draws whose mask leaves one spin only (p0 is
    then exactly 0 or 1; 0 also where a row has left the sector and both are masked).  mask_delay: the defect study's knob - the
    mask of site n computed as that of site n - mask_delay; 0 is the model."""
    prm = cast(params, dtype)
    s = np.asarray(samples)
    B, N = s.shape
    Wa, ba = prm[scope + "/wf_dense_ampl/kernel"], prm[scope + "/wf_dense_ampl/bias"]
    x = np.zeros((B, 2), dtype=dtype)
    states = M._zero_states(prm, scope, B, dtype)
    p0 = np.empty((B, N), dtype=dtype)
    forced = np.zeros((B, N), dtype=bool)
    for n in range(N):
        out, states = M.multi_gru(x, states, prm, scope)
        m = n - mask_delay
        num_up = s[:, :max(m, 0)].sum(axis=1).astype(dtype)
        ampl = M._crnn_masked_ampl(out, Wa, ba, m, N, num_up)
        w = ampl * ampl
        tot = w.sum(axis=1)
        p0[:, n] = np.where(tot > 0, w[:, 0] / np.where(tot > 0, tot, 1), 0)
        forced[:, n] = (w[:, 0] == 0) | (w[:, 1] == 0)
        x = M._one_hot(s[:, n], dtype)
    return p0, forced


def path_spins(samples):
    """(ns, Nx, Ny) -> (ns, Nx * Ny) in the zig-zag visiting order: column k is the k-th visited site."""
    s = np.asarray(samples)
    _, Nx, Ny = s.shape
    return np.stack([s[:, nx, ny] for nx, ny, _ in M.zigzag_order(Nx, Ny)], axis=1)


def mdrnn_p0(params, samples, dtype, scope=SCOPE):
    """samples (B, Nx, Ny); p0 (B, Nx * Ny) in PATH order (column k: the k-th visited site)."""
    prm = cast(params, dtype)
    s = np.asarray(samples)
    B, Nx, Ny = s.shape
    nh = prm[scope + "/Wh_rnn_0"].shape[0]
    Wd, bd = prm[scope + "/wf_dense/kernel"], prm[scope + "/wf_dense/bias"]
    zeros_h, zeros_x = np.zeros((B, nh), dtype=dtype), np.zeros((B, 2), dtype=dtype)
    h, x = {}, {}
    p0 = np.empty((B, Nx * Ny), dtype=dtype)
    with np.errstate(over="ignore", invalid="ignore"):
        for k, (nx, ny, nxh) in enumerate(M.zigzag_order(Nx, Ny)):
            hh, xh = h.get((nxh, ny), zeros_h), x.get((nxh, ny), zeros_x)
            hv, xv = h.get((nx, ny - 1), zeros_h), x.get((nx, ny - 1), zeros_x)
            hn = M.mdrnn_cell(xh, xv, hh, hv, prm, scope).astype(dtype)
            p0[:, k] = M.softmax(hn @ Wd + bd)[:, 0]
            h[(nx, ny)] = hn
            x[(nx, ny)] = M._one_hot(s[:, nx, ny], dtype)
    return p0


def lstm_p0(params, samples, dtype, shape, scope=SCOPE):
    with np.errstate(over="ignore"):
        return L.lstm_site_probs(params, samples, shape[0], shape[1], scope, dtype)


def conditionals(family, params, samples, shape=None, scope=SCOPE, **kw):
    """(p0_f64, p0_f32, forced or None, decisions) - all (ns, N) in DRAW order; decisions are the spins in that order."""
    s = np.asarray(samples)
    ns = len(s)
    p64, p32, forced = [], [], []
    for k in range(0, ns, CHUNK):
        blk = s[k:k + CHUNK]
        for dtype, out in ((np.float64, p64), (np.float32, p32)):
            if family in ("gru", "gru64", "parity"):
                out.append(gru_p0(params, blk, dtype, scope))
            elif family == "crnn":
                p, f = crnn_p0(params, blk, dtype, scope, **kw)
                out.append(p)
                if dtype == np.float64:
                    forced.append(f)
            elif family == "mdrnn":
                out.append(mdrnn_p0(params, blk, dtype, scope))
            elif family == "lstm":
                out.append(lstm_p0(params, blk, dtype, shape, scope))
            else:
                raise ValueError(family)
    dec = path_spins(s) if family == "mdrnn" else s.reshape(ns, -1)
    return (np.concatenate(p64).astype(np.float64), np.concatenate(p32).astype(np.float64),
            np.concatenate(forced) if forced else None, dec.astype(np.int64))


# ---- the judgement ---------------------------------------------------------------------------------------------------------------

def band_of(p64, p32, float64_family=False, forced=None):
    """(band, y) of every draw; y is the running maximum of |p0_f32 - p0_f64| along the row."""
    with np.errstate(invalid="ignore"):
        d = np.abs(p32 - p64)
    d = np.where(np.isfinite(d), d, 1.0)                     # float32 overflowed where float64 did not: no precision left there
    y = np.maximum.accumulate(d, axis=1)
    band = FACTOR * np.maximum(y, FLOOR) * (F64_OVER_F32 if float64_family else 1.0)
    if forced is not None:
        band = np.where(forced, 0.0, band)
    return band, y


def judge(decisions, u, p64, p32, float64_family=False, forced=None, keep=20):
    """dict(draws, rows, unexcused, excused, excused_rows, share, row_share, within_cap, mismatches=[(row, draw, u, p0, band)]).
    excused counts every draw inside its band, whether it matches or not."""
    band, y = band_of(p64, p32, float64_family, forced)
    must = (u >= p64).astype(np.int64)
    in_band = np.abs(u - p64) < band
    wrong = (decisions != must) & ~in_band
    rows, draws = decisions.shape
    excused = int(in_band.sum())
    excused_rows = int(in_band.any(axis=1).sum())
    where = np.argwhere(wrong)
    res = dict(draws=rows * draws, rows=rows, unexcused=int(wrong.sum()), excused=excused, excused_rows=excused_rows,
               share=excused / float(rows * draws), row_share=excused_rows / float(rows),
               mismatches=[(int(r), int(n), float(u[r, n]), float(p64[r, n]), float(band[r, n])) for r, n in where[:keep]],
               wrong_rows=np.unique(where[:, 0]), wrong_draws=np.unique(where[:, 1]), max_y=float(y.max()), median_y=float(np.median(y)))
    res["within_cap"] = res["share"] <= CAP_DRAWS and res["row_share"] <= CAP_ROWS
    return res


def check(family, params, samples, seed, step, sample_offset=0, shape=None, rows=None, scope=SCOPE):
    """Judge a drawn sample matrix.  rows: the indices (a fixed stride, never chosen by outcome) of the rows to check, default all;
    row b consumed the uniforms of global index sample_offset + b."""
    t0 = time.time()
    s = np.asarray(samples)
    ns = len(s)
    N = int(np.prod(s.shape[1:]))
    rows = np.arange(ns) if rows is None else np.asarray(rows)
    u = philox.uniforms(seed, step, sample_offset, ns, N)[rows]
    p64, p32, forced, dec = conditionals(family, params, s[rows], shape, scope)
    res = judge(dec, u, p64, p32, family in FLOAT64_FAMILIES, forced)
    res["seconds"] = time.time() - t0
    res["row_index"] = rows
    return res


def line(label, res):
    return ("%s draws %d  unexcused %d  excused %d (share %.2e, %d rows = %.2e of rows)  max |p32 - p64| %.1e  reference %.1f s" %
            (label, res["draws"], res["unexcused"], res["excused"], res["share"], res["excused_rows"], res["row_share"],
             res["max_y"], res.get("seconds", 0.0)))


def failure_text(res):
    return "unexcused draws (row, draw, u, p0, band): %s" % (res["mismatches"],)


# ---- log-probability of drawn rows from the conditionals (return_log=True) -------------------------------------------------------

def log_prob_of(decisions, p64):
    with np.errstate(divide="ignore"):
        return np.where(decisions == 0, np.log(p64), np.log1p(-p64)).sum(axis=1)


# ---- the cases of tests/test_gpu_sampler_full.py, and the oracle's own sampler for the CPU study of the cap ----------------------

HEADS = ("wf_dense_ampl", "wf_dense_phase")


def build_params(family, units, seed=111, sharp=3.0):
    """Sharpened parameters as tests/test_gpu_gradient_full.py builds them: kernels x sharp, every bias randomised (seed + 1);
    sharp None: the glorot initialisation untouched."""
    from rnnwavefunctions_amd import params as P
    if family == "mdrnn":
        prm = P.init_mdrnn_params(units[0], seed=seed)
    elif family == "lstm":
        prm = P.init_lstm_params(list(units), seed=seed)
    elif family == "crnn":
        prm = P.init_gru_params(list(units), seed=seed, heads=HEADS)
    elif family == "gru64":
        prm = P.init_gru_params(list(units), seed=seed, dtype=np.float64)
    else:
        prm = P.init_gru_params(list(units), seed=seed)
    return prm if sharp is None else P.randomize_biases(P.scale_kernels(prm, sharp), seed + 1)


def oracle_draw(family, params, shape, u, scope=SCOPE):
    """The CPU oracle's own sampler of the family on the uniforms u, in the arithmetic the HIP model uses."""
    N = shape[0] * shape[1]
    if family in ("gru", "parity"):
        return M.prnn_sample(params, N, u, scope)[0]
    if family == "gru64":
        return M.prnn_sample(params, N, u, scope, dtype=np.float64)[0]
    if family == "crnn":
        return M.crnn_sample(params, N, u, scope)
    if family == "mdrnn":
        return M.mdrnn_sample(params, shape[0], shape[1], u, scope)[0]
    if family == "lstm":
        return L.lstm_sample(params, shape[0], shape[1], u, scope)[0]
    raise ValueError(family)


# id, family, lattice, units, samples, kernel scale (None: glorot), stride of the checked rows, forward engine after vmc_step (None: not
# asserted), environment of the handle.  Kernel scale 3 as tests/test_gpu_sharpened.py unless the CPU study below says otherwise.
# Cap study on the CPU oracle's own sampler (test_sampler_reference.py::test_clean_oracle_batches_stay_inside_the_cap runs it on
# min(samples, 2 048) rows - the share is a rate per draw; config 2 on all 10 000): see the table in that test's docstring.
CASES = [
    ("cfg2-x3", "gru", (80, 1), (50,), 10000, 3.0, 1, "bf16x3", {}),
    ("cfg2-x3-ragged", "gru", (80, 1), (50,), 10007, 3.0, 1, "bf16x3", {}),
    ("cfg2-glorot", "gru", (80, 1), (50,), 10000, None, 1, "bf16x3", {}),
    ("cfg2-glorot-ragged", "gru", (80, 1), (50,), 10007, None, 1, "bf16x3", {}),
    ("cfg2-x3-40000", "gru", (80, 1), (50,), 40000, 3.0, 4, "bf16x3", {}),
    ("cfg2-x3-40000-basef32", "gru", (80, 1), (50,), 40000, 3.0, 4, None, {"RNNWF_BASE": "f32"}),
    ("cfg5-x1.5", "gru", (200, 1), (100,), 32768, 1.5, 8, "bf16x3", {}),
    ("cfg5-x3", "gru", (200, 1), (100,), 32768, 3.0, 8, "bf16x3", {}),
    # one width per class of the bf16x3 engine: flat <= 36 | aligned 37..50 | padded 51..52 | riders 53..68 | streamed 69..100
    ("width-36", "gru", (40, 1), (36,), 4096, 3.0, 1, "bf16x3", {}),
    ("width-44", "gru", (40, 1), (44,), 4096, 3.0, 1, "bf16x3", {}),
    ("width-52", "gru", (40, 1), (52,), 4096, 3.0, 1, "bf16x3", {}),
    ("width-64", "gru", (40, 1), (64,), 4096, 3.0, 1, "bf16x3", {}),
    ("width-96", "gru", (40, 1), (96,), 4096, 3.0, 1, "bf16x3", {}),
    ("wide-128", "gru", (40, 1), (128,), 4096, 3.0, 1, "f32mfma", {}),
    ("long-1000", "gru", (1000, 1), (50,), 96, 2.0, 1, None, {}),      # x 3 breaks the cap on the CPU oracle (17 of 96 rows)
    ("cfg2_l2", "gru", (80, 1), (50, 50), 10000, 3.0, 1, "bf16x3", {}),
    ("stack-64-20", "gru", (40, 1), (64, 20), 10000, 3.0, 2, "f32mfma", {}),
    ("stack-3-layers", "gru", (40, 1), (50, 50, 50), 4096, 3.0, 1, None, {}),
    ("parity-40", "parity", (40, 1), (50,), 9008, 3.0, 1, "bf16x3", {}),
    ("cfg3", "crnn", (40, 1), (50,), 10000, 3.0, 1, "bf16x3", {}),
    ("cfg3_l2", "crnn", (40, 1), (50, 50), 10000, 3.0, 1, "bf16x3", {}),
    ("cfg4-x1.25", "mdrnn", (12, 12), (50,), 10000, 1.25, 2, "f64mfma", {}),
    ("gru64-100", "gru64", (12, 12), (100,), 2048, 3.0, 1, "f64mfma", {}),
    ("gru64-50-50", "gru64", (12, 12), (50, 50), 2048, 3.0, 1, "f64mfma", {}),
    ("lstm-50", "lstm", (12, 12), (50,), 2048, 3.0, 1, None, {}),
    ("lstm-68", "lstm", (12, 12), (68,), 2048, 3.0, 1, None, {}),
    ("lstm-50-passes", "lstm", (12, 12), (50,), 2048, 3.0, 1, None, {"RNNWF_STATE_BUDGET_MB": "1"}),
]
