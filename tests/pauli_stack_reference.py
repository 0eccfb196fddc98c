"""Float64 reference of the Pauli-string estimator for STACKED GRU layers (docs/pauli_stack.md), independent of the library: plain
NumPy on the oracle's stacked GRU (oracle.models.prnn_log_probability over multi_gru; layers of unequal width included).  TEST
INFRASTRUCTURE ONLY; validated by tests/test_pauli_stack_reference.py.

    O = (prod_{i in S} sz_i)(prod_{i in F} sx_i),   v(sigma) = prod_{i in S} (2 sigma_i - 1) * exp(1/2 [log P(sigma ^ F) - log P(sigma)])

Brute force on purpose, as tests/pauli_reference.py: every flipped configuration is written out in full and scored from site 0 - no
first site, no checkpoint, no packed words.  The one thing taken from the library's conventions is the ORDER of the log-ratio rows:
the distinct non-empty flip masks in order of first appearance (observables.group_by_mask).

Bounds, none taken from a kernel under test:
  float64   |log r - ref| <= 1e-11 N per log-ratio: the project's float64 bound (tests/test_gpu_raster_eloc_full.py applies it to
            float64 stacks).
  float32   twice the error of the EXISTING stack flip pass (the log-probability queue of tfim_eloc against this oracle) measured at
            the same shape on the code before the stack entries existed: F32_MEASURED below, docs/pauli_stack.md has the table.
  E_loc     from the reference's own ratios: |E - ref| <= sum_k |c_k| r_k (expm1(tol) + 1e-13), r_k = exp(ref log-ratio) (1 for a
            diagonal term): what the log-ratio bound lets through, and a few float64 roundings of the sum
            (tests/raster_eloc_reference.py builds its bound the same way).
"""
import math

import numpy as np

import pauli_reference as PR
import sampler_reference as R
from oracle import models as M
from rnnwavefunctions_amd import observables as O

SCOPE = R.SCOPE
SUM_TOL = 1e-13

# max |lp - lp_ref| over the whole log-probability queue (N + 1 rows x ns chains drawn with sample(ns, seed=111, step=0)) of the
# existing stack flip pass, float32, weights build_params("gru", units, seed=111, sharp=3): (units, N, ns) -> error.  Measured on an
# MI355X with the library of the commit before the stack entries (tfim_eloc(..., log_probs=), f32-input MFMA flip kernel
# prnn_ml_flip_kernel; this change leaves those kernels' assembly as it was, and its own build measures the same values to the bit).
F32_MEASURED = {
    ((10, 10), 6, 37): 1.999e-06, ((10, 10, 10), 6, 37): 1.803e-06, ((10, 10, 10, 10), 6, 37): 2.440e-06, ((20, 20), 6, 37): 1.502e-06,
    ((37, 37), 6, 37): 1.553e-06, ((50, 50), 6, 37): 2.092e-06, ((68, 68), 6, 37): 2.568e-06, ((100, 100), 6, 37): 2.516e-06,
    ((10, 20), 6, 37): 3.867e-06, ((37, 20), 6, 37): 1.235e-06, ((10, 10), 34, 37): 1.442e-05, ((10, 10), 34, 4000): 2.356e-05,
}


def f64_tol(N):
    return 1e-11 * N


def f32_tol(units, N, ns):
    """twice the existing flip pass's measured error at this shape"""
    return 2.0 * F32_MEASURED[tuple(units), N, ns]


def weights(family, units, seed=111, sharp=3.0):
    """sharpened weights (kernels x sharp, every bias randomised), as the full-size tests of the flip passes build them"""
    return R.build_params(family, units, seed=seed, sharp=sharp)


def scorer(prm, dtype=np.float64):
    p = R.cast(prm, dtype)
    return lambda x: M.prnn_log_probability(p, np.asarray(x), dtype=dtype)


def reference(prm, samples, ham):
    """dict(log_ratio (nmasks, ns) - rows: the distinct non-empty flip masks in order of first appearance -, values (K, ns), eloc
    (ns,), term_sums (K, 2), bound_weight (ns,) = sum_k |c_k| r_k) of the Hamiltonian `ham` on `samples` (ns, N), float64."""
    samples = np.asarray(samples).reshape(len(samples), -1)
    log_p = scorer(prm)
    masks, index = O.group_by_mask(ham.flip)
    with np.errstate(over="ignore"):
        lr = PR.log_ratio_masks(log_p, samples, masks)
        r = np.where(index[:, None] >= 0, np.exp(lr[np.maximum(index, 0)]), 1.0) if len(masks) else np.ones((len(index), len(samples)))
    v = PR.signs(samples, ham.sign) * r
    coeff = np.asarray(ham.coeff, dtype=np.float64)
    return dict(log_ratio=lr, values=v, eloc=coeff @ v, term_sums=PR.sums_from_values(v), bound_weight=np.abs(coeff) @ r)


def eloc_bound(ref, tol):
    return ref["bound_weight"] * (math.expm1(tol) + SUM_TOL)


def judge(label, out, ref, tol, echo=print):
    """asserts log-ratios, E_loc and per-term sums of a pauli_step_stack result against `reference`; returns the figures"""
    lr, e, sums = out["log_ratio"], out["eloc"], out["term_sums"]
    assert lr.shape == ref["log_ratio"].shape and np.all(np.isfinite(lr)) and np.all(np.isfinite(e))
    d = np.abs(lr - ref["log_ratio"])
    worst = np.unravel_index(int(np.argmax(d)), d.shape) if d.size else (0, 0)
    lr_err = float(d.max()) if d.size else 0.0
    eb = eloc_bound(ref, tol)
    e_over = float((np.abs(e - ref["eloc"]) / eb).max())
    # the sums add ns values v held to |v| expm1(tol) each (v^2: v^2 expm1(2 tol)): bounded by the sums of those bounds, per term
    r = np.abs(ref["values"])
    s_bound = np.stack([r.sum(axis=1) * (math.expm1(tol) + SUM_TOL), (r * r).sum(axis=1) * (math.expm1(2.0 * tol) + SUM_TOL)], axis=1)
    s_over = float((np.abs(sums - ref["term_sums"]) / s_bound).max())
    echo("%s: max |d log r| %.3e = %.3f x tol %.3e (mask row %d, chain %d); E_loc %.3f x bound; term sums %.3f x bound; log r in [%.2f, %.2f]"
         % (label, lr_err, lr_err / tol, tol, worst[0], worst[1], e_over, s_over,
            ref["log_ratio"].min() if d.size else 0.0, ref["log_ratio"].max() if d.size else 0.0))
    assert lr_err <= tol, "%s: mask row %d, chain %d (block %d): |log r - ref| = %.3e > %.3e" % (label, worst[0], worst[1], worst[1] // 16, lr_err, tol)
    assert e_over <= 1.0, "%s: E_loc beyond its bound by %.3f" % (label, e_over)
    assert s_over <= 1.0, "%s: per-term sums beyond their bound by %.3f" % (label, s_over)
    return dict(lr_err=lr_err, e_over=e_over, s_over=s_over)


# ---- Hamiltonians of the tests -------------------------------------------------------------------------------------------------------

def hamiltonian(name, N):
    """xxz: pair masks; tfim: single-site masks, site 0 and site N - 1 among them; diagonal: no flip mask; mixed: a three-site string,
    a long-range XX between the first and the last site, a string across every 32-site word boundary, the dense mask."""
    zz = [(-(1.0 + 0.1 * i), [("Z", i), ("Z", i + 1)]) for i in range(N - 1)]
    if name == "xxz":
        return O.xxz_hamiltonian(N, -1.0, 0.5)
    if name == "tfim":
        return O.Hamiltonian(N, zz + [(-(0.5 + 0.07 * k), [("X", k)]) for k in range(N)])
    if name == "diagonal":
        return O.Hamiltonian(N, zz + [(0.3, [("Z", k)]) for k in range(N)])
    if name == "mixed":
        terms = O.xxz_hamiltonian(N, -1.0, 0.5).terms + [(0.4, [("X", 0), ("Z", 1), ("X", 2)]), (-0.3, [("X", 0), ("X", N - 1)]),
                                                        (0.25, [("X", N - 1)]), (0.2, [("X", 0)]), (0.15, [("X", i) for i in range(N)])]
        for w in range(32, N, 32):
            terms.append((0.35, [("X", i) for i in range(w - 2, min(N, w + 3))]))
        return O.Hamiltonian(N, terms)
    raise KeyError(name)


def dense(ham):
    return sum(c * PR.dense_string({i: p for p, i in st}, ham.N).real for c, st in ham.terms)
