"""The masked-tail pass of rnnwf_pauli_step_2d (mdrnn_masked_tail_kernel, csrc/mdrnn_pauli_kernels.h) against an independent float64
reference on lattices of three to eight spin words: the smallest lattices that reach each word count (13x5 / 5x13: 3, 9x11: 4,
12x12 - config 4's - : 5, 16x16: 8, the largest the model accepts), after the pattern of tests/test_gpu_pauli_full.py.

Each case draws its chains on the device (seed 111, step 0) from pauli_2d_reference.weights(H, 111, 1.0) and checks

  (a) log r of EVERY mask of pauli_2d_reference.mask_set_2d (coverage asserted by check_case_2d) on the chain subset of
      pauli_reference.choose_chains (asserted by check_subset: every chain of the first, a middle and the last full 16-chain block and
      of the ragged last block, >= 32 chains) against explicit_log_ratio: the flipped configurations written out and scored by
      oracle.models.mdrnn_log_probability in float64 NumPy - the very chains the device drew.  Bound: 1e-11 N (Q.BOUND), the project's
      float64 bound, never derived from the kernel.  dev64, the deviation of the reference's own float64 re-ordering (kernel_form
      against explicit), is computed at run time, printed, and must stay below 1/16 of the bound;
  (b) the inputs are not bland: every reference entry finite, max |log r| > 0.1, at least a quarter of the entries above 0.01;
  (c) on 12x12: masks x blocks >= 16 384 tiles = 2 x 256 CUs x 32 wave slots, so every wave of the persistent grid takes at least two
      tiles (its LDS word slot and column slots reused under another mask and f) in ONE launch, and the work counter is exact;
  (d) term_sums and E_loc of sign_strings_2d (Z and Y letters in every word) against exactly rounded sums (math.fsum) of the device's
      own log r with the signs taken in NumPy from the returned samples by lattice index: relative 1e-12 (E_loc, a signed sum of K
      terms: relative to sum_k |c_k v_k|); the string of odd n_Y is exactly 0 +- 0;
  (e) the returned samples passed back as the caller's give the same log-ratio bits.

Kernels x 1: sharper kernels drive the elu state of flipped configurations off to where the float64 reference is -inf.  A case whose
device-drawn chains give a non-finite reference at x 1 runs at x 0.75 instead and says so in its line (SCALES).
Every case prints one PAULI_2D_FULL line; docs/pauli_2d.md records the figures.
"""
import math
import time

import numpy as np
import pytest

import pauli_2d_reference as Q
import pauli_reference as PR
import renyi_reference as RR
from oracle import models as M
from rnnwavefunctions_amd import observables as O
from rnnwavefunctions_amd import observables_2d as O2

pytestmark = pytest.mark.gpu

SCALES = (1.0, 0.75)
DENORMAL = 5e-324            # per summand: where a sum lies in the denormal range, a double no longer carries a relative 1e-12


def make_wf(Nx, Ny, H, prm):
    from rnnwavefunctions_amd import _lib
    wf = _lib.NativeWavefunction(_lib.MODEL_MDRNN2D, Nx, Ny, (H,))
    wf.set_params(prm, scope=Q.SCOPE)
    wf.timing_enable(True)
    return wf


def mask_set(Nx, Ny):
    names, masks = zip(*Q.mask_set_2d(Nx, Ny, fill=Q.FILL.get((Nx, Ny), Q.MIN_MASKS)))
    masks = np.stack(masks)
    Q.check_case_2d(Nx, Ny, masks)
    return list(names), masks


def run(wf, masks, ns, **kw):
    wf.timing_reset()
    out = wf.pauli_step_2d(masks, np.zeros_like(masks), np.ones(len(masks)), ns, want_log_ratio=True, **kw)
    out["timing"] = wf.timing_get(1)
    return out


def drawn(wf, masks, ns):
    return run(wf, masks, ns, seed=111, step=0, want_samples=True)


def reference(prm, s, masks):
    """(explicit float64 log r (M, chains), dev64 = its deviation from the kernel's order of the same float64 arithmetic)"""
    ref = Q.explicit_log_ratio(lambda x: M.mdrnn_log_probability(prm, x), s, masks)
    if not np.all(np.isfinite(ref)):
        return ref, float("nan")
    return ref, float(np.abs(Q.kernel_form(prm, s, masks) - ref).max())


def sums_rel(got, want, ns):
    """asserts |got - want| <= 1e-12 |want| (+ one denormal step per summand); returns the largest relative deviation"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape and np.all(np.isfinite(want))
    assert np.all(np.abs(got - want) <= 1e-12 * np.abs(want) + ns * DENORMAL), "sums beyond relative 1e-12"
    big = np.abs(want) > 1e-280
    return float(np.abs(got[big] / want[big] - 1.0).max()) if big.any() else 0.0


def check_log_ratio(label, prm, shape, ns, names, masks, out, ref=None, dev64=None, t0=None):
    """(a), (b) and the flip-only sums of one result with log_ratio and samples; prints the case's line, returns the ratio"""
    t0 = time.time() if t0 is None else t0
    Nx, Ny = shape
    N = Nx * Ny
    lr, sums, s = out["log_ratio"], out["term_sums"], out["samples"]
    assert lr.shape == (len(masks), ns) and sums.shape == (len(masks), 2) and s.shape == (ns, Nx, Ny)
    assert np.all(np.isfinite(lr)) and np.all(np.isfinite(sums)) and np.all((s == 0) | (s == 1))
    idx = PR.choose_chains(ns)
    PR.check_subset(ns, N, idx, Q.to_visit_order(masks, Nx, Ny))
    if ref is None:
        ref, dev64 = reference(prm, s[idx], masks)
    assert ref.shape == (len(masks), len(idx)) and len(idx) >= 32           # every mask on every chosen chain
    assert np.all(np.isfinite(ref)), "the float64 reference is not finite"
    mx, share = RR.nontrivial(ref)
    bound = Q.BOUND * N
    d = np.abs(lr[:, idx] - ref)
    k, c = np.unravel_index(int(np.argmax(d)), d.shape)
    err, ratio = float(d[k, c]), float(d[k, c] / bound)
    rel = sums_rel(sums, RR.sums_from_log_ratio(lr), ns)                     # the device's own log r, re-summed exactly
    t = out["timing"]
    print("PAULI_2D_FULL %-26s err %.3e mask %3d (%s) chain %4d block %3d | bound %.3e ratio %6.3f | dev64 %.2e | %d masks x %d chains | "
          "max |log r| %.1f, %.0f %% above 0.01 | sums rel %.1e | %d tiles, %d launch(es), tail %.2f ms | ref %.1f s"
          % (label, err, k, names[k], idx[c], idx[c] // 16, bound, ratio, dev64, len(masks), len(idx), mx, 100 * share, rel,
             len(masks) * ((ns + 15) // 16), t["launches"], t["total_ms"], time.time() - t0))
    assert mx > 0.1 and share >= 0.25, "bland inputs: max |log r| %.3f, share above 0.01 %.2f" % (mx, share)
    assert dev64 <= bound / 16, "the reference's own re-ordering deviates by %.2e > bound / 16" % dev64
    assert err <= bound, "%s: |d log r| %.3e > bound %.3e at mask %d (%s), chain %d" % (label, err, bound, k, names[k], idx[c])
    return ratio


def check_strings(wf, shape, ns, s):
    """(d): term sums and E_loc of sign_strings_2d on the chains s, against the device's own log r and NumPy's signs"""
    Nx, Ny = shape
    N = Nx * Ny
    strings = Q.sign_strings_2d(Nx, Ny)
    flip, sign, factor = O.pauli_terms(strings, N)
    even = np.flatnonzero(factor.imag == 0)
    assert len(even) == len(strings) - 1 and factor[-1].imag != 0
    flip, sign, coeff = flip[even], sign[even], factor.real[even]
    out = wf.pauli_step_2d(flip, sign, coeff, ns, samples=s, want_log_ratio=True, want_eloc=True)
    _, index = O.group_by_mask(flip)
    assert np.any(index < 0) and out["log_ratio"].shape == (index.max() + 1, ns)
    v = PR.signs(s.reshape(ns, N), sign) * np.where(index[:, None] >= 0, np.exp(out["log_ratio"][np.maximum(index, 0)]), 1.0)
    assert np.all(np.abs(v).max(axis=1) > 0) and (v < 0).any() and (v > 0).any()             # the signs are at work
    rel = sums_rel(out["term_sums"], PR.sums_from_values(v), ns)
    cv = coeff[:, None] * v
    e_ref = np.array([math.fsum(col) for col in cv.T])
    e_rel = float((np.abs(out["eloc"] - e_ref) / np.abs(cv).sum(axis=0)).max())
    assert e_rel <= 1e-12, "E_loc beyond 1e-12 of sum |c v|: %.2e" % e_rel
    ex = O2.pauli_expectations(wf, strings, ns, samples=s)
    assert ex["value"][-1] == 0.0 and ex["err"][-1] == 0.0                                   # odd n_Y: exactly 0 +- 0
    assert np.array_equal(ex["value"][:-1], coeff * (out["term_sums"][:, 0] / ns))
    return max(rel, e_rel), len(strings)


# (Nx, Ny), units, chains, what the case is for
CASES = [
    ((13, 5), 36, 1006, "one position in the third word; Nx odd; row turns off the word grid"),
    ((5, 13), 68, 1006, "the same sites, 13 rows; the NFULL 5 row at occupancy 1 (68 units)"),
    ((9, 11), 17, 1006, "four words; NFULL 1 with remainder 1"),
    ((12, 12), 50, 2006, "config 4's lattice, five words; the tile loop; ragged block of 6 chains"),
    ((16, 16), 20, 406, "256 sites, the largest lattice the model accepts: bit 31 of word 7"),
    ((16, 16), 84, 406, "the widest width on the largest lattice"),
]


def _id(c):
    return "%dx%d-%d-%d" % (c[0][0], c[0][1], c[1], c[2])


@pytest.mark.parametrize("shape,H,ns,why", CASES, ids=[_id(c) for c in CASES])
def test_log_ratio_sums_and_strings_against_the_float64_reference(shape, H, ns, why):
    t0 = time.time()
    Nx, Ny = shape
    N = Nx * Ny
    names, masks = mask_set(Nx, Ny)
    idx = PR.choose_chains(ns)
    for scale in SCALES:                                 # x 0.75 only where the chains drawn at x 1 give a non-finite reference
        prm = Q.weights(H, 111, scale)
        wf = make_wf(Nx, Ny, H, prm)
        out = drawn(wf, masks, ns)
        ref, dev64 = reference(prm, out["samples"][idx], masks)
        if np.all(np.isfinite(ref)):
            break
        print("[%s] kernels x %.2f: %d of %d reference entries are not finite" % (_id((shape, H, ns)), scale, int((~np.isfinite(ref)).sum()), ref.size))
    label = "[%s x%.2f]" % (_id((shape, H, ns)), scale)
    check_log_ratio(label, prm, shape, ns, names, masks, out, ref, dev64, t0)
    # (c) the work of the one launch; on 12x12 every wave of the persistent grid takes at least two tiles
    firsts = [int(np.flatnonzero(m)[0]) for m in Q.to_visit_order(masks, Nx, Ny)]
    assert out["timing"]["launches"] == 1 and out["timing"]["cell_evals"] == ns * sum(N - 1 - f for f in firsts)
    if shape == (12, 12):
        assert len(masks) * ((ns + 15) // 16) >= 16384
    # (d)
    rel, nstr = check_strings(wf, shape, ns, out["samples"])
    # (e) the caller's-samples path
    fed = run(wf, masks, ns, samples=out["samples"])
    assert np.array_equal(fed["log_ratio"], out["log_ratio"]) and np.array_equal(fed["term_sums"], out["term_sums"])
    print("%s %d sign strings: sums and E_loc rel %.1e; the returned samples fed back give the same bits" % (label, nstr, rel))


def test_several_passes_equal_one_pass_and_the_reference(monkeypatch):
    """12x12, 50 units, 2006 chains under a 15 MB state budget: at least three passes of whole 16-chain blocks, the last one ragged.
    Bit-equal per chain to the one-pass call, and checked against the reference."""
    shape, H, ns = (12, 12), 50, 2006
    prm = Q.weights(H, 111, 1.0)
    names, masks = mask_set(*shape)
    one = drawn(make_wf(12, 12, H, prm), masks, ns)
    monkeypatch.setenv("RNNWF_STATE_BUDGET_MB", "15")
    many = drawn(make_wf(12, 12, H, prm), masks, ns)
    passes = many["timing"]["launches"]                                       # one masked-tail launch per pass
    print("[12x12-50-2006 passes] %d pass(es) by default, %d under RNNWF_STATE_BUDGET_MB=15" % (one["timing"]["launches"], passes))
    assert one["timing"]["launches"] == 1 and passes >= 3 and ns % 16 != 0
    assert np.array_equal(many["samples"], one["samples"]) and np.array_equal(many["log_ratio"], one["log_ratio"])
    assert np.allclose(many["term_sums"], one["term_sums"], rtol=1e-12, atol=0)
    check_log_ratio("[12x12-50-2006 passes]", prm, shape, ns, names, masks, many)


def test_single_x_masks_against_tfim2d_eloc_on_12x12():
    """The single-X rows of every lattice site against rnnwf_tfim2d_eloc's queue on the same samples (tests/test_gpu_pauli_2d.py's
    case 3 on five words)."""
    Nx, Ny, H, ns = 12, 12, 50, 100
    N = Nx * Ny
    wf = make_wf(Nx, Ny, H, Q.weights(H, 111, 1.0))
    s = wf.sample(ns, seed=3)
    lpq = np.empty((N + 1, ns))
    wf.tfim_eloc(s, np.ones((Nx, Ny)), 1.0, log_probs=lpq)
    out = run(wf, np.eye(N, dtype=np.int32), ns, samples=s)
    ref = 0.5 * (lpq[1:] - lpq[0][None, :])                             # queue row nx*Ny + ny + 1 = the flip of lattice site k
    err = float(np.abs(out["log_ratio"] - ref).max())
    print("PAULI_2D_FULL [12x12-50-100 tfim queue] max |log r_k - queue| = %.3e | bound %.3e ratio %.3f" % (err, Q.BOUND * N, err / (Q.BOUND * N)))
    assert np.all(np.isfinite(ref)) and np.abs(ref).max() > 0.1
    assert err <= Q.BOUND * N
