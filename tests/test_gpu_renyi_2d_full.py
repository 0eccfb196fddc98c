"""The paired masked-tail pass of rnnwf_renyi2_regions_2d (mdrnn_masked_tail_kernel<..., PAIRED = true>, csrc/mdrnn_pauli_kernels.h)
against an independent float64 reference on lattices of three to eight spin words: the cases of tests/test_gpu_pauli_2d_full.py,
chains (2p, 2p + 1) a replica pair, after the pattern of tests/test_gpu_renyi_regions_full.py.

Each case draws its pairs on the device (seed 111, step 0) from pauli_2d_reference.weights(H, 111, 1.0) and checks

  (a) log r of EVERY region of renyi_2d_reference.region_set_2d (coverage asserted by check_case_2d) on the whole pairs of the chain
      subset of pauli_reference.choose_chains (asserted by check_subset: every chain of the first, a middle and the last full 16-chain
      block and of the ragged last block, >= 32 chains) against log_ratio_regions: both swapped configurations written out and scored
      by oracle.models.mdrnn_log_probability in float64 NumPy - the very chains the device drew.  Bound: 1e-11 N (R.BOUND), never
      derived from the kernel.  dev64, the deviation of the reference's own float64 re-ordering (kernel_form against the brute
      force), is computed at run time, printed, and must stay below 1/16 of the bound;
  (b) the inputs are not bland: every reference entry finite, max |log r| > 0.1, at least a quarter of the entries above 0.01;
  (c) on 12x12: non-empty regions x blocks >= 16 384 tiles = 2 x 256 CUs x 32 wave slots, so every wave of the persistent grid takes at
      least two tiles in ONE launch, and the work counter is exact;
  (d) sums against exactly rounded sums (math.fsum) of the device's own log r, all pairs: relative 1e-12; the empty and the full region
      give log r = 0 and sums = npairs exactly;
  (e) the returned samples passed back as the caller's give the same log-ratio bits.

Kernels x 1, and x 0.75 for a case whose device-drawn chains give a non-finite reference at x 1, which its line then says (SCALES).
Every case prints one RENYI_2D_FULL line; docs/renyi_2d.md records the figures.
"""
import time

import numpy as np
import pytest

import pauli_2d_reference as Q
import pauli_reference as PR
import renyi_2d_reference as R
import renyi_reference as RR
from oracle import models as M

pytestmark = pytest.mark.gpu

SCALES = (1.0, 0.75)


def make_wf(Nx, Ny, H, prm):
    from rnnwavefunctions_amd import _lib
    wf = _lib.NativeWavefunction(_lib.MODEL_MDRNN2D, Nx, Ny, (H,))
    wf.set_params(prm, scope=R.SCOPE)
    wf.timing_enable(True)
    return wf


def region_set(Nx, Ny):
    names, masks = zip(*R.region_set_2d(Nx, Ny, fill=Q.FILL.get((Nx, Ny), Q.MIN_MASKS)))
    masks = np.stack(masks)
    R.check_case_2d(Nx, Ny, masks)
    return list(names), masks


def run(wf, masks, npairs, **kw):
    wf.timing_reset()
    out = wf.renyi2_regions_2d(masks, npairs, log_ratio=True, **kw)
    out["timing"] = wf.timing_get(1)
    return out


def drawn(wf, masks, npairs):
    return run(wf, masks, npairs, seed=111, step=0)


def choose_pair_chains(ns):
    """pauli_reference.choose_chains' subset, which holds whole pairs: (chains, their pairs)"""
    idx = PR.choose_chains(ns)
    assert set((idx ^ 1).tolist()) == set(idx.tolist()) and np.array_equal(idx[0::2] + 1, idx[1::2])
    return idx, idx[0::2] // 2


def reference(prm, s, masks):
    """(brute-force float64 log r (R, pairs), dev64 = its deviation from the kernel's order of the same float64 arithmetic)"""
    ref = R.log_ratio_regions(lambda x: M.mdrnn_log_probability(prm, x), s, masks)
    if not np.all(np.isfinite(ref)):
        return ref, float("nan")
    return ref, float(np.abs(R.kernel_form(prm, s, masks) - ref).max())


def check(label, prm, shape, npairs, names, masks, out, ref=None, dev64=None, t0=None):
    """(a), (b) and (d) of one result with log_ratio and samples; prints the case's line, returns the ratio"""
    t0 = time.time() if t0 is None else t0
    Nx, Ny = shape
    N, ns = Nx * Ny, 2 * npairs
    lr, sums, s = out["log_ratio"], out["sums"], out["samples"]
    assert lr.shape == (len(masks), npairs) and sums.shape == (len(masks), 2) and s.shape == (ns, Nx, Ny)
    assert np.all(np.isfinite(lr)) and np.all(np.isfinite(sums)) and np.all((s == 0) | (s == 1))
    idx, pidx = choose_pair_chains(ns)
    mv = Q.to_visit_order(masks, Nx, Ny)
    PR.check_subset(ns, N, idx, mv[mv.any(axis=1)])
    if ref is None:
        ref, dev64 = reference(prm, s[idx], masks)
    assert ref.shape == (len(masks), len(pidx)) and len(idx) >= 32              # every region on every chosen pair
    assert np.all(np.isfinite(ref)), "the float64 reference is not finite"
    mx, share = RR.nontrivial(ref)
    bound = R.BOUND * N
    d = np.abs(lr[:, pidx] - ref)
    k, c = np.unravel_index(int(np.argmax(d)), d.shape)
    err, ratio = float(d[k, c]), float(d[k, c] / bound)
    resum = RR.sums_from_log_ratio(lr)                                           # the device's own log r, re-summed exactly
    rel = float(np.abs(sums / resum - 1.0).max())
    trivial = [k for k, m in enumerate(masks) if not m.any() or m.all()]
    active = sum(R.normalise(m)[1] > 0 for m in mv)
    t = out["timing"]
    print("RENYI_2D_FULL %-26s err %.3e region %3d (%s) pair %4d chains %d/%d block %3d | bound %.3e ratio %6.3f | dev64 %.2e | "
          "%d regions x %d pairs | max |log r| %.1f, %.0f %% above 0.01 | sums rel %.1e | %d tiles, %d launch(es), tail %.2f ms | ref %.1f s"
          % (label, err, k, names[k], pidx[c], 2 * pidx[c], 2 * pidx[c] + 1, pidx[c] // 8, bound, ratio, dev64, len(masks), len(pidx), mx,
             100 * share, rel, active * ((ns + 15) // 16), t["launches"], t["total_ms"], time.time() - t0))
    assert mx > 0.1 and share >= 0.25, "bland inputs: max |log r| %.3f, share above 0.01 %.2f" % (mx, share)
    assert dev64 <= bound / 16, "the reference's own re-ordering deviates by %.2e > bound / 16" % dev64
    assert rel <= 1e-12
    assert len(trivial) == 2 and np.all(lr[trivial] == 0.0) and np.all(sums[trivial] == float(npairs))
    assert err <= bound, "%s: |d log r| %.3e > bound %.3e at region %d (%s), pair %d" % (label, err, bound, k, names[k], pidx[c])
    return ratio


# (Nx, Ny), units, chains (pairs = chains / 2), what the case is for
CASES = [
    ((13, 5), 36, 1006, "one position in the third word; Nx odd; row turns off the word grid"),
    ((5, 13), 68, 1006, "the same sites, 13 rows; the NFULL 5 row at occupancy 1 (68 units)"),
    ((9, 11), 17, 1006, "four words; NFULL 1 with remainder 1"),
    ((12, 12), 50, 2006, "config 4's lattice, five words; the tile loop; ragged block of 6 chains = 3 pairs"),
    ((16, 16), 20, 406, "256 sites, the largest lattice the model accepts: bit 31 of word 7"),
    ((16, 16), 84, 406, "the widest width on the largest lattice"),
]


def _id(c):
    return "%dx%d-%d-%d" % (c[0][0], c[0][1], c[1], c[2])


@pytest.mark.parametrize("shape,H,ns,why", CASES, ids=[_id(c) for c in CASES])
def test_log_ratio_and_sums_against_the_float64_reference(shape, H, ns, why):
    t0 = time.time()
    Nx, Ny = shape
    N, npairs = Nx * Ny, ns // 2
    names, masks = region_set(Nx, Ny)
    idx, _ = choose_pair_chains(ns)
    for scale in SCALES:                                 # x 0.75 only where the chains drawn at x 1 give a non-finite reference
        prm = Q.weights(H, 111, scale)
        wf = make_wf(Nx, Ny, H, prm)
        out = drawn(wf, masks, npairs)
        ref, dev64 = reference(prm, out["samples"][idx], masks)
        if np.all(np.isfinite(ref)):
            break
        print("[%s] kernels x %.2f: %d of %d reference entries are not finite" % (_id((shape, H, ns)), scale, int((~np.isfinite(ref)).sum()), ref.size))
    label = "[%s x%.2f]" % (_id((shape, H, ns)), scale)
    check(label, prm, shape, npairs, names, masks, out, ref, dev64, t0)
    # (c) the work of the one launch; on 12x12 every wave of the persistent grid takes at least two tiles
    firsts = [R.normalise(m)[1] for m in Q.to_visit_order(masks, Nx, Ny)]
    assert out["timing"]["launches"] == 1 and out["timing"]["cell_evals"] == ns * sum(N - 1 - f for f in firsts if f > 0)
    if shape == (12, 12):
        assert sum(f > 0 for f in firsts) * ((ns + 15) // 16) >= 16384
    # (e) the caller's-samples path
    fed = run(wf, masks, npairs, samples=out["samples"])
    assert "samples" not in fed and np.array_equal(fed["log_ratio"], out["log_ratio"]) and np.array_equal(fed["sums"], out["sums"])


def test_several_passes_equal_one_pass_and_the_reference(monkeypatch):
    """12x12, 50 units, 1003 pairs under a 15 MB state budget: at least three passes of whole 16-chain blocks, the last one ragged
    (3 pairs).  Bit-equal per pair to the one-pass call, and checked against the reference."""
    shape, H, ns = (12, 12), 50, 2006
    prm = Q.weights(H, 111, 1.0)
    names, masks = region_set(*shape)
    one = drawn(make_wf(12, 12, H, prm), masks, ns // 2)
    monkeypatch.setenv("RNNWF_STATE_BUDGET_MB", "15")
    many = drawn(make_wf(12, 12, H, prm), masks, ns // 2)
    passes = many["timing"]["launches"]                                       # one masked-tail launch per pass
    print("[12x12-50-2006 passes] %d pass(es) by default, %d under RNNWF_STATE_BUDGET_MB=15" % (one["timing"]["launches"], passes))
    assert one["timing"]["launches"] == 1 and passes >= 3 and ns % 16 != 0
    assert np.array_equal(many["samples"], one["samples"]) and np.array_equal(many["log_ratio"], one["log_ratio"])
    assert np.allclose(many["sums"], one["sums"], rtol=1e-12, atol=0)
    check("[12x12-50-2006 passes]", prm, shape, ns // 2, names, masks, many)
