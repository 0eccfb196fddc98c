"""The region pass of the second Renyi entropy (rnnwf_renyi2_regions: csrc/renyi_regions.hip, csrc/renyi_region_kernels.h) against
an independent float64 reference, at the sizes the library is used and measured at.

Each case draws its chains on the device from SHARPENED weights (kernels x 3, x 2 above 60 units, every bias randomised, as
tests/test_gpu_renyi_full.py), takes log r of every pair and region, the sums and the samples, and checks

  * log r per pair and region against tests/renyi_regions_reference.py (brute force in float64 NumPy on the oracle's GRU, scoring the
    very chains the device drew; validated by tests/test_renyi_regions_reference.py) for EVERY region of the case's set - all column
    cuts, corner and bulk squares (2D), bulk intervals, intervals ending and starting on each 32-site word boundary, a two-piece
    region, a checkerboard, a region containing site 0 - on a chain subset that the test asserts (check_subset) to contain all 8 pairs
    of the first, a middle and the last full 16-chain block and EVERY pair of the ragged last block; >= 32 pairs per region;
  * sums against an exactly rounded float64 re-summation (math.fsum) of the device's OWN log r array, all pairs: relative 1e-12;
  * everything finite and the inputs non-trivial: max |log r| > 0.1 and at least a quarter of the checked entries above 0.01.

Bounds - the rule and factor of tests/test_gpu_renyi_full.py, never derived from the kernels:
  * float32: 16 x dev32, dev32 = the largest deviation of the FLOAT32 NumPy oracle from the float64 reference on the same pairs and
    regions, computed here at run time; capped at 2 (2e-6 N + 2e-6).  Where dev32 itself is beyond the cap, the case says so and
    16 x dev32 stands uncapped.
  * float64: 1e-11 N.

Measured on MI355X: profiles/renyi_regions_full_size.txt.
"""
import time

import numpy as np
import pytest

import renyi_reference as R
import renyi_regions_reference as G
from rnnwavefunctions_amd import params as P

pytestmark = pytest.mark.gpu

SCOPE = "RNNwavefunction"


def sharpened(H, f64, seed=111):
    prm = P.init_gru_params([H], seed=seed, dtype=np.float64 if f64 else np.float32)
    return P.randomize_biases(P.scale_kernels(prm, 2.0 if H > 60 else 3.0), seed + 1)


def make_wf(f64, Nx, Ny, H, prm):
    from rnnwavefunctions_amd import _lib
    wf = _lib.NativeWavefunction(_lib.MODEL_GRU1D_F64 if f64 else _lib.MODEL_GRU1D, Nx, Ny, (H,))
    wf.set_params(prm, scope=SCOPE)
    return wf


def check(label, f64, prm, shape, npairs, names, masks, out):
    """Everything a case asserts about one renyi2_regions result with log_ratio and samples.  Returns the comparator's record."""
    t0 = time.time()
    N = shape[0] * shape[1]
    lr, sums, s = out["log_ratio"], out["sums"], out["samples"]
    assert lr.shape == (len(masks), npairs) and sums.shape == (len(masks), 2) and s.shape == (2 * npairs, N)
    assert np.all(np.isfinite(lr)) and np.all(np.isfinite(sums)) and np.all((s == 0) | (s == 1))

    idx = G.choose_pairs(npairs)
    G.check_subset(npairs, N, idx, masks)
    ref = G.log_ratio(prm, s, masks, dtype=np.float64, pair_idx=idx)
    assert ref.shape == (len(masks), len(idx)) and len(idx) >= 32           # every region on every chosen pair
    mx, share = R.nontrivial(ref)
    if f64:
        bound, dev32, how = R.f64_bound(N), float("nan"), "1e-11 N"
    else:
        dev32 = float(np.abs(G.log_ratio(prm, s, masks, dtype=np.float32, pair_idx=idx) - ref).max())
        bound, capped = R.f32_bound(dev32, N)
        how = "capped at 2 (2e-6 N + 2e-6)" if capped else "16 x dev32"
        if dev32 > R.f32_ceiling(N):
            how = "16 x dev32 UNCAPPED: the float32 oracle itself is beyond the ceiling %.2e" % R.f32_ceiling(N)
    print("%s %d pairs, %d checked x %d regions; max |log r| = %.2f, %.0f %% of %d entries above 0.01; dev32 = %.2e; bound %.3e (%s)"
          % (label, npairs, len(idx), len(masks), mx, 100 * share, ref.size, dev32, bound, how))
    pi, ri = np.meshgrid(idx, np.arange(len(masks)), indexing="xy")
    res = R.compare(label, lr[:, idx].ravel(), ref.ravel(), pi.ravel(), ri.ravel(), bound,
                    echo=lambda line: print(line.replace(" at cut ", " at region ")))
    print("%s worst region: %s" % (label, names[res["cut"]]))

    resum = R.sums_from_log_ratio(lr)                                       # the device's own log r, re-summed exactly
    rel = float(np.abs(sums / resum - 1.0).max())
    seconds = time.time() - t0
    print("RENYI_REGIONS_FULL %-32s err %.3e region %2d pair %5d block %4d | bound %.3e ratio %6.3f | dev32 %.2e | sums rel %.1e | ref %.1f s"
          % (label, res["err"], res["cut"], res["pair"], res["block"], bound, res["ratio"], dev32, rel, seconds))
    assert mx > 0.1 and share >= 0.25, "bland inputs: max |log r| %.3f, share above 0.01 %.2f" % (mx, share)
    assert rel <= 1e-12
    assert res["finite"] and res["err"] <= bound, "%s: |d log r| %.3e > bound %.3e at region %d (%s), pair %d (block %d)" % (
        label, res["err"], bound, res["cut"], names[res["cut"]], res["pair"], res["block"])
    return res


# f64, (Nx, Ny), units, pairs, what the case is for
CASES = [
    (False, (80, 1), 50, 5003, "the size docs/renyi_regions.md measures; ragged last block of 6 chains"),
    (False, (33, 1), 20, 500, "one site in the second word of spins and masks"),
    (False, (33, 1), 36, 500, "one site in the second word of spins and masks"),
    (False, (64, 1), 20, 500, "two full words"),
    (False, (64, 1), 36, 500, "two full words"),
    (False, (65, 1), 20, 500, "one site in the third word"),
    (False, (65, 1), 36, 500, "one site in the third word"),
    (False, (40, 1), 128, 203, "image read from global memory"),
    (False, (40, 1), 256, 203, "image read from global memory"),
    (False, (100, 1), 100, 301, "four words, the widest LDS-resident f32 image"),
    (True, (6, 6), 50, 1003, "raster model at a lattice size"),                       # weight seed 36, see WEIGHT_SEED
    (True, (4, 8), 53, 301, "the 4-wave instantiations"),
    (True, (4, 8), 68, 301, "the 4-wave instantiations"),
    (True, (8, 8), 100, 301, "the widest f64 model, two words, 7 column cuts"),
]

# Weight seed 111 (biases 112), with the exception tests/test_gpu_renyi_full.py makes and explains: 6 x 6, 50 units, float64 uses 36.
WEIGHT_SEED = {(True, (6, 6), 50): 36}


def _id(c):
    return "%s-%dx%d-%d-%d" % ("f64" if c[0] else "f32", c[1][0], c[1][1], c[2], c[3])


def region_set(shape):
    names, masks = zip(*G.region_set(*shape))
    return list(names), np.stack(masks)


@pytest.mark.parametrize("f64,shape,H,npairs,why", CASES, ids=[_id(c) for c in CASES])
def test_log_ratio_and_sums_against_the_float64_reference(f64, shape, H, npairs, why):
    prm = sharpened(H, f64, seed=WEIGHT_SEED.get((f64, shape, H), 111))
    wf = make_wf(f64, shape[0], shape[1], H, prm)
    names, masks = region_set(shape)
    out = wf.renyi2_regions(masks, npairs, seed=111, step=0, log_ratio=True)
    check("[%s]" % _id((f64, shape, H, npairs)), f64, prm, shape, npairs, names, masks, out)


def test_several_passes_equal_one_pass_and_the_reference(monkeypatch):
    """N = 80, 50 units, 5 003 pairs under a 30 MB state budget: at least three passes of whole 16-chain blocks, the last one partial
    and ragged.  Bit-equal per pair to the one-pass call, and checked against the reference."""
    f64, shape, H, npairs = False, (80, 1), 50, 5003
    prm = sharpened(H, f64)
    names, masks = region_set(shape)

    def run(wf):
        wf.timing_enable(True)
        wf.timing_reset()
        out = wf.renyi2_regions(masks, npairs, seed=111, step=0, log_ratio=True)
        return out, wf.timing_get(2)["launches"]                           # one assembly bracket per pass

    one, passes_one = run(make_wf(f64, 80, 1, H, prm))
    monkeypatch.setenv("RNNWF_STATE_BUDGET_MB", "30")
    many, passes = run(make_wf(f64, 80, 1, H, prm))
    print("[f32-80x1-50-5003 passes] %d pass(es) by default, %d under RNNWF_STATE_BUDGET_MB=30" % (passes_one, passes))
    assert passes_one == 1 and passes >= 3 and npairs % 8 != 0
    assert np.array_equal(many["samples"], one["samples"]) and np.array_equal(many["log_ratio"], one["log_ratio"])
    assert np.allclose(many["sums"], one["sums"], rtol=1e-13, atol=0)
    check("[f32-80x1-50-5003 passes]", f64, prm, shape, npairs, names, masks, many)
