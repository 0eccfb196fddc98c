"""The paired tail pass of rnnwf_renyi2_regions_complex (csrc/crnn_renyi.hip, csrc/crnn_renyi_kernels.h) against an independent
float64 reference at the size the complex RNN is measured at (bench.py's cfg3: N = 40, 50 units) and on a chain of three mask words
(N = 70, 20 units), after the pattern of tests/test_gpu_renyi_regions_full.py.

Each case draws its pairs on the device from sharpened weights (kernels x 2, every bias randomised), takes the complex log r of every
pair and region of tests/renyi_regions_reference.region_set (the full-size list of docs/renyi_regions.md for a chain) and checks

  * both components per pair and region against tests/crnn_renyi_reference.py (brute force in float64 NumPy on the oracle's complex
    RNN, scoring the very chains the device drew; validated by tests/test_crnn_renyi_reference.py) on the pair subset of
    tests/renyi_regions_reference.py (choose_pairs, asserted by check_subset: every pair of the first, a middle and the last full
    block, every pair of the ragged last block, >= 32 pairs);
  * the dead entries exactly, all pairs: (-inf, 0) where and only where the two chains carry different numbers of ups in the region,
    and out_in_sector equal to that count;
  * sums against an exactly rounded float64 re-summation (math.fsum) of the device's own r, all pairs: relative 1e-12.

Bound - never derived from the kernels: 16 x dev32, dev32 = the largest deviation of the FLOAT32 NumPy oracle from the float64
reference on the same pairs and regions, computed here at run time; capped at 2e-6 N + 2e-6 (tests/correlations_reference.py).
Each case prints one CRNN_RENYI_FULL line; docs/renyi_complex.md records the figures.
"""
import math
import time

import numpy as np
import pytest

import crnn_pauli_reference as CR
import crnn_renyi_reference as RR
import pauli_reference as PR
import renyi_regions_reference as RG

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("N,H,npairs", [(40, 50, 5003), (70, 20, 5003)])
def test_log_ratio_and_sums_against_the_float64_reference(N, H, npairs):
    from rnnwavefunctions_amd import _lib
    t0 = time.time()
    prm = CR.weights(H, seed=111, scale=2.0)
    wf = _lib.NativeWavefunction(_lib.MODEL_CRNN_U1, N, 1, (H,))
    wf.set_params(prm, scope=CR.SCOPE)
    names, regions = zip(*RG.region_set(N, 1))
    regions = np.stack(regions)
    out = wf.renyi2_regions_complex(regions, npairs, seed=111, step=0, log_ratio=True)
    lr, sums, s = out["log_ratio"], out["sums"], out["samples"]
    assert lr.shape == (len(regions), npairs) and sums.shape == (len(regions), 4) and s.shape == (2 * npairs, N)
    assert np.all(np.isfinite(sums)) and np.all(CR.in_sector(s)) and not np.any(np.isnan(lr.real)) and not np.any(np.isnan(lr.imag))

    idx = RG.choose_pairs(npairs)
    RG.check_subset(npairs, N, idx, regions)
    assert len(idx) >= 32
    rows = np.stack([2 * idx, 2 * idx + 1], axis=1).reshape(-1)
    ref = RR.explicit_log_ratio(prm, s[rows], regions)
    dev32 = RR.max_abs_diff(RR.explicit_log_ratio_f32(prm, s[rows], regions), ref)
    bound, capped = PR.f32_bound(dev32, N)
    fin = ~np.isneginf(ref.real)
    assert fin.sum() >= ref.size // 8 and (~fin).sum() >= ref.size // 8 and np.abs(ref[fin]).max() > 0.1
    err = RR.max_abs_diff(lr[:, idx], ref)                         # asserts that the (-inf, 0) entries coincide exactly
    for k, m in enumerate(regions):                                # every pair: dead where and only where the charges differ
        alive = RR.popcount_rule(s, m)
        assert np.array_equal(~np.isneginf(lr[k].real), alive), names[k]
        assert out["in_sector"][k] == alive.sum(), names[k]
    r = RR.ratio(lr)
    resum = np.array([[math.fsum(v.real), math.fsum(v.imag), math.fsum(v.real ** 2), math.fsum(v.imag ** 2)] for v in r])
    nz = np.abs(resum) > 0
    rel = float(np.abs(sums[nz] / resum[nz] - 1.0).max())
    print("CRNN_RENYI_FULL [f32-%dx1-%d-%d] err %.3e | bound %.3e (%s) ratio %6.3f | dev32 %.2e | %d pairs checked x %d regions, %d finite | "
          "survivor fraction %.3f..%.3f | sums rel %.1e | ref %.1f s"
          % (N, H, npairs, err, bound, "capped at 2e-6 N + 2e-6" if capped else "16 x dev32", err / bound, dev32, len(idx), len(regions),
             int(fin.sum()), out["in_sector"].min() / npairs, out["in_sector"].max() / npairs, rel, time.time() - t0))
    assert rel <= 1e-12 and np.all(sums[~nz] == 0.0)
    assert err <= bound
