"""The masked-tail pass of rnnwf_pauli_step_complex (csrc/crnn_pauli.hip, csrc/crnn_pauli_kernels.h) against an independent float64
reference at the size the complex RNN is measured at (bench.py's cfg3: N = 40, 50 units), after the pattern of
tests/test_gpu_pauli_full.py.

The case draws its chains on the device from sharpened weights (kernels x 2, every bias randomised), takes the complex log-ratio of
every chain and mask and checks

  * both components per chain and mask against tests/crnn_pauli_reference.py (brute force in float64 NumPy on the oracle's complex
    RNN, scoring the very chains the device drew; validated by tests/test_crnn_pauli_reference.py) for EVERY mask of the set, on the
    chain subset of tests/pauli_reference.py (choose_chains, asserted by check_subset: all 16 chains of the first, a middle and the
    last full block, every chain of the ragged last block, >= 32 chains);
  * the out-of-sector entries exactly: (-inf, 0) where and only where the flipped configuration leaves the sector;
  * sums against an exactly rounded float64 re-summation (math.fsum) of the device's own v, all chains: relative 1e-12.

Bound - never derived from the kernels: 16 x dev32, dev32 = the largest deviation of the FLOAT32 NumPy oracle from the float64
reference on the same chains and masks, computed here at run time; capped at 2e-6 N + 2e-6 (tests/correlations_reference.py).
The case prints one CRNN_PAULI_FULL line; docs/pauli_complex.md says which figures have been recorded.
"""
import math
import time

import numpy as np
import pytest

import crnn_pauli_reference as CR
import pauli_reference as PR

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("N,H,ns", [(40, 50, 1006)])
def test_log_ratio_and_sums_against_the_float64_reference(N, H, ns):
    from rnnwavefunctions_amd import _lib
    t0 = time.time()
    prm = CR.weights(H, seed=111, scale=2.0)
    wf = _lib.NativeWavefunction(_lib.MODEL_CRNN_U1, N, 1, (H,))
    wf.set_params(prm, scope=CR.SCOPE)
    masks = CR.case_masks(N)
    zero = np.zeros_like(masks)
    out = wf.pauli_step_complex(masks, zero, np.ones(len(masks)), ns, seed=111, step=0, want_log_ratio=True, want_samples=True)
    lr, sums, s = out["log_ratio"], out["term_sums"], out["samples"]
    assert lr.shape == (len(masks), ns) and sums.shape == (len(masks), 4) and s.shape == (ns, N)
    assert np.all(np.isfinite(sums)) and np.all(CR.in_sector(s)) and not np.any(np.isnan(lr.real)) and not np.any(np.isnan(lr.imag))

    idx = PR.choose_chains(ns)
    PR.check_subset(ns, N, idx, masks)
    ref = CR.explicit_log_ratio(prm, s[idx], masks)
    dev32 = CR.max_abs_diff(CR.explicit_log_ratio_f32(prm, s[idx], masks), ref)
    bound, capped = PR.f32_bound(dev32, N)
    fin = ~np.isneginf(ref.real)
    assert fin.sum() >= ref.size // 8 and (~fin).sum() >= ref.size // 8 and np.abs(ref[fin]).max() > 0.1
    err = CR.max_abs_diff(lr[:, idx], ref)                         # asserts that the (-inf, 0) entries coincide exactly
    # every chain: out of the sector where and only where the flipped configuration is
    for k, m in enumerate(masks):
        assert np.array_equal(np.isneginf(lr[k].real), ~CR.in_sector(s ^ m[None, :])), k
    v = CR.local_values(lr, s, masks, zero)
    resum = np.array([[math.fsum(r.real), math.fsum(r.imag), math.fsum(r.real ** 2), math.fsum(r.imag ** 2)] for r in v])
    nz = np.abs(resum) > 0
    rel = float(np.abs(sums[nz] / resum[nz] - 1.0).max())
    print("CRNN_PAULI_FULL [f32-%dx1-%d-%d] err %.3e | bound %.3e (%s) ratio %6.3f | dev32 %.2e | %d checked x %d masks, %d finite | "
          "sums rel %.1e | ref %.1f s" % (N, H, ns, err, bound, "capped at 2e-6 N + 2e-6" if capped else "16 x dev32", err / bound, dev32,
                                          len(idx), len(masks), int(fin.sum()), rel, time.time() - t0))
    assert rel <= 1e-12 and np.all(sums[~nz] == 0.0)
    assert err <= bound
