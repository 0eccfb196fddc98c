"""The float64 reference of tests/test_gpu_renyi_stack.py (tests/renyi_stack_reference.py), validated on its own - no GPU:

1. summed over every pair of configurations with the weights P(sigma) P(tau), the brute force gives Tr rho_A^2 from the dense vector
   of all 2^N amplitudes to relative 1e-12: N = 6 with two float64 layers of 10 units and 3x2 with three (a bulk interval, a two-piece
   region, a single site and a column cut among the regions); r_A = r_complement; the empty and the full mask give exactly 0; the
   site-resolved form of the stack kernels is the same number;
2. the bounds have teeth at N = 34, (10, 10) units, sharpened weights, model-drawn chains: the site-resolved form with one defect
   applied in NumPy is REJECTED at the float64 bound 1e-11 N and, by a factor of 10 at least, at the float32 bound
   test_gpu_renyi_stack.py enforces (16 x the float32 oracle's deviation from float64, capped at 2 (2e-6 N + 2e-6)).

Measured factors max |d log r| / float32 bound (64 pairs x 8 regions): printed by the test.
"""
import numpy as np
import pytest

import renyi_stack_reference as S
from conftest import all_configs
from oracle import models as M


@pytest.mark.parametrize("shape,units", [((6, 1), (10, 10)), ((3, 2), (10, 10, 10))], ids=["6-10x10", "3x2-10x10x10"])
def test_brute_force_over_all_pairs_gives_the_exact_purity(shape, units):
    Nx, Ny = shape
    N = Nx * Ny
    prm = S.weights(True, units)
    names, masks = zip(*S.small_regions(Nx, Ny))
    masks = np.stack(masks)
    assert {"interval 2..4", "two pieces", "site N-1"} <= set(names) and ("column 0" in names) == (Ny > 1)
    c = all_configs(N).astype(np.int32)
    lp = M.prnn_log_probability(prm, c, dtype=np.float64)
    assert abs(np.exp(lp).sum() - 1.0) < 1e-13
    i, j, pairs = S.all_pairs(c)
    lr = S.log_ratio(prm, pairs, masks)
    purity = (np.exp(lp[i] + lp[j])[None, :] * np.exp(lr)).sum(axis=1)
    exact = np.array([S.purity_of_region(np.exp(0.5 * lp), N, m) for m in masks])
    rel = np.abs(purity / exact - 1.0)
    print("%dx%d %s: Tr rho_A^2 = %s, max rel %.2e" % (Nx, Ny, units, np.round(exact, 4), rel.max()))
    assert -np.log(exact.min()) > 0.05                            # entangled: the identity is not trivially 1 = 1
    assert rel.max() <= 1e-12
    # r_A = r_complement; nothing or everything swapped: exactly 0; the site-resolved form of the kernels is the same number
    sub = pairs[:2 * 200]
    assert np.abs(S.log_ratio(prm, sub, masks) - S.log_ratio(prm, sub, 1 - masks)).max() <= 1e-12
    ends = S.log_ratio(prm, sub, np.stack([np.zeros(N, dtype=np.int32), np.ones(N, dtype=np.int32)]))
    assert np.all(ends == 0.0)
    assert np.array_equal(S.stack_form(prm, sub, np.stack([np.zeros(N, dtype=np.int32), np.ones(N, dtype=np.int32)])), ends)
    assert np.abs(S.stack_form(prm, sub, masks) - S.log_ratio(prm, sub, masks)).max() <= 1e-12


@pytest.fixture(scope="module")
def boundary_case():
    """N = 34, (10, 10) float32 units, 64 pairs drawn by the oracle from the wave function itself, the word-boundary region set.  At
    these sharpened weights the last sites are nearly decided: the stream of uniforms is one under which a pair differs beyond
    site 31 (asserted), or no mask word beyond the first could matter."""
    N, units, npairs = 34, (10, 10), 64
    prm = S.weights(False, units)
    u = np.random.RandomState(2).random_sample((2 * npairs, N))
    s = M.prnn_sample(prm, N, u)[0].astype(np.int32)
    assert np.any(s[0::2, 32:] != s[1::2, 32:])
    masks = np.stack([m for _, m in S.boundary_regions(N)])
    assert S.word_boundaries_covered(N, masks)
    ref = S.log_ratio(prm, s, masks)
    mx, share = S.nontrivial(ref)
    dev32 = float(np.abs(S.log_ratio(prm, s, masks, dtype=np.float32) - ref).max())
    b32, capped = S.f32_bound(dev32, N)
    print("N = 34, %d pairs x %d regions: max |log r| = %.2f, %.0f %% above 0.01; dev32 = %.2e, float32 bound %.2e (%s), float64 bound %.1e"
          % (npairs, len(masks), mx, 100 * share, dev32, b32, "capped" if capped else "16 x dev32", S.f64_bound(N)))
    assert mx > 0.1 and share >= 0.25
    return dict(N=N, prm=prm, s=s, masks=masks, ref=ref, b32=b32, b64=S.f64_bound(N))


def test_the_site_resolved_form_is_within_the_float64_bound(boundary_case):
    c = boundary_case
    assert np.abs(S.stack_form(c["prm"], c["s"], c["masks"]) - c["ref"]).max() <= 0.01 * c["b64"]


@pytest.mark.parametrize("defect", sorted(S.DEFECTS))
def test_bounds_reject_a_defect_of_the_stack_form(boundary_case, defect):
    c = boundary_case
    err = float(np.abs(S.stack_form(c["prm"], c["s"], c["masks"], defect=defect) - c["ref"]).max())
    print("%s: max |d log r| = %.3e = %.3g x the float64 bound, %.3g x the float32 bound" % (S.DEFECTS[defect], err, err / c["b64"], err / c["b32"]))
    assert err > c["b64"]
    assert err >= 10.0 * c["b32"]
