"""CPU validation of tests/renyi_2d_reference.py (the float64 brute force of the 2D RNN's region swap estimator and the restatement
of the paired masked-tail form), the defect study behind the GPU bound 1e-11 N, and the inputs of the exact and statistical GPU tests."""
import functools
import itertools

import numpy as np
import pytest

import pauli_2d_reference as Q
import renyi_2d_reference as R
from conftest import all_configs
from oracle import models as M


def scorer(prm):
    return lambda x: M.mdrnn_log_probability(prm, x)


def all_pairs(N, Nx, Ny):
    """every (sigma, tau) of the lattice as (2 * 4^N, Nx, Ny) pairs, and the configuration indices (i, j) of each pair"""
    c = all_configs(N).reshape(-1, Nx, Ny)
    i, j = np.meshgrid(np.arange(2 ** N), np.arange(2 ** N), indexing="ij")
    pairs = np.empty((2 * i.size, Nx, Ny), dtype=np.int64)
    pairs[0::2], pairs[1::2] = c[i.ravel()], c[j.ravel()]
    return pairs, i.ravel(), j.ravel()


def purity_regions(Nx, Ny):
    N = Nx * Ny
    if N <= 6:                                       # every non-trivial region
        return np.array([m for m in itertools.product([0, 1], repeat=N) if 0 < sum(m) < N], dtype=np.int32)
    return np.stack(R.row_cuts(Nx, Ny) + R.column_cuts(Nx, Ny) + [R.rectangle(Nx, Ny, 0, 2, 0, 2), R.mask_of(Nx, Ny, [(1, 1)]),
                    R.mask_of(Nx, Ny, [(0, 1), (2, 2)]), R.mask_of(Nx, Ny, [(0, 0), (2, 1)]), R.mask_of(Nx, Ny, [(1, 0), (1, 1), (1, 2)])])


# 1. sum over every (sigma, tau) of P(sigma) P(tau) r_A = Tr rho_A^2 from the dense vector
@pytest.mark.parametrize("Nx,Ny", [(2, 3), (3, 2), (3, 3)])
def test_brute_force_sums_to_the_purity(Nx, Ny):
    N = Nx * Ny
    prm = R.exact_weights()
    lp = M.mdrnn_log_probability(prm, all_configs(N).reshape(-1, Nx, Ny))
    psi = np.exp(0.5 * lp)
    masks = purity_regions(Nx, Ny)
    pairs, i, j = all_pairs(N, Nx, Ny)
    lr = R.log_ratio_regions(scorer(prm), pairs, masks)
    got = (np.exp(lp[i] + lp[j])[None, :] * np.exp(lr)).sum(axis=1)
    exact = np.array([R.purity_of_region(psi, N, m) for m in masks])
    rel = np.abs(got / exact - 1.0).max()
    print("%dx%d: %d regions, max rel |sum P P r_A - Tr rho_A^2| = %.2e" % (Nx, Ny, len(masks), rel))
    assert abs(np.exp(lp).sum() - 1.0) < 1e-12 and rel <= 1e-12


def setup(Nx, Ny, H=10, npairs=8):
    prm = Q.weights(H, Nx * Ny, 1.0)
    pairs = np.random.RandomState(Nx + 10 * Ny).randint(0, 2, size=(2 * npairs, Nx, Ny)).astype(np.int64)
    masks = R.case_regions(Nx, Ny)
    return prm, pairs, masks, R.log_ratio_regions(scorer(prm), pairs, masks)


# 2. exact identities of the brute force
@pytest.mark.parametrize("Nx,Ny", [(3, 4), (5, 7)])
def test_identities_of_the_brute_force(Nx, Ny):
    N = Nx * Ny
    prm, pairs, masks, ref = setup(Nx, Ny)
    lp = scorer(prm)
    comp = R.log_ratio_regions(lp, pairs, 1 - masks)
    assert np.abs(comp - ref).max() <= 1e-13 * N                                    # r_A = r_complement
    empty, full = [k for k, m in enumerate(masks) if not m.any()], [k for k, m in enumerate(masks) if m.all()]
    assert len(empty) == 1 and len(full) == 1
    assert np.abs(ref[empty + full]).max() <= 1e-13 * N                             # r = 1
    selfp = np.repeat(pairs[0::2], 2, axis=0)
    assert np.abs(R.log_ratio_regions(lp, selfp, masks)).max() <= 1e-13 * N         # self pairs
    # pairs that differ only on A: the swapped configurations are (tau, sigma), so log r = 0, while both mixed chains differ from
    # their own (the tails are not the suffixes)
    worst, moved = 0.0, 0
    for m in masks:
        if not m.any() or m.all():
            continue
        d = pairs.copy()
        in_a = m.reshape(1, Nx, Ny).astype(bool)
        d[1::2] = np.where(in_a, 1 - d[0::2], d[0::2])
        worst = max(worst, np.abs(R.log_ratio_regions(lp, d, m[None, :])).max())
        moved += int(np.abs(lp(d[0::2]) - lp(d[1::2])).max() > 1e-3)
    assert worst <= 1e-13 * N and moved > 0


# 3. the accepted form
@pytest.mark.parametrize("Nx,Ny", [(3, 3), (3, 4), (4, 3), (5, 7), (1, 5), (5, 1)])
def test_kernel_form_is_the_brute_force(Nx, Ny):
    prm, pairs, masks, ref = setup(Nx, Ny)
    err = np.abs(R.kernel_form(prm, pairs, masks) - ref).max()
    print("%dx%d: %d regions, max |kernel form - brute force| = %.2e, max |log r| = %.2f" % (Nx, Ny, len(masks), err, np.abs(ref).max()))
    assert np.all(np.isfinite(ref)) and err <= R.BOUND * Nx * Ny and np.abs(ref).max() > 1e-2


# 4. every defect must move max |d log r| orders of magnitude over the bound (mask words need more than 32 sites)
@pytest.mark.parametrize("defect,Nx,Ny", [(d, Nx, Ny) for d in R.DEFECTS for Nx, Ny in [(3, 4), (5, 7)] if d != "mask_word_0" or Nx * Ny > 32])
def test_defects_are_rejected_by_orders_of_magnitude(defect, Nx, Ny):
    prm, pairs, masks, ref = setup(Nx, Ny)
    err = np.abs(R.kernel_form(prm, pairs, masks, defect=defect) - ref).max()
    bound = R.BOUND * Nx * Ny
    print("%-18s %dx%d: max |d log r| = %.3g = %.2g x bound" % (defect, Nx, Ny, err, err / bound))
    assert err >= 1e6 * bound


def test_case_regions_cover_what_the_log_ratio_test_promises():
    for Nx, Ny in [(3, 4), (4, 3), (1, 5), (5, 1), (5, 7), (7, 5)]:
        N = Nx * Ny
        masks = R.case_regions(Nx, Ny)
        mv = Q.to_visit_order(masks, Nx, Ny)
        firsts = {R.normalise(m)[1] for m in mv}
        turns = {p for ny in range(1, Ny) for p in (ny * Nx - 1, ny * Nx)}
        assert firsts >= turns | {N - 1} and 0 in firsts                            # row turns, f = N-1, empty after normalisation
        assert any(m[0] and not m.all() for m in mv)                                # complemented by the driver
        singles = {int(np.flatnonzero(m)[0]) for m in mv if m.sum() == 1}
        assert singles >= turns
        if N > 32:
            assert any(m[31] and m[32] and m.sum() < N for m in mv) and {31, 32} <= singles


# 5. the inputs of the exact and statistical GPU tests
def test_exact_inputs_are_what_the_gpu_tests_assume():
    prm = R.exact_weights()
    for (Nx, Ny), want in R.EXACT_S2.items():
        N = Nx * Ny
        lp = M.mdrnn_log_probability(prm, all_configs(N).reshape(-1, Nx, Ny))
        psi = np.exp(0.5 * lp)
        S2 = np.array([-np.log(R.purity_of_region(psi, N, m)) for _, m in R.exact_regions(Nx, Ny)])
        print("%dx%d exact S2 %s" % (Nx, Ny, np.round(S2, 4)))
        assert np.abs(S2 - np.array(want)).max() <= 5.1e-4
        if (Nx, Ny) not in R.EXACT_I2:
            continue
        i2 = []
        for a, b in R.i2_pairs(Nx, Ny):
            assert not np.any(a & b)
            sa, sb, sab = (-np.log(R.purity_of_region(psi, N, m)) for m in (a, b, a | b))
            i2.append(sa + sb - sab)
        print("%dx%d exact I2 %s" % (Nx, Ny, np.round(i2, 4)))
        assert np.abs(np.array(i2) - np.array(R.EXACT_I2[(Nx, Ny)])).max() <= 5.1e-4 and min(i2) >= R.FLOOR
    # the two-block pair on 3x4 is below the floor: it is not among the pairs
    Nx, Ny, N = 3, 4, 12
    psi = np.exp(0.5 * M.mdrnn_log_probability(prm, all_configs(N).reshape(-1, Nx, Ny)))
    a, b = R.mask_of(Nx, Ny, [(0, 0), (0, 1)]), R.mask_of(Nx, Ny, [(2, 3), (2, 2)])
    sa, sb, sab = (-np.log(R.purity_of_region(psi, N, m)) for m in (a, b, a | b))
    assert abs(sa + sb - sab - 0.025) <= 5.1e-4 and len(R.i2_pairs(Nx, Ny)) == 1


# 6. the lattice-indexed builders of observables_2d against the reference's
def test_builders_and_python_refusals():
    from rnnwavefunctions_amd import _lib
    from rnnwavefunctions_amd import observables_2d as O2

    class FakeNative(_lib.NativeWavefunction):
        """A NativeWavefunction without a library handle: enough for the checks Python makes before the C call."""

        def __init__(self, model, nx, ny):
            self.h, self.lib, self.model, self.nx, self.ny, self.N = None, None, model, nx, ny, nx * ny

    for Nx, Ny in [(3, 4), (4, 3), (5, 7)]:
        assert np.array_equal(O2.row_cut_regions(Nx, Ny), np.stack(R.row_cuts(Nx, Ny)))
        assert np.array_equal(O2.column_cut_regions(Nx, Ny), np.stack(R.column_cuts(Nx, Ny)))
        assert np.array_equal(O2.rectangle_region(Nx, Ny, 1, 3, 0, 2), R.rectangle(Nx, Ny, 1, 3, 0, 2))
        assert O2.rectangle_region(Nx, Ny, 1, 2, 2, 3)[O2.site(Nx, Ny, 1, 2)] == 1 and O2.rectangle_region(Nx, Ny, 1, 2, 2, 3).sum() == 1
        # the row cuts are the prefixes of the path
        for c, m in enumerate(Q.to_visit_order(O2.row_cut_regions(Nx, Ny), Nx, Ny), start=1):
            assert np.array_equal(m, (np.arange(Nx * Ny) < c * Nx).astype(np.int32))
    for bad in [lambda: O2.rectangle_region(3, 4, 0, 4, 0, 1), lambda: O2.rectangle_region(3, 4, 2, 1, 0, 1), lambda: O2.rectangle_region(3, 4, 0, 1, -1, 1),
                lambda: O2.rectangle_region(0, 4, 0, 0, 0, 1), lambda: O2.row_cut_regions(3, 1), lambda: O2.column_cut_regions(1, 3)]:
        with pytest.raises(ValueError):
            bad()
    wf = FakeNative(_lib.MODEL_MDRNN2D, 3, 2)
    for shape in [(1, 7), (1, 2, 3), (0, 6), (2, 3)]:
        with pytest.raises(ValueError, match="shape"):
            wf.renyi2_regions_2d(np.zeros(shape, dtype=np.int32), 4)
    with pytest.raises(ValueError, match="0 and 1"):
        wf.renyi2_regions_2d(np.zeros((1, 6)) + 0.5, 4)
    with pytest.raises(ValueError, match="samples"):
        wf.renyi2_regions_2d(np.zeros((1, 6), dtype=np.int32), 4, samples=np.zeros((7, 3, 2), dtype=np.int32))
    with pytest.raises(ValueError, match="disjoint"):
        O2.renyi2_mutual_information(wf, R.mask_of(3, 2, [(1, 1)]), R.mask_of(3, 2, [(1, 1), (0, 0)]), 4)
    with pytest.raises(ValueError, match="MDRNN2D"):
        O2.renyi2_regions(FakeNative(_lib.MODEL_GRU1D_F64, 3, 2), np.zeros((1, 6), dtype=np.int32), 4)


def test_header_binding_and_build_list_name_the_entry_point():
    import os
    import re
    from rnnwavefunctions_amd import _lib, build
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "rnnwf.h")).read()
    assert re.search(r"int rnnwf_renyi2_regions_2d\(rnnwf_handle\* h, const int32_t\* regions", header)
    assert _lib.PROTOTYPES["rnnwf_renyi2_regions_2d"] == _lib.PROTOTYPES["rnnwf_renyi2_regions"]
    assert "mdrnn_renyi.hip" in build.SOURCES and build.compile_flags("mdrnn_renyi.hip") == build.compile_flags("mdrnn.hip")


# ---- lattices of three to eight spin words: what tests/test_gpu_renyi_2d_full.py rests on -------------------------------------------------
FULL_LATTICES = [(13, 5), (5, 13), (9, 11), (12, 12), (16, 16)]             # the lattices of the full-size GPU cases
FULL_SCALE = 0.75                                                           # tests/test_pauli_2d_reference.py: full_setup


def test_full_size_region_sets_cover_what_the_cases_promise():
    for Nx, Ny in FULL_LATTICES:
        names, masks = zip(*R.region_set_2d(Nx, Ny))
        R.check_case_2d(Nx, Ny, masks)
        assert len(set(names)) == len(names)
        thin = np.stack([m for _, m in R.region_set_2d(Nx, Ny, thin=True)])
        assert {m.tobytes() for m in thin} <= {m.tobytes() for m in masks}
        active = sum(R.normalise(m)[1] > 0 for m in Q.to_visit_order(np.stack(masks), Nx, Ny))
        print("%dx%d: %d regions (%d thin), %d non-empty after normalisation" % (Nx, Ny, len(masks), len(thin), active))
        if (Nx, Ny) == (12, 12):                                     # the tiles of the paired pass on 2006 chains
            assert active >= Q.MIN_MASKS and active * ((2006 + 15) // 16) >= 16384
    with pytest.raises(AssertionError):                              # the set of the existing cases has no single site per word edge
        R.check_case_2d(5, 7, R.case_regions(5, 7))


@functools.lru_cache(maxsize=None)
def full_setup(Nx, Ny, npairs=4):
    """10 units (kernels x 0.75), pairs drawn by the oracle, the thinned region set; the brute force computed once per lattice"""
    prm = Q.weights(10, 111, FULL_SCALE)
    pairs, _ = M.mdrnn_sample(prm, Nx, Ny, np.random.RandomState(Nx + 10 * Ny).random_sample((2 * npairs, Nx * Ny)))
    masks = np.stack([m for _, m in R.region_set_2d(Nx, Ny, thin=True)])
    ref = R.log_ratio_regions(scorer(prm), pairs, masks)
    ref.setflags(write=False)
    return prm, pairs, masks, ref


@pytest.mark.parametrize("Nx,Ny", FULL_LATTICES)
def test_kernel_form_is_the_brute_force_on_three_to_eight_words(Nx, Ny):
    prm, pairs, masks, ref = full_setup(Nx, Ny)
    err = np.abs(R.kernel_form(prm, pairs, masks) - ref).max()
    print("%dx%d: %d regions, max |kernel form - brute force| = %.2e, max |log r| = %.2f" % (Nx, Ny, len(masks), err, np.abs(ref).max()))
    assert np.all(np.isfinite(ref)) and err <= R.BOUND * Nx * Ny and np.abs(ref).max() > 0.1


# the defects of the word index that only a third word shows: none moves a bit on 5x7 (two words), each is rejected by the bound of the
# full-size cases by at least three orders of magnitude on three, five and eight words
@pytest.mark.parametrize("defect", R.WORD_DEFECTS)
def test_word_defects_are_invisible_on_two_words_and_rejected_from_three(defect):
    prm, pairs, masks, ref = full_setup(5, 7)
    assert np.array_equal(R.kernel_form(prm, pairs, masks, defect=defect), R.kernel_form(prm, pairs, masks))
    assert np.array_equal(R.kernel_form(prm, pairs, R.case_regions(5, 7), defect=defect), R.kernel_form(prm, pairs, R.case_regions(5, 7)))
    for Nx, Ny in [(13, 5), (12, 12), (16, 16)]:
        prm, pairs, masks, ref = full_setup(Nx, Ny)
        err = np.abs(R.kernel_form(prm, pairs, masks, defect=defect) - ref).max()
        bound = R.BOUND * Nx * Ny
        print("%-24s %dx%d: max |d log r| = %.3g = %.2g x bound" % (defect, Nx, Ny, err, err / bound))
        assert err >= 1e3 * bound
