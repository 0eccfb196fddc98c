"""CPU validation of tests/pauli_2d_reference.py (the float64 restatement of the 2D RNN's masked-tail form) and the defect study
behind the GPU bound 1e-11 N: which errors of the pass the bound rejects."""
import numpy as np
import pytest

import pauli_2d_reference as Q
import pauli_reference as PR
from conftest import all_configs
from oracle import models as M
from rnnwavefunctions_amd import observables as O


def setup(Nx, Ny, H=10, ns=12):
    prm = Q.weights(H, Nx * Ny, 1.0)         # the elu cell is unbounded: sharper kernels drive conditionals to exactly 0 on 35 sites
    s = np.random.RandomState(Nx + 10 * Ny).randint(0, 2, size=(ns, Nx, Ny)).astype(np.int64)
    masks = Q.case_masks(Nx, Ny)
    ref = Q.explicit_log_ratio(lambda x: M.mdrnn_log_probability(prm, x), s, masks)
    return prm, s, masks, ref


@pytest.mark.parametrize("Nx,Ny", [(3, 3), (3, 4), (4, 3), (5, 7), (1, 5), (5, 1)])
def test_kernel_form_is_the_explicit_log_ratio(Nx, Ny):
    prm, s, masks, ref = setup(Nx, Ny)
    err = np.abs(Q.kernel_form(prm, s, masks) - ref).max()
    print("%dx%d: %d masks, max |kernel form - explicit| = %.2e, max |log r| = %.2f" % (Nx, Ny, len(masks), err, np.abs(ref).max()))
    assert np.all(np.isfinite(ref)) and err <= Q.BOUND * Nx * Ny and np.abs(ref).max() > 1e-2


# defect, lattice: every defect must move max |d log r| orders of magnitude over the bound (mask words need more than 32 sites)
@pytest.mark.parametrize("defect,Nx,Ny", [(d, Nx, Ny) for d in Q.DEFECTS for Nx, Ny in [(3, 4), (4, 3), (5, 7)]
                                          if d != "mask_word_0" or Nx * Ny > 32])
def test_defects_are_rejected_by_orders_of_magnitude(defect, Nx, Ny):
    prm, s, masks, ref = setup(Nx, Ny)
    err = np.abs(Q.kernel_form(prm, s, masks, defect=defect) - ref).max()
    bound = Q.BOUND * Nx * Ny
    print("%-18s %dx%d: max |d log r| = %.3g = %.2g x bound" % (defect, Nx, Ny, err, err / bound))
    assert err >= 1e6 * bound


def test_case_masks_cover_what_the_log_ratio_test_promises():
    for Nx, Ny in [(4, 3), (3, 3), (2, 2), (1, 5), (5, 1), (5, 7), (7, 5)]:
        N = Nx * Ny
        mv = Q.to_visit_order(Q.case_masks(Nx, Ny), Nx, Ny)
        firsts = {int(np.flatnonzero(m)[0]) for m in mv}
        assert firsts >= set(range(N))                              # f = 0, first row, every row turn, f = N-1
        assert any(m.all() for m in mv)
        if N > 32:
            assert any(m[31] and m[32] and m.sum() < N for m in mv)


def test_exact_strings_are_not_vacuous():
    """The weights and strings of the exact and statistical GPU tests: every exact value is at least FLOOR in magnitude, and
    sum_sigma P v of the brute-force local values is psi^T O psi."""
    prm = Q.exact_weights()
    for Nx, Ny in Q.EXACT_LATTICES:
        N = Nx * Ny
        c = all_configs(N)
        lp = M.mdrnn_log_probability(prm, c.reshape(-1, Nx, Ny))
        psi = np.exp(0.5 * lp)
        assert abs(np.exp(lp).sum() - 1.0) < 1e-12
        strings = Q.exact_strings(Nx, Ny)
        flip, sign, factor = O.pauli_terms(strings, N)
        assert np.all(factor.imag == 0)
        assert np.array_equal(c @ (1 << np.arange(N - 1, -1, -1)), np.arange(len(c)))
        exact = np.array([Q.string_expectation(psi, c, st) for st in strings])           # psi^T O psi without the 4096 x 4096 matrix
        print("%dx%d exact values %s" % (Nx, Ny, np.round(exact, 4)))
        assert np.abs(exact).min() >= Q.FLOOR
    # on a lattice small enough for dense matrices the same contraction is PR.dense_string's
    Nx, Ny = 2, 3
    c = all_configs(6)
    psi = np.exp(0.5 * M.mdrnn_log_probability(prm, c.reshape(-1, Nx, Ny)))
    for st in [[("X", 0)], [("Y", 1), ("Y", 4)], [("Z", 0), ("X", 5)], [("Y", 0), ("Z", 2), ("Y", 3), ("X", 4)]]:
        assert abs(Q.string_expectation(psi, c, st) - (psi @ PR.dense_string({i: p for p, i in st}, 6) @ psi).real) < 1e-14
