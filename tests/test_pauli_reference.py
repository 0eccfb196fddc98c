"""CPU validation of tests/pauli_reference.py (the brute-force restatement the GPU tests of rnnwf_pauli_step compare with) and the
defect study behind the GPU bounds: which errors of the flip-mask pass the bounds reject, and which rounding they accept.
"""
import numpy as np
import pytest

import ed
import pauli_reference as PR
import renyi_reference as R
from conftest import all_configs
from rnnwavefunctions_amd import observables as O
from rnnwavefunctions_amd import params as P


def weights(H, seed, f64=True, scale=3.0):
    prm = P.init_gru_params([H], seed=seed, dtype=np.float64 if f64 else np.float32)
    return P.randomize_biases(P.scale_kernels(prm, scale), seed + 1)


def state(prm, N):
    c = all_configs(N)
    log_p = R._scorer(R.to64(prm), np.float64)
    lp = log_p(c)
    return c, log_p, lp, np.exp(0.5 * lp)


def dense(st, N):
    return PR.dense_string({i: p for p, i in st}, N)


@pytest.mark.parametrize("N", [4, 5, 6, 7, 8])
def test_weighted_local_values_are_the_dense_expectations(N):
    """sum_sigma P(sigma) v_k(sigma) = psi^T O_k psi to 1e-12, strings with X, Y and Z, site 0 included."""
    c, log_p, lp, psi = state(weights(8, N), N)
    rng = np.random.RandomState(N)
    strings = [[("X", 0)], [("Y", 0), ("Y", N - 1)], [("Z", 0), ("X", 0 + 1)], [("X", i) for i in range(N)], [("Z", i) for i in range(N)],
               [("Y", 0), ("Y", 1), ("X", 2), ("Z", 3)]]
    for _ in range(10):                              # random strings with an even number of Y
        letters = rng.choice(list("IXYZ"), size=N)
        if np.sum(letters == "Y") % 2:
            letters[np.flatnonzero(letters == "Y")[0]] = "X"
        strings.append([(p, i) for i, p in enumerate(letters)])
    flip, sign, factor = O.pauli_terms(strings, N)
    assert np.all(factor.imag == 0)
    v = PR.local_values(log_p, c, flip, sign)
    got = factor.real * (np.exp(lp)[None, :] * v).sum(axis=1)
    exact = np.array([(psi @ dense(st, N) @ psi).real for st in strings])
    assert np.abs(got - exact).max() <= 1e-12
    for k, st in enumerate(strings):                 # the (flip, sign, factor) decomposition is the matrix itself
        assert np.allclose(factor[k] * PR.dense_term(flip[k], sign[k]), dense(st, N), atol=0)


@pytest.mark.parametrize("Nx,Ny", [(2, 3), (3, 2)])
def test_raster_energies_of_the_builders(Nx, Ny):
    N = Nx * Ny
    c, log_p, lp, psi = state(weights(8, 11), N)
    Jz = np.random.RandomState(3).uniform(0.5, 1.5, size=(Nx, Ny))
    ham = O.tfim_hamiltonian(Jz, 1.7)
    e = PR.local_energy(log_p, c, ham.flip, ham.sign, ham.coeff)
    Hd = sum(cf * dense(st, N).real for cf, st in ham.terms)
    assert np.allclose(Hd, ed.tfim2d_hamiltonian(Jz, 1.7, Nx, Ny), atol=1e-14)
    assert abs((np.exp(lp) * e).sum() - psi @ Hd @ psi) <= 1e-12
    xxz = O.xxz_hamiltonian(N, 0.8, -0.3, periodic=True)
    Hx = sum(cf * dense(st, N).real for cf, st in xxz.terms)
    e = PR.local_energy(log_p, c, xxz.flip, xxz.sign, xxz.coeff)
    assert abs((np.exp(lp) * e).sum() - psi @ Hx @ psi) <= 1e-12 and np.allclose(Hx, Hx.T)


@pytest.mark.parametrize("N", [4, 6, 8])
def test_chain_energies_of_the_builders(N):
    c, log_p, lp, psi = state(weights(8, 2 * N), N)
    Jz = np.random.RandomState(N).uniform(0.5, 1.5, size=N)
    ham = O.tfim_hamiltonian(Jz, 0.9)
    Hd = sum(cf * dense(st, N).real for cf, st in ham.terms)
    assert np.allclose(Hd, ed.tfim_hamiltonian(Jz, 0.9, N), atol=1e-14)
    e = PR.local_energy(log_p, c, ham.flip, ham.sign, ham.coeff)
    assert abs((np.exp(lp) * e).sum() - psi @ Hd @ psi) <= 1e-12
    for periodic in (False, True):
        xxz = O.xxz_hamiltonian(N, -1.0, 0.5, periodic=periodic)
        Hx = sum(cf * dense(st, N).real for cf, st in xxz.terms)
        # sx sx + sy sy = 2 (s+ s- + s- s+): the hopping of a pair of unequal neighbours, amplitude 2 Jxy
        k = int("01" + "0" * (N - 2), 2)
        assert Hx[int("10" + "0" * (N - 2), 2), k] == -2.0
        e = PR.local_energy(log_p, c, xxz.flip, xxz.sign, xxz.coeff)
        assert abs((np.exp(lp) * e).sum() - psi @ Hx @ psi) <= 1e-12
        if periodic is False:                        # the ferromagnetic XY ground state is positive
            w, vec = np.linalg.eigh(Hx + np.diag(np.full(2 ** N, 0.0)))
            assert w[0] < 0


def test_statistical_strings_are_not_vacuous():
    """The strings and weights tests/test_gpu_pauli.py draws 2^16 samples for: every exact value at least 0.05 in magnitude."""
    import test_gpu_pauli as T
    for f64, Nx, Ny, H in T.EXACT_CASES:
        N = Nx * Ny
        c, log_p, lp, psi = state(T.trained_like(H, T.EXACT_SEED, f64), N)
        psi = psi / np.linalg.norm(psi)
        exact = np.array([(psi @ dense(st, N) @ psi).real for st in T.exact_strings(N)])
        assert np.abs(exact).min() >= T.FLOOR, np.round(exact, 3)


def test_kernel_form_equals_the_brute_force_and_full_size_sets_are_complete():
    N = 40
    prm = weights(12, 5)
    s = np.random.RandomState(0).randint(0, 2, size=(20, N)).astype(np.int32)
    names, masks = zip(*PR.mask_set(N, 1))
    masks = np.stack(masks)
    assert np.abs(PR.kernel_form(prm, s, masks) - PR.log_ratio(prm, s, masks)).max() <= 1e-12
    for Nx, Ny, ns in [(80, 1, 5003), (33, 1, 500), (64, 1, 500), (65, 1, 500), (40, 1, 203), (100, 1, 301), (6, 6, 1003), (4, 8, 301), (8, 8, 301)]:
        _, m = zip(*PR.mask_set(Nx, Ny))
        PR.check_subset(ns, Nx * Ny, PR.choose_chains(ns), np.stack(m))
        assert len({mm.tobytes() for mm in m}) == len(m)


# ---- the defect study: what the GPU bounds reject and accept (ratios in docs/pauli.md) ------------------------------------------------
DEFECTS = ["mask_shifted", "mask_word_0", "checkpoint_f"]


@pytest.mark.parametrize("N,H", [(40, 20), (70, 30)])
def test_the_bounds_reject_the_defects_and_accept_float32_in_another_order(N, H):
    prm = weights(H, 111, f64=False)
    s = np.random.RandomState(1).randint(0, 2, size=(48, N)).astype(np.int32)
    names, masks = zip(*PR.mask_set(N, 1))
    masks = np.stack(masks)
    ref = PR.log_ratio(prm, s, masks, dtype=np.float64)
    dev32 = float(np.abs(PR.log_ratio(prm, s, masks, dtype=np.float32) - ref).max())
    bound, _ = PR.f32_bound(dev32, N)                # the full-size rule
    small = 1e-5 * N                                 # the small-size rule
    other = float(np.abs(PR.log_ratio_other_order(prm, s, masks) - ref).max())
    print("N=%d H=%d: dev32 %.2e, bound %.2e (small-size bound %.2e); float32 in another order %.2e = %.2f x bound"
          % (N, H, dev32, bound, small, other, other / bound))
    assert other <= bound and other <= small
    for d in DEFECTS:
        got = PR.kernel_form(prm, s, masks, defect=d, dtype=np.float32)
        hit = [k for k in range(len(masks)) if np.abs(got[k] - ref[k]).max() > max(bound, small)]
        worst = float(np.abs(got - ref).max())
        print("  defect %-13s max |d log r| = %.2e = %.1e x bound, %d of %d masks beyond it" % (d, worst, worst / bound, len(hit), len(masks)))
        assert hit and worst > 100 * max(bound, small)
    # a sign read from the flipped configuration instead of the sampled one: a term whose S and F overlap in an odd number of sites
    # changes sign in every sample.  Strings with an even number of Y overlap evenly (the defect cannot touch them); raw terms
    # such as sz_0 sx_0 do not, and tests/test_gpu_pauli.py feeds two of them: their sums of v over the samples turn round, a
    # relative change of 2 against the 1e-12 the sums are held to
    n = 8
    c, log_p, lp, psi = state(weights(8, 3), n)
    flip, sign, factor = O.pauli_terms([[("Y", 1), ("Y", 2)], [("Y", 0)], [("Y", 1), ("X", 2)], [("Y", 2), ("Y", 4)]], n)
    lr = PR.log_ratio_masks(log_p, c, flip)
    right = (PR.signs(c, sign) * np.exp(lr)).sum(axis=1)
    wrong = np.stack([(PR.signs(c ^ flip[k][None, :], sign[k:k + 1])[0] * np.exp(lr[k])).sum() for k in range(len(flip))])
    rel = np.abs(wrong / right - 1.0)
    print("  sign from the flipped configuration: relative change of the sums of v %s" % np.round(rel, 3))
    assert rel[0] < 1e-12 and rel[3] < 1e-12         # even overlap: the same sign
    assert abs(rel[1] - 2.0) < 1e-12 and abs(rel[2] - 2.0) < 1e-12
