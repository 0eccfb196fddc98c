"""CPU validation of tests/pauli_stack_reference.py, the float64 restatement the GPU tests of rnnwf_pauli_step_stack compare with: on
N = 6 with all 64 configurations enumerated, sum_sigma P(sigma) E_loc(sigma) is <psi|H|psi> of the dense matrix to 1e-12, for stacks
of 2 and 3 layers (equal and unequal widths) and the four Hamiltonians of the GPU tests.
"""
import numpy as np
import pytest

import ed
import pauli_stack_reference as SR
from conftest import all_configs
from rnnwavefunctions_amd import observables as O

N = 6


@pytest.mark.parametrize("name", ["xxz", "tfim", "diagonal", "mixed"])
@pytest.mark.parametrize("family,units", [("gru64", (8, 8)), ("gru64", (8, 8, 8)), ("gru64", (9, 5)), ("gru", (8, 8))],
                         ids=["2-layers", "3-layers", "unequal-widths", "float32-weights"])
def test_weighted_local_energies_are_the_dense_expectation(family, units, name):
    prm = SR.weights(family, units, seed=7)
    c = all_configs(N)
    lp = SR.scorer(prm)(c)
    psi = np.exp(0.5 * lp)
    assert abs(np.exp(lp).sum() - 1.0) <= 1e-12                     # the stack's P is normalised: the oracle runs every layer
    ham = SR.hamiltonian(name, N)
    Hd = SR.dense(ham)
    assert Hd.shape == (64, 64) and np.allclose(Hd, Hd.T, atol=0)
    ref = SR.reference(prm, c, ham)
    assert abs((np.exp(lp) * ref["eloc"]).sum() - psi @ Hd @ psi) <= 1e-12
    # per term: sum_sigma P v_k = <psi|O_k|psi>, and the sums are those of the values
    exact = np.array([psi @ SR.PR.dense_term(f, s) @ psi for f, s in zip(ham.flip, ham.sign)])
    assert np.abs((np.exp(lp)[None, :] * ref["values"]).sum(axis=1) - exact).max() <= 1e-12
    assert np.allclose(ref["term_sums"][:, 0], ref["values"].sum(axis=1), rtol=1e-14, atol=1e-14)
    # the rows of the log-ratios: distinct non-empty masks in order of first appearance, each scored from site 0
    masks, index = O.group_by_mask(ham.flip)
    assert ref["log_ratio"].shape == (len(masks), 64) and (len(masks) == 0) == (name == "diagonal")
    log_p = SR.scorer(prm)
    for m, row in zip(masks, ref["log_ratio"]):
        assert np.array_equal(row, 0.5 * (log_p(c ^ m[None, :].astype(c.dtype)) - lp))
    # the E_loc bound's weight is sum_k |c_k| r_k, from the reference alone
    r = np.where(index[:, None] >= 0, np.exp(ref["log_ratio"][np.maximum(index, 0)]) if len(masks) else 1.0, 1.0)
    assert np.allclose(ref["bound_weight"], np.abs(ham.coeff) @ r, rtol=1e-14)


def test_builders_agree_with_exact_diagonalisation_helpers():
    Jz = 1.0 + 0.1 * np.arange(N)
    tf = O.tfim_hamiltonian(Jz, 0.9)
    assert np.allclose(SR.dense(tf), ed.tfim_hamiltonian(Jz, 0.9, N), atol=1e-14)
    # the mixed Hamiltonian carries what the GPU cases need: first site 0, first site N - 1, the dense mask
    for n in (6, 34):
        ham = SR.hamiltonian("mixed", n)
        firsts = {int(np.flatnonzero(m)[0]) for m in ham.flip if m.any()}
        assert 0 in firsts and n - 1 in firsts and any(m.all() for m in ham.flip)
        if n > 32:
            assert any(m[30:35].all() and m.sum() == min(n, 35) - 30 for m in ham.flip)      # one run across the word boundary


def test_a_reference_with_one_layer_skipped_is_rejected_by_the_bounds():
    """the bounds see a stack evaluated without its upper layer's recurrence (the defect of restoring a layer from the wrong rows
    has this size): the float64 and the widest float32 tolerance are both far below it"""
    prm = SR.weights("gru64", (8, 8), seed=7)
    c = all_configs(N)
    ham = SR.hamiltonian("xxz", N)
    ref = SR.reference(prm, c, ham)
    bad = dict(prm)
    k = SR.SCOPE + "/" + SR.M.GRU % 1 + "candidate/hidden_projection/kernel"
    bad[k] = np.zeros_like(prm[k])
    wrong = SR.reference(bad, c, ham)
    assert np.abs(wrong["log_ratio"] - ref["log_ratio"]).max() > 1e3 * max(SR.f64_tol(N), 1e-4)
