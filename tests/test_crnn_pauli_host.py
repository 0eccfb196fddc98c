"""Host side of the complex RNN's Pauli-string observables (rnnwavefunctions_amd/observables_complex.py): term factors, hermiticity
by pairing, the construction and grouping of the spin-correlation terms, the structure factor of a known matrix, the refusals
Python makes before the C call, and the wiring of the entry point.  No GPU."""
import os
import re
import warnings

import numpy as np
import pytest

import crnn_pauli_reference as CR
from conftest import ROOT
from rnnwavefunctions_amd import _lib
from rnnwavefunctions_amd import observables_complex as OC
from rnnwavefunctions_amd.observables import group_by_mask


class FakeNative(_lib.NativeWavefunction):
    """A NativeWavefunction without a library handle: enough for the checks Python makes before the C call."""

    def __init__(self, model, N):
        self.h, self.lib, self.model, self.nx, self.ny, self.N = None, None, model, N, 1, N


def test_complex_hamiltonian_factors_carry_the_powers_of_minus_i():
    N = 4
    ham = OC.ComplexHamiltonian(N, [(2.0, "XXII"), (3.0, "YYII"), (1.5, "XYII"), (0.5j, "YYYI"), (1.0, "ZIIZ")])
    assert np.array_equal(ham.coeff, np.array([2.0, -3.0, -1.5j, 0.5j * 1j, 1.0]))
    assert np.array_equal(ham.flip[2], [1, 1, 0, 0]) and np.array_equal(ham.sign[2], [0, 1, 0, 0])
    assert not ham.flip[4].any() and np.array_equal(ham.sign[4], [1, 0, 0, 1])
    dense = CR.dense_hamiltonian(ham)
    want = (2.0 * CR.dense_string("XXII", N) + 3.0 * CR.dense_string("YYII", N) + 1.5 * CR.dense_string("XYII", N)
            + 0.5j * CR.dense_string("YYYI", N) + CR.dense_string("ZIIZ", N))
    assert np.abs(dense - want).max() == 0.0
    with pytest.raises(ValueError):
        OC.ComplexHamiltonian(N, [])


def test_is_hermitian_pairs_terms_and_agrees_with_the_dense_matrix():
    N = 4
    cases = [([(1.0, "XYII")], True), ([(1j, "XYII")], False), ([(1.0, "XXII"), (0.3, "YZIX")], True),
             ([(0.5 + 0.5j, "XXII"), (0.5 - 0.5j, "XXII")], True),            # duplicates are summed before the check
             ([(0.5 + 0.5j, "XXII")], False), ([(1.0, "ZZII"), (2j, "IIZZ")], False)]
    for terms, want in cases:
        ham = OC.ComplexHamiltonian(N, terms)
        dense = CR.dense_hamiltonian(ham)
        assert ham.is_hermitian() == want == bool(np.abs(dense - dense.conj().T).max() < 1e-12), terms
    raw = OC.ComplexHamiltonian(N, [(1.0, "XIII")])
    raw.sign[0, 0] = 1                                             # the raw term sz_0 sx_0 = i sy_0 with a real coefficient
    assert not raw.is_hermitian()
    raw.coeff[0] = 1j
    assert raw.is_hermitian()


def test_j1j2_hamiltonian_terms():
    N = 6
    J1, J2, Bz = np.ones(N), np.zeros(N), np.zeros(N)
    ham = OC.j1j2_hamiltonian(J1, J2, Bz)
    assert len(ham) == 3 * (N - 1)                                 # J2 = 0 and Bz = 0 add nothing
    assert len(OC.j1j2_hamiltonian(J1, J1, J1, periodic=True)) == 3 * 2 * N + N
    mar = OC.j1j2_hamiltonian(J1, J2, Bz, marshall=True)
    assert np.array_equal(mar.coeff[0::3], -ham.coeff[0::3]) and np.array_equal(mar.coeff[1::3], -ham.coeff[1::3])
    assert np.array_equal(mar.coeff[2::3], ham.coeff[2::3])
    with pytest.raises(ValueError):
        OC.j1j2_hamiltonian(np.ones(4), np.ones(5), np.ones(4))
    with pytest.raises(ValueError):
        OC.j1j2_hamiltonian(np.zeros(4), np.zeros(4), np.zeros(4))


def test_spin_correlation_terms_construction_and_grouping():
    N = 6
    pairs, strings = OC.spin_correlation_terms(N)
    assert len(pairs) == N * (N - 1) // 2 and len(strings) == 3 * len(pairs)
    assert [tuple(p) for p in pairs] == [(i, j) for i in range(N) for j in range(i + 1, N)]
    from rnnwavefunctions_amd.observables import pauli_terms
    flip, sign, factor = pauli_terms(strings, N)
    masks, index = group_by_mask(flip)
    assert len(masks) == len(pairs)                                # one mask per pair: XX and YY share it, ZZ has none
    assert np.array_equal(index[0::3], np.arange(len(pairs))) and np.array_equal(index[1::3], index[0::3])
    assert np.all(index[2::3] == -1)
    assert np.all(factor[0::3] == 1.0) and np.all(factor[1::3] == -1.0) and np.all(factor[2::3] == 1.0)
    # 1/4 (XX + YY + ZZ) of pair (1, 4) is S_1 . S_4
    k = [tuple(p) for p in pairs].index((1, 4))
    dense = 0.25 * sum(CR.dense_string(s, N) for s in strings[3 * k:3 * k + 3])
    half = {c: 0.5 * CR.PAULI[c] for c in "XYZ"}
    want = sum(np.kron(np.kron(np.kron(np.eye(2), half[c]), np.eye(4)), np.kron(half[c], np.eye(2))) for c in "XYZ")
    assert np.abs(dense - want).max() < 1e-15


def test_structure_factor_of_known_matrices():
    N = 8
    neel = 0.25 * (-1.0) ** (np.arange(N)[:, None] - np.arange(N)[None, :])
    assert OC.structure_factor(neel, np.pi) == pytest.approx(0.25 * N, abs=1e-12)
    assert OC.structure_factor(neel, 0.0) == pytest.approx(0.0, abs=1e-12)
    ident = 0.75 * np.eye(N)
    q = np.linspace(0.0, 2 * np.pi, 5)
    assert np.allclose(OC.structure_factor(ident, q), 0.75, atol=1e-14) and OC.structure_factor(ident, q).shape == (5,)
    rng = np.random.RandomState(0)
    c = rng.standard_normal((N, N))
    c = c + c.T
    x = 0.7
    want = sum(np.exp(1j * x * (j - k)) * c[j, k] for j in range(N) for k in range(N)).real / N
    assert OC.structure_factor(c, x) == pytest.approx(want, abs=1e-12)
    with pytest.raises(ValueError):
        OC.structure_factor(np.zeros((3, 4)), 0.0)


def test_value_errors_before_the_c_call():
    ham = OC.ComplexHamiltonian(6, [(1.0, "XXIIII")])
    for model in (_lib.MODEL_GRU1D, _lib.MODEL_GRU1D_PARITY, _lib.MODEL_GRU1D_F64, _lib.MODEL_MDRNN2D, _lib.MODEL_LSTM1D_F64):
        wf = FakeNative(model, 6)
        for call in (lambda: OC.pauli_expectations(wf, ["XXIIII"], 8), lambda: OC.energy(wf, ham, 8), lambda: OC.spin_correlations(wf, 8),
                     lambda: OC.minimize_hamiltonian(wf, ham, 8, 1, 1e-3, params={})):
            with pytest.raises(ValueError, match="CRNN_U1"):
                call()
    with pytest.raises(ValueError):
        OC.energy(object(), ham, 8)
    wf = FakeNative(_lib.MODEL_CRNN_U1, 8)
    with pytest.raises(ValueError, match="sites"):
        OC.energy(wf, ham, 8)
    with pytest.raises(ValueError, match="sites"):
        OC.minimize_hamiltonian(wf, ham, 8, 1, 1e-3, params={})
    with pytest.raises(ValueError, match="params"):
        OC.minimize_hamiltonian(wf, OC.ComplexHamiltonian(8, [(1.0, "XXIIIIII")]), 8, 1, 1e-3)
    with pytest.raises(ValueError, match="shape"):
        wf.pauli_step_complex(np.zeros((1, 7)), np.zeros((1, 7)), [1.0], 8)
    with pytest.raises(ValueError, match="coeff"):
        wf.pauli_step_complex(np.zeros((2, 8)), np.zeros((2, 8)), [1.0], 8)
    with pytest.raises(ValueError, match="integers"):
        wf.pauli_step_complex(np.full((1, 8), 0.5), np.zeros((1, 8)), [1.0], 8)
    with pytest.raises(ValueError, match="samples"):
        wf.pauli_step_complex(np.ones((1, 8)), np.zeros((1, 8)), [1.0], 8, samples=np.zeros((7, 8)))


def test_energy_warns_for_a_non_hermitian_hamiltonian():
    class Recorder(FakeNative):
        def pauli_step_complex(self, flip, sign, coeff, ns, **kw):
            return {"moments": np.array([2.0, 6.0, 4.0, 1.0])}

    wf = Recorder(_lib.MODEL_CRNN_U1, 4)
    with pytest.warns(UserWarning, match="not Hermitian"):
        res = OC.energy(wf, OC.ComplexHamiltonian(4, [(1j, "XXII")]), 4)
    assert res["mean"] == complex(0.5, 0.25) and res["var"] == pytest.approx(1.5 - 0.25)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        OC.energy(wf, OC.ComplexHamiltonian(4, [(1.0, "XXII")]), 4)


def test_header_binding_and_build_list_name_the_entry_point():
    header = open(os.path.join(ROOT, "include", "rnnwf.h")).read()
    assert re.search(r"int rnnwf_pauli_step_complex\(rnnwf_handle\* h, const int32_t\* flip", header)
    assert "#define RNNWF_ABI_VERSION 1" in header
    assert "rnnwf_pauli_step_complex" in _lib.PROTOTYPES
    from rnnwavefunctions_amd import build
    assert "crnn_pauli.hip" in build.SOURCES and build.compile_flags("crnn_pauli.hip") == build.compile_flags("crnn.hip")
