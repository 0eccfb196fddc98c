"""CPU tests of the host side of the Pauli-string observables (rnnwavefunctions_amd.observables): the parser, the Hamiltonian class
and its refusals, the builders, the grouping by flip mask, the statistics from the sums and minimize_hamiltonian's refusal.
"""
import numpy as np
import pytest

import pauli_reference as PR
from rnnwavefunctions_amd import observables as O


def test_parser_masks_and_factors():
    flip, sign, factor = O.pauli_terms(["XZIY", [("Y", 0), ("Y", 3)], [("z", 1)], "IIII", [("Y", 0), ("Y", 1), ("Y", 2), ("Y", 3)]], 4)
    assert flip.dtype == sign.dtype == np.int32
    assert flip.tolist() == [[1, 0, 0, 1], [1, 0, 0, 1], [0, 0, 0, 0], [0, 0, 0, 0], [1, 1, 1, 1]]
    assert sign.tolist() == [[0, 1, 0, 1], [1, 0, 0, 1], [0, 1, 0, 0], [0, 0, 0, 0], [1, 1, 1, 1]]
    assert factor.tolist() == [-1j, -1.0, 1.0, 1.0, 1.0]
    # YY = -(ZX)(ZX), on matrices
    zx = PR.SZ @ PR.SX
    assert np.array_equal(np.kron(PR.SY, PR.SY), -np.kron(zx, zx))
    for k, st in enumerate(["XZIY", "YIIY", "IZII", "IIII", "YYYY"]):
        assert np.allclose(factor[k] * PR.dense_term(flip[k], sign[k]), PR.dense_string(st, 4), atol=0)


def test_parser_and_hamiltonian_refusals():
    with pytest.raises(ValueError, match="I, X, Y, Z"):
        O.pauli_terms(["XAII"], 4)
    with pytest.raises(ValueError, match="out of range"):
        O.pauli_terms([[("X", 4)]], 4)
    with pytest.raises(ValueError, match="out of range"):
        O.Hamiltonian(4, [(1.0, [("Z", -1)])])
    with pytest.raises(ValueError, match="one letter per site"):
        O.pauli_terms(["XX"], 4)
    with pytest.raises(ValueError, match="twice"):
        O.pauli_terms([[("X", 1), ("Z", 1)]], 4)
    with pytest.raises(ValueError, match="imaginary matrix elements in the σᶻ basis"):
        O.Hamiltonian(4, [(1.0, "XXII"), (0.5, "XYII")])
    with pytest.raises(ValueError, match="real"):
        O.Hamiltonian(4, [(1.0 + 1.0j, "XXII")])
    with pytest.raises(ValueError, match="at least one term"):
        O.Hamiltonian(4, [])
    h = O.Hamiltonian(4, [(2.0, "YYII"), (3.0, "ZIIZ")])
    assert h.coeff.tolist() == [-2.0, 3.0] and len(h) == 2


def test_odd_y_strings_are_zero_without_a_wave_function():
    import rnnwavefunctions_amd._lib as L
    wf = object.__new__(L.NativeWavefunction)        # no handle, no library
    wf.N = 5
    out = O.pauli_expectations(wf, ["YIIII", [("X", 0), ("Y", 3)], "YYYII"], 100)
    assert out["value"].tolist() == [0.0, 0.0, 0.0] and out["err"].tolist() == [0.0, 0.0, 0.0]


def test_grouping_by_mask():
    xxz = O.xxz_hamiltonian(6, 1.0, 0.5, periodic=True)
    masks, index = O.group_by_mask(xxz.flip)
    assert len(xxz) == 18 and masks.shape == (6, 6)                    # XX and YY of a bond share one mask, ZZ has none
    assert index.reshape(6, 3).tolist() == [[b, b, -1] for b in range(6)]
    assert all(np.array_equal(masks[index[k]], xxz.flip[k]) for k in range(18) if index[k] >= 0)
    perm = np.random.RandomState(0).permutation(18)
    m2, i2 = O.group_by_mask(xxz.flip[perm])
    assert sorted(map(tuple, m2.tolist())) == sorted(map(tuple, masks.tolist()))
    assert all(np.array_equal(m2[i2[k]], xxz.flip[perm[k]]) for k in range(18) if i2[k] >= 0)
    tf = O.tfim_hamiltonian(np.ones((3, 4)), 2.0)
    masks, index = O.group_by_mask(tf.flip)
    assert len(tf) == 17 + 12 and masks.shape == (12, 12) and np.array_equal(masks, np.eye(12, dtype=np.int32))


def test_statistics_from_sums():
    v = np.random.RandomState(0).normal(0.3, 1.0, size=(3, 1000))
    mean, err = O.pauli_from_sums(PR.sums_from_values(v), 1000)
    assert np.allclose(mean, v.mean(axis=1)) and np.allclose(err, v.std(axis=1) / np.sqrt(1000))


def test_builders_refuse_bad_shapes_and_minimize_refuses_a_communicator():
    from rnnwavefunctions_amd.training import minimize_hamiltonian
    with pytest.raises(ValueError):
        O.xxz_hamiltonian(2, 1.0, 1.0, periodic=True)
    with pytest.raises(ValueError):
        O.tfim_hamiltonian(np.ones((2, 2, 2)), 1.0)
    with pytest.raises(ValueError, match="communicator"):
        minimize_hamiltonian(None, O.xxz_hamiltonian(4, 1.0, 1.0), {}, comm="env")
