"""Host-side checks of the 2D RNN's Pauli pass that need no GPU: the lattice -> visit mapping of the masks, the lattice index, the
2D XXZ builder and the ValueErrors raised in Python."""
import os
import re

import numpy as np
import pytest

import pauli_2d_reference as Q
import pauli_reference as PR
from oracle import models as M
from rnnwavefunctions_amd import _lib
from rnnwavefunctions_amd import observables_2d as O2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def driver_pos_of_site(Nx, Ny, k):
    """pos_of_site of csrc/mdrnn_observable.h, restated (the GPU tests check the compiled one through the log-ratios)."""
    nx, ny = divmod(k, Ny)
    return ny * Nx + (nx if ny % 2 == 0 else Nx - 1 - nx)


@pytest.mark.parametrize("Nx,Ny", [(3, 4), (4, 3)])
def test_lattice_masks_map_to_the_zigzag_order(Nx, Ny):
    N = Nx * Ny
    order = M.zigzag_order(Nx, Ny)
    pos = Q.visit_positions(Nx, Ny)
    assert sorted(pos) == list(range(N))
    for p, (nx, ny, _) in enumerate(order):
        k = O2.site(Nx, Ny, nx, ny)
        assert pos[k] == p == driver_pos_of_site(Nx, Ny, k)
        one = np.zeros(N, dtype=np.int32)
        one[k] = 1
        assert np.flatnonzero(Q.to_visit_order(one, Nx, Ny)).tolist() == [p]
    # the driver's formula is in the source as restated here
    src = open(os.path.join(ROOT, "rnnwavefunctions_amd", "csrc", "mdrnn_observable.h")).read()
    assert "const int nx = k / h->Ny, ny = k % h->Ny;" in src and "ny * h->Nx + (ny % 2 == 0 ? nx : h->Nx - 1 - nx)" in src
    # a mask that is not symmetric under the map: the first flipped POSITION is not the first flipped lattice index
    m = np.zeros(N, dtype=np.int32)
    m[[O2.site(Nx, Ny, Nx - 1, 1), O2.site(Nx, Ny, 0, 2)]] = 1
    assert np.flatnonzero(Q.to_visit_order(m, Nx, Ny))[0] == Nx


def test_site_is_the_c_order_index_of_the_samples():
    idx = np.arange(12).reshape(3, 4)
    for nx in range(3):
        for ny in range(4):
            assert O2.site(3, 4, nx, ny) == idx[nx, ny]
    for bad in [(3, 0), (0, 4), (-1, 0), (0.5, 0)]:
        with pytest.raises(ValueError):
            O2.site(3, 4, *bad)


def test_xxz_hamiltonian_2d_terms_and_hermiticity():
    Nx, Ny = 2, 3
    ham = O2.xxz_hamiltonian_2d(Nx, Ny, -1.0, 0.5)
    bonds = (Nx - 1) * Ny + Nx * (Ny - 1)
    assert len(ham) == 3 * bonds and ham.N == 6
    pairs = {tuple(sorted(i for _, i in st)) for _, st in ham.terms}
    want = {(O2.site(Nx, Ny, i, j), O2.site(Nx, Ny, i + 1, j)) for i in range(Nx - 1) for j in range(Ny)}
    want |= {(O2.site(Nx, Ny, i, j), O2.site(Nx, Ny, i, j + 1)) for i in range(Nx) for j in range(Ny - 1)}
    assert pairs == want
    Hd = sum(c * PR.dense_string({i: p for p, i in st}, 6) for c, st in ham.terms)
    assert np.abs(Hd.imag).max() == 0 and np.allclose(Hd, Hd.T.conj(), atol=0)
    # the (flip, sign, coeff) form is the same matrix
    H2 = sum(c * PR.dense_term(f, s) for c, f, s in zip(ham.coeff, ham.flip, ham.sign))
    assert np.allclose(H2, Hd.real, atol=1e-15)
    assert len(O2.xxz_hamiltonian_2d(1, 5, 1.0, 1.0)) == 12 and len(O2.xxz_hamiltonian_2d(5, 1, 1.0, 1.0)) == 12
    with pytest.raises(ValueError):
        O2.xxz_hamiltonian_2d(1, 1, 1.0, 1.0)


class FakeNative(_lib.NativeWavefunction):
    """A NativeWavefunction without a library handle: enough for the checks Python makes before the C call."""

    def __init__(self, model, nx, ny):
        self.h, self.lib, self.model, self.nx, self.ny, self.N = None, None, model, nx, ny, nx * ny


def test_python_refusals():
    wf = FakeNative(_lib.MODEL_MDRNN2D, 3, 2)
    one = np.zeros((1, 6), dtype=np.int32)
    with pytest.raises(ValueError, match="shape"):
        wf.pauli_step_2d(np.zeros((1, 7)), np.zeros((1, 7)), [1.0], 8)
    with pytest.raises(ValueError, match="shape"):
        wf.pauli_step_2d(np.zeros((1, 2, 3)), np.zeros((1, 2, 3)), [1.0], 8)          # (K, Ny, Nx) is not (K, Nx, Ny)
    with pytest.raises(ValueError, match="0 and 1"):
        wf.pauli_step_2d(one + 0.5, one, [1.0], 8)
    with pytest.raises(ValueError, match="coeff"):
        wf.pauli_step_2d(one, one, [1.0, 2.0], 8)
    with pytest.raises(ValueError, match="samples"):
        wf.pauli_step_2d(one, one, [1.0], 8, samples=np.zeros((8, 5), dtype=np.int32))
    with pytest.raises(ValueError, match="MDRNN2D"):
        O2.pauli_expectations(FakeNative(_lib.MODEL_GRU1D_F64, 3, 2), ["XIIIII"], 8)
    with pytest.raises(ValueError, match="MDRNN2D"):
        O2.energy(FakeNative(_lib.MODEL_GRU1D, 6, 1), O2.xxz_hamiltonian_2d(3, 2, 1.0, 1.0), 8)
    with pytest.raises(TypeError):
        O2.correlations(object(), 8)
    with pytest.raises(ValueError, match="sites"):
        O2.energy(wf, O2.xxz_hamiltonian_2d(3, 3, 1.0, 1.0), 8)
    with pytest.raises(ValueError, match="odd number of Y"):
        O2.Hamiltonian(6, [(1.0, [("Y", 0)])])
    with pytest.raises(ValueError, match="distinct"):
        O2.correlations(wf, 8, pairs=[(1, 1)])
    with pytest.raises(ValueError, match="distinct"):
        O2.correlations(wf, 8, pairs=[(0, 6)])
    # strings with an odd number of Y alone: 0 +- 0, and the handle-less wave function is never called
    out = O2.pauli_expectations(wf, ["YIIIII", [("X", 0), ("Y", 3)]], 8)
    assert np.all(out["value"] == 0) and np.all(out["err"] == 0)


def test_header_binding_and_build_list_name_the_entry_point():
    header = open(os.path.join(ROOT, "include", "rnnwf.h")).read()
    assert re.search(r"int rnnwf_pauli_step_2d\(rnnwf_handle\* h, const int32_t\* flip", header)
    assert _lib.PROTOTYPES["rnnwf_pauli_step_2d"] == _lib.PROTOTYPES["rnnwf_pauli_step"]
    from rnnwavefunctions_amd import build
    assert "mdrnn_pauli.hip" in build.SOURCES and build.compile_flags("mdrnn_pauli.hip") == build.compile_flags("mdrnn.hip")
