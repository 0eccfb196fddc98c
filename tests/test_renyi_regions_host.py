"""Host-side tests of the second Renyi entropy of arbitrary regions (rnnwf_renyi2_regions, rnnwavefunctions_amd.observables): the C
ABI declares and exports it with the bindings' argument types, the region builders follow the raster convention and refuse bad
bounds, and the mutual-information statistics equal the formula written out again."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT


def test_header_prototypes_and_library_declare_renyi2_regions():
    header = open(os.path.join(ROOT, "include", "rnnwf.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"int\s+rnnwf_renyi2_regions\s*\(\s*rnnwf_handle\s*\*\s*h\s*,\s*const\s+int32_t\s*\*\s*regions\s*,\s*int32_t\s+nregions"
                     r"\s*,\s*const\s+int32_t\s*\*\s*samples\s*,\s*int64_t\s+npairs\s*,\s*uint64_t\s+seed\s*,\s*uint64_t\s+step\s*,"
                     r"\s*int64_t\s+pair_offset\s*,\s*double\s*\*\s*sums\s*,\s*double\s*\*\s*out_log_ratio\s*,\s*int32_t\s*\*\s*out_samples"
                     r"\s*\)\s*;", code)
    assert "#define RNNWF_ABI_VERSION 1" in header
    from rnnwavefunctions_amd import _lib, build
    assert _lib.ABI_VERSION == 1
    res, args = _lib.PROTOTYPES["rnnwf_renyi2_regions"]
    i32p, f64p = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double)
    assert res is ctypes.c_int
    assert args == [ctypes.c_void_p, i32p, ctypes.c_int32, i32p, ctypes.c_int64, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int64,
                    f64p, f64p, i32p]
    lib = ctypes.CDLL(build.build())
    assert hasattr(lib, "rnnwf_renyi2_regions") and hasattr(lib, "rnnwf_renyi2_swap")
    assert hasattr(_lib.NativeWavefunction, "renyi2_regions")


def test_interval_region():
    from rnnwavefunctions_amd.observables import interval_region
    m = interval_region(10, 3, 7)
    assert m.dtype == np.int32 and m.shape == (10,) and m.tolist() == [0, 0, 0, 1, 1, 1, 1, 0, 0, 0]
    assert interval_region(5, 0, 5).tolist() == [1] * 5 and interval_region(5, 2, 2).tolist() == [0] * 5
    for bad in [(5, -1, 3), (5, 3, 2), (5, 0, 6), (0, 0, 0)]:
        with pytest.raises(ValueError):
            interval_region(*bad)


def test_rectangle_region_follows_the_raster_convention():
    from rnnwavefunctions_amd.observables import rectangle_region
    Nx, Ny = 4, 3
    m = rectangle_region(Nx, Ny, 1, 3, 0, 2)
    assert m.dtype == np.int32 and m.shape == (Nx * Ny,)
    want = [ny * Nx + nx for ny in range(0, 2) for nx in range(1, 3)]
    assert np.flatnonzero(m).tolist() == sorted(want) == [1, 2, 5, 6]
    assert np.flatnonzero(rectangle_region(Nx, Ny, 0, 1, 0, Ny)).tolist() == [0, 4, 8]          # column 0: stride Nx
    assert np.flatnonzero(rectangle_region(Nx, Ny, 0, Nx, 1, 2)).tolist() == [4, 5, 6, 7]       # row 1: contiguous
    # a chain as Nx x 1 is an interval
    assert rectangle_region(7, 1, 2, 5, 0, 1).tolist() == [0, 0, 1, 1, 1, 0, 0]
    for bad in [(4, 3, -1, 2, 0, 1), (4, 3, 2, 1, 0, 1), (4, 3, 0, 5, 0, 1), (4, 3, 0, 1, 0, 4), (4, 3, 0, 1, 2, 1), (0, 3, 0, 0, 0, 1)]:
        with pytest.raises(ValueError):
            rectangle_region(*bad)


def test_column_cut_regions():
    from rnnwavefunctions_amd.observables import column_cut_regions
    Nx, Ny = 4, 3
    m = column_cut_regions(Nx, Ny)
    assert m.dtype == np.int32 and m.shape == (Nx - 1, Nx * Ny)
    for c in range(1, Nx):
        assert np.array_equal(m[c - 1], (np.arange(Nx * Ny) % Nx < c).astype(np.int32))
    assert column_cut_regions(2, 1).tolist() == [[1, 0]]
    for bad in [(1, 3), (0, 3), (3, 0)]:
        with pytest.raises(ValueError):
            column_cut_regions(*bad)


def test_mutual_information_from_log_ratios_against_the_formula_written_out():
    from rnnwavefunctions_amd.observables import mutual_information2_from_log_ratios
    rng = np.random.RandomState(0)
    n = 1000
    la, lb, lab = rng.normal(-0.3, 0.5, n), rng.normal(-0.2, 0.4, n), rng.normal(-0.6, 0.7, n)
    I2, err = mutual_information2_from_log_ratios(la, lb, lab)
    ma = sum(np.exp(v) for v in la) / n
    mb = sum(np.exp(v) for v in lb) / n
    mab = sum(np.exp(v) for v in lab) / n
    want = (-np.log(ma)) + (-np.log(mb)) - (-np.log(mab))
    g = np.array([-np.exp(la[k]) / ma - np.exp(lb[k]) / mb + np.exp(lab[k]) / mab for k in range(n)])
    var = np.mean(g * g) - np.mean(g) ** 2
    assert abs(I2 - want) <= 1e-13
    assert abs(err / np.sqrt(var / n) - 1.0) <= 1e-10
    assert err > 0
    # the delta method is the linearisation: a finite-difference check of dI2 / d(weights) at the empirical distribution
    eps = 1e-6
    w = np.full(n, 1.0 / n)
    def i2_of(w):
        return -np.log(w @ np.exp(la)) - np.log(w @ np.exp(lb)) + np.log(w @ np.exp(lab))
    k = 17
    w2 = w.copy()
    w2[k] += eps
    assert abs((i2_of(w2) - i2_of(w)) / eps - g[k]) <= 1e-4


def test_mutual_information_is_exactly_zero_for_a_constant_product():
    """r_AB = r_A r_B pair by pair with constant r: I2 = 0 and err = 0 exactly."""
    from rnnwavefunctions_amd.observables import mutual_information2_from_log_ratios
    n = 64
    la, lb = np.full(n, np.log(0.5)), np.full(n, np.log(0.25))
    I2, err = mutual_information2_from_log_ratios(la, lb, la + lb)
    assert I2 == 0.0 and err == 0.0
    with pytest.raises(ValueError):
        mutual_information2_from_log_ratios(la, lb[:-1], la)
    with pytest.raises(ValueError):
        mutual_information2_from_log_ratios(la[None], lb[None], la[None])


def test_mutual_information_refuses_overlapping_regions_before_touching_the_wave_function():
    from rnnwavefunctions_amd.observables import interval_region, renyi2_mutual_information
    a, b = interval_region(8, 1, 4), interval_region(8, 3, 6)
    with pytest.raises(ValueError, match="disjoint"):
        renyi2_mutual_information(None, a, b, 10)                  # wf is not looked at: the masks are checked first
    with pytest.raises(ValueError):
        renyi2_mutual_information(None, a, interval_region(9, 5, 6), 10)
    with pytest.raises(ValueError):
        renyi2_mutual_information(None, 2 * a, interval_region(8, 5, 6), 10)
    with pytest.raises(TypeError):                                 # disjoint masks pass the check; None is no wave function
        renyi2_mutual_information(None, a, interval_region(8, 5, 6), 10)
