"""Host-side logic of the complex RNN's Renyi-2 entropies (rnnwavefunctions_amd/observables_complex.py, docs/renyi_complex.md):
the arithmetic on the four sums, the symmetry-resolved entropies on synthetic inputs, the overlap refusal, the ABI symbol.  No GPU."""
import os
import re

import numpy as np
import pytest

from rnnwavefunctions_amd import _lib
from rnnwavefunctions_amd import observables as O
from rnnwavefunctions_amd import observables_complex as OC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_entry_point_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "rnnwf.h")).read()
    assert re.search(r"\bint rnnwf_renyi2_regions_complex\(rnnwf_handle\* h, const int32_t\* regions, int32_t nregions,", header)
    assert "#define RNNWF_ABI_VERSION 1" in header
    restype, argtypes = _lib.PROTOTYPES["rnnwf_renyi2_regions_complex"]
    assert len(argtypes) == 12
    lib = _lib.load_library()
    assert lib.rnnwf_renyi2_regions_complex is not None and lib.rnnwf_abi_version() == 1
    assert "crnn_renyi.hip" in __import__("rnnwavefunctions_amd.build", fromlist=["SOURCES"]).SOURCES


def test_renyi2_from_sums_arithmetic():
    rng = np.random.RandomState(0)
    n = 1000
    r = rng.rand(3, n) * np.exp(1j * 0.3 * rng.standard_normal((3, n)))
    r[:, rng.rand(n) < 0.6] = 0.0                                # dead pairs enter as exact zeros
    sums = np.stack([r.real.sum(1), r.imag.sum(1), (r.real ** 2).sum(1), (r.imag ** 2).sum(1)], axis=1)
    out = OC.renyi2_from_sums(sums, n)
    assert np.allclose(out["S2"], -np.log(r.real.mean(1)), rtol=1e-13)
    assert np.allclose(out["err"], r.real.std(1) / (np.sqrt(n) * r.real.mean(1)), rtol=1e-10)
    assert np.allclose(out["imag"], r.imag.mean(1), rtol=1e-13, atol=1e-16)
    assert np.allclose(out["err_imag"], r.imag.std(1) / np.sqrt(n), rtol=1e-10)
    # r = 1 for every pair (an empty region): S2 = 0 exactly, no error
    one = OC.renyi2_from_sums(np.array([[7.0, 0.0, 7.0, 0.0]]), 7)
    assert one["S2"][0] == 0.0 and one["err"][0] == 0.0 and one["imag"][0] == 0.0 and one["err_imag"][0] == 0.0
    # a mean that is not positive has no logarithm
    assert np.isnan(OC.renyi2_from_sums(np.array([[-1.0, 0.0, 1.0, 0.0]]), 4)["S2"][0])
    with pytest.raises(ValueError):
        OC.renyi2_from_sums(np.zeros((2, 2)), 4)
    with pytest.raises(ValueError):
        OC.renyi2_from_sums(np.zeros((2, 4)), 0)


def test_mutual_information_on_values_is_the_log_ratio_arithmetic():
    rng = np.random.RandomState(1)
    la, lb, lab = rng.standard_normal((3, 500)) * 0.3
    assert O.mutual_information2_from_log_ratios(la, lb, lab) == O.mutual_information2_from_values(np.exp(la), np.exp(lb), np.exp(lab))


def test_overlapping_regions_are_refused_before_the_wave_function_is_looked_at():
    with pytest.raises(ValueError, match="disjoint; both contain the sites \\[2\\]"):
        OC.renyi2_mutual_information(object(), [0, 1, 1, 0], [0, 0, 1, 1], 10)
    with pytest.raises(ValueError, match="CRNN_U1|facade"):
        OC.renyi2_regions(object(), [0, 1, 1, 0], 10)


def test_symmetry_resolved_entropies_on_synthetic_pairs():
    # N = 4, A = {1, 2}; the pairs are written out so that every number can be checked by hand
    region = np.array([0, 1, 1, 0])
    sig = np.array([[1, 0, 1, 0], [1, 0, 1, 0], [0, 1, 1, 0], [1, 0, 0, 1], [0, 1, 0, 1], [1, 1, 0, 0]])      # q = 1 1 2 0 1 1
    tau = np.array([[0, 1, 0, 1], [0, 0, 1, 1], [0, 1, 1, 0], [1, 0, 0, 1], [1, 1, 0, 0], [0, 0, 1, 1]])      # q = 1 1 2 0 1 1
    tau[4] = [1, 0, 0, 1]                                                                                     # q = 0: pair 4 is dead
    samples = np.empty((12, 4), dtype=np.int32)
    samples[0::2], samples[1::2] = sig, tau
    lr = np.log(np.array([0.5, 0.25, 0.8, 0.4, 1.0, 0.2])).astype(np.complex128)
    lr[1] += 1j * np.pi / 3                                    # Re r = 0.125
    lr[4] = complex(-np.inf, 0.0)
    out = OC.symmetry_resolved_renyi2(lr, samples, region)
    assert np.array_equal(out["q"], [0, 1, 2])
    # p_q from both chains of every pair: q = 0: (1 + 1 + 1) / 12, q = 1: (2 + 2 + 1 + 2) / 12, q = 2: 2 / 12
    assert np.allclose(out["p"], [3 / 12, 7 / 12, 2 / 12])
    assert np.allclose(out["trace"], [0.4 / 6, (0.5 + 0.125 + 0.2) / 6, 0.8 / 6])
    assert abs(out["trace"].sum() - np.mean([0.5, 0.125, 0.8, 0.4, 0.0, 0.2])) <= 1e-15
    assert np.allclose(out["S2"], -np.log(out["trace"] / out["p"] ** 2))
    t1 = np.array([0.5, 0.125, 0.0, 0.0, 0.0, 0.2])
    u1 = np.array([1.0, 1.0, 0.0, 0.0, 0.5, 1.0])
    assert np.allclose(out["trace_err"][1], t1.std() / np.sqrt(6)) and np.allclose(out["p_err"][1], u1.std() / np.sqrt(6))
    assert np.allclose(out["S2_err"][1], (-t1 / t1.mean() + 2 * u1 / u1.mean()).std() / np.sqrt(6))
    # a charge nobody shows
    wide = OC.symmetry_resolved_renyi2(lr[2:3], samples[4:6], np.array([1, 1, 1, 0]))
    assert wide["p"][3] == 0.0 and np.isnan(wide["S2"][3]) and wide["p"][2] == 1.0 and abs(wide["S2"][2] + np.log(0.8)) <= 1e-15
    # inputs that do not belong together: a live pair with different charges
    bad = lr.copy()
    bad[4] = 0.0
    with pytest.raises(ValueError, match="different charges"):
        OC.symmetry_resolved_renyi2(bad, samples, region)
    with pytest.raises(ValueError):
        OC.symmetry_resolved_renyi2(lr, samples[:10], region)
