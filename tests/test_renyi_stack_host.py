"""CPU tests of the host side of rnnwf_renyi2_regions_stack (docs/renyi_stack.md): the header, the ctypes prototype and the
NativeWavefunction method agree with the one-layer entry's, and observables_stack validates its arguments before it touches the wave
function.  No device: the wave functions are fakes."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from rnnwavefunctions_amd import observables as O
from rnnwavefunctions_amd import observables_stack as OS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY, ONE_LAYER = "rnnwf_renyi2_regions_stack", "rnnwf_renyi2_regions"


def test_header_prototype_export_and_method_agree():
    from rnnwavefunctions_amd import _lib, build
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rnnwf.h")).read(), flags=re.S)
    assert re.search(r"#define\s+RNNWF_ABI_VERSION\s+1\b", header)
    decl = {name: re.search(r"\b%s\s*\(([^)]*)\)" % name, header) for name in (ENTRY, ONE_LAYER)}
    assert all(decl.values())
    args, args_1 = ([" ".join(a.split()) for a in m.group(1).split(",")] for m in decl.values())
    assert len(args) == 11 and args == args_1                              # the argument list is the one-layer entry's
    assert _lib.PROTOTYPES[ENTRY] is _lib.PROTOTYPES[ONE_LAYER]            # one object, not a copy
    assert hasattr(ctypes.CDLL(build.build()), ENTRY)
    assert _lib.ABI_VERSION == 1 and _lib.load_library().rnnwf_abi_version() == 1
    assert "renyi_stack.hip" in build.SOURCES and build.compile_flags("renyi_stack.hip") == build.compile_flags("pauli_stack.hip")
    W = _lib.NativeWavefunction
    p, p_1 = inspect.signature(W.renyi2_regions_stack).parameters, inspect.signature(W.renyi2_regions).parameters
    assert list(p) == list(p_1) and [v.default for v in p.values()] == [v.default for v in p_1.values()]


def test_module_interface():
    assert OS.RENYI_API == ["renyi2_regions", "renyi2_entropy", "renyi2_mutual_information", "interval_region", "rectangle_region",
                            "column_cut_regions", "renyi2_from_sums"]
    assert all(callable(getattr(OS, name)) for name in OS.RENYI_API)
    for name in ("renyi2_regions", "renyi2_entropy", "renyi2_mutual_information"):
        a, b = inspect.signature(getattr(OS, name)).parameters, inspect.signature(getattr(O, name)).parameters
        assert list(a) == list(b) and [v.default for v in a.values()] == [v.default for v in b.values()], name
    for name in ("interval_region", "rectangle_region", "column_cut_regions", "renyi2_from_sums"):
        assert getattr(OS, name) is getattr(O, name)                       # the existing builders, not copies


def _handle(model, units, N=6, answer=None):
    """passes observables._native without a library or a device.  answer None: every library call raises; otherwise
    renyi2_regions_stack records its arguments and returns answer(regions, numpairs, log_ratio)"""
    from rnnwavefunctions_amd import _lib

    class NoLibrary(_lib.NativeWavefunction):
        def __init__(self):
            self.model, self.N, self.nx, self.ny, self.units, self.calls = model, N, N, 1, tuple(units), []

        def __del__(self):
            pass

        def __getattribute__(self, name):
            if name in ("lib", "h") or (name == "renyi2_regions_stack" and answer is None):
                raise AssertionError("the library was touched: %s" % name)
            return object.__getattribute__(self, name)

        def renyi2_regions_stack(self, regions, numpairs, samples=None, seed=111, step=0, pair_offset=0, log_ratio=False):
            self.calls.append(dict(regions=np.array(regions), numpairs=numpairs, samples=samples, seed=seed, step=step, log_ratio=log_ratio))
            return answer(np.asarray(regions), numpairs, log_ratio)
    return NoLibrary()


def test_refusals_fire_before_any_library_call():
    from rnnwavefunctions_amd import _lib
    a, b = O.interval_region(6, 1, 2), O.interval_region(6, 3, 5)
    calls = [lambda w: OS.renyi2_regions(w, [a, b], 10), lambda w: OS.renyi2_entropy(w, 10), lambda w: OS.renyi2_mutual_information(w, a, b, 10)]
    for model in (_lib.MODEL_GRU1D, _lib.MODEL_GRU1D_F64):
        for call in calls:
            with pytest.raises(ValueError, match="one layer; observables.py"):
                call(_handle(model, (10,)))
    for model in (_lib.MODEL_GRU1D_PARITY, _lib.MODEL_CRNN_U1, _lib.MODEL_MDRNN2D, _lib.MODEL_LSTM1D_F64):
        for call in calls:
            with pytest.raises(ValueError, match="positive GRU models"):
                call(_handle(model, (10, 10)))
    with pytest.raises(TypeError):
        OS.renyi2_entropy(object(), 10)
    with pytest.raises(ValueError, match="disjoint"):
        OS.renyi2_mutual_information(_handle(_lib.MODEL_GRU1D, (8, 8)), a, a, 10)


def test_entropy_and_mutual_information_are_the_arithmetic_of_observables():
    from rnnwavefunctions_amd import _lib
    N, n = 6, 40
    rng = np.random.RandomState(0)
    lr = rng.normal(-0.2, 0.5, size=(N + 1, n))

    def answer(regions, numpairs, log_ratio):
        assert numpairs == n
        rows = lr[:len(regions)].copy()
        trivial = np.all(regions == regions[:, :1], axis=1)              # empty or full: the library returns exactly 0
        rows[trivial] = 0.0
        out = {"sums": np.stack([np.exp(rows).sum(axis=1), np.exp(2 * rows).sum(axis=1)], axis=1)}
        if log_ratio:
            out["log_ratio"] = rows
        return out
    wf = _handle(_lib.MODEL_GRU1D_F64, (8, 8, 8), N, answer)
    samples = rng.randint(0, 2, size=(2 * n, 3, 2))
    S2, err = OS.renyi2_entropy(wf, n, seed=7, step=3, samples=samples)
    call = wf.calls[-1]
    assert call["regions"].shape == (N + 1, N) and call["samples"].shape == (2 * n, N) and (call["seed"], call["step"]) == (7, 3)
    for l in range(N + 1):                                                  # cut l as its complement, the suffix {l..N-1}
        assert np.array_equal(call["regions"][l], (np.arange(N) >= l).astype(np.int32))
    rows = lr.copy()
    rows[[0, N]] = 0.0
    want = O.renyi2_from_sums(np.stack([np.exp(rows).sum(axis=1), np.exp(2 * rows).sum(axis=1)], axis=1), n)
    assert np.array_equal(S2, want[0]) and np.array_equal(err, want[1])
    assert S2[0] == 0.0 and S2[N] == 0.0 and err[0] == 0.0 and err[N] == 0.0 and np.all(err[1:N] > 0.0)
    a, b = O.interval_region(N, 1, 2), O.interval_region(N, 3, 5)
    got = OS.renyi2_mutual_information(wf, a, b, n)
    call = wf.calls[-1]
    assert np.array_equal(call["regions"], np.stack([a, b, a | b])) and call["log_ratio"] and call["samples"] is None
    assert got == O.mutual_information2_from_log_ratios(lr[0], lr[1], lr[2])
    S2r, errr = OS.renyi2_regions(wf, [a, b], n)
    want = O.renyi2_from_sums(np.stack([np.exp(lr[:2]).sum(axis=1), np.exp(2 * lr[:2]).sum(axis=1)], axis=1), n)
    assert np.array_equal(S2r, want[0]) and np.array_equal(errr, want[1])
