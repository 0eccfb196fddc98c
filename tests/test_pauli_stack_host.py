"""CPU tests of the host side of rnnwf_pauli_step_stack / rnnwf_pauli_train_steps_stack (docs/pauli_stack.md): the header, the ctypes
prototypes and the NativeWavefunction methods agree with the one-layer entries', and observables_stack validates its arguments before
it touches the wave function.  No device: the wave functions are fakes that record their calls."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from rnnwavefunctions_amd import observables as O
from rnnwavefunctions_amd import observables_stack as OS
from rnnwavefunctions_amd import params as P
from rnnwavefunctions_amd import training as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCOPE = "RNNwavefunction"
PAIRS = [("rnnwf_pauli_step_stack", "rnnwf_pauli_step", 15), ("rnnwf_pauli_train_steps_stack", "rnnwf_pauli_train_steps", 17)]


def test_header_prototypes_exports_and_methods_agree():
    from rnnwavefunctions_amd import _lib, build
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rnnwf.h")).read(), flags=re.S)
    assert re.search(r"#define\s+RNNWF_ABI_VERSION\s+1\b", header)
    lib = ctypes.CDLL(build.build())
    for entry, one_layer, nargs in PAIRS:
        decl = {name: re.search(r"\b%s\s*\(([^)]*)\)" % name, header) for name in (entry, one_layer)}
        assert all(decl.values()), entry
        args, args_1 = ([" ".join(a.split()) for a in m.group(1).split(",")] for m in decl.values())
        assert len(args) == nargs and args == args_1                          # the argument list is the one-layer entry's
        assert _lib.PROTOTYPES[entry] is _lib.PROTOTYPES[one_layer]           # one object, not a copy
        assert hasattr(lib, entry)
    assert _lib.ABI_VERSION == 1 and _lib.load_library().rnnwf_abi_version() == 1
    assert "pauli_stack.hip" in build.SOURCES and build.compile_flags("pauli_stack.hip") == build.compile_flags("prnn.hip")
    W = _lib.NativeWavefunction
    for m, m_1 in [(W.pauli_step_stack, W.pauli_step), (W.pauli_train_steps_stack, W.pauli_train_steps)]:
        p, p_1 = inspect.signature(m).parameters, inspect.signature(m_1).parameters
        assert list(p) == list(p_1) and [v.default for v in p.values()] == [v.default for v in p_1.values()]


def test_module_interface():
    assert OS.__all__ == ["pauli_expectations", "energy", "correlations", "minimize_hamiltonian"]
    for name in ("pauli_expectations", "energy"):
        a, b = inspect.signature(getattr(OS, name)).parameters, inspect.signature(getattr(O, name)).parameters
        assert list(a) == list(b) and [v.default for v in a.values()] == [v.default for v in b.values()], name
    a, b = inspect.signature(OS.minimize_hamiltonian).parameters, inspect.signature(T.minimize_hamiltonian).parameters
    assert list(a) == list(b) and [v.default for v in a.values()] == [v.default for v in b.values()]
    assert a["device_steps"].default is None
    from rnnwavefunctions_amd import observables_2d as O2
    a, b = inspect.signature(OS.correlations).parameters, inspect.signature(O2.correlations).parameters
    assert list(a) == list(b) and [v.default for v in a.values()] == [v.default for v in b.values()]
    assert OS.Hamiltonian is O.Hamiltonian and OS.pauli_terms is O.pauli_terms      # the existing parsing, not a copy


def _handle(model, units, N=6):
    """passes observables._native without a library or a device; every library call raises"""
    from rnnwavefunctions_amd import _lib

    class NoLibrary(_lib.NativeWavefunction):
        def __init__(self):
            self.model, self.N, self.nx, self.ny, self.units, self.calls = model, N, N, 1, tuple(units), []

        def __del__(self):
            pass

        def __getattribute__(self, name):
            if name in ("pauli_step_stack", "pauli_train_steps_stack", "set_params", "adam_set_state", "get_params_dict", "lib", "h"):
                raise AssertionError("the library was touched: %s" % name)
            return object.__getattribute__(self, name)
    return NoLibrary()


def test_refusals_fire_before_any_library_call():
    from rnnwavefunctions_amd import _lib
    ham = O.xxz_hamiltonian(6, -1.0, 0.5)
    prm = P.init_gru_params([8, 8], seed=3)
    calls = [lambda w: OS.pauli_expectations(w, ["XXIIII"], 10), lambda w: OS.energy(w, ham, 10), lambda w: OS.correlations(w, 10),
             lambda w: OS.minimize_hamiltonian(w, ham, prm, numsteps=1, numsamples=10),
             lambda w: OS.minimize_hamiltonian(w, ham, prm, numsteps=1, numsamples=10, device_steps=2)]
    # a one-layer handle, with the pointer to the module that serves it
    for model in (_lib.MODEL_GRU1D, _lib.MODEL_GRU1D_F64):
        for call in calls:
            with pytest.raises(ValueError, match="one layer; observables.py"):
                call(_handle(model, (10,)))
    # every other model, stacked or not
    for model in (_lib.MODEL_GRU1D_PARITY, _lib.MODEL_CRNN_U1, _lib.MODEL_MDRNN2D, _lib.MODEL_LSTM1D_F64):
        for call in calls:
            with pytest.raises(ValueError, match="positive GRU models"):
                call(_handle(model, (10, 10)))
    with pytest.raises(TypeError):
        OS.energy(object(), ham, 10)
    # a stack, but: a communicator, a Hamiltonian of another size, opt= with device_steps, a bad device_steps, a pair (k, k)
    stack = lambda N=6: _handle(_lib.MODEL_GRU1D, (8, 8), N)
    for ds in (None, 4):
        with pytest.raises(ValueError, match="communicator"):
            OS.minimize_hamiltonian(stack(), ham, prm, numsteps=1, numsamples=10, comm=object(), device_steps=ds)
        with pytest.raises(ValueError, match="6 sites, the wave function 5"):
            OS.minimize_hamiltonian(stack(5), ham, prm, numsteps=1, numsamples=10, device_steps=ds)
    with pytest.raises(ValueError, match="6 sites, the wave function 5"):
        OS.energy(stack(5), ham, 10)
    with pytest.raises(ValueError, match="custom optimizer"):
        OS.minimize_hamiltonian(stack(), ham, prm, numsteps=1, numsamples=10, opt=T.Adam(), device_steps=2)
    for bad in (0, -3, 2.5, "4", True):
        with pytest.raises(ValueError, match="device_steps"):
            OS.minimize_hamiltonian(stack(), ham, prm, numsteps=1, numsamples=10, device_steps=bad)
    with pytest.raises(ValueError, match="distinct sites"):
        OS.correlations(stack(), 10, pairs=[(2, 2)])
    with pytest.raises(ValueError, match="one letter per site"):
        OS.pauli_expectations(stack(), ["XX"], 10)


class _Fake:
    """what observables_stack.minimize_hamiltonian needs of a NativeWavefunction on the device_steps path; records its calls"""

    def __init__(self, N=6):
        self.N, self.calls, self.adam = N, [], None

    def set_params(self, params, scope=None):
        self.calls.append(("set_params", scope))

    def adam_set_state(self, m, v, t):
        self.adam = (m, v, t)

    def pauli_train_steps_stack(self, flip, sign, coeff, numsamples, seed, step0, learning_rates):
        K = len(learning_rates)
        self.calls.append((K, numsamples, seed, step0, tuple(learning_rates)))
        k = np.arange(step0, step0 + K, dtype=np.float64)
        return np.stack([-(k + 1.0) * numsamples, (k + 1.0) ** 2 * numsamples + k, np.full(K, float(numsamples)), 0.0 * k], axis=1)

    def pauli_step_stack(self, *a, **k):
        raise AssertionError("the host loop ran")

    def get_params_dict(self, like, scope=None):
        return {k: v + 1 for k, v in like.items()}


def test_device_steps_runs_numsteps_plus_one_iterations_in_chunks(monkeypatch):
    monkeypatch.setattr(OS, "_native_stack", lambda wf: wf)
    prm = P.init_gru_params([8, 8], seed=3)
    ham = O.xxz_hamiltonian(6, -1.0, 0.5)
    wf = _Fake()
    mean, var = OS.minimize_hamiltonian(wf, ham, prm, numsteps=6, numsamples=10, learningrate=2e-2, seed=5, device_steps=3)
    assert wf.calls == [("set_params", SCOPE), (3, 10, 5, 0, (2e-2,) * 3), (3, 10, 5, 3, (2e-2,) * 3), (1, 10, 5, 6, (2e-2,))]
    assert wf.adam == (None, None, 0) and len(mean) == len(var) == 7
    assert np.array_equal(mean, -(np.arange(7) + 1.0)) and np.allclose(var, np.arange(7) / 10.0, rtol=0, atol=1e-12)
    assert all(np.array_equal(OS.minimize_hamiltonian.last_params[k], prm[k] + 1) for k in prm)
