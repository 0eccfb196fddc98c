"""CPU tests of the host side of rnnwf_pauli_train_steps_2d (docs/pauli_train.md, "2D RNN"): the header, the ctypes prototype and the
NativeWavefunction method agree, and observables_2d.minimize_hamiltonian validates its arguments before it touches the wave function
and routes device_steps to the device entry in chunks.  No device: the wave function is a fake that records its calls."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from rnnwavefunctions_amd import observables_2d as O2
from rnnwavefunctions_amd import params as P
from rnnwavefunctions_amd import training as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCOPE = "RNNwavefunction"
ENTRY = "rnnwf_pauli_train_steps_2d"


def test_header_prototype_export_and_method_agree():
    from rnnwavefunctions_amd import _lib, build
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rnnwf.h")).read(), flags=re.S)
    decl = {name: re.search(r"\b%s\s*\(([^)]*)\)" % name, header) for name in (ENTRY, "rnnwf_pauli_train_steps")}
    assert all(decl.values())
    args, args_1d = ([" ".join(a.split()) for a in m.group(1).split(",")] for m in decl.values())
    assert len(args) == 17 and args == args_1d                                 # the argument list is rnnwf_pauli_train_steps's
    assert _lib.PROTOTYPES[ENTRY] is _lib.PROTOTYPES["rnnwf_pauli_train_steps"]  # one object, not a copy
    assert hasattr(ctypes.CDLL(build.build()), ENTRY)
    assert _lib.ABI_VERSION == 1 and _lib.load_library().rnnwf_abi_version() == 1
    assert "mdrnn_pauli.hip" in build.SOURCES and build.compile_flags("mdrnn_pauli.hip") == build.compile_flags("mdrnn.hip")
    p, p_1d = (inspect.signature(m).parameters for m in (_lib.NativeWavefunction.pauli_train_steps_2d, _lib.NativeWavefunction.pauli_train_steps))
    assert list(p) == list(p_1d) and [v.default for v in p.values()] == [v.default for v in p_1d.values()]


class _Fake:
    """what observables_2d.minimize_hamiltonian needs of a NativeWavefunction on the device_steps path; records its calls"""

    def __init__(self, prm, N=6):
        self.N, self.prm, self.calls, self.adam = N, prm, [], None

    def set_params(self, params, scope=None):
        self.calls.append(("set_params", scope))

    def adam_set_state(self, m, v, t):
        self.adam = (m, v, t)

    def pauli_train_steps_2d(self, flip, sign, coeff, numsamples, seed, step0, learning_rates):
        K = len(learning_rates)
        self.calls.append((K, numsamples, seed, step0, tuple(learning_rates)))
        k = np.arange(step0, step0 + K, dtype=np.float64)
        return np.stack([-(k + 1.0) * numsamples, (k + 1.0) ** 2 * numsamples + k, np.full(K, float(numsamples)), 0.5 * k], axis=1)

    def pauli_step_2d(self, *a, **k):
        raise AssertionError("the host loop ran")

    def get_params_dict(self, like, scope=None):
        return {k: v + 1 for k, v in like.items()}


def test_validation_happens_before_the_wave_function_is_touched(monkeypatch):
    prm = P.init_mdrnn_params(7, seed=3)
    ham = O2.xxz_hamiltonian_2d(3, 2, -1.0, 0.5)
    sig = inspect.signature(O2.minimize_hamiltonian).parameters
    assert list(sig) == list(inspect.signature(T.minimize_hamiltonian).parameters)
    assert [v.default for v in sig.values()] == [v.default for v in inspect.signature(T.minimize_hamiltonian).parameters.values()]
    assert "minimize_hamiltonian" in O2.__all__
    # every model but the 2D RNN, and what is no wave function at all
    with pytest.raises((TypeError, ValueError)):
        O2.minimize_hamiltonian(_Fake(prm), ham, prm, numsteps=1, numsamples=10)
    monkeypatch.setattr(O2, "_native_2d", lambda wf: wf)
    fakes = []

    def fake(**kw):
        fakes.append(_Fake(prm, **kw))
        return fakes[-1]
    for ds in (None, 4):
        with pytest.raises(ValueError, match="communicator"):
            O2.minimize_hamiltonian(fake(), ham, prm, numsteps=1, numsamples=10, comm=object(), device_steps=ds)
        with pytest.raises(ValueError, match="6 sites, the wave function 5"):
            O2.minimize_hamiltonian(fake(N=5), ham, prm, numsteps=1, numsamples=10, device_steps=ds)
    for bad in (0, -3, 2.5, "4", True):
        with pytest.raises(ValueError, match="device_steps"):
            O2.minimize_hamiltonian(fake(), ham, prm, numsteps=1, numsamples=10, device_steps=bad)
    with pytest.raises(ValueError, match="custom optimizer"):
        O2.minimize_hamiltonian(fake(), ham, prm, numsteps=1, numsamples=10, opt=T.Adam(), device_steps=2)
    assert len(fakes) == 10 and all(f.calls == [] and f.adam is None for f in fakes)


def test_refuses_every_model_but_the_2d_rnn():
    from rnnwavefunctions_amd import _lib

    class NotMd(_lib.NativeWavefunction):                  # passes observables._native without a library or a device
        def __init__(self, model):
            self.model, self.N = model, 6

        def __del__(self):
            pass
    ham = O2.xxz_hamiltonian_2d(3, 2, -1.0, 0.5)
    for model in (_lib.MODEL_GRU1D, _lib.MODEL_GRU1D_F64, _lib.MODEL_CRNN_U1):
        for ds in (None, 4):
            with pytest.raises(ValueError, match="2D RNN"):
                O2.minimize_hamiltonian(NotMd(model), ham, {}, numsteps=1, numsamples=10, device_steps=ds)


def test_device_steps_runs_numsteps_plus_one_iterations_in_chunks(monkeypatch):
    monkeypatch.setattr(O2, "_native_2d", lambda wf: wf)
    prm = P.init_mdrnn_params(7, seed=3)
    ham = O2.xxz_hamiltonian_2d(3, 2, -1.0, 0.5)
    wf = _Fake(prm)
    mean, var = O2.minimize_hamiltonian(wf, ham, prm, numsteps=6, numsamples=10, learningrate=2e-2, seed=5, device_steps=3)
    assert wf.calls == [("set_params", SCOPE), (3, 10, 5, 0, (2e-2,) * 3), (3, 10, 5, 3, (2e-2,) * 3), (1, 10, 5, 6, (2e-2,))]
    assert wf.adam == (None, None, 0)
    assert len(mean) == len(var) == 7
    assert np.array_equal(mean, -(np.arange(7) + 1.0)) and np.allclose(var, np.arange(7) / 10.0, rtol=0, atol=1e-12)
    assert all(np.array_equal(O2.minimize_hamiltonian.last_params[k], prm[k] + 1) for k in prm)
    # a chunk is at most one call's 1024 iterations, whatever device_steps asks for
    wf = _Fake(prm)
    mean, _ = O2.minimize_hamiltonian(wf, ham, prm, numsteps=1030, numsamples=10, device_steps=5000)
    assert [c[:4] for c in wf.calls[1:]] == [(1024, 10, 111, 0), (7, 10, 111, 1024)] and len(mean) == 1031
