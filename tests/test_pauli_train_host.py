"""CPU tests of the host side of rnnwf_pauli_train_steps / rnnwf_pauli_train_steps_complex (docs/pauli_train.md): the header, the
ctypes prototypes and the NativeWavefunction methods agree, and the two minimize_hamiltonian drivers validate device_steps before they
touch the wave function and route an accepted value to the device entry in chunks.  No device: the wave function is a fake that
counts its calls."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from rnnwavefunctions_amd import observables as O
from rnnwavefunctions_amd import observables_complex as OC
from rnnwavefunctions_amd import params as P
from rnnwavefunctions_amd import training as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCOPE = "RNNwavefunction"
ENTRIES = ("rnnwf_pauli_train_steps", "rnnwf_pauli_train_steps_complex")


def test_header_prototypes_exports_and_methods_agree():
    from rnnwavefunctions_amd import _lib, build
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rnnwf.h")).read(), flags=re.S)
    lib = ctypes.CDLL(build.build())
    for name in ENTRIES:
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, header)
        assert m and name in _lib.PROTOTYPES
        args = [a.strip() for a in m.group(1).split(",")]
        assert len(args) == 17 == len(_lib.PROTOTYPES[name][1])
        assert args[5] == "int32_t K" and args[10] == "const double* learning_rates" and args[14] == "double* moments"
        assert args[15] == "double* term_sums"
        assert hasattr(lib, name)
    assert _lib.ABI_VERSION == 1 and _lib.load_library().rnnwf_abi_version() == 1
    for meth in (_lib.NativeWavefunction.pauli_train_steps, _lib.NativeWavefunction.pauli_train_steps_complex):
        p = inspect.signature(meth).parameters
        assert list(p)[1:8] == ["flip", "sign", "coeff", "numsamples", "seed", "step0", "learning_rates"]
        assert (p["beta1"].default, p["beta2"].default, p["epsilon"].default) == (0.9, 0.999, 1e-8)
        assert p["sample_offset"].default == 0 and p["want_term_sums"].default is False


class _Fake:
    """what the device_steps path of the minimize_hamiltonian drivers needs of a NativeWavefunction; records its calls"""
    model = None

    def __init__(self, prm, N=6):
        self.N, self.prm, self.calls, self.adam = N, prm, [], None

    def set_params(self, params, scope=None):
        self.calls.append(("set_params", scope))

    def adam_set_state(self, m, v, t):
        self.adam = (m, v, t)

    def _steps(self, flip, sign, coeff, numsamples, seed, step0, learning_rates):
        K = len(learning_rates)
        self.calls.append((K, numsamples, seed, step0, tuple(learning_rates)))
        k = np.arange(step0, step0 + K, dtype=np.float64)
        return np.stack([-(k + 1.0) * numsamples, (k + 1.0) ** 2 * numsamples + k, np.full(K, float(numsamples)), 0.5 * k], axis=1)

    pauli_train_steps = pauli_train_steps_complex = _steps

    def pauli_step(self, *a, **k):
        raise AssertionError("the host loop ran")

    pauli_step_complex = pauli_step

    def get_params_dict(self, like, scope=None):
        return {k: v + 1 for k, v in like.items()}


def test_both_drivers_accept_device_steps_and_keep_their_refusals():
    prm = P.init_gru_params([7], seed=3)
    ham = O.xxz_hamiltonian(6, -1.0, 0.5)
    assert inspect.signature(T.minimize_hamiltonian).parameters["device_steps"].default is None
    assert inspect.signature(OC.minimize_hamiltonian).parameters["device_steps"].default is None
    for ds in (None, 4):
        with pytest.raises(ValueError, match="communicator"):
            T.minimize_hamiltonian(_Fake(prm), ham, prm, numsteps=1, numsamples=10, comm=object(), device_steps=ds)
        with pytest.raises(ValueError, match="6 sites, the wave function 5"):
            T.minimize_hamiltonian(_Fake(prm, N=5), ham, prm, numsteps=1, numsamples=10, device_steps=ds)
    for bad in (0, -3, 2.5, "4", True):
        with pytest.raises(ValueError, match="device_steps"):
            T.minimize_hamiltonian(_Fake(prm), ham, prm, numsteps=1, numsamples=10, device_steps=bad)
    with pytest.raises(ValueError, match="custom optimizer"):
        T.minimize_hamiltonian(_Fake(prm), ham, prm, numsteps=1, numsamples=10, opt=T.Adam(), device_steps=2)


def test_complex_driver_keeps_its_refusals(monkeypatch):
    prm = P.init_gru_params([7], seed=3, heads=("wf_dense_ampl", "wf_dense_phase"))
    ham = OC.j1j2_hamiltonian(np.ones(6), np.zeros(6), np.zeros(6))
    monkeypatch.setattr(OC, "_native_complex", lambda wf: wf)
    for ds in (None, 4):
        with pytest.raises(ValueError, match="6 sites, the wave function 5"):
            OC.minimize_hamiltonian(_Fake(prm, N=5), ham, 10, 1, 1e-2, params=prm, device_steps=ds)
        with pytest.raises(ValueError, match="needs its parameters"):
            OC.minimize_hamiltonian(_Fake(prm), ham, 10, 1, 1e-2, device_steps=ds)
    with pytest.raises(ValueError, match="device_steps"):
        OC.minimize_hamiltonian(_Fake(prm), ham, 10, 1, 1e-2, params=prm, device_steps=0)
    with pytest.raises(ValueError, match="custom optimizer"):
        OC.minimize_hamiltonian(_Fake(prm), ham, 10, 1, 1e-2, params=prm, opt=T.Adam(), device_steps=2)


def test_device_steps_runs_numsteps_plus_one_iterations_in_chunks(monkeypatch):
    prm = P.init_gru_params([7], seed=3)
    ham = O.xxz_hamiltonian(6, -1.0, 0.5)
    wf = _Fake(prm)
    mean, var = T.minimize_hamiltonian(wf, ham, prm, numsteps=6, numsamples=10, learningrate=2e-2, seed=5, device_steps=3)
    assert wf.calls == [("set_params", SCOPE), (3, 10, 5, 0, (2e-2,) * 3), (3, 10, 5, 3, (2e-2,) * 3), (1, 10, 5, 6, (2e-2,))]
    assert wf.adam == (None, None, 0)
    assert np.array_equal(mean, -(np.arange(7) + 1.0)) and np.allclose(var, np.arange(7) / 10.0, rtol=0, atol=1e-12)
    assert all(np.array_equal(T.minimize_hamiltonian.last_params[k], prm[k] + 1) for k in prm)
    # the complex driver: complex means from the fourth moment, the same chunks
    monkeypatch.setattr(OC, "_native_complex", lambda w: w)
    wf = _Fake(prm)
    cham = OC.j1j2_hamiltonian(np.ones(6), np.zeros(6), np.zeros(6))
    mean, var = OC.minimize_hamiltonian(wf, cham, 10, 4, 1e-2, params=prm, seed=5, device_steps=2)
    assert [c[:4] for c in wf.calls[1:]] == [(2, 10, 5, 0), (2, 10, 5, 2), (1, 10, 5, 4)]
    assert mean == [complex(-(k + 1.0), 0.5 * k / 10.0) for k in range(5)] and len(var) == 5
    assert all(np.array_equal(OC.minimize_hamiltonian.last_params[k], prm[k] + 1) for k in prm)
