"""The LSTM wave function's stochastic reconfiguration (docs/sr_lstm.md): header, library, binding and facade agree, and the
Python-side refusals hold.  No device."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIVE = (("rnnwf_log_derivatives_lstm", 4), ("rnnwf_sr_gram_lstm", 3), ("rnnwf_sr_apply_lstm", 3), ("rnnwf_sr_solve_lstm", 3),
        ("rnnwf_sr_direction_lstm", 3))
ENTRIES = FIVE + (("rnnwf_lstm_load_batch", 4), ("rnnwf_sr_step_lstm", 11))


def header():
    return open(os.path.join(ROOT, "include", "rnnwf.h")).read()


def test_built_library_exports_the_seven_entries():
    from rnnwavefunctions_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, _ in ENTRIES:
        assert hasattr(lib, name), name


def test_header_declares_and_binding_binds_the_entries():
    from rnnwavefunctions_amd import _lib
    code = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    for name, nargs in ENTRIES:
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, code)
        assert m and len(m.group(1).split(",")) == nargs == len(_lib.PROTOTYPES[name][1]), name
    for name, _ in FIVE:
        assert _lib.PROTOTYPES[name] == _lib.PROTOTYPES[name[:-len("_lstm")]]      # the same signatures as the positive model's entries


def test_abi_version_stays_one():
    from rnnwavefunctions_amd import _lib
    assert re.search(r"#define RNNWF_ABI_VERSION 1\b", header()) and _lib.ABI_VERSION == 1


def test_facade_has_the_methods_and_functions():
    from rnnwavefunctions_amd import _lib, sr
    for m in ("log_derivatives_lstm", "sr_gram_lstm", "sr_apply_lstm", "sr_solve_lstm", "sr_direction_lstm", "lstm_load_batch", "sr_step_lstm"):
        assert callable(getattr(_lib.NativeWavefunction, m))
    for f in ("minsr_direction_lstm", "qgt_lstm", "train_tfim_lstm"):
        assert callable(getattr(sr, f))


def test_pinned_export_lists_are_unchanged():
    from rnnwavefunctions_amd import observables_lstm, training_lstm
    assert training_lstm.__all__ == ["run_2DTFIM_1DRNN_LSTM", "lstm_training_loop"]
    assert observables_lstm.__all__ == ["pauli_expectations", "energy", "correlations", "minimize_hamiltonian"]


class _Fake:
    """what sr.py needs of an LSTM NativeWavefunction, from a random Jacobian: no device"""

    def __init__(self, o, e):
        self.N, self.o, self.e = 6, o, e

    def _layout(self):
        return [("theta", self.o.shape[1])]

    def set_params_flat(self, flat):
        raise AssertionError("a refused call must not reach the handle")

    def log_derivatives_lstm(self):
        return self.o

    def sr_gram_lstm(self):
        d = self.o - self.o.mean(axis=0)
        return d @ d.T, self.e - self.e.mean()

    def sr_apply_lstm(self, y):
        return (self.o - self.o.mean(axis=0)).T @ y


@pytest.fixture(scope="module")
def fake():
    rng = np.random.RandomState(11)
    return _Fake(rng.standard_normal((19, 30)), rng.standard_normal(19))


def test_minsr_direction_and_qgt_through_the_facade(fake):
    from rnnwavefunctions_amd import sr
    d = fake.o - fake.o.mean(axis=0)
    ref = d.T @ np.linalg.solve(d @ d.T + 19 * 1e-2 * np.eye(19), fake.e - fake.e.mean())
    assert np.linalg.norm(sr.minsr_direction_lstm(fake, 1e-2) - ref) <= 1e-10 * np.linalg.norm(ref)
    assert np.allclose(sr.qgt_lstm(fake), d.T @ d / 19, rtol=0, atol=1e-15 * np.abs(d.T @ d).max())


def test_host_side_argument_refusals(fake):
    from rnnwavefunctions_amd import sr
    prm = {"RNNwavefunction/theta": np.zeros(30)}
    for bad in (0.0, -1e-3, np.inf, np.nan):
        with pytest.raises(ValueError, match="diag_shift"):
            sr.minsr_direction_lstm(fake, bad)
        with pytest.raises(ValueError, match="diag_shift"):
            sr.train_tfim_lstm(fake, 1.0, 3.0, prm, 1, 10, 1e-2, bad, 1)
    for solver in ("gpu", None):
        with pytest.raises(ValueError, match="solver"):
            sr.minsr_direction_lstm(fake, 1e-3, solver=solver)
        with pytest.raises(ValueError, match="solver"):
            sr.train_tfim_lstm(fake, 1.0, 3.0, prm, 1, 10, 1e-2, 1e-3, 1, solver=solver)
    with pytest.raises(ValueError, match="numsamples"):
        sr.train_tfim_lstm(fake, 1.0, 3.0, prm, 1, 1, 1e-2, 1e-3, 1)
    with pytest.raises(ValueError, match="numsteps"):
        sr.train_tfim_lstm(fake, 1.0, 3.0, prm, -1, 10, 1e-2, 1e-3, 1)
    with pytest.raises(ValueError, match="Jz"):
        sr.train_tfim_lstm(fake, np.ones(5), 3.0, prm, 1, 10, 1e-2, 1e-3, 1)
    with pytest.raises(TypeError):                      # whole iterations on the device are not offered for the LSTM
        sr.train_tfim_lstm(fake, 1.0, 3.0, prm, 1, 10, 1e-2, 1e-3, 1, device_steps=4)
