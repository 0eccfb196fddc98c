"""CPU tests of the host side of the device solve of stochastic reconfiguration (docs/sr.md, "Solve on the device"): the header, the
ctypes prototypes and the NativeWavefunction methods agree, the block width the GPU tests import mirrors the kernels', and
sr.minsr_direction / sr.train_tfim route `solver` as documented.  No device: the wave function is a fake built on the reference
Jacobian, like the one of tests/test_sr_reference.py."""
import os
import re

import numpy as np
import pytest

import autograd_reference as A
import sr_reference as R
from rnnwavefunctions_amd import params as P
from rnnwavefunctions_amd import sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def case():
    N, H, ns = 6, 7, 19
    rng = np.random.RandomState(5)
    prm = P.randomize_biases(P.scale_kernels(P.init_gru_params([H], seed=3, dtype=np.float64), 2.0), 4)
    s = rng.randint(0, 2, size=(ns, N)).astype(np.int32)
    e = rng.standard_normal(ns)
    return prm, s, e, R.jacobian(prm, s)


class _Fake:
    """what sr.py needs of a NativeWavefunction, computed from the reference Jacobian: no device.  Counts its calls."""

    def __init__(self, prm, o, e):
        self.N, self.o, self.e, self.prm = 6, o, e, prm
        self.calls = {"sr_gram": 0, "sr_apply": 0, "sr_direction": 0}
        self.shifts = []

    def _layout(self):
        return [(k[len(A.SCOPE) + 1:], int(self.prm[k].size)) for k in R.names(self.prm)]

    def sr_gram(self):
        self.calls["sr_gram"] += 1
        return R.gram(self.o), R.epsilon(self.e)

    def sr_apply(self, y):
        self.calls["sr_apply"] += 1
        return R.centred(self.o).T @ y

    def sr_direction(self, diag_shift):
        self.calls["sr_direction"] += 1
        self.shifts.append(diag_shift)
        return R.minsr_direction(self.o, self.e, diag_shift)

    # train_tfim: a fixed batch whatever the parameters
    def set_params_flat(self, flat):
        self.flat = np.array(flat)

    def vmc_step(self, ns, seed, it, couplings):
        return {"moments": (float(self.e.sum()), float((self.e ** 2).sum()), float(len(self.e)), 0.0)}


def test_header_prototypes_and_methods_agree():
    from rnnwavefunctions_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rnnwf.h")).read(), flags=re.S)
    for name in ("rnnwf_sr_solve", "rnnwf_sr_direction"):
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, header)
        assert m and len(m.group(1).split(",")) == 3 == len(_lib.PROTOTYPES[name][1]), name
        assert "double diag_shift" in m.group(1)
    assert re.search(r"RNNWF_ERR_NUMERIC\s*=\s*-6\b", header)
    for m in ("sr_solve", "sr_direction"):
        assert callable(getattr(_lib.NativeWavefunction, m))


def test_block_width_mirrors_the_kernels():
    from rnnwavefunctions_amd import _lib
    src = open(os.path.join(ROOT, "rnnwavefunctions_amd", "csrc", "sr_solve_kernels.h")).read()
    m = re.search(r"constexpr\s+int\s+kSrNB\s*=\s*(\d+)\s*;", src)
    assert m and int(m.group(1)) == _lib.SR_BLOCK


def test_solver_is_validated(case):
    prm, s, e, o = case
    wf = _Fake(prm, o, e)
    for bad in ("gpu", "", None, "Device"):
        with pytest.raises(ValueError, match="solver"):
            sr.minsr_direction(wf, 1e-2, solver=bad)
        with pytest.raises(ValueError, match="solver"):
            sr.train_tfim(wf, np.ones(6), 1.0, prm, 1, 10, 1e-2, 1e-3, 1, solver=bad)
    assert not any(wf.calls.values())
    for bad in (0.0, -1e-3, np.inf, np.nan):
        with pytest.raises(ValueError, match="diag_shift"):
            sr.minsr_direction(wf, bad, solver="device")
    assert not any(wf.calls.values())


def test_device_solver_routes_to_sr_direction(case):
    prm, s, e, o = case
    wf = _Fake(prm, o, e)
    ref = R.minsr_direction(o, e, 1e-2)
    got = sr.minsr_direction(wf, 1e-2, solver="device")
    assert np.array_equal(got, ref)
    assert wf.calls == {"sr_gram": 0, "sr_apply": 0, "sr_direction": 1} and wf.shifts == [1e-2]


def test_host_solver_never_calls_sr_direction(case):
    prm, s, e, o = case
    wf = _Fake(prm, o, e)
    ref = R.minsr_direction(o, e, 1e-2)
    for got in (sr.minsr_direction(wf, 1e-2), sr.minsr_direction(wf, 1e-2, solver="host")):
        assert np.linalg.norm(got - ref) <= 1e-10 * np.linalg.norm(ref)
    assert wf.calls == {"sr_gram": 2, "sr_apply": 2, "sr_direction": 0}


def test_train_tfim_passes_the_solver_on(case):
    prm, s, e, o = case
    dev, host = _Fake(prm, o, e), _Fake(prm, o, e)
    sr.train_tfim(dev, np.ones(6), 1.0, prm, numsteps=2, numsamples=len(e), learningrate=1e-2, diag_shift=1e-2, seed=1, solver="device")
    sr.train_tfim(host, np.ones(6), 1.0, prm, numsteps=2, numsamples=len(e), learningrate=1e-2, diag_shift=1e-2, seed=1)
    assert dev.calls == {"sr_gram": 0, "sr_apply": 0, "sr_direction": 3}
    assert host.calls == {"sr_gram": 3, "sr_apply": 3, "sr_direction": 0}
    assert np.linalg.norm(dev.flat - host.flat) <= 1e-10 * np.linalg.norm(host.flat)
