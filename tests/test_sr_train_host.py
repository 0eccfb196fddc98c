"""CPU tests of the host side of rnnwf_sr_train_steps (docs/sr.md, "Iterations on the device"): the header, the ctypes prototype and
the NativeWavefunction method agree, and sr.train_tfim validates device_steps before it touches the wave function and routes an
accepted value to sr_train_steps in chunks.  No device: the wave function is a fake that counts its calls."""
import os
import re

import numpy as np
import pytest

from rnnwavefunctions_amd import params as P
from rnnwavefunctions_amd import sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCOPE = "RNNwavefunction"


def test_header_prototype_and_method_agree():
    from rnnwavefunctions_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rnnwf.h")).read(), flags=re.S)
    m = re.search(r"\brnnwf_sr_train_steps\s*\(([^)]*)\)", header)
    assert m and "rnnwf_sr_train_steps" in _lib.PROTOTYPES
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 11 == len(_lib.PROTOTYPES["rnnwf_sr_train_steps"][1])
    assert args[8] == "const double* learning_rates" and args[9] == "const double* diag_shifts" and args[10] == "double* moments"
    assert callable(_lib.NativeWavefunction.sr_train_steps)
    assert _lib.ABI_VERSION == 1


def test_device_steps_is_validated_before_the_wave_function_is_touched():
    prm = P.init_gru_params([7], seed=3)
    for bad in (0, -3, 2.5, "4", True):
        with pytest.raises(ValueError, match="device_steps"):
            sr.train_tfim(object(), np.ones(6), 1.0, prm, 1, 10, 1e-2, 1e-3, 1, device_steps=bad)


class _Fake:
    """what the device_steps path of sr.train_tfim needs of a NativeWavefunction; records its calls"""

    def __init__(self, prm):
        self.N, self.prm, self.calls = 6, prm, []

    def _layout(self):
        return [(k[len(SCOPE) + 1:], int(self.prm[k].size)) for k in sorted(self.prm)]

    def set_params_flat(self, flat):
        self.flat = np.array(flat)

    def sr_train_steps(self, K, numsamples, seed, step0, couplings, learning_rates, diag_shifts, sample_offset=0):
        self.calls.append((K, numsamples, seed, step0, learning_rates, diag_shifts, sample_offset))
        k = np.arange(step0, step0 + K, dtype=np.float64)
        return np.stack([-(k + 1.0) * numsamples, (k + 1.0) ** 2 * numsamples + k, np.full(K, float(numsamples)), np.zeros(K)], axis=1)

    def get_params_dict(self, like, scope=None):
        return {k: v.copy() for k, v in like.items()}


def test_device_steps_runs_numsteps_plus_one_iterations_in_chunks():
    prm = P.init_gru_params([7], seed=3)
    wf = _Fake(prm)
    mean, var = sr.train_tfim(wf, np.ones(6), 1.0, prm, numsteps=6, numsamples=10, learningrate=2e-2, diag_shift=3e-3, seed=5, solver="host",
                              device_steps=3)
    assert wf.calls == [(3, 10, 5, 0, 2e-2, 3e-3, 0), (3, 10, 5, 3, 2e-2, 3e-3, 0), (1, 10, 5, 6, 2e-2, 3e-3, 0)]
    assert wf.flat.shape == (sum(v.size for v in prm.values()),)
    assert np.array_equal(mean, -(np.arange(7) + 1.0)) and np.allclose(var, np.arange(7) / 10.0, rtol=0, atol=1e-12)
    assert sr.train_tfim.last_params.keys() == prm.keys()
