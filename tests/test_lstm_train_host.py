"""CPU tests of the host side of the LSTM's device-resident training (rnnwf_lstm_train_steps, rnnwf_lstm_pauli_train_steps;
docs/lstm.md, "Device-resident training"): header, prototypes and methods agree; training_lstm validates device_steps before it touches
the library; on_gradient is refused with device_steps; the blocks of the device loop end where the saver acts.  No device: the wave
functions are stand-ins whose every library call raises."""
import inspect
import os
import re

import numpy as np
import pytest

from rnnwavefunctions_amd import _lib as _LIB
from rnnwavefunctions_amd import observables as O
from rnnwavefunctions_amd import params as P
from rnnwavefunctions_amd import training as T
from rnnwavefunctions_amd import training_lstm as TL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCOPE = "RNNwavefunction"
BAD_DEVICE_STEPS = (0, -3, 2.5, "4", True)
NATIVE = _LIB.NativeWavefunction           # the class itself: the no_library fixture replaces the module's name


def test_header_prototypes_and_methods_agree():
    from rnnwavefunctions_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rnnwf.h")).read(), flags=re.S)
    assert re.search(r"#define\s+RNNWF_ABI_VERSION\s+1\b", header) and _lib.ABI_VERSION == 1
    for new, old in (("rnnwf_lstm_train_steps", "rnnwf_train_steps"), ("rnnwf_lstm_pauli_train_steps", "rnnwf_pauli_train_steps")):
        decl = {name: re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, header) for name in (new, old)}
        assert all(decl.values()), new
        args, args_old = ([" ".join(a.split()) for a in m.group(1).split(",")] for m in decl.values())
        assert args == args_old, new                                          # the argument list of the entry it mirrors
        assert new in _lib.PROTOTYPES and _lib.PROTOTYPES[new] is _lib.PROTOTYPES[old]
        assert len(_lib.PROTOTYPES[new][1]) == len(args)
    W = _lib.NativeWavefunction
    for new, old in (("lstm_train_steps", "train_steps"), ("lstm_pauli_train_steps", "pauli_train_steps")):
        a, b = inspect.signature(getattr(W, new)).parameters, inspect.signature(getattr(W, old)).parameters
        assert list(a) == list(b) and [v.default for v in a.values()] == [v.default for v in b.values()], new


def test_the_built_library_exports_the_entries():
    import ctypes
    from rnnwavefunctions_amd import build
    lib = ctypes.CDLL(build.build())
    assert hasattr(lib, "rnnwf_lstm_train_steps") and hasattr(lib, "rnnwf_lstm_pauli_train_steps")
    assert lib.rnnwf_abi_version() == 1


def test_module_interface():
    for name in TL.DEVICE_API:
        assert callable(getattr(TL, name)), name
    assert "minimize_hamiltonian_device" in TL.DEVICE_API
    for fn in (TL.lstm_training_loop, TL.run_2DTFIM_1DRNN_LSTM):
        p = inspect.signature(fn).parameters
        assert "device_steps" in p and p["device_steps"].default is None
    from rnnwavefunctions_amd import observables_lstm as OL
    a, b = inspect.signature(TL.minimize_hamiltonian_device).parameters, inspect.signature(OL.minimize_hamiltonian).parameters
    assert list(a) == list(b)


def _handle(model, units, N=6):
    """passes observables._native without a library or a device; every library call raises (tests/test_lstm_pauli_host.py)"""
    class NoLibrary(NATIVE):
        def __init__(self):
            self.model, self.N, self.nx, self.ny, self.units = model, N, N, 1, tuple(units)

        def __del__(self):
            pass

        def __getattribute__(self, name):
            if name in ("lstm_train_steps", "lstm_pauli_train_steps", "lstm_pauli_gradient_step", "lstm_vmc_gradient_step", "set_params",
                        "adam_set_state", "adam_get_state", "get_params_dict", "lib", "h"):
                raise AssertionError("the library was touched: %s" % name)
            return object.__getattribute__(self, name)
    return NoLibrary()


@pytest.fixture
def no_library(monkeypatch):
    """creating a NativeWavefunction or loading the library fails the test"""
    from rnnwavefunctions_amd import _lib

    def touched(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "NativeWavefunction", touched)
    monkeypatch.setattr(_lib, "load_library", touched)


@pytest.mark.parametrize("bad", BAD_DEVICE_STEPS, ids=repr)
def test_bad_device_steps_are_refused_before_the_library_is_touched(bad, no_library):
    from rnnwavefunctions_amd import _lib
    with pytest.raises(ValueError, match="device_steps"):
        TL.run_2DTFIM_1DRNN_LSTM(numsteps=2, systemsize_x=3, systemsize_y=2, num_units=8, numsamples=10, verbose=False, device_steps=bad)
    ham = O.xxz_hamiltonian(6, -1.0, 0.5)
    prm = P.init_lstm_params([8], seed=3)
    with pytest.raises(ValueError, match="device_steps"):
        TL.minimize_hamiltonian_device(_handle(_lib.MODEL_LSTM1D_F64, (8,)), ham, prm, numsteps=1, numsamples=10, device_steps=bad)
    with pytest.raises(ValueError, match="device_steps"):
        TL.lstm_training_loop(_handle(_lib.MODEL_LSTM1D_F64, (8,)), prm, SCOPE, np.ones(7), 1, 10, 1, 1e-2, lambda lr, it: lr, T.Adam(),
                              device_steps=bad)


def test_minimize_hamiltonian_device_refusals_fire_before_any_library_call():
    from rnnwavefunctions_amd import _lib
    ham = O.xxz_hamiltonian(6, -1.0, 0.5)
    prm = P.init_lstm_params([8], seed=3)
    lstm = lambda N=6: _handle(_lib.MODEL_LSTM1D_F64, (8,), N)
    with pytest.raises(ValueError, match="device_steps"):
        TL.minimize_hamiltonian_device(lstm(), ham, prm, numsteps=1, numsamples=10, device_steps=None)
    with pytest.raises(ValueError, match="observables_lstm serves the LSTM wave function"):
        TL.minimize_hamiltonian_device(_handle(_lib.MODEL_GRU1D_F64, (8,)), ham, prm, numsteps=1, numsamples=10, device_steps=2)
    with pytest.raises(ValueError, match="communicator"):
        TL.minimize_hamiltonian_device(lstm(), ham, prm, numsteps=1, numsamples=10, device_steps=2, comm=object())
    with pytest.raises(ValueError, match="6 sites, the wave function 5"):
        TL.minimize_hamiltonian_device(lstm(5), ham, prm, numsteps=1, numsamples=10, device_steps=2)

    class Sgd:
        pass
    with pytest.raises(ValueError, match="custom optimizer"):
        TL.minimize_hamiltonian_device(lstm(), ham, prm, numsteps=1, numsamples=10, device_steps=2, opt=Sgd())


def test_on_gradient_with_device_steps_raises():
    from rnnwavefunctions_amd import _lib
    prm = P.init_lstm_params([8], seed=3)
    with pytest.raises(ValueError, match="on_gradient"):
        TL.lstm_training_loop(_handle(_lib.MODEL_LSTM1D_F64, (8,)), prm, SCOPE, np.ones(7), 1, 10, 1, 1e-2, lambda lr, it: lr, T.Adam(),
                              on_gradient=lambda it, params, out: None, device_steps=3)
    assert TL.check_device_steps(None, on_gradient=lambda *a: None) is None        # the host loop keeps it
    assert TL.check_device_steps(np.int64(7)) == 7 and type(TL.check_device_steps(np.int64(7))) is int


@pytest.mark.parametrize("numsteps", [0, 1, 9, 10, 12, 499, 500, 501, 1003, 2600])
@pytest.mark.parametrize("device_steps", [1, 3, 5, 10, 50, 1024, 5000])
def test_blocks_end_where_the_saver_acts(numsteps, device_steps):
    blocks = TL.device_blocks(numsteps, device_steps)
    assert sum(K for _, K in blocks) == numsteps + 1
    assert blocks[0][0] == 0
    for (it, K), nxt in zip(blocks, blocks[1:] + [(numsteps + 1, 0)]):
        assert 1 <= K <= min(device_steps, 1024)
        assert it + K == nxt[0]                                               # contiguous, in order
        inside = range(it + 1, it + K)                                        # iterations of the block other than its first
        assert not any(j % 10 == 0 for j in inside), (it, K)                  # energies every 10, the model every 500 = 50 x 10
        assert not any(j % 500 == 0 for j in inside), (it, K)


def test_the_device_loop_shows_the_saver_what_the_host_loop_shows():
    """a stand-in device: Adam on the host behind lstm_train_steps' interface.  The saver's calls - iteration, histories, parameters and
    optimizer state at the multiples of 500 - are the host loop's"""
    prm0 = P.init_lstm_params([4], seed=3)
    lay = [(k[len(SCOPE) + 1:], v.size) for k, v in sorted(prm0.items())]

    def grads_of(params, it):
        return {k: np.cos(v * (it + 1.0)) for k, v in params.items()}

    def moments_of(it):
        return np.array([-(it + 1.0) * 10, (it + 1.0) ** 2 * 10 + it, 10.0, 0.0])

    class Host:
        def lstm_vmc_gradient_step(self, numsamples, seed, step, couplings, shapes, want_samples=False, want_eloc=False):
            return {"moments": moments_of(step), "grads": {k[len(SCOPE) + 1:]: g for k, g in grads_of(self.params, step).items()}}

        def set_params(self, params, scope=None):
            self.params = {k: v.copy() for k, v in params.items()}

    class Device(Host):
        def _layout(self):
            return lay

        def adam_set_state(self, m, v, t):
            self.opt = T.Adam()
            if m is not None:
                self.opt.from_flat(self, self.params, SCOPE, m, v, t)
            self.opt.t = t

        def adam_get_state(self):
            m, v = self.opt.to_flat(self, self.params, SCOPE)
            return m, v, self.opt.t

        def get_params_dict(self, like, scope=None):
            return {k: self.params[k].copy() for k in like}

        def lstm_train_steps(self, numsamples, seed, step0, couplings, learning_rates, beta1, beta2, epsilon):
            mom = []
            for k, lr in enumerate(learning_rates):
                mom.append(moments_of(step0 + k))
                self.params = self.opt.step(self.params, grads_of(self.params, step0 + k), lr)
            return np.array(mom)

    def run(wf, device_steps):
        seen = []

        def on_step(it, meanE, varE, params, opt):
            if it % 500 == 0:
                seen.append((it, list(meanE), list(varE), {k: v.copy() for k, v in params.items()}, opt.t, opt.to_flat(Device(), params, SCOPE)))
            elif it % 10 == 0:
                seen.append((it, list(meanE), list(varE)))
        wf.set_params(prm0)
        out = TL.lstm_training_loop(wf, {k: v.copy() for k, v in prm0.items()}, SCOPE, np.ones(5), 1013, 10, 1, np.float64(1e-2),
                                    lambda lr0, it: 1.0 / ((1.0 / lr0) + it / 10), T.Adam(), on_step=on_step, device_steps=device_steps)
        return seen, out
    host, (mh, vh, ph) = run(Host(), None)
    dev, (md, vd, pd) = run(Device(), 7)
    assert mh == md and vh == vd and all(np.array_equal(ph[k], pd[k]) for k in ph)
    assert len(host) == len(dev) == 102
    for a, b in zip(host, dev):
        assert a[:3] == b[:3]
        if a[0] % 500 == 0:
            assert all(np.array_equal(a[3][k], b[3][k]) for k in a[3]) and a[4] == b[4], a[0]
            assert np.array_equal(a[5][0], b[5][0]) and np.array_equal(a[5][1], b[5][1]), a[0]
