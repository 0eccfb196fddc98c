"""CPU tests of the host side of rnnwf_pauli_step_lstm / rnnwf_lstm_pauli_gradient_step (docs/pauli_lstm.md): header, prototypes and
methods agree; observables_lstm validates its arguments before it touches the wave function; and, on the float64 reference alone, the
1e-11 N bound of tests/test_gpu_lstm_pauli.py rejects three defects of the kernels' bookkeeping on that test's own shapes.  No device:
the wave functions are fakes."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import lstm_pauli_reference as Q
import pauli_reference as PR
from rnnwavefunctions_amd import observables as O
from rnnwavefunctions_amd import observables_lstm as OL
from rnnwavefunctions_amd import observables_stack as OS
from rnnwavefunctions_amd import params as P
from rnnwavefunctions_amd import training as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCOPE = "RNNwavefunction"


def test_header_prototypes_exports_and_methods_agree():
    from rnnwavefunctions_amd import _lib, build
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rnnwf.h")).read(), flags=re.S)
    assert re.search(r"#define\s+RNNWF_ABI_VERSION\s+1\b", header)
    lib = ctypes.CDLL(build.build())
    decl = {name: re.search(r"\b%s\s*\(([^)]*)\)" % name, header) for name in ("rnnwf_pauli_step_lstm", "rnnwf_pauli_step")}
    assert all(decl.values())
    args, args_1 = ([" ".join(a.split()) for a in m.group(1).split(",")] for m in decl.values())
    assert len(args) == 15 and args == args_1                                  # rnnwf_pauli_step's argument list
    assert _lib.PROTOTYPES["rnnwf_pauli_step_lstm"] is _lib.PROTOTYPES["rnnwf_pauli_step"]
    grad = re.search(r"\brnnwf_lstm_pauli_gradient_step\s*\(([^)]*)\)", header)
    assert grad and len(grad.group(1).split(",")) == 13 == len(_lib.PROTOTYPES["rnnwf_lstm_pauli_gradient_step"][1])
    assert hasattr(lib, "rnnwf_pauli_step_lstm") and hasattr(lib, "rnnwf_lstm_pauli_gradient_step")
    assert _lib.ABI_VERSION == 1 and _lib.load_library().rnnwf_abi_version() == 1
    assert "lstm_pauli.hip" in build.SOURCES and build.compile_flags("lstm_pauli.hip") == build.compile_flags("lstm.hip")
    W = _lib.NativeWavefunction
    p, p_1 = inspect.signature(W.pauli_step_lstm).parameters, inspect.signature(W.pauli_step).parameters
    assert list(p) == list(p_1) and [v.default for v in p.values()] == [v.default for v in p_1.values()]
    assert list(inspect.signature(W.lstm_pauli_gradient_step).parameters)[:8] == ["self", "flip", "sign", "coeff", "numsamples", "seed", "step",
                                                                                  "shapes"]


def test_module_interface():
    assert OL.__all__ == ["pauli_expectations", "energy", "correlations", "minimize_hamiltonian"]
    for name in ("pauli_expectations", "energy"):
        a, b = inspect.signature(getattr(OL, name)).parameters, inspect.signature(getattr(O, name)).parameters
        assert list(a) == list(b) and [v.default for v in a.values()] == [v.default for v in b.values()], name
    for name, other in (("minimize_hamiltonian", T.minimize_hamiltonian), ("correlations", OS.correlations)):
        a, b = inspect.signature(getattr(OL, name)).parameters, inspect.signature(other).parameters
        assert list(a) == list(b) and [v.default for v in a.values()] == [v.default for v in b.values()], name
    assert OL.Hamiltonian is O.Hamiltonian and OL.pauli_terms is O.pauli_terms      # the existing parsing, not a copy
    assert OL.tfim_hamiltonian is O.tfim_hamiltonian and OL.xxz_hamiltonian is O.xxz_hamiltonian
    assert OL.lr_schedule(1e-2, 0) == 1e-2 and OL.lr_schedule(1e-2, 300) == 1.0 / (100.0 + 30.0)      # run_2DTFIM_1DRNN_LSTM's rule


def _handle(model, units, N=6):
    """passes observables._native without a library or a device; every library call raises"""
    from rnnwavefunctions_amd import _lib

    class NoLibrary(_lib.NativeWavefunction):
        def __init__(self):
            self.model, self.N, self.nx, self.ny, self.units, self.calls = model, N, N, 1, tuple(units), []

        def __del__(self):
            pass

        def __getattribute__(self, name):
            if name in ("pauli_step_lstm", "lstm_pauli_gradient_step", "set_params", "adam_set_state", "get_params_dict", "lib", "h"):
                raise AssertionError("the library was touched: %s" % name)
            return object.__getattribute__(self, name)
    return NoLibrary()


def test_refusals_fire_before_any_library_call():
    from rnnwavefunctions_amd import _lib
    ham = O.xxz_hamiltonian(6, -1.0, 0.5)
    prm = P.init_lstm_params([8], seed=3)
    calls = [lambda w: OL.pauli_expectations(w, ["XXIIII"], 10), lambda w: OL.energy(w, ham, 10), lambda w: OL.correlations(w, 10),
             lambda w: OL.minimize_hamiltonian(w, ham, prm, numsteps=1, numsamples=10),
             lambda w: OL.minimize_hamiltonian(w, ham, prm, numsteps=1, numsamples=10, device_steps=2)]
    # every other model, with the module that serves it
    for model, units, word in [(_lib.MODEL_GRU1D, (10,), r"observables\.py serves the GRU models"),
                               (_lib.MODEL_GRU1D_F64, (10,), r"observables\.py serves the GRU models"),
                               (_lib.MODEL_GRU1D, (10, 10), r"observables_stack\.py"),
                               (_lib.MODEL_GRU1D_PARITY, (10,), "parity"),
                               (_lib.MODEL_CRNN_U1, (10,), r"observables_complex\.py serves the complex RNN"),
                               (_lib.MODEL_MDRNN2D, (10,), r"observables_2d\.py serves the 2D RNN")]:
        for call in calls:
            with pytest.raises(ValueError, match=word):
                call(_handle(model, units))
            with pytest.raises(ValueError, match="observables_lstm serves the LSTM wave function"):
                call(_handle(model, units))
    with pytest.raises(ValueError, match="facade or a NativeWavefunction"):
        OL.energy(object(), ham, 10)
    # an LSTM, but: device_steps, a communicator, a Hamiltonian of another size, a pair (k, k), a string of the wrong length
    lstm = lambda N=6: _handle(_lib.MODEL_LSTM1D_F64, (8,), N)
    with pytest.raises(ValueError, match=r"device_steps.*no device-resident Adam \(docs/lstm\.md"):
        OL.minimize_hamiltonian(lstm(), ham, prm, numsteps=1, numsamples=10, device_steps=4)
    for bad in (0, -3, 2.5, "4", True):
        with pytest.raises(ValueError, match="device_steps"):
            OL.minimize_hamiltonian(lstm(), ham, prm, numsteps=1, numsamples=10, device_steps=bad)
    with pytest.raises(ValueError, match="communicator"):
        OL.minimize_hamiltonian(lstm(), ham, prm, numsteps=1, numsamples=10, comm=object())
    with pytest.raises(ValueError, match="6 sites, the wave function 5"):
        OL.minimize_hamiltonian(lstm(5), ham, prm, numsteps=1, numsamples=10)
    with pytest.raises(ValueError, match="6 sites, the wave function 5"):
        OL.energy(lstm(5), ham, 10)
    with pytest.raises(ValueError, match="distinct sites"):
        OL.correlations(lstm(), 10, pairs=[(2, 2)])
    with pytest.raises(ValueError, match="one letter per site"):
        OL.pauli_expectations(lstm(), ["XX"], 10)


def test_odd_y_strings_give_zero_without_device_work():
    from rnnwavefunctions_amd import _lib
    out = OL.pauli_expectations(_handle(_lib.MODEL_LSTM1D_F64, (8,)), ["YIIIII", [("X", 0), ("Y", 3)], "XYZYYI"], 100)
    assert np.all(out["value"] == 0) and np.all(out["err"] == 0) and out["value"].shape == (3,)


class _Fake:
    """what observables_lstm.minimize_hamiltonian needs of a NativeWavefunction; records its calls"""

    def __init__(self, prm, N=6):
        self.N, self.calls, self.prm = N, [], prm

    def set_params(self, params, scope=None):
        self.calls.append(("set_params", scope))

    def pauli_step_lstm(self, *a, **k):
        raise AssertionError("the unfused step ran")

    def vmc_gradient(self, *a, **k):
        raise AssertionError("vmc_gradient does not serve the LSTM")

    def lstm_pauli_gradient_step(self, flip, sign, coeff, numsamples, seed, step, shapes):
        self.calls.append(("fused", numsamples, seed, step, sorted(shapes)))
        grads = {k[len(SCOPE) + 1:]: np.full(v.shape, 1.0 + step) for k, v in self.prm.items()}
        return {"moments": np.array([-(step + 1.0) * numsamples, (step + 1.0) ** 2 * numsamples + step, float(numsamples), 0.0]), "grads": grads}


class _Recorder(T.Adam):
    def __init__(self):
        super().__init__()
        self.rates = []

    def step(self, params, grads, lr):
        self.rates.append(lr)
        assert set(grads) == set(params)
        return super().step(params, grads, lr)


def test_minimize_runs_one_fused_call_per_iteration_at_the_lstm_drivers_learning_rate(monkeypatch):
    monkeypatch.setattr(OL, "_native_lstm", lambda wf: wf)
    prm = P.init_lstm_params([8], seed=3)
    ham = O.xxz_hamiltonian(6, -1.0, 0.5)
    wf, opt = _Fake(prm), _Recorder()
    mean, var = OL.minimize_hamiltonian(wf, ham, prm, numsteps=3, numsamples=10, learningrate=2e-2, seed=5, opt=opt)
    names = sorted(k[len(SCOPE) + 1:] for k in prm)
    assert wf.calls == [("set_params", SCOPE)] + [c for it in range(4) for c in (("fused", 10, 5, it, names), ("set_params", SCOPE))]
    assert opt.rates == [1.0 / ((1.0 / 2e-2) + it / 10) for it in range(4)]
    assert np.array_equal(mean, -(np.arange(4) + 1.0)) and np.allclose(var, np.arange(4) / 10.0, rtol=0, atol=1e-12)
    assert all(np.all(OL.minimize_hamiltonian.last_params[k] < prm[k]) for k in prm)          # positive gradients: every element moved down


# ---- what the GPU test's bound rejects -------------------------------------------------------------------------------------------------
# FACTOR: the smallest max |defective log r - brute force| / (1e-11 N) a defect must reach on every lattice where it can show
FACTOR = 1e6
SHOWS = {"checkpoint_f": lambda N: N >= 3,      # f - 1 and f name different checkpoints for some mask with 1 <= f <= N - 2
         "c_from_h": lambda N: N >= 2,          # some mask has f >= 1
         "mask_word_0": lambda N: N > 32}       # some mask has a site in a second word


@pytest.mark.parametrize("units", [10, 37])
def test_the_bound_accepts_the_kernel_form_and_rejects_three_defects(units):
    """per lattice of the GPU test: the restated bookkeeping agrees with brute force far inside the bound, each defect is far outside"""
    prm = Q.parameters(units)
    for Nx, Ny in Q.LATTICES:
        N = Nx * Ny
        s, masks = Q.samples_of(Nx, Ny, units), Q.masks_of(Nx, Ny)
        assert PR.word_boundaries_covered(N, masks)
        ref = PR.log_ratio_masks(Q.log_p(prm, Nx, Ny), s, masks)
        good = np.abs(Q.kernel_form(prm, s, masks) - ref).max()
        assert good <= 0.01 * Q.bound(N), (Nx, Ny, good)
        line = "LSTMPAULI defects %dx%d, %d units: kernel form %.1e of the bound" % (Nx, Ny, units, good / Q.bound(N))
        for defect in Q.DEFECTS:
            if not SHOWS[defect](N):
                continue
            factor = np.abs(Q.kernel_form(prm, s, masks, defect) - ref).max() / Q.bound(N)
            line += "; %s %.1e x" % (defect, factor)
            assert factor >= FACTOR, (Nx, Ny, defect, factor)
        print(line)
