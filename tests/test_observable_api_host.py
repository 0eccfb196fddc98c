"""Characterisation of the Python layer above the library: the Pauli / Renyi / correlation / minimize wrappers of observables.py,
observables_stack.py, observables_2d.py, observables_complex.py and training.minimize_hamiltonian, and the NativeWavefunction methods
below them (pauli_step*, pauli_train_steps*, renyi2_regions*, the minSR methods).  No GPU and no library: every wave function is a
NativeWavefunction without a handle whose `lib` is a fake that records each entry it is called with - entry name and, per argument,
type, value, dtype and shape - and fills the output buffers deterministically.  set_params, adam_set_state, get_params_dict and
vmc_gradient are recorded as methods.

Every scenario's trace (the calls in order, the returned value or the exception's type and full text, what it printed) is compared
with tests/golden/observable_api_trace.json, entry by entry; floats are compared by their repr, so equality is exact.  The file holds
what this package computed when the scenarios were written; `python tests/test_observable_api_host.py` rewrites it from the package
that is importable.  A change of the Python layer that keeps its behaviour leaves this test and its file untouched."""
import contextlib
import ctypes
import io
import json
import os
import sys
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from rnnwavefunctions_amd import _lib  # noqa: E402
from rnnwavefunctions_amd import observables as O  # noqa: E402
from rnnwavefunctions_amd import observables_2d as O2  # noqa: E402
from rnnwavefunctions_amd import observables_complex as OC  # noqa: E402
from rnnwavefunctions_amd import observables_stack as OS  # noqa: E402
from rnnwavefunctions_amd import training as T  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "observable_api_trace.json")
SCOPE = "RNNwavefunction"


def enc(x):
    """a JSON value that pins type, dtype, shape and every element of x"""
    if x is None or isinstance(x, (bool, str)):
        return x
    if isinstance(x, np.ndarray):
        return {"dtype": str(x.dtype), "shape": list(x.shape), "data": " ".join(repr(v) for v in x.ravel().tolist())}
    if isinstance(x, np.generic):
        return [str(x.dtype), repr(x.item())]
    if isinstance(x, (int, float, complex)):
        return [type(x).__name__, repr(x)]
    if isinstance(x, dict):
        return {str(k): enc(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [enc(v) for v in x]
    return [type(x).__name__]


# ---- the fake library ------------------------------------------------------------------------------------------------------------
# One argument list per entry: (name, "val") a scalar, (name, "in", shape) an input array, (name, "out", shape) an output buffer;
# shape is a function of the scalar arguments (and N, resident, nparams of the wave function).

def _c(cplx):
    return (2,) if cplx else ()


def _pauli_step(cplx):
    return [("flip", "in", lambda a: (a["K"], a["N"])), ("sign", "in", lambda a: (a["K"], a["N"])), ("coeff", "in", lambda a: (a["K"],) + _c(cplx)),
            ("K", "val"), ("samples", "in", lambda a: (a["ns"], a["N"])), ("ns", "val"), ("seed", "val"), ("step", "val"), ("offset", "val"),
            ("term_sums", "out", lambda a: (a["K"], 4 if cplx else 2)), ("eloc", "out", lambda a: (a["ns"],) + _c(cplx)),
            ("moments", "out", lambda a: (4,)), ("log_ratio", "out", lambda a: (a["nmasks"], a["ns"]) + _c(cplx)),
            ("drawn", "out", lambda a: (a["ns"], a["N"]))]


def _pauli_train(cplx):
    return [("flip", "in", lambda a: (a["K"], a["N"])), ("sign", "in", lambda a: (a["K"], a["N"])), ("coeff", "in", lambda a: (a["K"],) + _c(cplx)),
            ("K", "val"), ("iters", "val"), ("ns", "val"), ("seed", "val"), ("step0", "val"), ("offset", "val"),
            ("learning_rates", "in", lambda a: (a["iters"],)), ("beta1", "val"), ("beta2", "val"), ("epsilon", "val"),
            ("moments", "out", lambda a: (a["iters"], 4)), ("term_sums", "out", lambda a: (a["iters"], a["K"], 4 if cplx else 2)),
            ("eloc", "out", lambda a: (a["ns"],) + _c(cplx))]


def _regions(cplx):
    spec = [("regions", "in", lambda a: (a["R"], a["N"])), ("R", "val"), ("samples", "in", lambda a: (2 * a["npairs"], a["N"])), ("npairs", "val"),
            ("seed", "val"), ("step", "val"), ("offset", "val"), ("sums", "out", lambda a: (a["R"], 4 if cplx else 2)),
            ("log_ratio", "out", lambda a: (a["R"], a["npairs"]) + _c(cplx))]
    return spec + ([("in_sector", "out", lambda a: (a["R"],))] if cplx else []) + [("drawn", "out", lambda a: (2 * a["npairs"], a["N"]))]


def _sr(suffix):
    rows = (lambda a: 2 * a["resident"]) if suffix == "_complex" else (lambda a: a["resident"])
    return {"rnnwf_log_derivatives" + suffix: [("out", "out", lambda a: ((2,) if suffix == "_complex" else ()) + (a["ns"], a["n"])), ("ns", "val"),
                                               ("n", "val")],
            "rnnwf_sr_gram" + suffix: [("gram", "out", lambda a: (rows(a), rows(a))), ("eps", "out", lambda a: (rows(a),))],
            "rnnwf_sr_apply" + suffix: [("y", "in", lambda a: (rows(a),)), ("out", "out", lambda a: (a["nparams"],))],
            "rnnwf_sr_solve" + suffix: [("diag_shift", "val"), ("y", "out", lambda a: (rows(a),))],
            "rnnwf_sr_direction" + suffix: [("diag_shift", "val"), ("out", "out", lambda a: (a["nparams"],))]}


SPECS = {"rnnwf_pauli_step": _pauli_step(False), "rnnwf_pauli_step_2d": _pauli_step(False), "rnnwf_pauli_step_stack": _pauli_step(False),
         "rnnwf_pauli_step_complex": _pauli_step(True), "rnnwf_pauli_train_steps": _pauli_train(False),
         "rnnwf_pauli_train_steps_2d": _pauli_train(False), "rnnwf_pauli_train_steps_stack": _pauli_train(False),
         "rnnwf_pauli_train_steps_complex": _pauli_train(True), "rnnwf_renyi2_regions": _regions(False),
         "rnnwf_renyi2_regions_2d": _regions(False), "rnnwf_renyi2_regions_stack": _regions(False),
         "rnnwf_renyi2_regions_complex": _regions(True),
         "rnnwf_renyi2_swap": [("samples", "in", lambda a: (2 * a["npairs"], a["N"])), ("npairs", "val"), ("seed", "val"), ("step", "val"),
                               ("offset", "val"), ("sums", "out", lambda a: (a["N"] + 1, 2)), ("log_ratio", "out", lambda a: (a["N"] + 1, a["npairs"])),
                               ("drawn", "out", lambda a: (2 * a["npairs"], a["N"]))],
         "rnnwf_correlations": [("samples", "in", lambda a: (a["ns"], a["N"])), ("ns", "val"), ("seed", "val"), ("step", "val"), ("offset", "val"),
                                ("z_sums", "out", lambda a: (a["N"],)), ("zz_sums", "out", lambda a: (a["N"], a["N"])),
                                ("x_sums", "out", lambda a: (a["N"], 2)), ("xx_sums", "out", lambda a: (a["N"], a["N"], 5)),
                                ("log_ratio", "out", lambda a: (a["N"] + a["N"] * (a["N"] - 1) // 2, a["ns"])),
                                ("drawn", "out", lambda a: (a["ns"], a["N"]))]}
for _s in ("", "_complex", "_2d"):
    SPECS.update(_sr(_s))


class FakeLib:
    """stands in for the ctypes library of one wave function"""

    def __init__(self, wf):
        self.wf = wf

    def rnnwf_last_error(self, h):
        return b""

    def rnnwf_destroy(self, h):
        return 0

    def rnnwf_resident_samples(self, h):
        self.wf.calls.append(["rnnwf_resident_samples"])
        return self.wf.resident

    def rnnwf_num_params(self, h):
        self.wf.calls.append(["rnnwf_num_params"])
        return self.wf.nparams

    def __getattr__(self, entry):
        spec = SPECS[entry]                                   # KeyError: an entry this test does not know

        def call(h, *args):
            assert h is None and len(args) == len(spec), entry
            wf = self.wf
            a = {"N": wf.N, "resident": wf.resident, "nparams": wf.nparams}
            a.update({s[0]: v for s, v in zip(spec, args) if s[1] == "val"})
            rec = {}
            for kind in ("val", "in", "out"):
                for s, v in zip(spec, args):
                    if s[1] != kind:
                        continue
                    if kind == "val":
                        rec[s[0]] = enc(v)
                    elif v is None:
                        rec[s[0]] = None
                    else:
                        assert isinstance(v, ctypes._Pointer), (entry, s[0])
                        shape = tuple(int(d) for d in s[2](a))
                        buf = np.ctypeslib.as_array(v, shape=shape) if int(np.prod(shape)) else np.zeros(shape)
                        if kind == "in":
                            rec[s[0]] = [type(v).__name__, enc(np.array(buf))]
                            if s[0] == "flip":
                                a["nmasks"] = len({r.tobytes() for r in np.array(buf) if r.any()})
                        else:
                            rec[s[0]] = [type(v).__name__, list(shape)]
                            k = np.arange(buf.size).reshape(shape)
                            if buf.dtype == np.int32:
                                buf[...] = (k * 7 // 3 + len(wf.calls)) % 2
                            elif buf.dtype == np.int64:
                                buf[...] = k % 3
                            else:
                                buf[...] = 0.25 * k + len(s[0]) + 0.125 * len(wf.calls)
                                if s[0] == "log_ratio":
                                    buf[...] = 0.03125 * k - 0.5
                                    if shape[-1:] == (2,) and len(shape) == 3:
                                        buf[0, 0] = (-np.inf, 0.0)      # a configuration outside the sector
            wf.calls.append([entry, [rec[s[0]] for s in spec]])
            return 0
        return call


class Rec(_lib.NativeWavefunction):
    """a NativeWavefunction without a handle on the fake library; records the methods the drivers call around the entries"""

    def __init__(self, model, nx, ny=1, units=(5,), resident=0, nparams=0):
        self.h, self.model, self.nx, self.ny, self.N, self.units = None, model, nx, ny, nx * ny, tuple(units)
        self.resident, self.nparams, self.calls = resident, nparams, []
        self.lib = FakeLib(self)

    def set_params(self, params, scope=None):
        self.calls.append(["set_params", enc(params), scope])

    def adam_set_state(self, m, v, t):
        self.calls.append(["adam_set_state", enc(m), enc(v), enc(t)])

    def get_params_dict(self, like, scope=None):
        self.calls.append(["get_params_dict", enc(like), scope])
        return {k: v + 1 for k, v in like.items()}

    def vmc_gradient(self, mean_energy, norm, shapes, allreduce=False):
        self.calls.append(["vmc_gradient", enc(mean_energy), enc(norm), enc(shapes), allreduce])
        return {k: np.full(s, 0.01 * (i + 1) * len(self.calls)) for i, (k, s) in enumerate(shapes.items())}


class Facade:
    """what observables._native and observables_complex.minimize_hamiltonian need of a reference-named facade"""
    scope = "ScopeOfTheFacade"

    def __init__(self, nat):
        self._native = nat

    def get_params(self):
        return params(self.scope)

    def set_params(self, p):
        self._native.calls.append(["facade.set_params", enc(p)])


def params(scope=SCOPE):
    return {scope + "/a": np.arange(3, dtype=np.float32), scope + "/b": 0.5 * np.ones((2, 2))}


def gru():
    return Rec(_lib.MODEL_GRU1D, 4)


def stack():
    return Rec(_lib.MODEL_GRU1D, 4, units=(5, 5))


def mdrnn():
    return Rec(_lib.MODEL_MDRNN2D, 2, 2)


def crnn():
    return Rec(_lib.MODEL_CRNN_U1, 4)


def spins(rows, N=4):
    return (np.arange(rows * N).reshape(rows, N) * 5 // 3) % 2


HAM = O.Hamiltonian(4, [(-1.0, "ZZII"), (0.5, "IXXI"), (0.25, "YYII"), (-0.5, [("X", 3)])])
HAM5 = O.tfim_hamiltonian(np.ones(5), 1.0)
CHAM = OC.ComplexHamiltonian(4, [(1.0, "XXII"), (0.5, "YZII"), (0.25 + 0.5j, "IIZZ"), (0.25 - 0.5j, "IIZZ"), (1.0, "ZYII")])
CHAM_NH = OC.ComplexHamiltonian(4, [(1j, "XXII")])
CHAM5 = OC.j1j2_hamiltonian(np.ones(5), np.zeros(5), np.zeros(5))
STRINGS = ["XXII", "YIII", [("Z", 0), ("Z", 3)], "YYII", "IXXI"]
A, B = np.array([1, 1, 0, 0]), np.array([0, 0, 0, 1])
MASKS = np.array([[1, 0, 0, 0], [0, 1, 1, 0]])


def scenarios():
    """{name: (wave function or None, callable taking it)}"""
    S = {}

    def real_family(tag, mod, make, minimize, shape):
        smp = lambda rows: spins(rows).reshape((rows,) + shape)
        S[tag + "/pauli_expectations/draw"] = (make(), lambda w: mod.pauli_expectations(w, STRINGS, 4, seed=7, step=3))
        S[tag + "/pauli_expectations/samples"] = (make(), lambda w: mod.pauli_expectations(w, STRINGS, 4, samples=smp(4)))
        S[tag + "/pauli_expectations/flat_samples"] = (make(), lambda w: mod.pauli_expectations(w, STRINGS, np.int64(4), samples=spins(4).ravel()))
        S[tag + "/pauli_expectations/odd_y_only"] = (make(), lambda w: mod.pauli_expectations(w, ["YIII", "XYII"], 4))
        S[tag + "/pauli_expectations/facade"] = (make(), lambda w: mod.pauli_expectations(Facade(w), ["XXII"], 4))
        S[tag + "/pauli_expectations/short_string"] = (make(), lambda w: mod.pauli_expectations(w, ["XX"], 4))
        S[tag + "/pauli_expectations/bad_samples"] = (make(), lambda w: mod.pauli_expectations(w, ["XXII"], 4, samples=spins(3)))
        S[tag + "/energy/draw"] = (make(), lambda w: mod.energy(w, HAM, 4, seed=7, step=3))
        S[tag + "/energy/samples_eloc"] = (make(), lambda w: mod.energy(w, HAM, 4, samples=smp(4), want_eloc=True))
        S[tag + "/energy/wrong_N"] = (make(), lambda w: mod.energy(w, HAM5, 4))
        S[tag + "/energy/no_wavefunction"] = (None, lambda w: mod.energy("no wave function", HAM, 4))
        S[tag + "/correlations/draw"] = (make(), lambda w: mod.correlations(w, 4, seed=7, step=3))
        S[tag + "/correlations/samples"] = (make(), lambda w: mod.correlations(w, 4, samples=smp(4)))
        S[tag + "/renyi2_regions/draw"] = (make(), lambda w: mod.renyi2_regions(w, MASKS, 3, seed=7, step=3))
        S[tag + "/renyi2_regions/samples_one_mask"] = (make(), lambda w: mod.renyi2_regions(w, A, 3, samples=smp(6)))
        S[tag + "/renyi2_regions/bad_shape"] = (make(), lambda w: mod.renyi2_regions(w, np.zeros((2, 5)), 3))
        S[tag + "/renyi2_regions/not_integers"] = (make(), lambda w: mod.renyi2_regions(w, 0.5 * MASKS, 3))
        S[tag + "/renyi2_regions/bad_samples"] = (make(), lambda w: mod.renyi2_regions(w, MASKS, 3, samples=spins(5)))
        S[tag + "/mutual_information/draw"] = (make(), lambda w: mod.renyi2_mutual_information(w, A, B, 3, seed=7, step=3))
        S[tag + "/mutual_information/samples"] = (make(), lambda w: mod.renyi2_mutual_information(w, A, B, 3, samples=smp(6)))
        S[tag + "/mutual_information/overlap"] = (make(), lambda w: mod.renyi2_mutual_information(w, A, A, 3))
        S[tag + "/mutual_information/overlap_no_wavefunction"] = (None, lambda w: mod.renyi2_mutual_information("no wave function", A, A, 3))
        S[tag + "/mutual_information/two_dimensional_masks"] = (make(), lambda w: mod.renyi2_mutual_information(w, A.reshape(2, 2), B.reshape(2, 2), 3))
        S[tag + "/mutual_information/not_masks"] = (make(), lambda w: mod.renyi2_mutual_information(w, 2 * A, B, 3))
        for ds in (None, 2):
            d = "/device_steps=%r" % ds
            S[tag + "/minimize" + d] = (make(), lambda w, ds=ds: (minimize(w, HAM, params(), numsteps=2, numsamples=4, learningrate=0.125, seed=7,
                                                                          device_steps=ds), minimize.last_params))
            S[tag + "/minimize/verbose_scope" + d] = (make(), lambda w, ds=ds: (minimize(w, HAM, params("S"), 10, 4, scope="S", verbose=True,
                                                                                        device_steps=ds), minimize.last_params))
            S[tag + "/minimize/comm" + d] = (make(), lambda w, ds=ds: minimize(w, HAM, params(), 2, 4, comm="a communicator", device_steps=ds))
            S[tag + "/minimize/wrong_N" + d] = (make(), lambda w, ds=ds: minimize(w, HAM5, params(), 2, 4, device_steps=ds))
        S[tag + "/minimize/opt"] = (make(), lambda w: (minimize(w, HAM, params(), 2, 4, opt=T.Adam(beta1=0.5)), minimize.last_params))
        S[tag + "/minimize/opt_with_device_steps"] = (make(), lambda w: minimize(w, HAM, params(), 2, 4, opt="my optimizer", device_steps=2))
        for bad in (0, 2.5, "4", True):
            S[tag + "/minimize/device_steps=%r" % (bad,)] = (make(), lambda w, bad=bad: minimize(w, HAM, params(), 2, 4, device_steps=bad))
        S[tag + "/minimize/comm_before_wavefunction"] = (None, lambda w: minimize("no wave function", HAM, params(), 2, 4, comm=1))

    real_family("gru", O, gru, T.minimize_hamiltonian, (4,))
    real_family("stack", OS, stack, OS.minimize_hamiltonian, (4,))
    real_family("2d", O2, mdrnn, O2.minimize_hamiltonian, (2, 2))
    for tag, mod, make in (("stack", OS, stack), ("2d", O2, mdrnn)):
        S[tag + "/correlations/pairs"] = (make(), lambda w, mod=mod: mod.correlations(w, 4, pairs=[(0, 3), (3, 0), (1, 2)], seed=7))
        S[tag + "/correlations/pair_kk"] = (make(), lambda w, mod=mod: mod.correlations(w, 4, pairs=[(2, 2)]))
        S[tag + "/correlations/pair_out_of_range"] = (make(), lambda w, mod=mod: mod.correlations(w, 4, pairs=[(0, 4)]))
        S[tag + "/wrong_model"] = (gru(), lambda w, mod=mod: mod.energy(w, HAM, 4))
        S[tag + "/wrong_model/minimize"] = (crnn(), lambda w, mod=mod: mod.minimize_hamiltonian(w, HAM, params(), 2, 4))
    S["gru/renyi2_entropy/draw"] = (gru(), lambda w: O.renyi2_entropy(w, 3, seed=7, step=3))
    S["gru/renyi2_entropy/samples"] = (gru(), lambda w: O.renyi2_entropy(w, 3, samples=spins(6)))
    S["stack/renyi2_entropy/draw"] = (stack(), lambda w: OS.renyi2_entropy(w, 3, seed=7, step=3))
    S["stack/renyi2_entropy/samples"] = (stack(), lambda w: OS.renyi2_entropy(w, 3, samples=spins(6)))
    S["2d/renyi2_regions/lattice_masks"] = (mdrnn(), lambda w: O2.renyi2_regions(w, MASKS.reshape(2, 2, 2), 3))
    S["2d/mutual_information/flat_masks_flat_samples"] = (mdrnn(), lambda w: O2.renyi2_mutual_information(w, A, B, 3, samples=spins(6)))

    # the complex RNN
    S["complex/pauli_expectations/draw"] = (crnn(), lambda w: OC.pauli_expectations(w, STRINGS, 4, seed=7, step=3))
    S["complex/pauli_expectations/samples"] = (crnn(), lambda w: OC.pauli_expectations(w, STRINGS, 4, samples=spins(4).ravel()))
    S["complex/pauli_expectations/facade"] = (crnn(), lambda w: OC.pauli_expectations(Facade(w), ["XXII"], 4))
    S["complex/pauli_expectations/bad_samples"] = (crnn(), lambda w: OC.pauli_expectations(w, ["XXII"], 4, samples=spins(3)))
    S["complex/energy/draw"] = (crnn(), lambda w: OC.energy(w, CHAM, 4, seed=7, step=3))
    S["complex/energy/samples_eloc"] = (crnn(), lambda w: OC.energy(w, CHAM, 4, samples=spins(4), want_eloc=True))
    S["complex/energy/not_hermitian"] = (crnn(), lambda w: OC.energy(w, CHAM_NH, 4))
    S["complex/energy/wrong_N"] = (crnn(), lambda w: OC.energy(w, CHAM5, 4))
    S["complex/energy/no_wavefunction"] = (None, lambda w: OC.energy("no wave function", CHAM, 4))
    S["complex/wrong_model"] = (gru(), lambda w: OC.energy(w, CHAM, 4))
    S["complex/spin_correlations/draw"] = (crnn(), lambda w: OC.spin_correlations(w, 4, seed=7, step=3))
    S["complex/spin_correlations/samples"] = (crnn(), lambda w: OC.spin_correlations(w, 4, samples=spins(4)))
    S["complex/renyi2_regions/draw"] = (crnn(), lambda w: OC.renyi2_regions(w, MASKS, 3, seed=7, step=3))
    S["complex/renyi2_regions/draw_log_ratio"] = (crnn(), lambda w: OC.renyi2_regions(w, MASKS, 3, want_log_ratio=True))
    S["complex/renyi2_regions/samples_log_ratio"] = (crnn(), lambda w: OC.renyi2_regions(w, A, 3, samples=spins(6).ravel(), want_log_ratio=True))
    S["complex/renyi2_regions/three_dimensional"] = (crnn(), lambda w: OC.renyi2_regions(w, MASKS.reshape(2, 2, 2), 3))
    S["complex/renyi2_regions/not_integers"] = (crnn(), lambda w: OC.renyi2_regions(w, 0.5 * MASKS, 3))
    S["complex/renyi2_entropy/draw"] = (crnn(), lambda w: OC.renyi2_entropy(w, 3, seed=7, step=3))
    S["complex/renyi2_entropy/samples"] = (crnn(), lambda w: OC.renyi2_entropy(w, 3, samples=spins(6)))
    S["complex/mutual_information/draw"] = (crnn(), lambda w: OC.renyi2_mutual_information(w, A, B, 3, seed=7, step=3))
    S["complex/mutual_information/samples"] = (crnn(), lambda w: OC.renyi2_mutual_information(w, A, B, 3, samples=spins(6)))
    S["complex/mutual_information/overlap"] = (crnn(), lambda w: OC.renyi2_mutual_information(w, A, A, 3))
    for ds in (None, 2):
        d = "/device_steps=%r" % ds
        S["complex/minimize" + d] = (crnn(), lambda w, ds=ds: (OC.minimize_hamiltonian(w, CHAM, 4, 2, 0.125, params=params(), seed=7, device_steps=ds),
                                                              OC.minimize_hamiltonian.last_params))
        S["complex/minimize/facade_verbose" + d] = (crnn(), lambda w, ds=ds: (OC.minimize_hamiltonian(Facade(w), CHAM, np.int64(4), 10.0, 0.125,
                                                                                                      verbose=True, device_steps=ds),
                                                                             OC.minimize_hamiltonian.last_params))
        S["complex/minimize/wrong_N" + d] = (crnn(), lambda w, ds=ds: OC.minimize_hamiltonian(w, CHAM5, 4, 2, 0.125, params=params(), device_steps=ds))
        S["complex/minimize/no_params" + d] = (crnn(), lambda w, ds=ds: OC.minimize_hamiltonian(w, CHAM, 4, 2, 0.125, device_steps=ds))
    S["complex/minimize/opt"] = (crnn(), lambda w: (OC.minimize_hamiltonian(w, CHAM, 4, 2, 0.125, params=params(), opt=T.Adam(beta1=0.5)),
                                                    OC.minimize_hamiltonian.last_params))
    S["complex/minimize/opt_with_device_steps"] = (crnn(), lambda w: OC.minimize_hamiltonian(w, CHAM, 4, 2, 0.125, params=params(), opt="my optimizer",
                                                                                            device_steps=2))
    S["complex/minimize/device_steps=0"] = (crnn(), lambda w: OC.minimize_hamiltonian(w, CHAM, 4, 2, 0.125, params=params(), device_steps=0))
    S["complex/minimize/wrong_model"] = (gru(), lambda w: OC.minimize_hamiltonian(w, CHAM, 4, 2, 0.125, params=params()))

    # the NativeWavefunction methods themselves
    fl, sg = np.array([[1, 1, 0, 0], [0, 0, 0, 0], [1, 1, 0, 0], [0, 0, 1, 0]]), np.array([[0, 0, 0, 0], [1, 0, 0, 1], [1, 1, 0, 0], [0, 0, 0, 0]])
    co, cc = [1.0, -2.0, 0.5, 3.0], [1.0, -2.0j, 0.5 + 1j, 3.0]
    every = dict(want_eloc=True, want_log_ratio=True, want_samples=True)
    steps = (("pauli_step", gru, co), ("pauli_step_stack", stack, co), ("pauli_step_2d", mdrnn, co), ("pauli_step_complex", crnn, cc))
    for name, make, c in steps:
        t = "lib/" + name
        S[t + "/draw_everything"] = (make(), lambda w, name=name, c=c: getattr(w, name)(fl, sg, c, 3, seed=7, step=3, sample_offset=5, **every))
        S[t + "/samples_everything"] = (make(), lambda w, name=name, c=c: getattr(w, name)(fl.astype(float), sg.astype(bool), c, 3, spins(3), **every))
        S[t + "/flat_samples"] = (make(), lambda w, name=name, c=c: getattr(w, name)(fl, sg, c, 3, samples=spins(3).ravel()))
        S[t + "/lattice_samples"] = (make(), lambda w, name=name, c=c: getattr(w, name)(fl, sg, c, 3, samples=spins(3).reshape(3, 2, 2)))
        S[t + "/one_term"] = (make(), lambda w, name=name, c=c: getattr(w, name)(fl[0], sg[0], c[0], 3.0, want_samples=True))
        S[t + "/lattice_masks"] = (make(), lambda w, name=name, c=c: getattr(w, name)(fl.reshape(4, 2, 2), sg.reshape(4, 2, 2), c, 3))
        S[t + "/lattice_masks_transposed"] = (make(), lambda w, name=name, c=c: getattr(w, name)(fl.reshape(4, 1, 4), sg.reshape(4, 1, 4), c, 3))
        S[t + "/mask_width"] = (make(), lambda w, name=name, c=c: getattr(w, name)(np.zeros((4, 5)), np.zeros((4, 5)), c, 3))
        S[t + "/mask_shapes_differ"] = (make(), lambda w, name=name, c=c: getattr(w, name)(fl, sg[:3], c, 3))
        S[t + "/no_terms"] = (make(), lambda w, name=name, c=c: getattr(w, name)(fl[:0], sg[:0], [], 3))
        S[t + "/not_integers"] = (make(), lambda w, name=name, c=c: getattr(w, name)(fl, 0.5 * sg, c, 3))
        S[t + "/coeff_shape"] = (make(), lambda w, name=name, c=c: getattr(w, name)(fl, sg, c[:3], 3))
        S[t + "/samples_rows"] = (make(), lambda w, name=name, c=c: getattr(w, name)(fl, sg, c, 3, samples=spins(4)))
        S[t + "/samples_one_dimensional_wrong"] = (make(), lambda w, name=name, c=c: getattr(w, name)(fl, sg, c, 3, samples=np.zeros(11)))
    trains = (("pauli_train_steps", gru, co), ("pauli_train_steps_stack", stack, co), ("pauli_train_steps_2d", mdrnn, co),
              ("pauli_train_steps_complex", crnn, cc))
    for name, make, c in trains:
        t = "lib/" + name
        S[t + "/moments_only"] = (make(), lambda w, name=name, c=c: getattr(w, name)(fl, sg, c, 3, 7, 5, [0.125, 0.25]))
        S[t + "/everything"] = (make(), lambda w, name=name, c=c: getattr(w, name)(fl, sg, c, 3, 7, 5, [0.125, 0.25, 0.5], 0.5, 0.75, 1e-6, sample_offset=2,
                                                                                   want_term_sums=True, want_eloc=True))
        S[t + "/scalar_rate_one_term"] = (make(), lambda w, name=name, c=c: getattr(w, name)(fl[0], sg[0], c[0], 3, 7, 5, 0.125, want_eloc=True))
        S[t + "/lattice_masks"] = (make(), lambda w, name=name, c=c: getattr(w, name)(fl.reshape(4, 2, 2), sg.reshape(4, 2, 2), c, 3, 7, 5, [0.125]))
        S[t + "/mask_width"] = (make(), lambda w, name=name, c=c: getattr(w, name)(np.zeros((4, 5)), np.zeros((4, 5)), c, 3, 7, 5, [0.125]))
        S[t + "/not_integers"] = (make(), lambda w, name=name, c=c: getattr(w, name)(0.5 * fl, sg, c, 3, 7, 5, [0.125]))
        S[t + "/coeff_shape"] = (make(), lambda w, name=name, c=c: getattr(w, name)(fl, sg, c[:2], 3, 7, 5, [0.125]))
    regions = (("renyi2_regions", gru), ("renyi2_regions_stack", stack), ("renyi2_regions_2d", mdrnn), ("renyi2_regions_complex", crnn))
    for name, make in regions:
        t = "lib/" + name
        S[t + "/draw_log_ratio"] = (make(), lambda w, name=name: getattr(w, name)(MASKS, 3, seed=7, step=3, pair_offset=5, log_ratio=True))
        S[t + "/samples"] = (make(), lambda w, name=name: getattr(w, name)(MASKS.astype(float), 3.0, samples=spins(6)))
        S[t + "/lattice_samples_one_mask"] = (make(), lambda w, name=name: getattr(w, name)(A, 3, samples=spins(6).reshape(6, 2, 2), log_ratio=True))
        S[t + "/lattice_masks"] = (make(), lambda w, name=name: getattr(w, name)(MASKS.reshape(2, 2, 2), 3))
        S[t + "/lattice_masks_transposed"] = (make(), lambda w, name=name: getattr(w, name)(MASKS.reshape(2, 4, 1), 3))
        S[t + "/four_dimensional_masks"] = (make(), lambda w, name=name: getattr(w, name)(MASKS.reshape(2, 2, 2, 1), 3))
        S[t + "/mask_width"] = (make(), lambda w, name=name: getattr(w, name)(np.zeros((2, 5)), 3))
        S[t + "/no_regions"] = (make(), lambda w, name=name: getattr(w, name)(MASKS[:0], 3))
        S[t + "/not_integers"] = (make(), lambda w, name=name: getattr(w, name)(0.5 * MASKS, 3))
        S[t + "/samples_rows"] = (make(), lambda w, name=name: getattr(w, name)(MASKS, 3, samples=spins(5)))
    for suffix, model in (("", _lib.MODEL_GRU1D), ("_complex", _lib.MODEL_CRNN_U1), ("_2d", _lib.MODEL_MDRNN2D)):
        make = lambda model=model, resident=3: Rec(model, 2, 2 if model == _lib.MODEL_MDRNN2D else 1, resident=resident, nparams=5)
        rows = 6 if suffix == "_complex" else 3
        t = "lib/sr" + suffix
        S[t + "/log_derivatives"] = (make(), lambda w, s=suffix: getattr(w, "log_derivatives" + s)())
        S[t + "/sr_gram"] = (make(), lambda w, s=suffix: getattr(w, "sr_gram" + s)())
        S[t + "/sr_apply"] = (make(), lambda w, s=suffix, rows=rows: getattr(w, "sr_apply" + s)(np.arange(rows)))
        S[t + "/sr_apply/wrong_y"] = (make(), lambda w, s=suffix, rows=rows: getattr(w, "sr_apply" + s)(np.arange(rows + 1)))
        S[t + "/sr_apply/wrong_y_2d"] = (make(), lambda w, s=suffix, rows=rows: getattr(w, "sr_apply" + s)(np.zeros((rows, 1))))
        S[t + "/sr_apply/no_batch"] = (make(resident=0), lambda w, s=suffix: getattr(w, "sr_apply" + s)([1.0, 2.0]))
        S[t + "/sr_solve"] = (make(), lambda w, s=suffix: getattr(w, "sr_solve" + s)(np.float32(0.5)))
        S[t + "/sr_direction"] = (make(), lambda w, s=suffix: getattr(w, "sr_direction" + s)(1))
        S[t + "/no_batch"] = (make(resident=0), lambda w, s=suffix: [getattr(w, m + s)() for m in ("log_derivatives", "sr_gram")]
                              + [getattr(w, "sr_solve" + s)(0.5)])
    return S


def run(wf, call):
    """the trace of one scenario"""
    out, printed = {}, io.StringIO()
    with warnings.catch_warnings(record=True) as caught, contextlib.redirect_stdout(printed):
        warnings.simplefilter("always")
        try:
            out["result"] = enc(call(wf))
        except Exception as e:                                 # noqa: BLE001 - the type and the text are what is pinned
            out["raises"] = [type(e).__name__, str(e)]
    out["calls"] = wf.calls if wf is not None else []
    out["warnings"] = [[w.category.__name__, str(w.message)] for w in caught]
    out["printed"] = printed.getvalue()
    return json.loads(json.dumps(out))


SCENARIOS = scenarios()


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_golden_file_holds_exactly_these_scenarios():
    assert sorted(_golden()) == sorted(SCENARIOS)


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_trace(name):
    want, got = _golden()[name], run(*SCENARIOS[name])
    assert sorted(got) == sorted(want)
    for key in ("raises", "result", "warnings", "printed"):
        assert got.get(key) == want.get(key), key
    assert [c[0] for c in got["calls"]] == [c[0] for c in want["calls"]]
    for g, w in zip(got["calls"], want["calls"]):
        assert g == w, g[0]


def test_the_refusals_read_as_documented():
    """a few of the texts above, spelled out: each is raised before an entry that works on the device is called"""
    g = _golden()
    texts = {"stack/correlations/pair_kk": ["ValueError", "pairs must name two distinct sites in 0..3 each"],
             "2d/correlations/pair_kk": ["ValueError", "pairs must name two distinct lattice sites in 0..3 each"],
             "gru/energy/wrong_N": ["ValueError", "the Hamiltonian has 5 sites, the wave function 4"],
             "2d/minimize/comm/device_steps=None": ["ValueError", "minimize_hamiltonian runs in one process on one GPU: no communicator "
                                                    "(comm='a communicator')"],
             "stack/minimize/opt_with_device_steps": ["ValueError", "observables_stack.minimize_hamiltonian: device_steps runs Adam on the device; a "
                                                      "custom optimizer (opt='my optimizer') needs the host loop (device_steps=None)"],
             "gru/mutual_information/overlap": ["ValueError", "region_a and region_b must be disjoint; both contain the sites [0, 1]"],
             "lib/pauli_step_complex/mask_width": ["ValueError", "flip and sign must both have shape (nterms >= 1, 4), got (4, 5) and (4, 5)"],
             "lib/pauli_train_steps_2d/not_integers": ["ValueError", "flip and sign must hold the integers 0 and 1"],
             "lib/pauli_step_stack/coeff_shape": ["ValueError", "coeff must have shape (4,), got (3,)"],
             "lib/renyi2_regions_complex/lattice_masks": ["ValueError", "regions must have shape (nregions >= 1, 4), got (2, 2, 2)"],
             "lib/sr_complex/sr_apply/wrong_y": ["ValueError", "sr_apply_complex: y must have shape (6,), two entries per sample of the resident "
                                                 "batch, got (7,)"]}
    for name, want in texts.items():
        assert g[name]["raises"] == want and all(c == ["rnnwf_resident_samples"] for c in g[name]["calls"]), name


if __name__ == "__main__":
    with open(GOLDEN, "w") as f:
        json.dump({name: run(*SCENARIOS[name]) for name in sorted(SCENARIOS)}, f, indent=0, sort_keys=True, separators=(",", ":"))
        f.write("\n")
    print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes")
