"""ctypes binding of librnnwf_hip.so (include/rnnwf.h) and a thin NumPy-facing handle class.

There is deliberately no fallback: if the HIP library is not built, or no gfx950 device is
visible, the calls below raise.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "librnnwf_hip.so")

MODEL_GRU1D, MODEL_GRU1D_PARITY, MODEL_CRNN_U1, MODEL_GRU1D_F64, MODEL_MDRNN2D, MODEL_LSTM1D_F64 = range(6)
F32, F64 = 0, 1
ABI_VERSION = 1
MAX_LAYERS = 4
UNIQUE_ID_BYTES = 128
SR_BLOCK = 32          # block width of the device Cholesky solve (kSrNB in csrc/sr_solve_kernels.h)
SR_COMPLEX_MAX_SAMPLES = 2048    # RNNWF_SR_COMPLEX_MAX_SAMPLES: the complex RNN's minSR system has 2 ns <= 4096 rows


class Config(C.Structure):
    _fields_ = [("abi_version", C.c_int32), ("model", C.c_int32), ("nx", C.c_int32), ("ny", C.c_int32),
                ("num_layers", C.c_int32), ("units", C.c_int32 * MAX_LAYERS), ("device", C.c_int32),
                ("reserved", C.c_int32 * 6)]


_P = C.c_void_p
_I32P, _F64P, _F32P = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_float)
_I64, _U64, _I32, _F64 = C.c_int64, C.c_uint64, C.c_int32, C.c_double

# every symbol include/rnnwf.h declares: name -> (restype, argtypes)
PROTOTYPES = {
    "rnnwf_create": (C.c_int, [C.POINTER(Config), C.POINTER(_P)]),
    "rnnwf_destroy": (C.c_int, [_P]),
    "rnnwf_last_error": (C.c_char_p, [_P]),
    "rnnwf_backend_name": (C.c_char_p, []),
    "rnnwf_abi_version": (C.c_int, []),
    "rnnwf_set_param": (C.c_int, [_P, C.c_char_p, _P, _I64, _I32]),
    "rnnwf_get_param": (C.c_int, [_P, C.c_char_p, _P, _I64, _I32]),
    "rnnwf_commit_params": (C.c_int, [_P]),
    "rnnwf_init_params": (C.c_int, [_P, C.c_uint64]),
    "rnnwf_num_params": (_I64, [_P]),
    "rnnwf_sample": (C.c_int, [_P, _I64, _U64, _U64, _I64, _I32P, _F64P]),
    "rnnwf_log_prob": (C.c_int, [_P, _I32P, _I64, _F64P]),
    "rnnwf_log_amp": (C.c_int, [_P, _I32P, _I64, _F32P]),
    "rnnwf_tfim_eloc": (C.c_int, [_P, _I32P, _I64, _F64P, _F64, _F64P, _F64P]),
    "rnnwf_tfim2d_eloc": (C.c_int, [_P, _I32P, _I64, _F64P, _F64, _F64P, _F64P]),
    "rnnwf_j1j2_eloc": (C.c_int, [_P, _I32P, _I64, _F64P, _F64P, _F64P, _I32, _I32, _F32P, C.POINTER(_I64)]),
    "rnnwf_vmc_step": (C.c_int, [_P, _I64, _U64, _U64, _I64, _F64P, _I64, _I32P, _P, _F64P]),
    "rnnwf_vmc_gradient": (C.c_int, [_P, _F64, _F64, _F64]),
    "rnnwf_load_batch": (C.c_int, [_P, _I32P, _I64, _P]),
    "rnnwf_get_grad": (C.c_int, [_P, C.c_char_p, _P, _I64, _I32]),
    "rnnwf_set_params_flat": (C.c_int, [_P, _F64P, _I64]),
    "rnnwf_host_split_images": (C.c_int, [C.c_int32, _F64P, _I64, _P, _P, _I64, _I32P]),
    "rnnwf_host_split_range": (C.c_int, [C.c_int32, _F64P, _I64, _F64P, _I32P]),
    "rnnwf_get_grads_flat": (C.c_int, [_P, _F64P, _I64]),
    "rnnwf_param_name": (C.c_char_p, [_P, _I32, C.POINTER(_I64)]),
    "rnnwf_allreduce_grads": (C.c_int, [_P]),
    "rnnwf_comm_unique_id": (C.c_int, [_P]),
    "rnnwf_comm_init": (C.c_int, [_P, _P, _I32, _I32]),
    "rnnwf_allreduce_moments": (C.c_int, [_P, _F64P, _I32]),
    "rnnwf_allreduce_f64": (C.c_int, [_P, _F64P, _I64]),
    "rnnwf_comm_info": (C.c_int, [_P, _P, _P, _P]),
    "rnnwf_comm_reduce_in_step": (C.c_int, [_P, _I32]),
    "rnnwf_comm_destroy": (C.c_int, [_P]),
    "rnnwf_device_training_supported": (C.c_int, [_P]),
    "rnnwf_adam_step": (C.c_int, [_P, _F64, _F64, _F64, _F64]),
    "rnnwf_train_steps": (C.c_int, [_P, _I32, _I64, C.c_uint64, C.c_uint64, _I64, _F64P, _I64, _F64P, _F64, _F64, _F64, _F64P]),
    "rnnwf_adam_get_state": (C.c_int, [_P, _F64P, _F64P, _I64, C.POINTER(_I64)]),
    "rnnwf_adam_set_state": (C.c_int, [_P, _F64P, _F64P, _I64, _I64]),
    "rnnwf_renyi2_swap": (C.c_int, [_P, _I32P, _I64, C.c_uint64, C.c_uint64, _I64, _F64P, _F64P, _I32P]),
    "rnnwf_renyi2_regions": (C.c_int, [_P, _I32P, _I32, _I32P, _I64, C.c_uint64, C.c_uint64, _I64, _F64P, _F64P, _I32P]),
    "rnnwf_renyi2_regions_2d": (C.c_int, [_P, _I32P, _I32, _I32P, _I64, C.c_uint64, C.c_uint64, _I64, _F64P, _F64P, _I32P]),
    "rnnwf_renyi2_regions_complex": (C.c_int, [_P, _I32P, _I32, _I32P, _I64, C.c_uint64, C.c_uint64, _I64, _F64P, _F64P, C.POINTER(C.c_int64),
                                               _I32P]),
    "rnnwf_correlations": (C.c_int, [_P, _I32P, _I64, C.c_uint64, C.c_uint64, _I64, _F64P, _F64P, _F64P, _F64P, _F64P, _I32P]),
    "rnnwf_pauli_step": (C.c_int, [_P, _I32P, _I32P, _F64P, _I32, _I32P, _I64, C.c_uint64, C.c_uint64, _I64, _F64P, _F64P, _F64P, _F64P,
                                   _I32P]),
    "rnnwf_pauli_step_2d": (C.c_int, [_P, _I32P, _I32P, _F64P, _I32, _I32P, _I64, C.c_uint64, C.c_uint64, _I64, _F64P, _F64P, _F64P, _F64P,
                                      _I32P]),
    "rnnwf_pauli_step_complex": (C.c_int, [_P, _I32P, _I32P, _F64P, _I32, _I32P, _I64, C.c_uint64, C.c_uint64, _I64, _F64P, _F32P, _F64P,
                                           _F64P, _I32P]),
    "rnnwf_pauli_train_steps": (C.c_int, [_P, _I32P, _I32P, _F64P, _I32, _I32, _I64, C.c_uint64, C.c_uint64, _I64, _F64P, _F64, _F64, _F64,
                                          _F64P, _F64P, _F64P]),
    "rnnwf_pauli_train_steps_complex": (C.c_int, [_P, _I32P, _I32P, _F64P, _I32, _I32, _I64, C.c_uint64, C.c_uint64, _I64, _F64P, _F64, _F64,
                                                  _F64, _F64P, _F64P, _F32P]),
    "rnnwf_log_derivatives": (C.c_int, [_P, _F64P, _I64, _I64]),
    "rnnwf_sr_gram": (C.c_int, [_P, _F64P, _F64P]),
    "rnnwf_sr_apply": (C.c_int, [_P, _F64P, _F64P]),
    "rnnwf_sr_solve": (C.c_int, [_P, _F64, _F64P]),
    "rnnwf_sr_direction": (C.c_int, [_P, _F64, _F64P]),
    "rnnwf_sr_train_steps": (C.c_int, [_P, _I32, _I64, C.c_uint64, C.c_uint64, _I64, _F64P, _I64, _F64P, _F64P, _F64P]),
    "rnnwf_log_derivatives_complex": (C.c_int, [_P, _F64P, _I64, _I64]),
    "rnnwf_sr_gram_complex": (C.c_int, [_P, _F64P, _F64P]),
    "rnnwf_sr_apply_complex": (C.c_int, [_P, _F64P, _F64P]),
    "rnnwf_sr_solve_complex": (C.c_int, [_P, _F64, _F64P]),
    "rnnwf_sr_direction_complex": (C.c_int, [_P, _F64, _F64P]),
    "rnnwf_log_derivatives_2d": (C.c_int, [_P, _F64P, _I64, _I64]),
    "rnnwf_sr_gram_2d": (C.c_int, [_P, _F64P, _F64P]),
    "rnnwf_sr_apply_2d": (C.c_int, [_P, _F64P, _F64P]),
    "rnnwf_sr_solve_2d": (C.c_int, [_P, _F64, _F64P]),
    "rnnwf_sr_direction_2d": (C.c_int, [_P, _F64, _F64P]),
    "rnnwf_lstm_gradient": (C.c_int, [_P, _I32P, _I64, _F64P]),
    "rnnwf_lstm_vmc_gradient_step": (C.c_int, [_P, _I64, _U64, _U64, _I64, _F64P, _F64P, _I32P, _F64P]),
    "rnnwf_resident_samples": (_I64, [_P]),
    "rnnwf_timing_enable": (C.c_int, [_P, _I32]),
    "rnnwf_timing_reset": (C.c_int, [_P]),
    "rnnwf_timing_get": (C.c_int, [_P, _I32, _F64P, C.POINTER(_I64), _F64P]),
    "rnnwf_engine_name": (C.c_char_p, [_P]),
    "rnnwf_synchronize": (C.c_int, [_P]),
    "rnnwf_device_info": (C.c_int, [_P, C.POINTER(_I32), C.POINTER(_I32), C.POINTER(_I64), C.c_char_p]),
}
PROTOTYPES["rnnwf_pauli_train_steps_2d"] = PROTOTYPES["rnnwf_pauli_train_steps"]       # the same argument list, one object
PROTOTYPES["rnnwf_pauli_step_stack"] = PROTOTYPES["rnnwf_pauli_step"]                  # stacked layers (docs/pauli_stack.md): likewise
PROTOTYPES["rnnwf_pauli_train_steps_stack"] = PROTOTYPES["rnnwf_pauli_train_steps"]
PROTOTYPES["rnnwf_renyi2_regions_stack"] = PROTOTYPES["rnnwf_renyi2_regions"]          # docs/renyi_stack.md
PROTOTYPES["rnnwf_pauli_step_lstm"] = PROTOTYPES["rnnwf_pauli_step"]                   # the LSTM cell (docs/pauli_lstm.md): likewise
PROTOTYPES["rnnwf_renyi2_regions_lstm"] = PROTOTYPES["rnnwf_renyi2_regions_stack"]     # docs/renyi_lstm.md
PROTOTYPES["rnnwf_correlations_lstm"] = PROTOTYPES["rnnwf_correlations"]               # docs/correlations_lstm.md
PROTOTYPES["rnnwf_lstm_pauli_gradient_step"] = (C.c_int, [_P, _I32P, _I32P, _F64P, _I32, _I64, _U64, _U64, _I64, _F64P, _F64P, _I32P, _F64P])
PROTOTYPES["rnnwf_lstm_train_steps"] = PROTOTYPES["rnnwf_train_steps"]                 # the LSTM's device-resident Adam (docs/lstm.md): likewise
PROTOTYPES["rnnwf_lstm_pauli_train_steps"] = PROTOTYPES["rnnwf_pauli_train_steps"]
for _name in ("rnnwf_log_derivatives", "rnnwf_sr_gram", "rnnwf_sr_apply", "rnnwf_sr_solve", "rnnwf_sr_direction"):
    PROTOTYPES[_name + "_lstm"] = PROTOTYPES[_name]                                    # the LSTM's minSR (docs/sr_lstm.md): likewise
PROTOTYPES["rnnwf_lstm_load_batch"] = (C.c_int, [_P, _I32P, _I64, _F64P])
PROTOTYPES["rnnwf_sr_step_lstm"] = (C.c_int, [_P, _I64, _U64, _U64, _I64, _F64P, _I64, _F64, _F64P, _F64P, _I64])

_lib = None


def load_library(path=None):
    """Load the shared library and attach the prototypes.  Raises if it is missing."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise ImportError(
            "librnnwf_hip.so not found at %s - build it with `python -m rnnwavefunctions_amd.build` "
            "(hipcc, --offload-arch=gfx950).  There is no CPU fallback." % p)
    lib = C.CDLL(p)
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(lib, name)        # AttributeError if the .so lacks a declared symbol
        fn.restype = res
        fn.argtypes = args
    if lib.rnnwf_abi_version() != ABI_VERSION:
        raise ImportError("librnnwf_hip.so ABI %d != binding ABI %d" % (lib.rnnwf_abi_version(), ABI_VERSION))
    if path is None:
        _lib = lib
    return lib


class RnnwfError(RuntimeError):
    pass


def _i32(a):
    a = np.ascontiguousarray(a, dtype=np.int32)
    return a, a.ctypes.data_as(_I32P)


def _f64(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a, a.ctypes.data_as(_F64P)


class NativeWavefunction:
    """One rnnwf_handle: a wave function resident on one MI355X."""

    def __init__(self, model, nx, ny=1, units=(10,), device=0):
        self.lib = load_library()
        cfg = Config()
        cfg.abi_version = ABI_VERSION
        cfg.model = model
        cfg.nx, cfg.ny = int(nx), int(ny)
        cfg.num_layers = len(units)
        if len(units) > MAX_LAYERS:
            raise ValueError("at most %d layers" % MAX_LAYERS)
        for i, u in enumerate(units):
            cfg.units[i] = int(u)
        cfg.device = int(device)
        h = _P()
        rc = self.lib.rnnwf_create(C.byref(cfg), C.byref(h))
        if rc != 0:
            msg = self.lib.rnnwf_last_error(None).decode()
            raise (ValueError if rc == -1 else RnnwfError)(msg)
        self.h = h
        self.model = model
        self.N = int(nx) * int(ny)
        self.nx, self.ny = int(nx), int(ny)
        self.units = tuple(int(u) for u in units)

    # -- plumbing ---------------------------------------------------------------------------------
    def _check(self, rc):
        if rc != 0:
            msg = self.lib.rnnwf_last_error(self.h).decode()
            raise (ValueError if rc == -1 else RnnwfError)(msg or "rnnwf error %d" % rc)

    def close(self):
        if getattr(self, "h", None):
            self.lib.rnnwf_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- parameters -------------------------------------------------------------------------------
    def _layout(self):
        """[(tf name without scope, element count)] in the library's order (rnnwf_param_name)."""
        lay = getattr(self, "_param_layout", None)
        if lay is None:
            lay, i, cnt = [], 0, _I64()
            while True:
                nm = self.lib.rnnwf_param_name(self.h, i, C.byref(cnt))
                if nm is None:
                    break
                lay.append((nm.decode(), int(cnt.value)))
                i += 1
            self._param_layout = lay
        return lay

    def set_params(self, params, scope=None):
        """params: {tf_name: ndarray}; names may carry the ``<scope>/`` prefix.  A complete set goes over in one call
        (rnnwf_set_params_flat: what a training loop does every iteration), a partial one tensor by tensor."""
        lay = self._layout()
        pre = scope + "/" if scope else ""
        if len(params) == len(lay) and all((pre + nm in params or nm in params) and
                                           np.size(params[pre + nm] if pre + nm in params else params[nm]) == cnt for nm, cnt in lay):
            flat = np.empty(sum(cnt for _, cnt in lay), dtype=np.float64)
            off = 0
            for nm, cnt in lay:
                v = params[pre + nm] if pre + nm in params else params[nm]
                flat[off:off + cnt] = np.asarray(v, dtype=np.float64).ravel()
                off += cnt
            self._check(self.lib.rnnwf_set_params_flat(self.h, flat.ctypes.data_as(_F64P), flat.size))
            return
        for name, v in params.items():
            if scope and name.startswith(scope + "/"):
                name = name[len(scope) + 1:]
            v = np.ascontiguousarray(v)
            if v.dtype == np.float32:
                dt = F32
            else:
                v = np.ascontiguousarray(v, dtype=np.float64)
                dt = F64
            self._check(self.lib.rnnwf_set_param(self.h, name.encode(), v.ctypes.data_as(_P), v.size, dt))
        self._check(self.lib.rnnwf_commit_params(self.h))

    def init_params(self, seed):
        """Glorot-uniform kernels, gate bias 1, other biases 0 - the values of params.init_gru_params /
        init_mdrnn_params for the same seed, generated inside the library (C callers have no NumPy)."""
        self._check(self.lib.rnnwf_init_params(self.h, int(seed)))

    def get_param(self, name, shape, dtype=np.float64):
        out = np.empty(shape, dtype=dtype)
        dt = F32 if out.dtype == np.float32 else F64
        self._check(self.lib.rnnwf_get_param(self.h, name.encode(), out.ctypes.data_as(_P), out.size, dt))
        return out

    def num_params(self):
        return int(self.lib.rnnwf_num_params(self.h))

    # -- wave function ----------------------------------------------------------------------------
    def _sample_shape(self, n):
        return (n, self.nx, self.ny) if self.model == MODEL_MDRNN2D else (n, self.N)

    def sample(self, numsamples, seed, step=0, sample_offset=0, return_log=False):
        out = np.empty(self._sample_shape(numsamples), dtype=np.int32)
        lg = np.empty(numsamples, dtype=np.float64) if return_log else None
        self._check(self.lib.rnnwf_sample(self.h, numsamples, seed, step, sample_offset, out.ctypes.data_as(_I32P),
                                          lg.ctypes.data_as(_F64P) if return_log else None))
        return (out, lg) if return_log else out

    def log_prob(self, samples):
        s, sp = _i32(samples)
        B = s.shape[0] if s.ndim > 1 else 0
        if s.ndim < 2 or int(np.prod(s.shape[1:])) != self.N:
            raise ValueError("samples must have shape (B, %d) (or (B, Nx, Ny)), got %r" % (self.N, s.shape))
        out = np.empty(B, dtype=np.float64)
        self._check(self.lib.rnnwf_log_prob(self.h, sp, B, out.ctypes.data_as(_F64P)))
        return out

    def log_amp(self, samples):
        s, sp = _i32(samples)
        if s.ndim != 2 or s.shape[1] != self.N:
            raise ValueError("samples must have shape (B, %d), got %r" % (self.N, s.shape))
        out = np.empty((s.shape[0], 2), dtype=np.float32)
        self._check(self.lib.rnnwf_log_amp(self.h, sp, s.shape[0], out.ctypes.data_as(_F32P)))
        return out.view(np.complex64)[:, 0]

    # -- estimators -------------------------------------------------------------------------------
    def tfim_eloc(self, samples, Jz, Bx, log_probs=None):
        s, sp = _i32(samples)
        ns = s.shape[0]
        if s.ndim < 2 or ns < 1 or int(np.prod(s.shape[1:])) != self.N:
            raise ValueError("samples must be non-empty with %d sites per row, got shape %r" % (self.N, s.shape))
        jz, jzp = _f64(Jz)
        if jz.size != self.N:
            raise ValueError("Jz must have %d entries, got %d" % (self.N, jz.size))
        e = np.empty(ns, dtype=np.float64)
        lpp = None
        if log_probs is not None:
            if log_probs.dtype != np.float64 or not log_probs.flags.c_contiguous or log_probs.size < (self.N + 1) * ns:
                raise ValueError("log_probs must be a contiguous float64 array of (N+1)*numsamples entries")
            lpp = log_probs.ctypes.data_as(_F64P)
        two_d = self.model in (MODEL_GRU1D_F64, MODEL_MDRNN2D, MODEL_LSTM1D_F64)
        fn = self.lib.rnnwf_tfim2d_eloc if two_d else self.lib.rnnwf_tfim_eloc
        self._check(fn(self.h, sp, ns, jzp, float(Bx), e.ctypes.data_as(_F64P), lpp))
        return e

    def j1j2_eloc(self, samples, J1, J2, Bz, periodic=False, marshall=False):
        s, sp = _i32(samples)
        if s.ndim != 2 or s.shape[1] != self.N:
            raise ValueError("samples must have shape (ns, %d), got %r" % (self.N, s.shape))
        j1, j1p = _f64(J1)
        j2, j2p = _f64(J2)
        bz, bzp = _f64(Bz)
        if not (j1.size == j2.size == bz.size == self.N):
            raise ValueError("J1, J2, Bz must have %d entries" % self.N)
        e = np.empty((s.shape[0], 2), dtype=np.float32)
        ncon = _I64(0)
        self._check(self.lib.rnnwf_j1j2_eloc(self.h, sp, s.shape[0], j1p, j2p, bzp, int(bool(periodic)),
                                             int(bool(marshall)), e.ctypes.data_as(_F32P), C.byref(ncon)))
        return e.view(np.complex64)[:, 0], int(ncon.value)

    def vmc_step(self, numsamples, seed, step, couplings, sample_offset=0, want_samples=False, want_eloc=False):
        """Fused sample + local energies + moments.  Returns dict(moments=(4,), samples=?, eloc=?)."""
        c, cp = _f64(couplings)
        mom = np.zeros(4, dtype=np.float64)
        smp = np.empty(self._sample_shape(numsamples), dtype=np.int32) if want_samples else None
        if want_eloc:
            el = np.empty((numsamples, 2), dtype=np.float32) if self.model == MODEL_CRNN_U1 else \
                np.empty(numsamples, dtype=np.float64)
        else:
            el = None
        self._check(self.lib.rnnwf_vmc_step(self.h, numsamples, seed, step, sample_offset, cp, c.size,
                                            smp.ctypes.data_as(_I32P) if want_samples else None,
                                            el.ctypes.data_as(_P) if want_eloc else None, mom.ctypes.data_as(_F64P)))
        out = {"moments": mom}
        if want_samples:
            out["samples"] = smp
        if want_eloc:
            out["eloc"] = el.view(np.complex64)[:, 0] if self.model == MODEL_CRNN_U1 else el
        return out

    def load_batch(self, samples, eloc):
        """Make a caller-supplied batch (samples + their local energies) the one vmc_gradient works on."""
        s = np.ascontiguousarray(samples, dtype=np.int32)
        ns = s.shape[0]
        if self.model == MODEL_CRNN_U1:
            e = np.ascontiguousarray(np.asarray(eloc, dtype=np.complex64))
        else:
            e = np.ascontiguousarray(np.asarray(eloc, dtype=np.float64))
        if e.shape != (ns,):
            raise ValueError("load_batch: %d samples but local energies of shape %s" % (ns, e.shape))
        self._check(self.lib.rnnwf_load_batch(self.h, s.ctypes.data_as(_I32P), ns, e.ctypes.data_as(_P)))

    # -- gradient of the VMC cost -----------------------------------------------------------------
    def vmc_gradient(self, mean_energy, norm, shapes, allreduce=False):
        """Gradient of the reference's cost on the batch of the last vmc_step (mean_energy may be complex for
        the complex RNN).  shapes: {tf_name (without scope): shape}; returns {tf_name: float64 ndarray}."""
        me = complex(mean_energy)
        self._check(self.lib.rnnwf_vmc_gradient(self.h, me.real, me.imag, float(norm)))
        if allreduce:
            self._check(self.lib.rnnwf_allreduce_grads(self.h))
        lay = self._layout()
        if len(shapes) == len(lay) and all(nm in shapes and int(np.prod(shapes[nm], dtype=np.int64)) == cnt for nm, cnt in lay):
            flat = np.empty(sum(cnt for _, cnt in lay), dtype=np.float64)          # every tensor in one call
            self._check(self.lib.rnnwf_get_grads_flat(self.h, flat.ctypes.data_as(_F64P), flat.size))
            out, off = {}, 0
            for nm, cnt in lay:
                out[nm] = flat[off:off + cnt].reshape(shapes[nm])
                off += cnt
            return {name: out[name] for name in shapes}
        out = {}
        for name, shape in shapes.items():
            g = np.empty(shape, dtype=np.float64)
            self._check(self.lib.rnnwf_get_grad(self.h, name.encode(), g.ctypes.data_as(_P), g.size, F64))
            out[name] = g
        return out

    # -- gradient of the LSTM wave function (docs/lstm.md, "Gradient") ----------------------------
    def _grads(self, shapes):
        """{tf_name: float64 ndarray} of the gradient the library holds, every tensor of `shapes` in one call"""
        lay = self._layout()
        if not (len(shapes) == len(lay) and all(nm in shapes and int(np.prod(shapes[nm], dtype=np.int64)) == cnt for nm, cnt in lay)):
            raise ValueError("shapes must name every tensor of the model with its shape: %r" % ([nm for nm, _ in lay],))
        flat = np.empty(sum(cnt for _, cnt in lay), dtype=np.float64)
        self._check(self.lib.rnnwf_get_grads_flat(self.h, flat.ctypes.data_as(_F64P), flat.size))
        out, off = {}, 0
        for nm, cnt in lay:
            out[nm] = flat[off:off + cnt].reshape(shapes[nm])
            off += cnt
        return {name: out[name] for name in shapes}

    def lstm_gradient(self, samples, weights, shapes, allreduce=False):
        """d/dtheta sum_s weights[s] log P(samples[s]) of the LSTM wave function (rnnwf_lstm_gradient).  samples (B, N) or
        (B, Nx, Ny), weights (B,); shapes: {tf_name (without scope): shape}; returns {tf_name: float64 ndarray}.  With
        weights = (E - mean E) / B it is the gradient of the reference's cost; allreduce=True sums it over the communicator."""
        s, sp = _i32(samples)
        if s.ndim < 2 or s.shape[0] < 1 or int(np.prod(s.shape[1:])) != self.N:
            raise ValueError("samples must be non-empty with %d sites per row, got shape %r" % (self.N, s.shape))
        w, wp = _f64(weights)
        if w.shape != (s.shape[0],):
            raise ValueError("lstm_gradient: %d samples but weights of shape %r" % (s.shape[0], w.shape))
        self._check(self.lib.rnnwf_lstm_gradient(self.h, sp, s.shape[0], wp))
        if allreduce:
            self._check(self.lib.rnnwf_allreduce_grads(self.h))
        return self._grads(shapes)

    def lstm_vmc_gradient_step(self, numsamples, seed, step, couplings, shapes, sample_offset=0, want_samples=False, want_eloc=False):
        """vmc_step and the gradient of the reference's cost on its batch in one call with one host synchronisation
        (rnnwf_lstm_vmc_gradient_step; single process).  couplings: Jz (N) then Bx.  Returns dict(moments=(4,), grads={tf_name:
        float64 ndarray}, samples=?, eloc=?); moments, samples and eloc are vmc_step's bit for bit."""
        c, cp = _f64(couplings)
        if c.shape != (self.N + 1,):
            raise ValueError("lstm_vmc_gradient_step: couplings must hold Jz (%d) then Bx, got shape %r" % (self.N, c.shape))
        mom = np.zeros(4, dtype=np.float64)
        smp = np.empty((numsamples, self.N), dtype=np.int32) if want_samples else None
        el = np.empty(numsamples, dtype=np.float64) if want_eloc else None
        self._check(self.lib.rnnwf_lstm_vmc_gradient_step(self.h, numsamples, seed, step, sample_offset, cp, mom.ctypes.data_as(_F64P),
                                                          smp.ctypes.data_as(_I32P) if want_samples else None,
                                                          el.ctypes.data_as(_F64P) if want_eloc else None))
        out = {"moments": mom, "grads": self._grads(shapes)}
        if want_samples:
            out["samples"] = smp
        if want_eloc:
            out["eloc"] = el
        return out

    # -- stochastic reconfiguration: rnnwf_log_derivatives, rnnwf_sr_* (docs/sr.md) ---------------
    def set_params_flat(self, flat):
        """Every tensor in one float64 vector in the order of _layout() (rnnwf_set_params_flat); commits."""
        f, fp = _f64(np.ravel(flat))
        self._check(self.lib.rnnwf_set_params_flat(self.h, fp, f.size))

    def resident_samples(self):
        """samples of the batch the last vmc_step / load_batch left on the device, 0 without one (rnnwf_resident_samples)"""
        return int(self.lib.rnnwf_resident_samples(self.h))

    def _sr_rows(self, suffix):
        """rows of the minSR system on the resident batch: one per sample, two (real, imaginary) for the complex RNN"""
        return (2 if suffix == "_complex" else 1) * self.resident_samples()

    def _log_derivatives(self, suffix):
        ns, n = self.resident_samples(), self.num_params()
        out = np.empty((2, ns, n) if suffix == "_complex" else (ns, n), dtype=np.float64)
        self._check(getattr(self.lib, "rnnwf_log_derivatives" + suffix)(self.h, out.ctypes.data_as(_F64P), ns, n))
        return out[0] + 1j * out[1] if suffix == "_complex" else out

    def _sr_gram(self, suffix):
        n = self._sr_rows(suffix)
        gram, eps = np.empty((n, n), dtype=np.float64), np.empty(n, dtype=np.float64)
        self._check(getattr(self.lib, "rnnwf_sr_gram" + suffix)(self.h, gram.ctypes.data_as(_F64P), eps.ctypes.data_as(_F64P)))
        return gram, eps

    def _sr_apply(self, suffix, y):
        yv, yp = _f64(y)
        n = self._sr_rows(suffix)
        if n > 0 and yv.shape != (n,):
            raise ValueError("sr_apply%s: y must have shape (%d,), %s per sample of the resident batch, got %r"
                             % (suffix, n, "two entries" if suffix == "_complex" else "one entry", yv.shape))
        out = np.empty(self.num_params(), dtype=np.float64)
        self._check(getattr(self.lib, "rnnwf_sr_apply" + suffix)(self.h, yp if n > 0 else None, out.ctypes.data_as(_F64P)))
        return out

    def _sr_solve(self, suffix, diag_shift):
        y = np.empty(self._sr_rows(suffix), dtype=np.float64)
        self._check(getattr(self.lib, "rnnwf_sr_solve" + suffix)(self.h, float(diag_shift), y.ctypes.data_as(_F64P)))
        return y

    def _sr_direction(self, suffix, diag_shift):
        out = np.empty(self.num_params(), dtype=np.float64)
        self._check(getattr(self.lib, "rnnwf_sr_direction" + suffix)(self.h, float(diag_shift), out.ctypes.data_as(_F64P)))
        return out

    def log_derivatives(self):
        """(ns, num_params) float64: O[s, k] = d log psi(sigma_s) / d theta_k = 1/2 d log P / d theta_k on the resident batch of the
        last vmc_step / load_batch, theta in the flat order of _layout()."""
        return self._log_derivatives("")

    def sr_gram(self):
        """(gram, eps): the centred Gram matrix dO dO^T (ns, ns) and eps = E_loc - mean E (ns,) of the resident batch, float64;
        gram is exactly symmetric."""
        return self._sr_gram("")

    def sr_apply(self, y):
        """(num_params,) float64: dO^T y for y of one entry per sample of the resident batch, in the flat order of _layout()."""
        return self._sr_apply("", y)

    def sr_solve(self, diag_shift):
        """(ns,) float64: y of (dO dO^T + ns diag_shift I) y = eps on the resident batch, factorised and solved on the device
        (rnnwf_sr_solve); y is not centred."""
        return self._sr_solve("", diag_shift)

    def sr_direction(self, diag_shift):
        """(num_params,) float64: the minSR direction dO^T (dO dO^T + ns diag_shift I)^-1 eps of the resident batch, everything on
        the device (rnnwf_sr_direction), in the flat order of _layout()."""
        return self._sr_direction("", diag_shift)

    def sr_train_steps(self, K, numsamples, seed, step0, couplings, learning_rates, diag_shifts, sample_offset=0):
        """K whole minSR iterations (sample, local energies, Jacobian, Gram matrix, solve, theta -= lr delta, re-pack of the weight
        images) on the device with one host synchronisation (rnnwf_sr_train_steps); iteration k draws with step index step0 + k.
        learning_rates and diag_shifts: one value per iteration, or a scalar for all K.  Returns the (K, 4) moments of the K batches."""
        K = int(K)
        c, cp = _f64(couplings)
        lr, lrp = _f64(np.broadcast_to(np.asarray(learning_rates, dtype=np.float64), (max(K, 0),)))
        lam, lamp = _f64(np.broadcast_to(np.asarray(diag_shifts, dtype=np.float64), (max(K, 0),)))
        mom = np.empty((max(K, 0), 4), dtype=np.float64)
        self._check(self.lib.rnnwf_sr_train_steps(self.h, K, int(numsamples), seed, step0, sample_offset, cp, c.size, lrp, lamp,
                                                  mom.ctypes.data_as(_F64P)))
        return mom

    # -- stochastic reconfiguration for the complex RNN: rnnwf_*_complex (docs/sr_complex.md) ------
    def log_derivatives_complex(self):
        """(ns, num_params) complex128: O[s, k] = d log psi(sigma_s) / d theta_k = 1/2 d log P / d theta_k + i d phi / d theta_k on the
        resident batch, theta (real) in the flat order of _layout()."""
        return self._log_derivatives("_complex")

    def sr_gram_complex(self):
        """(gram, eps): Obar Obar^T (2 ns, 2 ns) for Obar = [Re dO ; Im dO] and eps = [Re (E_loc - mean E) ; Im (E_loc - mean E)]
        (2 ns,) of the resident batch, float64, each half centred with its own mean; gram is exactly symmetric."""
        return self._sr_gram("_complex")

    def sr_apply_complex(self, y):
        """(num_params,) float64: Obar^T y for y (2 ns,) = [weights of the real rows ; weights of the imaginary rows]."""
        return self._sr_apply("_complex", y)

    def sr_solve_complex(self, diag_shift):
        """(2 ns,) float64: y of (Obar Obar^T + ns diag_shift I) y = eps, factorised and solved on the device; y is not centred."""
        return self._sr_solve("_complex", diag_shift)

    def sr_direction_complex(self, diag_shift):
        """(num_params,) float64: the minSR direction Obar^T (Obar Obar^T + ns diag_shift I)^-1 eps of the resident batch, everything
        on the device (rnnwf_sr_direction_complex), in the flat order of _layout()."""
        return self._sr_direction("_complex", diag_shift)

    # -- stochastic reconfiguration for the 2D RNN: rnnwf_*_2d (docs/sr_2d.md) ----------------------
    def log_derivatives_2d(self):
        """(ns, num_params) float64: O[s, k] = 1/2 d log P(sigma_s) / d theta_k on the resident batch of the 2D RNN, theta in the flat
        order of _layout()."""
        return self._log_derivatives("_2d")

    def sr_gram_2d(self):
        """(gram, eps): the centred Gram matrix dO dO^T (ns, ns) and eps = E_loc - mean E (ns,) of the resident batch of the 2D RNN,
        float64; gram is exactly symmetric."""
        return self._sr_gram("_2d")

    def sr_apply_2d(self, y):
        """(num_params,) float64: dO^T y for y of one entry per sample of the resident batch of the 2D RNN."""
        return self._sr_apply("_2d", y)

    def sr_solve_2d(self, diag_shift):
        """(ns,) float64: y of (dO dO^T + ns diag_shift I) y = eps, factorised and solved on the device; y is not centred."""
        return self._sr_solve("_2d", diag_shift)

    def sr_direction_2d(self, diag_shift):
        """(num_params,) float64: the minSR direction dO^T (dO dO^T + ns diag_shift I)^-1 eps of the resident batch of the 2D RNN,
        everything on the device (rnnwf_sr_direction_2d), in the flat order of _layout()."""
        return self._sr_direction("_2d", diag_shift)

    # -- stochastic reconfiguration for the LSTM wave function: rnnwf_*_lstm (docs/sr_lstm.md) ------
    def lstm_load_batch(self, samples, eloc):
        """load_batch for the LSTM wave function (rnnwf_lstm_load_batch): samples (ns, N) or (ns, Nx, Ny) and their local energies
        (ns,) float64 become the resident batch the *_lstm calls below work on."""
        s, sp = _i32(samples)
        if s.ndim < 2 or s.shape[0] < 1 or int(np.prod(s.shape[1:])) != self.N:
            raise ValueError("samples must be non-empty with %d sites per row, got shape %r" % (self.N, s.shape))
        e, ep = _f64(eloc)
        if e.shape != (s.shape[0],):
            raise ValueError("lstm_load_batch: %d samples but local energies of shape %r" % (s.shape[0], e.shape))
        self._check(self.lib.rnnwf_lstm_load_batch(self.h, sp, s.shape[0], ep))

    def sr_step_lstm(self, numsamples, seed, step, couplings, diag_shift, sample_offset=0):
        """One minSR iteration's device work with one host synchronisation (rnnwf_sr_step_lstm; single process): vmc_step's fused
        step - couplings: Jz (N) then Bx - and the minSR direction of sr_direction_lstm on its batch, which stays resident with its
        Jacobian.  Returns dict(moments=(4,), direction=(num_params,)): moments are vmc_step's bit for bit, direction is what
        lstm_load_batch of that step's samples and energies followed by sr_direction_lstm returns, bit for bit."""
        c, cp = _f64(couplings)
        mom = np.zeros(4, dtype=np.float64)
        out = np.empty(self.num_params(), dtype=np.float64)
        self._check(self.lib.rnnwf_sr_step_lstm(self.h, int(numsamples), int(seed), int(step), int(sample_offset), cp, c.size,
                                                float(diag_shift), mom.ctypes.data_as(_F64P), out.ctypes.data_as(_F64P), out.size))
        return {"moments": mom, "direction": out}

    def log_derivatives_lstm(self):
        """(ns, num_params) float64: O[s, k] = 1/2 d log P(sigma_s) / d theta_k on the resident batch of the LSTM wave function
        (lstm_load_batch / sr_step_lstm), theta in the flat order of _layout()."""
        return self._log_derivatives("_lstm")

    def sr_gram_lstm(self):
        """(gram, eps): the centred Gram matrix dO dO^T (ns, ns) and eps = E_loc - mean E (ns,) of the resident batch of the LSTM
        wave function, float64; gram is exactly symmetric."""
        return self._sr_gram("_lstm")

    def sr_apply_lstm(self, y):
        """(num_params,) float64: dO^T y for y of one entry per sample of the resident batch of the LSTM wave function."""
        return self._sr_apply("_lstm", y)

    def sr_solve_lstm(self, diag_shift):
        """(ns,) float64: y of (dO dO^T + ns diag_shift I) y = eps, factorised and solved on the device; y is not centred."""
        return self._sr_solve("_lstm", diag_shift)

    def sr_direction_lstm(self, diag_shift):
        """(num_params,) float64: the minSR direction dO^T (dO dO^T + ns diag_shift I)^-1 eps of the resident batch of the LSTM wave
        function, everything on the device (rnnwf_sr_direction_lstm), in the flat order of _layout()."""
        return self._sr_direction("_lstm", diag_shift)

    # -- device-resident training iteration (rnnwf_train_steps; single-layer float32 GRU models) ------------------
    def device_training_supported(self):
        return bool(self.lib.rnnwf_device_training_supported(self.h))

    def train_steps(self, numsamples, seed, step0, couplings, learning_rates, beta1=0.9, beta2=0.999, epsilon=1e-8, sample_offset=0):
        """len(learning_rates) whole iterations (sample, local energies, gradient, Adam update, re-pack of the weight images) on
        the device with one host synchronisation; returns the (K, 4) moments of the K batches."""
        c, cp = _f64(couplings)
        lr, lrp = _f64(np.atleast_1d(learning_rates))
        mom = np.empty((lr.size, 4), dtype=np.float64)
        self._check(self.lib.rnnwf_train_steps(self.h, lr.size, numsamples, seed, step0, sample_offset, cp, c.size, lrp,
                                               float(beta1), float(beta2), float(epsilon), mom.ctypes.data_as(_F64P)))
        return mom

    def lstm_train_steps(self, numsamples, seed, step0, couplings, learning_rates, beta1=0.9, beta2=0.999, epsilon=1e-8, sample_offset=0):
        """train_steps for the LSTM wave function (rnnwf_lstm_train_steps; model LSTM1D_F64, single process): len(learning_rates)
        whole iterations of the host loop - lstm_vmc_gradient_step at step index step0 + k, training.Adam with learning_rates[k],
        set_params - on the device with one host synchronisation, bit for bit.  Returns the (K, 4) moments of the K batches; get_param
        returns the trained values, adam_get_state / adam_set_state the optimizer's."""
        c, cp = _f64(couplings)
        lr, lrp = _f64(np.atleast_1d(learning_rates))
        mom = np.empty((lr.size, 4), dtype=np.float64)
        self._check(self.lib.rnnwf_lstm_train_steps(self.h, lr.size, int(numsamples), int(seed), int(step0), int(sample_offset), cp, c.size, lrp,
                                                    float(beta1), float(beta2), float(epsilon), mom.ctypes.data_as(_F64P)))
        return mom

    def adam_step(self, learning_rate, beta1=0.9, beta2=0.999, epsilon=1e-8):
        """One Adam update on the device from the gradient of the last vmc_gradient, then the images' re-pack."""
        self._check(self.lib.rnnwf_adam_step(self.h, float(learning_rate), float(beta1), float(beta2), float(epsilon)))

    def adam_get_state(self):
        """(m_flat, v_flat, t): Adam's moments in the flat order of _layout() and the number of updates applied."""
        n = self.num_params()
        m, v, t = np.empty(n), np.empty(n), _I64(0)
        self._check(self.lib.rnnwf_adam_get_state(self.h, m.ctypes.data_as(_F64P), v.ctypes.data_as(_F64P), n, C.byref(t)))
        return m, v, int(t.value)

    def adam_set_state(self, m_flat, v_flat, t):
        if m_flat is None:
            self._check(self.lib.rnnwf_adam_set_state(self.h, None, None, self.num_params(), int(t)))
            return
        m, mp = _f64(m_flat)
        v, vp = _f64(v_flat)
        self._check(self.lib.rnnwf_adam_set_state(self.h, mp, vp, m.size, int(t)))

    def get_params_dict(self, like, scope=None):
        """{name: array} with the names, shapes and dtypes of `like`, read back from the library (after device-resident updates)."""
        pre = scope + "/" if scope else ""
        out = type(like)()
        for k, v in like.items():
            nm = k[len(pre):] if pre and k.startswith(pre) else k
            out[k] = self.get_param(nm, v.shape, v.dtype)
        return out

    def _chain_samples(self, samples, rows, rows_name):
        """(int32 array, pointer) of the caller's samples for an observable pass over `rows` chains, (None, None) for a device draw"""
        if samples is None:
            return None, None
        s, sp = _i32(samples)
        if s.ndim < 2 or s.shape[0] != rows or int(np.prod(s.shape[1:])) != self.N:
            raise ValueError("samples must have shape (%s, %d) = (%d, %d), got %r" % (rows_name, self.N, rows, self.N, s.shape))
        return s, sp

    # -- entanglement -----------------------------------------------------------------------------
    def renyi2_swap(self, npairs, samples=None, seed=0, step=0, pair_offset=0, want_log_ratio=False, want_samples=False):
        """Swap-trick sums of the second Renyi entropy for every cut l = 0..N (rnnwf_renyi2_swap).  samples: (2 npairs, N)
        int32, pair p = rows 2p, 2p + 1; None: drawn on the device as sample(2 npairs, seed, step, 2 pair_offset) draws them.
        Returns dict(sums=(N+1, 2) [sum r_l, sum r_l^2], log_ratio=(N+1, npairs)?, samples=(2 npairs, N)?)."""
        npairs = int(npairs)
        s, sp = self._chain_samples(samples, 2 * npairs, "2*npairs")
        sums = np.empty((self.N + 1, 2), dtype=np.float64)
        lr = np.empty((self.N + 1, max(npairs, 0)), dtype=np.float64) if want_log_ratio else None
        smp = np.empty((2 * max(npairs, 0), self.N), dtype=np.int32) if want_samples and samples is None else None
        self._check(self.lib.rnnwf_renyi2_swap(self.h, sp, npairs, int(seed), int(step), int(pair_offset), sums.ctypes.data_as(_F64P),
                                               lr.ctypes.data_as(_F64P) if lr is not None else None,
                                               smp.ctypes.data_as(_I32P) if smp is not None else None))
        out = {"sums": sums}
        if want_log_ratio:
            out["log_ratio"] = lr
        if want_samples:
            out["samples"] = smp if smp is not None else s
        return out

    def renyi2_regions(self, regions, numpairs, samples=None, seed=111, step=0, pair_offset=0, log_ratio=False):
        """Swap-trick sums of the second Renyi entropy of arbitrary regions (rnnwf_renyi2_regions).  regions: (R, N) masks of
        0 / 1 (or one mask of N entries), 1 = site in A, sites in the model's order.  samples: (2 numpairs, N) int32, pair p =
        rows 2p, 2p + 1; None: drawn on the device as sample(2 numpairs, seed, step, 2 pair_offset) draws them.  Returns
        dict(sums=(R, 2) [sum r_A, sum r_A^2], samples=(2 numpairs, N) when drawn, log_ratio=(R, numpairs) when asked)."""
        return self._regions_call("rnnwf_renyi2_regions", regions, numpairs, samples, seed, step, pair_offset, log_ratio)

    def renyi2_regions_stack(self, regions, numpairs, samples=None, seed=111, step=0, pair_offset=0, log_ratio=False):
        """renyi2_regions for stacked GRU layers (rnnwf_renyi2_regions_stack, docs/renyi_stack.md): models GRU1D and GRU1D_F64 with
        2..4 layers.  Arguments, shape checks and returns are renyi2_regions's."""
        return self._regions_call("rnnwf_renyi2_regions_stack", regions, numpairs, samples, seed, step, pair_offset, log_ratio)

    def renyi2_regions_lstm(self, regions, numpairs, samples=None, seed=111, step=0, pair_offset=0, log_ratio=False):
        """renyi2_regions for the LSTM wave function (rnnwf_renyi2_regions_lstm, docs/renyi_lstm.md): model LSTM1D_F64.  regions:
        (R, N) masks indexed by the chain position, the column of samples (2 numpairs, N), or any (R, ...) with N entries - (R, Nx, Ny)
        in the shape pauli_step_lstm accepts samples in.  samples: (2 numpairs, N) or (2 numpairs, Nx, Ny) int32, flattened in C order.
        Returns what renyi2_regions returns; no batch stays resident."""
        return self._regions_call("rnnwf_renyi2_regions_lstm", regions, numpairs, samples, seed, step, pair_offset, log_ratio)

    def _regions_call(self, entry, regions, numpairs, samples, seed, step, pair_offset, log_ratio, masks="any", lattice_draw=False, cplx=False):
        """The argument checks, buffers and result dict of the five renyi2_regions methods.  masks: which shapes of `regions` besides
        (R, N) and (N,) pass - "any": every (R, ...) with N entries per region; "lattice": (R, Nx, Ny); "flat": none.  lattice_draw:
        drawn samples come back as (2 numpairs, Nx, Ny).  cplx: sums (R, 4), complex log_ratio and the in_sector output."""
        npairs = int(numpairs)
        reg = np.asarray(regions)
        if reg.ndim == 1:
            reg = reg[None, :]
        if masks == "any":
            ok = reg.ndim >= 2 and int(np.prod(reg.shape[1:])) == self.N
        else:
            if masks == "lattice" and reg.ndim == 3 and reg.shape[1:] == (self.nx, self.ny):
                reg = reg.reshape(reg.shape[0], self.N)
            ok = reg.ndim == 2 and reg.shape[1] == self.N
        if not ok or reg.shape[0] < 1:
            if masks == "lattice":
                raise ValueError("regions must have shape (nregions >= 1, %d) or (nregions >= 1, %d, %d), got %r"
                                 % (self.N, self.nx, self.ny, reg.shape))
            raise ValueError("regions must have shape (nregions >= 1, %d), got %r" % (self.N, reg.shape))
        if not np.all(reg == reg.astype(np.int32)):
            raise ValueError("regions must hold the integers 0 and 1")
        reg, rp = _i32(reg.reshape(reg.shape[0], self.N))
        R = reg.shape[0]
        s, sp = self._chain_samples(samples, 2 * npairs, "2*numpairs")
        sums = np.empty((R, 4 if cplx else 2), dtype=np.float64)
        ins = np.empty(R, dtype=np.int64) if cplx else None
        lr = np.empty((R, max(npairs, 0)), dtype=np.complex128 if cplx else np.float64) if log_ratio else None
        smp = np.empty((2 * max(npairs, 0),) + ((self.nx, self.ny) if lattice_draw else (self.N,)), dtype=np.int32) if samples is None else None
        outputs = [sums.ctypes.data_as(_F64P), lr.ctypes.data_as(_F64P) if lr is not None else None]
        if cplx:
            outputs.append(ins.ctypes.data_as(C.POINTER(C.c_int64)))
        outputs.append(smp.ctypes.data_as(_I32P) if smp is not None else None)
        self._check(getattr(self.lib, entry)(self.h, rp, R, sp, npairs, int(seed), int(step), int(pair_offset), *outputs))
        out = {"sums": sums}
        if cplx:
            out["in_sector"] = ins
        if smp is not None:
            out["samples"] = smp
        if log_ratio:
            out["log_ratio"] = lr
        return out

    def renyi2_regions_2d(self, regions, numpairs, samples=None, seed=111, step=0, pair_offset=0, log_ratio=False):
        """renyi2_regions for the 2D RNN (rnnwf_renyi2_regions_2d).  regions: (R, Nx*Ny) masks of 0 / 1 indexed by the lattice index
        nx*Ny + ny, the C-order flattening of samples (2 numpairs, Nx, Ny), or (R, Nx, Ny), or one mask of Nx*Ny entries.  samples:
        (2 numpairs, Nx, Ny) or (2 numpairs, Nx*Ny) int32, pair p = rows 2p, 2p + 1; None: drawn on the device as sample(2 numpairs,
        seed, step, 2 pair_offset) draws them.  Returns dict(sums=(R, 2) [sum r_A, sum r_A^2], samples=(2 numpairs, Nx, Ny) when
        drawn, log_ratio=(R, numpairs) when asked)."""
        return self._regions_call("rnnwf_renyi2_regions_2d", regions, numpairs, samples, seed, step, pair_offset, log_ratio, masks="lattice",
                                  lattice_draw=True)

    def renyi2_regions_complex(self, regions, numpairs, samples=None, seed=111, step=0, pair_offset=0, log_ratio=False):
        """renyi2_regions for the complex RNN (rnnwf_renyi2_regions_complex).  regions: (R, N) masks of 0 / 1 (or one mask of N
        entries), 1 = site in A.  samples: (2 numpairs, N) int32 of the zero-magnetisation sector, pair p = rows 2p, 2p + 1; None:
        drawn on the device as sample(2 numpairs, seed, step, 2 pair_offset) draws them.  Returns dict(sums=(R, 4) [sum Re r, sum
        Im r, sum (Re r)^2, sum (Im r)^2], in_sector=(R,) int64 surviving pairs, samples=(2 numpairs, N) when drawn,
        log_ratio=(R, numpairs) complex128 when asked, -inf + 0j for a pair whose mixed chains leave the sector)."""
        return self._regions_call("rnnwf_renyi2_regions_complex", regions, numpairs, samples, seed, step, pair_offset, log_ratio, masks="flat",
                                  cplx=True)

    # -- correlation functions --------------------------------------------------------------------
    def correlations(self, ns, samples=None, seed=0, step=0, sample_offset=0, want_log_ratio=False, want_samples=False):
        """Sums of the diagonal and off-diagonal two-point functions over ns chains (rnnwf_correlations).  samples: (ns, N) int32;
        None: drawn on the device as sample(ns, seed, step, sample_offset) draws them.  Returns dict(z_sums=(N,), zz_sums=(N, N),
        x_sums=(N, 2), xx_sums=(N, N, 5), log_ratio=(N + N(N-1)/2, ns)?, samples=(ns, N)?); see include/rnnwf.h for the entries."""
        return self._correlations_call("rnnwf_correlations", ns, samples, seed, step, sample_offset, want_log_ratio, want_samples)

    def correlations_lstm(self, ns, samples=None, seed=0, step=0, sample_offset=0, want_log_ratio=False, want_samples=False):
        """correlations for the LSTM wave function (rnnwf_correlations_lstm, docs/correlations_lstm.md): model LSTM1D_F64.  Sites are
        the chain position, the column of samples (ns, N).  samples: (ns, N) or (ns, Nx, Ny) int32, as pauli_step_lstm takes them;
        None: drawn on the device as sample(ns, seed, step, sample_offset) draws them.  Returns what correlations returns; a batch of
        lstm_load_batch does not survive the call."""
        return self._correlations_call("rnnwf_correlations_lstm", ns, samples, seed, step, sample_offset, want_log_ratio, want_samples)

    def _correlations_call(self, entry, ns, samples, seed, step, sample_offset, want_log_ratio, want_samples):
        """the buffers and result dict the two correlations methods share"""
        ns = int(ns)
        N = self.N
        s, sp = self._chain_samples(samples, ns, "ns")
        z, zz = np.empty(N, dtype=np.float64), np.empty((N, N), dtype=np.float64)
        x, xx = np.empty((N, 2), dtype=np.float64), np.empty((N, N, 5), dtype=np.float64)
        lr = np.empty((N + N * (N - 1) // 2, max(ns, 0)), dtype=np.float64) if want_log_ratio else None
        smp = np.empty((max(ns, 0), N), dtype=np.int32) if want_samples and samples is None else None
        self._check(getattr(self.lib, entry)(self.h, sp, ns, int(seed), int(step), int(sample_offset), z.ctypes.data_as(_F64P),
                                             zz.ctypes.data_as(_F64P), x.ctypes.data_as(_F64P), xx.ctypes.data_as(_F64P),
                                             lr.ctypes.data_as(_F64P) if lr is not None else None,
                                             smp.ctypes.data_as(_I32P) if smp is not None else None))
        out = {"z_sums": z, "zz_sums": zz, "x_sums": x, "xx_sums": xx}
        if want_log_ratio:
            out["log_ratio"] = lr
        if want_samples:
            out["samples"] = smp if smp is not None else s
        return out

    # -- Pauli strings and arbitrary spin Hamiltonians ----------------------------------------------
    def pauli_step(self, flip, sign, coeff, ns, samples=None, seed=0, step=0, sample_offset=0, want_eloc=False, want_log_ratio=False,
                   want_samples=False):
        """Per-term sums and the local energy of terms (prod_sign sz)(prod_flip sx) (rnnwf_pauli_step).  flip, sign: (K, N) masks of
        0 / 1 (or one term of N entries), coeff: (K,).  samples: (ns, N) int32; None: drawn on the device as sample(ns, seed, step,
        sample_offset) draws them.  Returns dict(term_sums=(K, 2) [sum v_k, sum v_k^2], moments=(4,), eloc=(ns,)?,
        log_ratio=(distinct non-empty flip masks in order of first appearance, ns)?, samples=(ns, N)?).  A call that fits one pass
        leaves its batch resident for vmc_gradient."""
        return self._pauli_call("rnnwf_pauli_step", False, (max(int(ns), 0), self.N), flip, sign, coeff, ns, samples, seed, step,
                                sample_offset, want_eloc, want_log_ratio, want_samples)

    def pauli_step_2d(self, flip, sign, coeff, ns, samples=None, seed=0, step=0, sample_offset=0, want_eloc=False,
                      want_log_ratio=False, want_samples=False):
        """pauli_step for the 2D RNN (rnnwf_pauli_step_2d).  flip, sign: (K, Nx*Ny) masks indexed by the lattice index nx*Ny + ny, the
        C-order flattening of samples (ns, Nx, Ny), or (K, Nx, Ny).  samples: (ns, Nx, Ny) or (ns, Nx*Ny) int32; None: drawn on the
        device as sample(ns, seed, step, sample_offset) draws them, and returned as (ns, Nx, Ny).  Returns what pauli_step returns."""
        return self._pauli_call("rnnwf_pauli_step_2d", False, (max(int(ns), 0), self.nx, self.ny), *self._lattice_masks(flip, sign), coeff, ns,
                                samples, seed, step, sample_offset, want_eloc, want_log_ratio, want_samples)

    def pauli_step_stack(self, flip, sign, coeff, ns, samples=None, seed=0, step=0, sample_offset=0, want_eloc=False,
                         want_log_ratio=False, want_samples=False):
        """pauli_step for stacked GRU layers (rnnwf_pauli_step_stack, docs/pauli_stack.md): models GRU1D and GRU1D_F64 with 2..4
        layers.  Arguments and the returned dict are pauli_step's."""
        return self._pauli_call("rnnwf_pauli_step_stack", False, (max(int(ns), 0), self.N), flip, sign, coeff, ns, samples, seed, step,
                                sample_offset, want_eloc, want_log_ratio, want_samples)

    def pauli_step_lstm(self, flip, sign, coeff, ns, samples=None, seed=0, step=0, sample_offset=0, want_eloc=False,
                        want_log_ratio=False, want_samples=False):
        """pauli_step for the LSTM wave function (rnnwf_pauli_step_lstm, docs/pauli_lstm.md): model LSTM1D_F64.  flip, sign: (K, N)
        masks indexed by the chain position, the column of samples (ns, N), or (K, Nx, Ny) in the shape lstm_gradient accepts samples
        in.  samples: (ns, N) or (ns, Nx, Ny) int32; None: drawn on the device as sample(ns, seed, step, sample_offset) draws them.
        Returns what pauli_step returns; no batch stays resident."""
        return self._pauli_call("rnnwf_pauli_step_lstm", False, (max(int(ns), 0), self.N), *self._lattice_masks(flip, sign), coeff, ns,
                                samples, seed, step, sample_offset, want_eloc, want_log_ratio, want_samples)

    def lstm_pauli_gradient_step(self, flip, sign, coeff, numsamples, seed, step, shapes, sample_offset=0, want_samples=False,
                                 want_eloc=False):
        """One pass of pauli_step_lstm on numsamples drawn samples and the gradient of the VMC cost of the Hamiltonian
        sum_k coeff_k (prod_sign sz)(prod_flip sx) on its batch, in one call with one host synchronisation
        (rnnwf_lstm_pauli_gradient_step; single process).  Returns dict(moments=(4,), grads={tf_name: float64 ndarray},
        term_sums=(K, 2), samples=(numsamples, N)?, eloc=(numsamples,)?); moments, term_sums, samples and eloc are pauli_step_lstm's
        bit for bit, grads is lstm_gradient(samples, (eloc - s1 / n) * (1.0 / n))'s."""
        numsamples = int(numsamples)
        fl, sg, co = self._term_masks(*self._lattice_masks(flip, sign), coeff, False)
        K = fl.shape[0]
        mom = np.zeros(4, dtype=np.float64)
        sums = np.empty((K, 2), dtype=np.float64)
        smp = np.empty((max(numsamples, 0), self.N), dtype=np.int32) if want_samples else None
        el = np.empty(max(numsamples, 0), dtype=np.float64) if want_eloc else None
        self._check(self.lib.rnnwf_lstm_pauli_gradient_step(self.h, fl.ctypes.data_as(_I32P), sg.ctypes.data_as(_I32P), co.ctypes.data_as(_F64P), K,
                                                            numsamples, int(seed), int(step), int(sample_offset), mom.ctypes.data_as(_F64P),
                                                            sums.ctypes.data_as(_F64P), smp.ctypes.data_as(_I32P) if want_samples else None,
                                                            el.ctypes.data_as(_F64P) if want_eloc else None))
        out = {"moments": mom, "grads": self._grads(shapes), "term_sums": sums}
        if want_samples:
            out["samples"] = smp
        if want_eloc:
            out["eloc"] = el
        return out

    def _lattice_masks(self, flip, sign):
        """flip and sign given as (K, Nx, Ny) flattened to (K, Nx*Ny); everything else as it came"""
        fl, sg = np.asarray(flip), np.asarray(sign)
        if fl.ndim == 3 and fl.shape[1:] == (self.nx, self.ny) and sg.shape == fl.shape:
            fl, sg = fl.reshape(fl.shape[0], self.N), sg.reshape(sg.shape[0], self.N)
        return fl, sg

    def _term_masks(self, flip, sign, coeff, cplx):
        """(flip, sign, coeff) as contiguous arrays - (K, N) int32 twice, (K,) float64 or, with cplx, complex128 - after the checks every
        Pauli entry makes before the library is called"""
        fl, sg = np.asarray(flip), np.asarray(sign)
        if fl.ndim == 1:
            fl, sg = fl[None, :], sg[None, :]
        if fl.ndim != 2 or fl.shape[0] < 1 or fl.shape[1] != self.N or sg.shape != fl.shape:
            raise ValueError("flip and sign must both have shape (nterms >= 1, %d), got %r and %r" % (self.N, fl.shape, sg.shape))
        if not (np.all(fl == fl.astype(np.int32)) and np.all(sg == sg.astype(np.int32))):
            raise ValueError("flip and sign must hold the integers 0 and 1")
        fl, sg = np.ascontiguousarray(fl, dtype=np.int32), np.ascontiguousarray(sg, dtype=np.int32)
        co = np.ascontiguousarray(np.atleast_1d(coeff), dtype=np.complex128 if cplx else np.float64)
        if co.shape != (fl.shape[0],):
            raise ValueError("coeff must have shape (%d,), got %r" % (fl.shape[0], co.shape))
        return fl, sg, co

    def _pauli_call(self, entry, cplx, drawn_shape, flip, sign, coeff, ns, samples, seed, step, sample_offset, want_eloc, want_log_ratio,
                    want_samples):
        """the argument checks, buffers and result dict the four pauli_step methods share; cplx: complex coeff, eloc and log_ratio and
        four sums per term"""
        ns = int(ns)
        fl, sg, co = self._term_masks(flip, sign, coeff, cplx)
        K = fl.shape[0]
        s, sp = self._chain_samples(samples, ns, "ns")
        sums = np.empty((K, 4 if cplx else 2), dtype=np.float64)
        mom = np.zeros(4, dtype=np.float64)
        el = np.empty(max(ns, 0), dtype=np.complex64 if cplx else np.float64) if want_eloc else None
        nmasks = len({r.tobytes() for r in fl if r.any()})
        lr = np.empty((nmasks, max(ns, 0)), dtype=np.complex128 if cplx else np.float64) if want_log_ratio else None
        smp = np.empty(drawn_shape, dtype=np.int32) if want_samples and samples is None else None
        self._check(getattr(self.lib, entry)(self.h, fl.ctypes.data_as(_I32P), sg.ctypes.data_as(_I32P), co.ctypes.data_as(_F64P), K, sp, ns,
                                             int(seed), int(step), int(sample_offset), sums.ctypes.data_as(_F64P),
                                             el.ctypes.data_as(_F32P if cplx else _F64P) if el is not None else None,
                                             mom.ctypes.data_as(_F64P), lr.ctypes.data_as(_F64P) if lr is not None else None,
                                             smp.ctypes.data_as(_I32P) if smp is not None else None))
        out = {"term_sums": sums, "moments": mom}
        if want_eloc:
            out["eloc"] = el
        if want_log_ratio:
            out["log_ratio"] = lr
        if want_samples:
            out["samples"] = smp if smp is not None else s
        return out

    def pauli_step_complex(self, flip, sign, coeff, numsamples, samples=None, seed=0, step=0, sample_offset=0, want_eloc=False,
                           want_log_ratio=False, want_samples=False):
        """pauli_step for the complex RNN (rnnwf_pauli_step_complex).  flip, sign: (K, N) masks of 0 / 1 (or one term of N entries),
        coeff: (K,) complex.  samples: (ns, N) int32; None: drawn on the device as sample(ns, seed, step, sample_offset) draws them.
        Returns dict(term_sums=(K, 4) [sum Re v, sum Im v, sum (Re v)^2, sum (Im v)^2], moments=(4,) [sum Re E, sum (Re E)^2, ns,
        sum Im E], eloc=(ns,) complex64?, log_ratio=(distinct non-empty flip masks in order of first appearance, ns) complex128?
        (-inf + 0j where the flipped configuration leaves the zero-magnetisation sector), samples=(ns, N)?).  A call that fits one
        pass leaves its batch resident for vmc_gradient."""
        return self._pauli_call("rnnwf_pauli_step_complex", True, (max(int(numsamples), 0), self.N), flip, sign, coeff, numsamples, samples, seed,
                                step, sample_offset, want_eloc, want_log_ratio, want_samples)

    # -- device-resident Adam iterations on a Pauli-string Hamiltonian (docs/pauli_train.md) ---------
    def pauli_train_steps(self, flip, sign, coeff, numsamples, seed, step0, learning_rates, beta1=0.9, beta2=0.999, epsilon=1e-8,
                          sample_offset=0, want_term_sums=False, want_eloc=False):
        """len(learning_rates) whole iterations (sample at step index step0 + k, local energies of the Hamiltonian sum_k coeff_k
        (prod_sign sz)(prod_flip sx), gradient, Adam update with learning_rates[k], re-pack of the weight images) on the device with
        one host synchronisation (rnnwf_pauli_train_steps).  flip, sign, coeff as pauli_step takes them.  Returns the (K, 4) moments
        of the K batches, or - with want_term_sums or want_eloc - dict(moments=(K, 4), term_sums=(K, nterms, 2)?, eloc=(numsamples,)
        of the last iteration's batch?).  No batch is resident afterwards; get_param returns the trained values."""
        return self._pauli_train_call("rnnwf_pauli_train_steps", False, flip, sign, coeff, numsamples, seed, step0, learning_rates, beta1,
                                      beta2, epsilon, sample_offset, want_term_sums, want_eloc)

    def pauli_train_steps_complex(self, flip, sign, coeff, numsamples, seed, step0, learning_rates, beta1=0.9, beta2=0.999, epsilon=1e-8,
                                  sample_offset=0, want_term_sums=False, want_eloc=False):
        """pauli_train_steps for the complex RNN (rnnwf_pauli_train_steps_complex): coeff (nterms,) complex, term_sums (K, nterms, 4) as
        pauli_step_complex returns a row, eloc complex64."""
        return self._pauli_train_call("rnnwf_pauli_train_steps_complex", True, flip, sign, coeff, numsamples, seed, step0, learning_rates,
                                      beta1, beta2, epsilon, sample_offset, want_term_sums, want_eloc)

    def pauli_train_steps_2d(self, flip, sign, coeff, numsamples, seed, step0, learning_rates, beta1=0.9, beta2=0.999, epsilon=1e-8,
                             sample_offset=0, want_term_sums=False, want_eloc=False):
        """pauli_train_steps for the 2D RNN (rnnwf_pauli_train_steps_2d).  flip, sign: (nterms, Nx*Ny) masks indexed by the lattice
        index nx*Ny + ny, or (nterms, Nx, Ny), as pauli_step_2d takes them.  Returns what pauli_train_steps returns."""
        return self._pauli_train_call("rnnwf_pauli_train_steps_2d", False, *self._lattice_masks(flip, sign), coeff, numsamples, seed, step0,
                                      learning_rates, beta1, beta2, epsilon, sample_offset, want_term_sums, want_eloc)

    def pauli_train_steps_stack(self, flip, sign, coeff, numsamples, seed, step0, learning_rates, beta1=0.9, beta2=0.999, epsilon=1e-8,
                                sample_offset=0, want_term_sums=False, want_eloc=False):
        """pauli_train_steps for stacked GRU layers (rnnwf_pauli_train_steps_stack, docs/pauli_stack.md).  Arguments and what it
        returns are pauli_train_steps's."""
        return self._pauli_train_call("rnnwf_pauli_train_steps_stack", False, flip, sign, coeff, numsamples, seed, step0, learning_rates,
                                      beta1, beta2, epsilon, sample_offset, want_term_sums, want_eloc)

    def lstm_pauli_train_steps(self, flip, sign, coeff, numsamples, seed, step0, learning_rates, beta1=0.9, beta2=0.999, epsilon=1e-8,
                               sample_offset=0, want_term_sums=False, want_eloc=False):
        """pauli_train_steps for the LSTM wave function (rnnwf_lstm_pauli_train_steps; single process): iteration k is
        lstm_pauli_gradient_step at step index step0 + k, training.Adam with learning_rates[k] and set_params, bit for bit.  flip,
        sign: (nterms, N) masks by chain position or (nterms, Nx, Ny), as pauli_step_lstm takes them.  Returns what pauli_train_steps
        returns."""
        return self._pauli_train_call("rnnwf_lstm_pauli_train_steps", False, *self._lattice_masks(flip, sign), coeff, numsamples, seed, step0,
                                      learning_rates, beta1, beta2, epsilon, sample_offset, want_term_sums, want_eloc)

    def _pauli_train_call(self, entry, cplx, flip, sign, coeff, numsamples, seed, step0, learning_rates, beta1, beta2, epsilon,
                          sample_offset, want_term_sums, want_eloc):
        ns = int(numsamples)
        fl, sg, co = self._term_masks(flip, sign, coeff, cplx)
        nterms = fl.shape[0]
        lr, lrp = _f64(np.atleast_1d(learning_rates))
        K = lr.size
        mom = np.empty((K, 4), dtype=np.float64)
        sums = np.empty((K, nterms, 4 if cplx else 2), dtype=np.float64) if want_term_sums else None
        el = np.empty(max(ns, 0), dtype=np.complex64 if cplx else np.float64) if want_eloc else None
        self._check(getattr(self.lib, entry)(self.h, fl.ctypes.data_as(_I32P), sg.ctypes.data_as(_I32P), co.ctypes.data_as(_F64P), nterms, K, ns,
                                             int(seed), int(step0), int(sample_offset), lrp, float(beta1), float(beta2), float(epsilon), mom.ctypes.data_as(_F64P),
                                             sums.ctypes.data_as(_F64P) if sums is not None else None,
                                             el.ctypes.data_as(_F32P if cplx else _F64P) if el is not None else None))
        if not (want_term_sums or want_eloc):
            return mom
        out = {"moments": mom}
        if want_term_sums:
            out["term_sums"] = sums
        if want_eloc:
            out["eloc"] = el
        return out

    # -- multi-GPU --------------------------------------------------------------------------------
    def comm_unique_id(self):
        buf = C.create_string_buffer(UNIQUE_ID_BYTES)
        rc = self.lib.rnnwf_comm_unique_id(buf)
        if rc != 0:
            raise RnnwfError("rnnwf_comm_unique_id failed (%d)" % rc)
        return buf.raw

    def comm_init(self, unique_id, rank, nranks):
        self._check(self.lib.rnnwf_comm_init(self.h, C.c_char_p(unique_id), rank, nranks))

    def comm_reduce_in_step(self, on=True):
        """vmc_step returns the moments summed over all ranks (one in-stream RCCL all-reduce, one host sync per step)."""
        self._check(self.lib.rnnwf_comm_reduce_in_step(self.h, int(on)))

    def comm_info(self):
        """What the RCCL communicator itself reports (ncclCommCount / ncclCommUserRank) plus the handle's device."""
        n, r, d = _I32(0), _I32(0), _I32(0)
        self._check(self.lib.rnnwf_comm_info(self.h, C.byref(n), C.byref(r), C.byref(d)))
        return {"nranks": n.value, "rank": r.value, "device": d.value}

    def allreduce_moments(self, moments):
        m, mp = _f64(np.array(moments, dtype=np.float64))
        self._check(self.lib.rnnwf_allreduce_moments(self.h, mp, m.size))
        return m

    def allreduce_f64(self, a):
        """Sum over the ranks of a float64 array of any shape (rnnwf_allreduce_f64; identity without a communicator)."""
        m = np.array(a, dtype=np.float64, order="C")
        flat, fp = _f64(m.reshape(-1))
        self._check(self.lib.rnnwf_allreduce_f64(self.h, fp, flat.size))
        return flat.reshape(m.shape)

    def allreduce_grads(self, grads):
        """{name: array} summed over the ranks in ONE all-reduce (names in sorted order on every rank)."""
        names = sorted(grads)
        flat = self.allreduce_f64(np.concatenate([np.asarray(grads[k], dtype=np.float64).ravel() for k in names]))
        out, off = {}, 0
        for k in names:
            n = int(np.asarray(grads[k]).size)
            out[k] = flat[off:off + n].reshape(np.shape(grads[k]))
            off += n
        return out

    # -- measurement ------------------------------------------------------------------------------
    def timing_enable(self, on=True):
        self._check(self.lib.rnnwf_timing_enable(self.h, int(on)))

    def timing_reset(self):
        self._check(self.lib.rnnwf_timing_reset(self.h))

    def timing_get(self, kernel_id):
        ms, n = _F64(0), _I64(0)
        work = (C.c_double * 2)()
        self._check(self.lib.rnnwf_timing_get(self.h, kernel_id, C.byref(ms), C.byref(n), work))
        return {"total_ms": ms.value, "launches": n.value, "cell_evals": work[0], "mfma_flops": work[1]}

    def engine_name(self):
        return self.lib.rnnwf_engine_name(self.h).decode()

    def synchronize(self):
        self._check(self.lib.rnnwf_synchronize(self.h))

    def device_info(self):
        cu, mhz, hbm = _I32(0), _I32(0), _I64(0)
        name = C.create_string_buffer(64)
        self._check(self.lib.rnnwf_device_info(self.h, C.byref(cu), C.byref(mhz), C.byref(hbm), name))
        return {"cu_count": cu.value, "clock_mhz": mhz.value, "hbm_bytes": hbm.value, "name": name.value.decode()}
