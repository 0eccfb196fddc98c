"""Host-side tests of the correlation-function entry point (rnnwf_correlations): the header declares it, the binding's prototype
table has it with the documented argument types, the built library exports it, and the ABI version is unchanged."""
import ctypes as C
import os
import re

from conftest import ROOT


def test_header_prototypes_and_library_declare_correlations():
    header = open(os.path.join(ROOT, "include", "rnnwf.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    sp = r"\s*"
    args = [r"rnnwf_handle\s*\*\s*h", r"const\s+int32_t\s*\*\s*samples", r"int64_t\s+ns", r"uint64_t\s+seed", r"uint64_t\s+step",
            r"int64_t\s+sample_offset", r"double\s*\*\s*z_sums", r"double\s*\*\s*zz_sums", r"double\s*\*\s*x_sums",
            r"double\s*\*\s*xx_sums", r"double\s*\*\s*out_log_ratio", r"int32_t\s*\*\s*out_samples"]
    assert re.search(r"int\s+rnnwf_correlations\s*\(" + sp + (sp + "," + sp).join(args) + sp + r"\)\s*;", code)
    assert "#define RNNWF_ABI_VERSION 1" in header
    from rnnwavefunctions_amd import _lib, build
    assert _lib.ABI_VERSION == 1
    assert "rnnwf_correlations" in _lib.PROTOTYPES
    res, at = _lib.PROTOTYPES["rnnwf_correlations"]
    f64p, i32p = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    assert res is C.c_int
    assert at == [C.c_void_p, i32p, C.c_int64, C.c_uint64, C.c_uint64, C.c_int64, f64p, f64p, f64p, f64p, f64p, i32p]
    lib = C.CDLL(build.build())
    assert hasattr(lib, "rnnwf_correlations")
    lib.rnnwf_abi_version.restype = C.c_int
    assert lib.rnnwf_abi_version() == 1


def test_facade_method_and_observables_exist():
    from rnnwavefunctions_amd import _lib, observables
    assert callable(getattr(_lib.NativeWavefunction, "correlations"))
    assert callable(observables.correlations) and callable(observables.correlations_from_sums)
