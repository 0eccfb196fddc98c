"""The 2D RNN's stochastic reconfiguration (docs/sr_2d.md): header, binding and facade agree.  No device."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = (("rnnwf_log_derivatives_2d", 4), ("rnnwf_sr_gram_2d", 3), ("rnnwf_sr_apply_2d", 3), ("rnnwf_sr_solve_2d", 3),
           ("rnnwf_sr_direction_2d", 3))


def header():
    return open(os.path.join(ROOT, "include", "rnnwf.h")).read()


def test_header_declares_and_binding_binds_the_five_entries():
    from rnnwavefunctions_amd import _lib
    code = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    for name, nargs in ENTRIES:
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, code)
        assert m and len(m.group(1).split(",")) == nargs == len(_lib.PROTOTYPES[name][1]), name
        real = name[:-len("_2d")]
        assert _lib.PROTOTYPES[name] == _lib.PROTOTYPES[real]          # the same signatures as the positive model's entries


def test_abi_version_stays_one():
    from rnnwavefunctions_amd import _lib
    assert re.search(r"#define RNNWF_ABI_VERSION 1\b", header()) and _lib.ABI_VERSION == 1


def test_facade_has_the_methods_and_functions():
    from rnnwavefunctions_amd import _lib, sr
    for m in ("log_derivatives_2d", "sr_gram_2d", "sr_apply_2d", "sr_solve_2d", "sr_direction_2d"):
        assert callable(getattr(_lib.NativeWavefunction, m))
    for f in ("minsr_direction_2d", "qgt_2d", "train_tfim2d"):
        assert callable(getattr(sr, f))
