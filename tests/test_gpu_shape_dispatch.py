"""Every row of every family's shape table (csrc/shapes.h) is dispatched, and every shape past a table's last row is refused.

The host code picks its kernels from the handle's shape - element type, layers, NFULL - by walking one table per family.  This module
walks the same shapes from the outside: per model, the first and the last unit count of every width class (CLASS_WIDTHS of
tests/gradient_classes_reference.py, the list the gradient-class tests walk; for the f32 models also 50 and 51 units, where the
bf16x3 engine's width class 3 changes its layout), both ends for one layer, alternating over the stacks.  Each case is the smallest run
that still reaches every dispatch: 4 sites (2 x 2 for the lattice models), 16 samples, one seed.  It calls vmc_step, vmc_gradient, the
model's pauli_step* and renyi2_regions*, correlations, log_derivatives and one train_steps iteration at lr = 1e-12, and each call
must return finite numbers or raise ValueError exactly as SERVED says - the matrix below is the behaviour of the code before the
tables were shared, which this module passes unchanged.  PAST_THE_TABLES are the shapes one step beyond each family's last row: they
must be refused when the handle is created, never dispatched.  Nothing here checks a value; the modules named in SERVED's comments do.
"""
import numpy as np
import pytest

import gradient_classes_reference as G

pytestmark = pytest.mark.gpu
NS, SEED = 16, 111
FAMILIES = ("gru", "parity", "crnn", "gru64", "mdrnn", "lstm")
LATTICE = ("gru64", "mdrnn", "lstm")
# width classes with kernels: one layer, stacks (csrc/shapes.h)
ONE_LAYER = {"gru": (1, 2, 3, 4, 6, 8, 12, 16), "parity": (1, 2, 3, 4, 6, 8, 12, 16), "crnn": (1, 2, 3, 4, 6, 8, 12, 16),
             "gru64": (1, 2, 3, 4, 6), "mdrnn": (1, 2, 3, 4, 5), "lstm": (1, 2, 3, 4)}
STACKS = {"gru": (1, 2, 3, 4, 6), "parity": (1, 2, 3, 4, 6), "crnn": (1, 2, 3, 4, 6), "gru64": (1, 2, 3, 4)}
ENTRIES = ("vmc_step", "vmc_gradient", "log_derivatives", "pauli_step", "renyi2_regions", "correlations", "train_steps")


def nfull(family, units):
    return G.nfull("gru64" if family == "lstm" else family, units)


def SERVED(family, units, entry):
    """True: the entry returns finite results for this shape; False: it raises ValueError (RNNWF_ERR_INVALID)."""
    one = len(units) == 1
    if entry == "vmc_step":
        return True
    if entry in ("vmc_gradient", "train_steps"):               # test_gpu_gradient_classes.py, test_gpu_train_images.py
        return family != "lstm"                                # the LSTM cell has no gradient
    if entry in ("pauli_step", "renyi2_regions"):              # test_gpu_observable_driver.py; *_complex and *_2d for those two models
        return family == "mdrnn" or (family in ("gru", "gru64", "crnn") and one)
    if entry == "correlations":                                # test_gpu_correlations.py
        return family in ("gru", "gru64") and one
    if entry == "log_derivatives":                             # test_gpu_sr.py: one layer, up to 68 units
        return family in ("gru", "gru64") and one and nfull(family, units) <= 4
    raise KeyError(entry)


def _cases():
    cases = []
    for family in FAMILIES:
        for nf in ONE_LAYER[family]:
            widths = list(G.CLASS_WIDTHS[nf])
            if nf == 3 and family in ("gru", "parity", "crnn"):
                widths[1:1] = [50, 51]
            cases += [(family, (w,)) for w in widths]
        for nl in (2, 3, 4):
            for k, nf in enumerate(STACKS.get(family, ())):
                cases.append((family, (G.CLASS_WIDTHS[nf][(nl + k) % 2],) * nl))
    return cases


CASES = _cases()
# one step past each family's last row: (family, units)
PAST_THE_TABLES = [("gru", (261,)), ("parity", (261,)), ("crnn", (261,)), ("gru64", (101,)), ("mdrnn", (85,)), ("lstm", (69,)),
                   ("gru", (101, 101)), ("parity", (101, 101)), ("crnn", (101, 101)), ("gru64", (69, 69)), ("mdrnn", (20, 20)),
                   ("lstm", (20, 20)), ("gru", (20,) * 5), ("crnn", (20,) * 5), ("gru64", (20,) * 5)]


def ident(family, units):
    return "%s-%s" % (family, "x".join(map(str, units)))


def model_id(family):
    from rnnwavefunctions_amd import _lib
    return {"gru": _lib.MODEL_GRU1D, "parity": _lib.MODEL_GRU1D_PARITY, "crnn": _lib.MODEL_CRNN_U1, "gru64": _lib.MODEL_GRU1D_F64,
            "mdrnn": _lib.MODEL_MDRNN2D, "lstm": _lib.MODEL_LSTM1D_F64}[family]


def handle(family, units):
    from rnnwavefunctions_amd import _lib
    nx, ny = (2, 2) if family in LATTICE else (4, 1)
    return _lib.NativeWavefunction(model_id(family), nx, ny, units)


def finite(x):
    vals = x.values() if isinstance(x, dict) else [x]
    return all(np.all(np.isfinite(np.asarray(v, dtype=np.complex128))) for v in vals)


def calls(family, wf):
    """entry -> a call of it on wf, in ENTRIES' order: the gradient and the log-derivatives read the batch vmc_step leaves resident,
    train_steps drops it"""
    N = wf.N
    coupl = np.concatenate([np.ones(N), 0.5 * np.ones(N), np.zeros(N), [0.0, 0.0]]) if family == "crnn" else np.append(np.ones(N), 1.0)
    suffix = {"crnn": "_complex", "mdrnn": "_2d"}.get(family, "")
    flip = np.zeros((2, N), dtype=np.int32)
    flip[0, 1] = flip[0, 2] = flip[1, 0] = flip[1, 3] = 1      # pair flips: they keep half the complex RNN's chains in its sector
    sign = np.zeros((2, N), dtype=np.int32)
    sign[1, 1] = 1
    region = np.array([1, 1, 0, 0], dtype=np.int32)
    shapes = {nm: (cnt,) for nm, cnt in wf._layout()}
    return {
        "vmc_step": lambda: wf.vmc_step(NS, seed=SEED, step=0, couplings=coupl, want_eloc=True),
        "vmc_gradient": lambda: wf.vmc_gradient(0.0, NS, shapes),
        "log_derivatives": lambda: wf.log_derivatives(),
        "pauli_step": lambda: getattr(wf, "pauli_step" + suffix)(flip, sign, [0.5, -1.0], NS, seed=SEED),
        "renyi2_regions": lambda: getattr(wf, "renyi2_regions" + suffix)(region, NS // 2, seed=SEED),
        "correlations": lambda: wf.correlations(NS, seed=SEED),
        "train_steps": lambda: wf.train_steps(NS, SEED, 0, coupl, [1e-12]),
    }


@pytest.mark.parametrize("family,units", CASES, ids=[ident(*c) for c in CASES])
def test_every_entry_is_served_or_refused(family, units):
    wf = handle(family, units)
    try:
        wf.init_params(SEED)
        call = calls(family, wf)
        for entry in ENTRIES:
            if SERVED(family, units, entry):
                assert finite(call[entry]()), entry
            else:
                with pytest.raises(ValueError):
                    call[entry]()
    finally:
        wf.close()


@pytest.mark.parametrize("family,units", PAST_THE_TABLES, ids=[ident(*c) for c in PAST_THE_TABLES])
def test_shapes_past_the_tables_are_refused(family, units):
    with pytest.raises(ValueError):
        handle(family, units)


def test_the_cases_cover_every_row():
    """one case at least per (family, layers, width class) with kernels, and nothing else"""
    rows = {(f, len(u), nfull(f, u)) for f, u in CASES}
    want = {(f, 1, nf) for f in FAMILIES for nf in ONE_LAYER[f]} | {(f, nl, nf) for f in STACKS for nl in (2, 3, 4) for nf in STACKS[f]}
    assert rows == want
    assert len(want) == 2 * 23 + 23 + 17 + 5 + 4
