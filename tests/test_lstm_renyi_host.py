"""CPU tests of the host side of rnnwf_renyi2_regions_lstm (docs/renyi_lstm.md): the header, the ctypes prototype and the
NativeWavefunction method agree with the stack entry's; observables_lstm validates its arguments before it touches the wave function;
and, on the float64 reference alone: the brute force gives the exact purity of the dense vector, every case of
tests/test_gpu_lstm_renyi.py is nontrivial, the restated bookkeeping of the PAIRED kernel agrees with brute force within the 1e-11 N
bound and each of six defects of that bookkeeping is outside it on every lattice where it can show.  No device: the wave functions are
fakes."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import lstm_renyi_reference as Z
import renyi_reference as RR
import renyi_stack_reference as S
from conftest import all_configs
from rnnwavefunctions_amd import observables as O
from rnnwavefunctions_amd import observables_lstm as OL
from rnnwavefunctions_amd import observables_stack as OS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY, STACK = "rnnwf_renyi2_regions_lstm", "rnnwf_renyi2_regions_stack"


def test_header_prototype_export_and_method_agree():
    from rnnwavefunctions_amd import _lib, build
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rnnwf.h")).read(), flags=re.S)
    assert re.search(r"#define\s+RNNWF_ABI_VERSION\s+1\b", header)
    decl = {name: re.search(r"\b%s\s*\(([^)]*)\)" % name, header) for name in (ENTRY, STACK)}
    assert all(decl.values())
    args, args_1 = ([" ".join(a.split()) for a in m.group(1).split(",")] for m in decl.values())
    assert len(args) == 11 and args == args_1                              # the argument list is the stack entry's
    assert _lib.PROTOTYPES[ENTRY] is _lib.PROTOTYPES[STACK]                # one object, not a copy
    assert hasattr(ctypes.CDLL(build.build()), ENTRY)
    assert _lib.ABI_VERSION == 1 and _lib.load_library().rnnwf_abi_version() == 1
    assert "lstm_renyi.hip" in build.SOURCES and build.compile_flags("lstm_renyi.hip") == build.compile_flags("lstm_pauli.hip")
    W = _lib.NativeWavefunction
    p, p_1 = inspect.signature(W.renyi2_regions_lstm).parameters, inspect.signature(W.renyi2_regions_stack).parameters
    assert list(p) == list(p_1) and [v.default for v in p.values()] == [v.default for v in p_1.values()]


def test_module_interface():
    assert OL.RENYI_API == ["renyi2_regions", "renyi2_entropy", "renyi2_mutual_information", "interval_region", "rectangle_region",
                            "column_cut_regions", "renyi2_from_sums"]
    assert OL.RENYI_API == OS.RENYI_API
    assert OL.__all__ == ["pauli_expectations", "energy", "correlations", "minimize_hamiltonian"]
    assert all(callable(getattr(OL, name)) for name in OL.RENYI_API)
    for name in ("renyi2_regions", "renyi2_entropy", "renyi2_mutual_information"):
        a, b = inspect.signature(getattr(OL, name)).parameters, inspect.signature(getattr(O, name)).parameters
        assert list(a) == list(b) and [v.default for v in a.values()] == [v.default for v in b.values()], name
    for name in ("interval_region", "rectangle_region", "column_cut_regions", "renyi2_from_sums"):
        assert getattr(OL, name) is getattr(O, name)                       # the existing builders, not copies


def _handle(model, units, N=6, answer=None):
    """passes observables._native without a library or a device.  answer None: every library call raises; otherwise
    renyi2_regions_lstm records its arguments and returns answer(regions, numpairs, log_ratio)"""
    from rnnwavefunctions_amd import _lib

    class NoLibrary(_lib.NativeWavefunction):
        def __init__(self):
            self.model, self.N, self.nx, self.ny, self.units, self.calls = model, N, N, 1, tuple(units), []

        def __del__(self):
            pass

        def __getattribute__(self, name):
            if name in ("lib", "h") or (name == "renyi2_regions_lstm" and answer is None):
                raise AssertionError("the library was touched: %s" % name)
            return object.__getattribute__(self, name)

        def renyi2_regions_lstm(self, regions, numpairs, samples=None, seed=111, step=0, pair_offset=0, log_ratio=False):
            self.calls.append(dict(regions=np.array(regions), numpairs=numpairs, samples=samples, seed=seed, step=step, log_ratio=log_ratio))
            return answer(np.asarray(regions), numpairs, log_ratio)
    return NoLibrary()


def test_refusals_fire_before_any_library_call():
    from rnnwavefunctions_amd import _lib
    a, b = O.interval_region(6, 1, 2), O.interval_region(6, 3, 5)
    calls = [lambda w: OL.renyi2_regions(w, [a, b], 10), lambda w: OL.renyi2_entropy(w, 10), lambda w: OL.renyi2_mutual_information(w, a, b, 10)]
    for model, units in [(_lib.MODEL_GRU1D, (10,)), (_lib.MODEL_GRU1D_F64, (10,)), (_lib.MODEL_GRU1D, (10, 10)), (_lib.MODEL_GRU1D_PARITY, (10,)),
                         (_lib.MODEL_CRNN_U1, (10,)), (_lib.MODEL_MDRNN2D, (10,))]:
        for call in calls:
            with pytest.raises(ValueError, match="observables_lstm serves the LSTM wave function"):
                call(_handle(model, units))
    with pytest.raises(ValueError, match="facade or a NativeWavefunction"):
        OL.renyi2_entropy(object(), 10)
    with pytest.raises(ValueError, match="disjoint"):
        OL.renyi2_mutual_information(_handle(_lib.MODEL_LSTM1D_F64, (8,)), a, a, 10)


def test_entropy_and_mutual_information_are_the_arithmetic_of_observables():
    from rnnwavefunctions_amd import _lib
    N, n = 6, 40
    rng = np.random.RandomState(0)
    lr = rng.normal(-0.2, 0.5, size=(N + 1, n))

    def answer(regions, numpairs, log_ratio):
        assert numpairs == n
        rows = lr[:len(regions)].copy()
        trivial = np.all(regions == regions[:, :1], axis=1)              # empty or full: the library returns exactly 0
        rows[trivial] = 0.0
        out = {"sums": np.stack([np.exp(rows).sum(axis=1), np.exp(2 * rows).sum(axis=1)], axis=1)}
        if log_ratio:
            out["log_ratio"] = rows
        return out
    wf = _handle(_lib.MODEL_LSTM1D_F64, (8,), N, answer)
    samples = rng.randint(0, 2, size=(2 * n, 3, 2))
    S2, err = OL.renyi2_entropy(wf, n, seed=7, step=3, samples=samples)
    call = wf.calls[-1]
    assert call["regions"].shape == (N + 1, N) and call["samples"].shape == (2 * n, N) and (call["seed"], call["step"]) == (7, 3)
    assert np.array_equal(call["samples"], samples.reshape(2 * n, N))       # flattened in C order
    for l in range(N + 1):                                                  # cut l as its complement, the suffix {l..N-1}
        assert np.array_equal(call["regions"][l], (np.arange(N) >= l).astype(np.int32))
    rows = lr.copy()
    rows[[0, N]] = 0.0
    want = O.renyi2_from_sums(np.stack([np.exp(rows).sum(axis=1), np.exp(2 * rows).sum(axis=1)], axis=1), n)
    assert np.array_equal(S2, want[0]) and np.array_equal(err, want[1])
    assert S2[0] == 0.0 and S2[N] == 0.0 and err[0] == 0.0 and err[N] == 0.0 and np.all(err[1:N] > 0.0)
    a, b = O.interval_region(N, 1, 2), O.interval_region(N, 3, 5)
    got = OL.renyi2_mutual_information(wf, a, b, n)
    call = wf.calls[-1]
    assert np.array_equal(call["regions"], np.stack([a, b, a | b])) and call["log_ratio"] and call["samples"] is None
    assert got == O.mutual_information2_from_log_ratios(lr[0], lr[1], lr[2])
    S2r, errr = OL.renyi2_regions(wf, [a, b], n)
    want = O.renyi2_from_sums(np.stack([np.exp(lr[:2]).sum(axis=1), np.exp(2 * lr[:2]).sum(axis=1)], axis=1), n)
    assert np.array_equal(S2r, want[0]) and np.array_equal(errr, want[1])


# ---- the reference alone -------------------------------------------------------------------------------------------------------------

def test_brute_force_over_all_pairs_gives_the_exact_purity():
    """3 x 2, 10 units: the purity from all 64 x 64 pairs weighted with P(sigma) P(tau) equals Tr rho_A^2 of the dense vector to 1e-12;
    r_A = r_complement; the empty and the full mask give exactly 0; the restated bookkeeping is the same number"""
    Nx, Ny, N, units = 3, 2, 6, 10
    prm = Z.parameters(units)
    c = all_configs(N).astype(np.int32)
    lp = Z.log_p(prm, Nx, Ny)(c)
    assert abs(np.exp(lp).sum() - 1.0) < 1e-13
    masks = np.stack([S.mask_of(N, [2, 3]), S.mask_of(N, [1, 4]), S.mask_of(N, [5]), S.mask_of(N, [0, 3])])
    i, j, pairs = S.all_pairs(c)
    lr = Z.log_ratio(prm, Nx, Ny, pairs, masks)
    purity = (np.exp(lp[i] + lp[j])[None, :] * np.exp(lr)).sum(axis=1)
    exact = np.array([S.purity_of_region(np.exp(0.5 * lp), N, m) for m in masks])
    rel = np.abs(purity / exact - 1.0)
    print("LSTMRENYI 3x2-10: Tr rho_A^2 = %s, max rel %.2e" % (np.round(exact, 4), rel.max()))
    assert -np.log(exact.min()) > 0.05                            # entangled: the identity is not trivially 1 = 1
    assert rel.max() <= 1e-12
    sub = pairs[:2 * 200]
    assert np.abs(Z.log_ratio(prm, Nx, Ny, sub, masks) - Z.log_ratio(prm, Nx, Ny, sub, 1 - masks)).max() <= 1e-12
    trivial = np.stack([np.zeros(N, dtype=np.int32), np.ones(N, dtype=np.int32)])
    ends = Z.log_ratio(prm, Nx, Ny, sub, trivial)
    assert np.all(ends == 0.0)
    assert np.array_equal(Z.kernel_form(prm, sub, trivial), ends)
    assert np.abs(Z.kernel_form(prm, sub, masks) - Z.log_ratio(prm, Nx, Ny, sub, masks)).max() <= 1e-12


@pytest.mark.parametrize("shape", Z.LATTICES, ids=["%dx%d" % s for s in Z.LATTICES])
def test_every_case_is_nontrivial_on_the_reference_alone(shape):
    """a condition of the GPU test's cases, asserted here on the CPU for all of them: max |log r| > 0.1, a quarter of the entries above
    0.01"""
    Nx, Ny = shape
    N = Nx * Ny
    names, masks = Z.regions_of(Nx, Ny)
    assert any(m[0] for m in masks)                               # a region that the library normalises
    assert N <= 33 or S.word_boundaries_covered(N, masks)
    assert Z.pairs_of(Nx, Ny, 10).shape == (38, N)
    for units in Z.WIDTHS:
        ref = Z.log_ratio(Z.parameters(units), Nx, Ny, Z.pairs_of(Nx, Ny, units), masks)
        mx, share = RR.nontrivial(ref)
        print("LSTMRENYI nontrivial %dx%d-%d: max |log r| %.3f, %.0f %% above 0.01" % (Nx, Ny, units, mx, 100 * share))
        assert mx > 0.1 and share >= 0.25, (shape, units, mx, share)


@pytest.mark.parametrize("units", [10, 37])
def test_the_bound_accepts_the_kernel_form_and_rejects_six_defects(units):
    """per lattice of the GPU test: the restated bookkeeping agrees with brute force within the bound, each defect is outside it"""
    prm = Z.parameters(units)
    for Nx, Ny in Z.LATTICES:
        N = Nx * Ny
        pairs, masks = Z.pairs_of(Nx, Ny, units), Z.regions_of(Nx, Ny)[1]
        ref = Z.log_ratio(prm, Nx, Ny, pairs, masks)
        good = np.abs(Z.kernel_form(prm, pairs, masks) - ref).max()
        assert good <= Z.bound(N), (Nx, Ny, good)
        line = "LSTMRENYI defects %dx%d, %d units: kernel form %.1e of the bound" % (Nx, Ny, units, good / Z.bound(N))
        for defect in Z.DEFECTS:
            if not Z.SHOWS[defect](N):
                continue
            factor = np.abs(Z.kernel_form(prm, pairs, masks, defect) - ref).max() / Z.bound(N)
            line += "; %s %.1e x" % (defect, factor)
            assert factor > 1.0, (Nx, Ny, defect, factor)
        print(line)
