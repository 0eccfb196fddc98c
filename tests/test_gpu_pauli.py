"""GPU tests of Pauli-string expectation values and local energies of arbitrary spin Hamiltonians (rnnwf_pauli_step,
csrc/pauli_kernels.h, observables.pauli_expectations / energy, training.minimize_hamiltonian) on the positive GRU models: the f32
GRU1D and the f64 raster model GRU1D_F64.

Tolerances, the project's own (docs/renyi_regions.md, docs/correlations.md, tests/test_gpu_prnn.py): log r against flipped
configurations evaluated with rnnwf_log_prob: 1e-11 N (f64), 1e-5 N (f32).  Exact enumeration: relative 1e-12 (f64), 2e-5 (f32).
Against rnnwf_correlations' rows and rnnwf_tfim_eloc's queue on the same samples: 1e-11 N.  E_loc against rnnwf_tfim_eloc per
site: 1e-5 (f32-input MFMA engine), 1e-10 (f64).
"""
import ctypes as C

import numpy as np
import pytest

import autograd_reference as A
import pauli_reference as PR
from conftest import all_configs
from rnnwavefunctions_amd import observables as O
from rnnwavefunctions_amd import params as P

pytestmark = pytest.mark.gpu

SCOPE = "RNNwavefunction"


def trained_like(H, seed, f64, scale=3.0):
    prm = P.init_gru_params([H], seed=seed, dtype=np.float64 if f64 else np.float32)
    return P.randomize_biases(P.scale_kernels(prm, scale), seed + 1)


def make_wf(f64, Nx, Ny, H, prm):
    from rnnwavefunctions_amd import _lib
    wf = _lib.NativeWavefunction(_lib.MODEL_GRU1D_F64 if f64 else _lib.MODEL_GRU1D, Nx, Ny, (H,))
    wf.set_params(prm, scope=SCOPE)
    return wf


def mask_of(N, sites):
    m = np.zeros(N, dtype=np.int32)
    m[list(sites)] = 1
    return m


def flips_only(wf, masks, ns, **kw):
    """pauli_step on pure-X terms, one per mask, coefficient 1."""
    masks = np.asarray(masks)
    return wf.pauli_step(masks, np.zeros_like(masks), np.ones(len(masks)), ns, **kw)


def explicit_log_ratio(wf, s, masks):
    own = wf.log_prob(s)
    return np.stack([0.5 * (wf.log_prob((s ^ m[None, :]).astype(np.int32)) - own) for m in masks])


# The strings of the exact and statistical tests and their weights (seed 20, kernels x 3, biases randomised, 10 units), chosen on the CPU
# with the oracle (tests/test_pauli_reference.py: test_statistical_strings_are_not_vacuous asserts it) so that no exact value is below
# 0.05 in magnitude.
EXACT_SEED = 20
FLOOR = 0.05
EXACT_CASES = [(False, 10, 1, 10), (True, 3, 4, 10)]


def exact_strings(N):
    return [[("X", 0)], [("X", N - 1)], [("Z", 0)], [("Z", 2), ("Z", 3)], [("X", 1), ("X", 2)], [("Y", 1), ("Y", 2)],
            [("X", 0), ("Z", 1), ("X", 2)], [("Z", 0), ("X", 1), ("Z", 2)], [("Z", 2), ("Z", 3), ("X", 7)],
            [("Y", 0), ("Z", 2), ("Z", 3), ("Y", 1)], [("X", i) for i in range(N)], [("Z", 3), ("X", 5)],
            [("X", 0), ("X", 1), ("X", N - 1)], [("Z", 0), ("X", N - 1)]]


# 1. sum over every sigma of P(sigma) v_k(sigma) = psi^T O_k psi from the dense vector
@pytest.mark.parametrize("f64,Nx,Ny,H", EXACT_CASES)
def test_exact_enumeration_against_dense_operators(f64, Nx, Ny, H):
    N = Nx * Ny
    wf = make_wf(f64, Nx, Ny, H, trained_like(H, EXACT_SEED, f64))
    strings = exact_strings(N)
    flip, sign, factor = O.pauli_terms(strings, N)
    assert np.all(factor.imag == 0)
    c = all_configs(N)
    lp = wf.log_prob(c)
    psi = np.exp(0.5 * lp)
    out = wf.pauli_step(flip, sign, factor.real, len(c), samples=c, want_log_ratio=True, want_eloc=True)
    lr = out["log_ratio"]
    _, index = O.group_by_mask(flip)
    v = PR.signs(c, sign) * np.where(index[:, None] >= 0, np.exp(lr[np.maximum(index, 0)]), 1.0)
    got = factor.real * (np.exp(lp)[None, :] * v).sum(axis=1)
    exact = np.array([(psi @ PR.dense_string({i: p for p, i in st}, N) @ psi).real for st in strings])
    rel = np.abs(got / exact - 1.0)
    print("%s %dx%d: exact values %s, max rel %.2e" % ("f64" if f64 else "f32", Nx, Ny, np.round(exact, 4), rel.max()))
    assert np.abs(exact).min() >= FLOOR
    assert rel.max() <= (1e-12 if f64 else 2e-5)
    # term_sums are the plain sums of the same v, E_loc their coefficient-weighted sum
    assert np.allclose(out["term_sums"], PR.sums_from_values(v), rtol=1e-12, atol=1e-12 * len(c))
    assert np.allclose(out["eloc"], factor.real @ v, rtol=1e-12, atol=1e-12)
    m = out["moments"]
    assert m[2] == len(c) and np.isclose(m[0], out["eloc"].sum(), rtol=1e-12) and np.isclose(m[1], (out["eloc"] ** 2).sum(), rtol=1e-12)
    # raw terms whose sign and flip masks overlap in an odd number of sites (sz_0 sx_0; sz_1 sx_1 sx_2): the sign is the SAMPLED
    # configuration's - read from the flipped one, every v would change sign
    f2, s2, _ = O.pauli_terms([[("Y", 0)], [("Y", 1), ("X", 2)]], N)
    o2 = wf.pauli_step(f2, s2, [1.0, 1.0], len(c), samples=c, want_log_ratio=True)
    v2 = PR.signs(c, s2) * np.exp(o2["log_ratio"])
    assert np.allclose(o2["term_sums"], PR.sums_from_values(v2), rtol=1e-12, atol=0) and np.abs(o2["term_sums"][:, 0]).min() > 1.0


# 2. log r per chain against explicit flipped configurations; every NFULL of the dispatch table, partial last blocks, remainder widths
F32_WIDTHS = [(10, 7), (30, 7), (50, 7), (60, 6), (90, 6), (120, 5), (180, 5), (250, 4),      # NFULL 1 2 3 4 6 8 12 16
              (16, 7), (20, 7), (36, 7), (64, 6), (100, 6), (128, 5), (133, 5), (256, 4)]     # other remainders of the hidden width
F64_WIDTHS = [(10, 7), (30, 7), (50, 6), (60, 6), (90, 5), (16, 7), (36, 7), (53, 6), (68, 6), (100, 5)]


def small_masks(N):
    return np.stack([mask_of(N, [0]), mask_of(N, [1]), mask_of(N, [N - 1]), mask_of(N, range(N)), mask_of(N, range(0, N, 2)),
                     mask_of(N, [0, N - 1]), mask_of(N, [1, 2, N - 2]), mask_of(N, range(N // 2, N)), mask_of(N, range(1, N))])


@pytest.mark.parametrize("f64,H,N", [(False, H, N) for H, N in F32_WIDTHS] + [(True, H, N) for H, N in F64_WIDTHS])
def test_log_ratio_matches_explicit_flipped_configurations(f64, H, N):
    ns = 26                                          # the second block of 16 is partial
    wf = make_wf(f64, N, 1, H, trained_like(H, H, f64, scale=2.0 if H > 60 else 3.0))
    s = np.random.RandomState(H + N).randint(0, 2, size=(ns, N)).astype(np.int32)
    masks = small_masks(N)
    got = flips_only(wf, masks, ns, samples=s, want_log_ratio=True)["log_ratio"]
    ref = explicit_log_ratio(wf, s, masks)
    err = np.abs(got - ref).max()
    print("%s H=%d N=%d: max |log r - explicit| = %.2e (max |log r| %.2f)" % ("f64" if f64 else "f32", H, N, err, np.abs(ref).max()))
    assert got.shape == (len(masks), ns)
    assert err <= (1e-11 if f64 else 1e-5) * N
    assert np.abs(ref).max() > 1e-3


@pytest.mark.parametrize("f64,Nx,Ny,H", [(True, 3, 4, 20), (False, 70, 1, 20), (True, 9, 4, 20)])
def test_multi_word_masks_against_explicit_configurations(f64, Nx, Ny, H):
    """3x4 and 9x4 rasters (two spin words) and a 70-site chain (three words): masks around the word boundaries, site 0, only site
    N-1, everything."""
    N = Nx * Ny
    ns = 37
    wf = make_wf(f64, Nx, Ny, H, trained_like(H, 7, f64))
    s = np.random.RandomState(N).randint(0, 2, size=(ns, N)).astype(np.int32)
    masks = [mask_of(N, [0]), mask_of(N, [N - 1]), mask_of(N, range(N)), mask_of(N, range(1, N, 2)), mask_of(N, [0, N // 2, N - 1])]
    for w in range(32, N, 32):
        masks += [mask_of(N, range(w - 2, min(N, w + 3))), mask_of(N, [w - 1]), mask_of(N, [w]), mask_of(N, [1, w])]
    masks = np.stack(masks)
    got = flips_only(wf, masks, ns, samples=s, want_log_ratio=True)["log_ratio"]
    err = np.abs(got - explicit_log_ratio(wf, s, masks)).max()
    print("%s %dx%d: max |log r - explicit| = %.2e over %d masks" % ("f64" if f64 else "f32", Nx, Ny, err, len(masks)))
    assert err <= (1e-11 if f64 else 1e-5) * N


@pytest.mark.parametrize("N", [1, 2, 3])
@pytest.mark.parametrize("f64", [False, True])
def test_tiny_chains_with_every_mask(f64, N):
    wf = make_wf(f64, N, 1, 10, trained_like(10, 3, f64))
    c = all_configs(N)
    s = np.concatenate([c] * 5)[:19]
    masks = c[1:]                                    # every non-empty mask
    out = flips_only(wf, masks, len(s), samples=s, want_log_ratio=True)
    err = np.abs(out["log_ratio"] - explicit_log_ratio(wf, s, masks)).max()
    assert err <= (1e-11 if f64 else 1e-5) * N
    # all configurations: sum_sigma P v = psi^T X_F psi = sum_sigma psi(sigma) psi(sigma ^ F)
    lp = wf.log_prob(c)
    lr = flips_only(wf, masks, len(c), samples=c, want_log_ratio=True)["log_ratio"]
    psi = np.exp(0.5 * lp)
    for k, m in enumerate(masks):
        exact = psi @ PR.dense_term(m, np.zeros(N, dtype=int)) @ psi
        assert abs((np.exp(lp) * np.exp(lr[k])).sum() / exact - 1.0) <= (1e-12 if f64 else 2e-5)


# 3. against the hard-wired estimators on the same samples
@pytest.mark.parametrize("f64,Nx,Ny,H", [(False, 20, 1, 50), (False, 40, 1, 30), (True, 4, 5, 30)])
def test_single_x_terms_and_tfim_energy_against_tfim_eloc(f64, Nx, Ny, H, monkeypatch):
    monkeypatch.setenv("RNNWF_ENGINE", "f32")        # rnnwf_tfim_eloc on the f32-input MFMA engine, as the flip-mask pass
    N = Nx * Ny
    ns = 300
    wf = make_wf(f64, Nx, Ny, H, trained_like(H, 5, f64))
    s = wf.sample(ns, seed=3).reshape(ns, N)
    Jz = np.random.RandomState(1).uniform(0.5, 1.5, size=(Nx, Ny) if f64 else N)
    lpq = np.empty((N + 1, ns))
    e_ref = wf.tfim_eloc(s, Jz.ravel(), 1.3, log_probs=lpq)
    out = flips_only(wf, np.eye(N, dtype=np.int32), ns, samples=s, want_log_ratio=True)
    ref = 0.5 * (lpq[1:] - lpq[0][None, :])
    err = np.abs(out["log_ratio"] - ref).max()
    ham = O.tfim_hamiltonian(Jz, 1.3)
    e = O.energy(wf, ham, ns, samples=s, want_eloc=True)
    per_site = np.abs(e["eloc"] - e_ref).max() / N
    print("%s %dx%d: max |log r_i - queue| = %.2e; max |E_loc - tfim_eloc| / N = %.2e" % ("f64" if f64 else "f32", Nx, Ny, err, per_site))
    assert err <= (1e-11 if f64 else 1e-5) * N
    assert per_site <= (1e-10 if f64 else 1e-5)
    assert abs(e["mean"] - e_ref.mean()) / N <= (1e-10 if f64 else 1e-5)


@pytest.mark.parametrize("f64,Nx,Ny,H", [(False, 12, 1, 30), (False, 34, 1, 20), (True, 3, 4, 20)])
def test_one_and_two_x_strings_against_correlations(f64, Nx, Ny, H):
    N = Nx * Ny
    ns = 50
    wf = make_wf(f64, Nx, Ny, H, trained_like(H, 9, f64))
    s = np.random.RandomState(2).randint(0, 2, size=(ns, N)).astype(np.int32)
    ref = wf.correlations(ns, samples=s, want_log_ratio=True)["log_ratio"]
    masks = [mask_of(N, [i]) for i in range(N)] + [mask_of(N, [i, j]) for i in range(N) for j in range(i + 1, N)]
    got = flips_only(wf, np.stack(masks), ns, samples=s, want_log_ratio=True)["log_ratio"]
    err = np.abs(got - ref).max()
    print("%s %dx%d: max |log r - correlations rows| = %.2e over %d rows" % ("f64" if f64 else "f32", Nx, Ny, err, len(masks)))
    assert got.shape == ref.shape and err <= 1e-11 * N


# 4. statistics
@pytest.mark.parametrize("f64,Nx,Ny,H", EXACT_CASES)
def test_device_drawn_expectations_within_five_standard_errors(f64, Nx, Ny, H):
    N = Nx * Ny
    ns = 2 ** 16
    wf = make_wf(f64, Nx, Ny, H, trained_like(H, EXACT_SEED, f64))
    strings = exact_strings(N) + [[("Y", 3)], [("X", 1), ("Y", 2), ("Z", 3)]]
    psi = np.exp(0.5 * wf.log_prob(all_configs(N)))
    psi /= np.linalg.norm(psi)
    exact = np.array([(psi @ PR.dense_string({i: p for p, i in st}, N) @ psi).real for st in strings])
    out = O.pauli_expectations(wf, strings, ns, seed=111)
    z = np.abs(out["value"][:-2] - exact[:-2]) / out["err"][:-2]
    print("%s %dx%d: exact %s\n  got %s\n  |z| %s" % ("f64" if f64 else "f32", Nx, Ny, np.round(exact, 4), np.round(out["value"], 4), np.round(z, 2)))
    assert np.abs(exact[:-2]).min() >= FLOOR and np.all(out["err"][:-2] > 0)
    assert z.max() <= 5.0
    assert np.all(out["value"][-2:] == 0) and np.all(out["err"][-2:] == 0) and np.abs(exact[-2:]).max() < 1e-12     # odd n_Y
    ham = O.xxz_hamiltonian(N, -1.0, 0.5)
    Hd = sum(c * PR.dense_string({i: p for p, i in st}, N).real for c, st in ham.terms)
    e = O.energy(wf, ham, ns, seed=111)
    assert abs(e["mean"] - psi @ Hd @ psi) <= 5.0 * e["err"]


def test_odd_y_strings_alone_touch_no_device():
    wf = make_wf(False, 6, 1, 10, trained_like(10, 1, False))
    wf.timing_enable(True)
    wf.timing_reset()
    out = O.pauli_expectations(wf, ["YIIIII", [("X", 0), ("Y", 3)]], 100)
    assert np.all(out["value"] == 0) and np.all(out["err"] == 0)
    assert sum(wf.timing_get(k)["launches"] for k in range(3)) == 0


# 5. call behaviour
def test_repeat_shards_budget_permutation_and_work(monkeypatch):
    N, H, ns = 40, 30, 1000
    prm = trained_like(H, 4, False)
    wf = make_wf(False, N, 1, H, prm)
    strings = [[("X", 3)], [("X", 3), ("Z", 7)], [("Z", 1), ("Z", 2)], [("X", 0), ("X", 35)], [("Y", 33), ("Y", 34)], [("X", 33), ("X", 34)],
               [("X", i) for i in range(30, 36)]]
    flip, sign, factor = O.pauli_terms(strings, N)
    coeff = np.linspace(-1, 1, len(strings)) * factor.real
    kw = dict(seed=5, step=2, want_eloc=True, want_log_ratio=True, want_samples=True)
    wf.timing_enable(True)
    wf.timing_reset()
    a = wf.pauli_step(flip, sign, coeff, ns, **kw)
    work = wf.timing_get(1)["cell_evals"]
    firsts = [3, 0, 33, 30]                          # distinct non-empty masks in order of first appearance
    assert a["log_ratio"].shape == (4, ns) and work == ns * sum(N - f for f in firsts)
    assert np.array_equal(a["samples"], wf.sample(ns, seed=5, step=2).reshape(ns, N))
    b = wf.pauli_step(flip, sign, coeff, ns, **kw)
    for k in ("term_sums", "moments", "eloc", "log_ratio", "samples"):
        assert np.array_equal(a[k], b[k]), k
    # shards
    cut = 336
    s1 = wf.pauli_step(flip, sign, coeff, cut, sample_offset=0, **kw)
    s2 = wf.pauli_step(flip, sign, coeff, ns - cut, sample_offset=cut, **kw)
    assert np.array_equal(np.concatenate([s1["eloc"], s2["eloc"]]), a["eloc"])
    assert np.array_equal(np.concatenate([s1["log_ratio"], s2["log_ratio"]], axis=1), a["log_ratio"])
    assert np.allclose(s1["term_sums"] + s2["term_sums"], a["term_sums"], rtol=1e-13, atol=1e-12)
    assert np.allclose((s1["moments"] + s2["moments"])[:3], a["moments"][:3], rtol=1e-13)
    # permuted and duplicated terms
    perm = np.array([6, 0, 0, 5, 4, 3, 2, 1, 3])
    p = wf.pauli_step(flip[perm], sign[perm], coeff[perm], ns, **kw)
    assert np.array_equal(p["term_sums"], a["term_sums"][perm])
    # several passes
    monkeypatch.setenv("RNNWF_STATE_BUDGET_MB", "1")
    wf1 = make_wf(False, N, 1, H, prm)
    wf1.timing_enable(True)
    wf1.timing_reset()
    m = wf1.pauli_step(flip, sign, coeff, ns, **kw)
    passes = wf1.timing_get(1)["launches"]
    print("RNNWF_STATE_BUDGET_MB=1: %d passes" % passes)
    assert passes >= 3
    for k in ("eloc", "log_ratio", "samples"):
        assert np.array_equal(m[k], a[k]), k
    assert np.allclose(m["term_sums"], a["term_sums"], rtol=1e-13, atol=1e-12) and np.allclose(m["moments"][:3], a["moments"][:3], rtol=1e-13)
    with pytest.raises(Exception, match="rnnwf_vmc_step first"):
        wf1.vmc_gradient(0.0, ns, {"wf_dense/kernel": (H, 2)})


# 6. refusals
def test_refusals_through_the_c_call_and_the_facade():
    from rnnwavefunctions_amd import _lib
    N = 6
    wf = make_wf(False, N, 1, 10, trained_like(10, 1, False))
    one = np.zeros((1, N), dtype=np.int32)
    x0 = one.copy()
    x0[0, 0] = 1
    ok = wf.pauli_step(x0, one, [1.0], 32, seed=1)
    g0 = wf.vmc_gradient(ok["moments"][0] / 32, 32, {"wf_dense/kernel": (10, 2)})["wf_dense/kernel"]
    I32P, F64P = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    fp, sp = x0.ctypes.data_as(I32P), one.ctypes.data_as(I32P)
    co = np.ones(1)
    cp = co.ctypes.data_as(F64P)
    sums = np.zeros((1, 2))
    up = sums.ctypes.data_as(F64P)

    def call(flip=fp, sign=sp, coeff=cp, K=1, ns=32, offset=0, out=up):
        return wf.lib.rnnwf_pauli_step(wf.h, flip, sign, coeff, K, None, ns, 1, 0, offset, out, None, None, None, None)

    for kwargs, word in [(dict(K=0), "nterms"), (dict(ns=0), "ns must"), (dict(flip=None), "non-null"), (dict(sign=None), "non-null"),
                         (dict(coeff=None), "non-null"), (dict(out=None), "non-null"), (dict(offset=-1), "sample_offset")]:
        assert call(**kwargs) == -1, kwargs
        assert word in wf.lib.rnnwf_last_error(wf.h).decode(), (kwargs, wf.lib.rnnwf_last_error(wf.h).decode())
    bad = x0.copy()
    bad[0, 4] = 2
    assert call(flip=bad.ctypes.data_as(I32P)) == -1 and "flip[0][4] = 2" in wf.lib.rnnwf_last_error(wf.h).decode()
    assert call(sign=bad.ctypes.data_as(I32P)) == -1 and "sign[0][4] = 2" in wf.lib.rnnwf_last_error(wf.h).decode()
    with pytest.raises(ValueError, match="0 or 1"):
        wf.pauli_step(bad, one, [1.0], 32)
    with pytest.raises(ValueError):
        wf.pauli_step(x0, one, [1.0, 2.0], 32)
    with pytest.raises(ValueError):
        wf.pauli_step(np.zeros((1, N + 1)), np.zeros((1, N + 1)), [1.0], 32)
    # the refused calls left the resident batch usable
    g1 = wf.vmc_gradient(ok["moments"][0] / 32, 32, {"wf_dense/kernel": (10, 2)})["wf_dense/kernel"]
    assert np.array_equal(g0, g1)
    # refused models, with the other observables' reasons (the mask limit has its own test below)
    prm2 = P.init_gru_params([10, 10], seed=1)
    for model, nx, ny, units, prm, word in [
            (_lib.MODEL_GRU1D_PARITY, N, 1, (10,), trained_like(10, 1, False), "parity"),
            (_lib.MODEL_GRU1D, N, 1, (10, 10), prm2, "stacked layers"),
            (_lib.MODEL_CRNN_U1, N, 1, (10,), None, "complex RNN"),
            (_lib.MODEL_MDRNN2D, 3, 2, (10,), None, "MDRNN"),
            (_lib.MODEL_LSTM1D_F64, 3, 2, (10,), None, "LSTM")]:
        w = _lib.NativeWavefunction(model, nx, ny, units)
        if prm is not None:
            w.set_params(prm, scope=SCOPE)
        with pytest.raises(ValueError, match=word):
            w.pauli_step(x0, one, [1.0], 32)
        with pytest.raises(ValueError, match=word):
            O.pauli_expectations(w, ["XIIIII"], 32)
    # the three existing observable entry points refuse as before
    w = _lib.NativeWavefunction(_lib.MODEL_GRU1D_PARITY, N, 1, (10,))
    w.set_params(trained_like(10, 1, False), scope=SCOPE)
    for fn in (lambda: w.renyi2_swap(4), lambda: w.renyi2_regions(x0, 4), lambda: w.correlations(8)):
        with pytest.raises(ValueError, match="parity"):
            fn()


def test_more_than_65535_distinct_masks_are_refused_before_any_work():
    """65 536 distinct non-empty flip masks on N = 17 (the limit is the log-ratio kernel's grid): refused through the C call and the
    facade, before any device work, and the earlier resident batch still gives the same gradient; 65 535 masks are accepted."""
    N, H, ns = 17, 10, 32
    wf = make_wf(False, N, 1, H, trained_like(H, 1, False))
    ham = O.xxz_hamiltonian(N, -1.0, 0.5)
    ok = wf.pauli_step(ham.flip, ham.sign, ham.coeff, ns, seed=1)
    shapes = {"wf_dense/kernel": (H, 2)}
    g0 = wf.vmc_gradient(ok["moments"][0] / ns, ns, shapes)["wf_dense/kernel"]
    k = np.arange(1, 65537)                          # mask k = the binary digits of k: distinct and non-empty
    flip = np.ascontiguousarray(((k[:, None] >> np.arange(N)[None, :]) & 1).astype(np.int32))
    sign = np.zeros_like(flip)
    coeff = np.ones(len(flip))
    sums = np.zeros((len(flip), 2))
    I32P, F64P = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    wf.timing_enable(True)
    wf.timing_reset()
    rc = wf.lib.rnnwf_pauli_step(wf.h, flip.ctypes.data_as(I32P), sign.ctypes.data_as(I32P), coeff.ctypes.data_as(F64P), len(flip), None, ns,
                                 1, 0, 0, sums.ctypes.data_as(F64P), None, None, None, None)
    assert rc == -1 and "more than 65535 distinct flip masks" in wf.lib.rnnwf_last_error(wf.h).decode()
    with pytest.raises(ValueError, match="more than 65535 distinct flip masks"):
        wf.pauli_step(flip, sign, coeff, ns, seed=1)
    # duplicated masks do not count: 65 536 terms on 65 535 masks pass the check (refused calls launched nothing)
    assert sum(wf.timing_get(i)["launches"] for i in range(3)) == 0
    g1 = wf.vmc_gradient(ok["moments"][0] / ns, ns, shapes)["wf_dense/kernel"]
    assert np.array_equal(g0, g1)
    flip[-1] = flip[0]
    out = wf.pauli_step(flip, sign, coeff, 16, seed=1, want_log_ratio=True)
    assert out["log_ratio"].shape == (65535, 16) and np.array_equal(out["term_sums"][-1], out["term_sums"][0])
    assert np.all(np.isfinite(out["term_sums"]))


# 7. gradient hand-over
def test_gradient_of_an_xxz_energy_against_float64_autograd():
    import torch
    from rnnwavefunctions_amd.training import cost_gradient
    N, H, ns = 20, 30, 2000
    prm = trained_like(H, 111, False)
    wf = make_wf(False, N, 1, H, prm)
    ham = O.xxz_hamiltonian(N, -1.0, 0.7, periodic=True)
    out = wf.pauli_step(ham.flip, ham.sign, ham.coeff, ns, seed=111, want_eloc=True, want_samples=True)
    s, e = out["samples"], out["eloc"]
    assert np.isclose(out["moments"][0] / ns, e.mean(), rtol=1e-12) and e.std() > 0.1
    grads = cost_gradient(wf, prm, SCOPE, e.mean(), ns)
    g64 = A.gradient("gru", prm, s, e, dtype=torch.float64)
    g32 = A.gradient("gru", prm, s, e, dtype=torch.float32)
    assert set(grads) == set(prm)
    worst, failures = A.verdict(grads, g64, g32, unit_roundoff_ratio=1.0, label="[pauli xxz]")
    print("[pauli xxz] worst ratio deviation / yardstick = %.3f (bound %g)" % (worst, A.FACTOR))
    assert not failures, "tensors beyond %g x the yardstick: %s" % (A.FACTOR, failures)


# 8. minimising a Hamiltonian that is not hard-wired
def test_minimize_hamiltonian_lowers_the_energy_towards_the_ground_state():
    from rnnwavefunctions_amd import _lib
    from rnnwavefunctions_amd.training import minimize_hamiltonian
    N, H, ns, steps = 8, 20, 1000, 300
    xxz = O.xxz_hamiltonian(N, -1.0, 0.5)            # ferromagnetic XY coupling: the ground state is positive
    ham = O.Hamiltonian(N, xxz.terms + [(-0.8, [("X", i)]) for i in range(N)])
    Hd = sum(c * PR.dense_string({i: p for p, i in st}, N).real for c, st in ham.terms)
    assert np.allclose(Hd, Hd.T)
    e0 = np.linalg.eigvalsh(Hd)[0]
    prm = P.init_gru_params([H], seed=111)
    wf = _lib.NativeWavefunction(_lib.MODEL_GRU1D, N, 1, (H,))
    with pytest.raises(ValueError, match="communicator"):
        minimize_hamiltonian(wf, ham, prm, numsteps=1, numsamples=ns, comm=object())
    mean, var = minimize_hamiltonian(wf, ham, prm, numsteps=steps, numsamples=ns, learningrate=5e-3, seed=111)
    assert len(mean) == len(var) == steps + 1
    err_i, err_f = np.sqrt(var[0] / ns), np.sqrt(var[-1] / ns)
    print("minimize_hamiltonian: E %.4f +- %.4f -> %.4f +- %.4f, ground state %.4f" % (mean[0], err_i, mean[-1], err_f, e0))
    assert mean[-1] < mean[0] - 5.0 * np.hypot(err_i, err_f)
    assert mean[-1] >= e0 - 5.0 * err_f
