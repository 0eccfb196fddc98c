"""GPU tests of the LSTM wave function's Pauli pass (rnnwf_pauli_step_lstm, rnnwf_lstm_pauli_gradient_step,
csrc/lstm_pauli_kernels.h, observables_lstm; docs/pauli_lstm.md).

References: tests/lstm_reference.lstm_log_probability (NumPy float64) as the log P of tests/pauli_reference's brute-force estimator -
every flipped configuration written out and scored from site 0 -, tests/ed.py and pauli_reference's dense operators.  Tolerances, the
project's own for float64 (docs/pauli.md, docs/renyi_regions.md): 1e-11 N on a log-ratio, relative 1e-12 against exact enumeration,
1e-10 on E_loc against rnnwf_tfim2d_eloc.  tests/test_lstm_pauli_host.py shows on the reference alone that the log-ratio bound rejects
a restart from the wrong checkpoint, a cell state restored from h's rows and mask words read from word 0, by factors above 1e8.
"""
import ctypes as C
import time

import numpy as np
import pytest

import autograd_reference as A
import lstm_grad_reference as LG
import lstm_pauli_reference as Q
import lstm_reference as LR
import pauli_reference as PR
from conftest import all_configs
from rnnwavefunctions_amd import observables as O
from rnnwavefunctions_amd import observables_lstm as OL
from rnnwavefunctions_amd import params as P

pytestmark = pytest.mark.gpu
SCOPE = Q.SCOPE


def handle(shape, units, prm=None):
    from rnnwavefunctions_amd import _lib
    wf = _lib.NativeWavefunction(_lib.MODEL_LSTM1D_F64, shape[0], shape[1], (units,))
    if prm is not None:
        wf.set_params(prm, scope=SCOPE)
    return wf


def flips_only(wf, masks, ns, **kw):
    """pauli_step_lstm on pure-X terms, one per mask, coefficient 1"""
    masks = np.asarray(masks)
    return wf.pauli_step_lstm(masks, np.zeros_like(masks), np.ones(len(masks)), ns, **kw)


# ---- 1. log-ratios against explicitly flipped configurations scored in float64 ---------------------------------------------------------

CASES = [(shape, units) for shape in Q.LATTICES for units in Q.WIDTHS]


@pytest.mark.parametrize("shape,units", CASES, ids=["%dx%d-%d" % (s[0], s[1], u) for s, u in CASES])
def test_log_ratios_against_flipped_configurations_in_float64(shape, units):
    Nx, Ny = shape
    N = Nx * Ny
    prm = Q.parameters(units)
    s, masks = Q.samples_of(Nx, Ny, units), Q.masks_of(Nx, Ny)
    firsts = {int(np.flatnonzero(m)[0]) for m in masks}
    assert PR.word_boundaries_covered(N, masks) and {0, N - 1} <= firsts and np.any(masks.sum(axis=1) == N)
    for w in (32, 64):
        assert w >= N or any(np.array_equal(np.flatnonzero(m), [w - 1, w]) for m in masks)
    # the empty mask among the terms: sz_0 (diagonal), between the X strings
    flip = np.concatenate([masks[:1], np.zeros((1, N), dtype=np.int32), masks[1:]])
    sign = np.zeros_like(flip)
    sign[1, 0] = 1
    wf = handle(shape, units, prm)
    out = wf.pauli_step_lstm(flip, sign, np.ones(len(flip)), Q.NS, samples=s, want_log_ratio=True, want_eloc=True)
    wf.close()
    ref = PR.log_ratio_masks(Q.log_p(prm, Nx, Ny), s, masks)
    got = out["log_ratio"]
    err = np.abs(got - ref).max()
    print("LSTMPAULI %dx%d-%d NFULL %d: %d masks, max |log r - float64| = %.2e = %.2e of the bound (max |log r| %.2f)"
          % (Nx, Ny, units, LG.nfull(units), len(masks), err, err / Q.bound(N), np.abs(ref).max()))
    assert got.shape == (len(masks), Q.NS)                    # no row for the empty mask
    assert np.abs(ref).max() > 1e-3
    assert np.all(np.abs(got - ref) <= Q.bound(N))
    z0 = 2.0 * s[:, 0] - 1.0
    assert np.array_equal(out["term_sums"][1], [z0.sum(), float(Q.NS)])               # the diagonal term's sums are exact
    v = np.concatenate([np.exp(got[:1]), z0[None, :], np.exp(got[1:])])
    assert np.allclose(out["term_sums"], PR.sums_from_values(v), rtol=1e-12, atol=0)
    assert np.allclose(out["eloc"], v.sum(axis=0), rtol=1e-12, atol=1e-12)


# ---- 2. bit-for-bit and agreement checks ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape,units", [((4, 3), 20), ((7, 5), 37), ((3, 22), 68)])
def test_f0_path_and_log_p_are_log_probs_bit_for_bit(shape, units):
    """mask {0}: the tail runs all N sites from the zero state, the suffix is the pass's own log P.  Both are the base pass's additions
    in the base pass's order, so 1/2 (tail - log P) is 1/2 (log_prob(flipped) - log_prob(s)) bit for bit.  A diagonal Hamiltonian runs no
    recurrent kernel."""
    Nx, Ny = shape
    N = Nx * Ny
    prm = Q.parameters(units)
    s = Q.samples_of(Nx, Ny, units)
    m = Q.site_mask(N, [0])
    wf = handle(shape, units, prm)
    got = flips_only(wf, m[None, :], Q.NS, samples=s, want_log_ratio=True)["log_ratio"][0]
    ref = 0.5 * (wf.log_prob((s ^ m[None, :]).astype(np.int32)) - wf.log_prob(s))
    print("LSTMPAULI f = 0, %dx%d-%d: max |log r - log_prob's| = %.2e" % (Nx, Ny, units, np.abs(got - ref).max()))
    assert np.all(np.abs(got - ref) <= Q.bound(N))
    assert np.array_equal(got, ref)
    wf.timing_enable(True)
    wf.timing_reset()
    zz = np.zeros((1, N), dtype=np.int32)
    sg = zz.copy()
    sg[0, :2] = 1
    out = wf.pauli_step_lstm(zz, sg, [0.5], Q.NS, samples=s, want_eloc=True, want_log_ratio=True)
    assert wf.timing_get(0)["launches"] == 0 and wf.timing_get(1)["launches"] == 0
    wf.close()
    assert out["log_ratio"].shape == (0, Q.NS)
    assert np.array_equal(out["eloc"], 0.5 * (2.0 * s[:, 0] - 1.0) * (2.0 * s[:, 1] - 1.0))


@pytest.mark.parametrize("shape,units", [((4, 3), 20), ((7, 5), 50)])
def test_single_x_terms_and_tfim_energy_against_tfim2d_eloc(shape, units):
    Nx, Ny = shape
    N, ns = Nx * Ny, 300
    wf = handle(shape, units, Q.parameters(units))
    s = wf.sample(ns, seed=3).reshape(ns, N)
    Jz = np.random.RandomState(1).uniform(0.5, 1.5, size=(Nx, Ny))
    lpq = np.empty((N + 1, ns))
    e_ref = wf.tfim_eloc(s, Jz.ravel(), 1.3, log_probs=lpq)
    out = flips_only(wf, np.eye(N, dtype=np.int32), ns, samples=s, want_log_ratio=True)
    err = np.abs(out["log_ratio"] - 0.5 * (lpq[1:] - lpq[0][None, :])).max()
    e = OL.energy(wf, OL.tfim_hamiltonian(Jz, 1.3), ns, samples=s, want_eloc=True)
    wf.close()
    worst = np.abs(e["eloc"] - e_ref).max()
    print("LSTMPAULI %dx%d-%d: max |log r_i - queue| = %.2e; max |E_loc - tfim2d_eloc| = %.2e" % (Nx, Ny, units, err, worst))
    assert err <= Q.bound(N)
    assert worst <= 1e-10
    assert abs(e["mean"] - e_ref.mean()) <= 1e-10


# ---- 3. exact enumeration -------------------------------------------------------------------------------------------------------------
# 3 x 4, 10 units, init_lstm_params(seed 20) with kernels x 3 and biases randomised: no exact value below 0.02 in magnitude (float64
# reference: 0.023 is the smallest)
EXACT = dict(shape=(3, 4), units=10, seed=20, floor=0.02)


def exact_strings(N):
    return [[("X", 0)], [("X", N - 1)], [("Z", 0)], [("Z", 2), ("Z", 3)], [("X", 1), ("X", 2)], [("Y", 1), ("Y", 2)],
            [("X", 0), ("Z", 1), ("X", 2)], [("Z", 0), ("X", 1), ("Z", 2)], [("Z", 2), ("Z", 3), ("X", 7)],
            [("Y", 0), ("Z", 2), ("Z", 3), ("Y", 1)], [("X", i) for i in range(N)], [("Z", 3), ("X", 5)],
            [("X", 0), ("X", 1), ("X", N - 1)], [("Z", 0), ("X", N - 1)]]


def exact_case():
    Nx, Ny = EXACT["shape"]
    N = Nx * Ny
    prm = P.randomize_biases(P.scale_kernels(P.init_lstm_params([EXACT["units"]], seed=EXACT["seed"]), 3.0), EXACT["seed"] + 1)
    c = all_configs(N)
    lp = LR.lstm_log_probability(prm, c, Nx, Ny)
    psi = np.exp(0.5 * lp)
    assert abs(psi @ psi - 1.0) < 1e-12
    strings = exact_strings(N)
    exact = np.array([(psi @ PR.dense_string({i: p for p, i in st}, N) @ psi).real for st in strings])
    assert len(strings) == 14 and np.abs(exact).min() >= EXACT["floor"]
    return prm, c, lp, strings, exact


def test_exact_enumeration_against_dense_operators():
    prm, c, lp, strings, exact = exact_case()
    N = c.shape[1]
    wf = handle(EXACT["shape"], EXACT["units"], prm)
    flip, sign, factor = O.pauli_terms(strings, N)
    assert np.all(factor.imag == 0)
    out = wf.pauli_step_lstm(flip, sign, factor.real, len(c), samples=c, want_log_ratio=True, want_eloc=True)
    wf.close()
    _, index = O.group_by_mask(flip)
    v = PR.signs(c, sign) * np.where(index[:, None] >= 0, np.exp(out["log_ratio"][np.maximum(index, 0)]), 1.0)
    got = factor.real * (np.exp(lp)[None, :] * v).sum(axis=1)
    rel = np.abs(got / exact - 1.0)
    print("LSTMPAULI exact 3x4: values %s, max rel %.2e" % (np.round(exact, 4), rel.max()))
    assert rel.max() <= 1e-12
    assert np.allclose(out["term_sums"], PR.sums_from_values(v), rtol=1e-12, atol=1e-12 * len(c))
    assert np.allclose(out["eloc"], factor.real @ v, rtol=1e-12, atol=1e-12)
    m = out["moments"]
    assert m[2] == len(c) and np.isclose(m[0], out["eloc"].sum(), rtol=1e-12) and np.isclose(m[1], (out["eloc"] ** 2).sum(), rtol=1e-12)


def test_device_drawn_expectations_within_five_standard_errors():
    prm, c, lp, strings, exact = exact_case()
    wf = handle(EXACT["shape"], EXACT["units"], prm)
    out = OL.pauli_expectations(wf, strings + [[("Y", 3)], [("X", 1), ("Y", 2), ("Z", 3)]], 2 ** 16, seed=111)
    wf.close()
    z = np.abs(out["value"][:-2] - exact) / out["err"][:-2]
    print("LSTMPAULI drawn 3x4: |z| %s" % np.round(z, 2))
    assert np.all(out["err"][:-2] > 0) and z.max() <= 5.0
    assert np.all(out["value"][-2:] == 0) and np.all(out["err"][-2:] == 0)          # odd n_Y


# ---- 4. passes, shards, refusals ----------------------------------------------------------------------------------------------------------

def xxz_lattice(Nx, Ny, Jxy=-1.0, Jz=0.5):
    """XXZ couplings on the raster chain of Nx * Ny sites; Jxy < 0: stoquastic (every off-diagonal element <= 0)"""
    return OL.xxz_hamiltonian(Nx * Ny, Jxy, Jz)


def test_several_passes_shards_and_drawn_samples(monkeypatch):
    shape, units, ns = (7, 5), 21, 1000
    N = 35
    prm = Q.parameters(units)
    ham = xxz_lattice(*shape)
    kw = dict(seed=5, step=2, want_eloc=True, want_log_ratio=True, want_samples=True)
    wf = handle(shape, units, prm)
    wf.timing_enable(True)
    wf.timing_reset()
    a = wf.pauli_step_lstm(ham.flip, ham.sign, ham.coeff, ns, **kw)
    firsts = sorted({int(np.flatnonzero(r)[0]) for r in ham.flip if r.any()})
    assert wf.timing_get(1)["launches"] == 1 and wf.timing_get(1)["cell_evals"] == ns * sum(N - f for f in firsts)
    assert np.array_equal(a["samples"], wf.sample(ns, seed=5, step=2).reshape(ns, N))
    b = wf.pauli_step_lstm(ham.flip, ham.sign, ham.coeff, ns, **kw)
    for k in ("term_sums", "moments", "eloc", "log_ratio", "samples"):
        assert np.array_equal(a[k], b[k]), k
    cut = 336
    s1 = wf.pauli_step_lstm(ham.flip, ham.sign, ham.coeff, cut, sample_offset=0, **kw)
    s2 = wf.pauli_step_lstm(ham.flip, ham.sign, ham.coeff, ns - cut, sample_offset=cut, **kw)
    assert np.array_equal(np.concatenate([s1["samples"], s2["samples"]]), a["samples"])
    assert np.array_equal(np.concatenate([s1["eloc"], s2["eloc"]]), a["eloc"])
    assert np.array_equal(np.concatenate([s1["log_ratio"], s2["log_ratio"]], axis=1), a["log_ratio"])
    assert np.allclose(s1["term_sums"] + s2["term_sums"], a["term_sums"], rtol=1e-13, atol=1e-12)
    assert wf.resident_samples() == 0
    wf.close()
    monkeypatch.setenv("RNNWF_STATE_BUDGET_MB", "1")
    wf1 = handle(shape, units, prm)
    wf1.timing_enable(True)
    wf1.timing_reset()
    m = wf1.pauli_step_lstm(ham.flip, ham.sign, ham.coeff, ns, **kw)
    passes = wf1.timing_get(1)["launches"]
    print("LSTMPAULI RNNWF_STATE_BUDGET_MB=1: %d passes" % passes)
    assert passes >= 3
    for k in ("eloc", "log_ratio", "samples"):
        assert np.array_equal(m[k], a[k]), k
    assert np.allclose(m["term_sums"], a["term_sums"], rtol=1e-13, atol=1e-12) and np.allclose(m["moments"][:3], a["moments"][:3], rtol=1e-13)
    assert wf1.resident_samples() == 0                            # no resident state claimed
    # the fused step holds one pass: past it, it is refused and the gradient of an earlier call stays
    g0 = wf1.lstm_pauli_gradient_step(ham.flip, ham.sign, ham.coeff, 32, 5, 2, LG.shapes(prm))["grads"]
    from rnnwavefunctions_amd import _lib
    with pytest.raises(_lib.RnnwfError, match="rnnwf_lstm_pauli_gradient_step: 1000 samples exceed the state budget of one pass; split the batch"):
        wf1.lstm_pauli_gradient_step(ham.flip, ham.sign, ham.coeff, ns, 5, 2, LG.shapes(prm))
    g1 = wf1._grads(LG.shapes(prm))
    assert all(np.array_equal(g0[k], g1[k]) and np.any(g0[k] != 0) for k in g0)
    wf1.close()


def test_refusals_through_the_c_call_and_the_module():
    from rnnwavefunctions_amd import _lib
    shape, units, N, ns = (3, 2), 10, 6, 32
    prm = LG.parameters(units)
    shapes = LG.shapes(prm)
    wf = handle(shape, units, prm)
    one = np.zeros((1, N), dtype=np.int32)
    x0 = one.copy()
    x0[0, 0] = 1
    before = wf.lstm_pauli_gradient_step(x0, one, [1.0], ns, 1, 0, shapes)["grads"]
    params_before = wf.get_params_dict(prm, SCOPE)
    I32P, F64P = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    fp, sp = x0.ctypes.data_as(I32P), one.ctypes.data_as(I32P)
    co, sums, mom = np.ones(1), np.zeros((1, 2)), np.zeros(4)
    cp, up, mp = co.ctypes.data_as(F64P), sums.ctypes.data_as(F64P), mom.ctypes.data_as(F64P)
    bad = x0.copy()
    bad[0, 4] = 2

    def step(flip=fp, sign=sp, coeff=cp, K=1, n=ns, offset=0, out=up):
        return wf.lib.rnnwf_pauli_step_lstm(wf.h, flip, sign, coeff, K, None, n, 1, 0, offset, out, None, None, None, None)

    def fused(flip=fp, sign=sp, coeff=cp, K=1, n=ns, offset=0, out=up, moments=mp):
        return wf.lib.rnnwf_lstm_pauli_gradient_step(wf.h, flip, sign, coeff, K, n, 1, 0, offset, moments, out, None, None)

    for call, entry in ((step, "rnnwf_pauli_step_lstm"), (fused, "rnnwf_lstm_pauli_gradient_step")):
        for kwargs, word in [(dict(K=0), "nterms must be >= 1"), (dict(n=0), "must be >= 1"), (dict(flip=None), "non-null"),
                             (dict(sign=None), "non-null"), (dict(coeff=None), "non-null"), (dict(offset=-1), "sample_offset must be >= 0"),
                             (dict(flip=bad.ctypes.data_as(I32P)), "flip[0][4] = 2, a mask entry must be 0 or 1"),
                             (dict(sign=bad.ctypes.data_as(I32P)), "sign[0][4] = 2, a mask entry must be 0 or 1")]:
            assert call(**kwargs) == -1, (entry, kwargs)
            msg = wf.lib.rnnwf_last_error(wf.h).decode()
            assert msg.startswith(entry + ":") and word in msg, (kwargs, msg)
    assert step(out=None) == -1 and fused(moments=None) == -1
    with pytest.raises(ValueError, match="0 or 1"):
        wf.pauli_step_lstm(bad, one, [1.0], ns)
    with pytest.raises(ValueError, match="0 or 1"):
        wf.lstm_pauli_gradient_step(bad, one, [1.0], ns, 1, 0, shapes)
    with pytest.raises(ValueError):
        wf.pauli_step_lstm(x0, one, [1.0, 2.0], ns)
    # the refused calls left the gradient and the parameters as they were
    after = wf._grads(shapes)
    assert all(np.array_equal(before[k], after[k]) and np.any(before[k] != 0) for k in before)
    params_after = wf.get_params_dict(prm, SCOPE)
    assert all(np.array_equal(params_before[k], params_after[k]) for k in prm)
    again = wf.lstm_pauli_gradient_step(x0, one, [1.0], ns, 1, 0, shapes)["grads"]
    assert all(np.array_equal(before[k], again[k]) for k in before)
    wf.close()
    # parameters not committed
    raw = handle(shape, units)
    with pytest.raises(_lib.RnnwfError, match="parameters not committed"):
        raw.pauli_step_lstm(x0, one, [1.0], ns)
    with pytest.raises(_lib.RnnwfError, match="parameters not committed"):
        raw.lstm_pauli_gradient_step(x0, one, [1.0], ns, 1, 0, shapes)
    raw.close()
    # every other model, by name, with the entry (C call) or module that serves it
    gprm = P.init_gru_params([10], seed=1)
    for model, nx, ny, un, p, name, entry, module in [
            (_lib.MODEL_GRU1D, N, 1, (10,), gprm, "GRU1D", "rnnwf_pauli_step serves", r"observables\.py"),
            (_lib.MODEL_GRU1D_F64, 3, 2, (10,), P.init_gru_params([10], seed=1, dtype=np.float64), "GRU1D_F64", "rnnwf_pauli_step serves",
             r"observables\.py"),
            (_lib.MODEL_GRU1D, N, 1, (10, 10), P.init_gru_params([10, 10], seed=1), "GRU1D", "rnnwf_pauli_step_stack serves", "observables_stack"),
            (_lib.MODEL_GRU1D_PARITY, N, 1, (10,), gprm, "GRU1D_PARITY", "parity", "parity"),
            (_lib.MODEL_CRNN_U1, N, 1, (10,), None, "CRNN_U1", "rnnwf_pauli_step_complex serves", "observables_complex"),
            (_lib.MODEL_MDRNN2D, 3, 2, (10,), None, "MDRNN2D", "rnnwf_pauli_step_2d serves", "observables_2d")]:
        w = _lib.NativeWavefunction(model, nx, ny, un)
        if p is not None:
            w.set_params(p, scope=SCOPE)
        with pytest.raises(ValueError, match="rnnwf_pauli_step_lstm: serves the LSTM cell .* this handle's model is %s; .*%s" % (name, entry)):
            w.pauli_step_lstm(x0, one, [1.0], ns)
        with pytest.raises(ValueError, match="rnnwf_lstm_pauli_gradient_step: serves the LSTM cell .* this handle's model is %s; .*%s" % (name, entry)):
            w.lstm_pauli_gradient_step(x0, one, [1.0], ns, 1, 0, shapes)
        with pytest.raises(ValueError, match=module):
            OL.pauli_expectations(w, ["XIIIII"], ns)
        w.close()


# ---- 5. the fused gradient step ---------------------------------------------------------------------------------------------------------------

# 13 x 5: 65 sites, the backward pass's spin-word walk refetches word 0 at n = 64 (tests/test_gpu_lstm_grad.py)
@pytest.mark.parametrize("shape,units", [((4, 3), 20), ((4, 3), 53), ((13, 5), 37)], ids=["20", "53", "13x5-37"])
def test_fused_step_is_pauli_step_plus_lstm_gradient_bit_for_bit(shape, units):
    ns = 200
    prm = LG.parameters(units, sharp=1.5)
    ham = xxz_lattice(*shape)
    wf = handle(shape, units, prm)
    kw = dict(want_samples=True, want_eloc=True)
    fused = wf.lstm_pauli_gradient_step(ham.flip, ham.sign, ham.coeff, ns, 111, 3, LG.shapes(prm), **kw)
    two = wf.pauli_step_lstm(ham.flip, ham.sign, ham.coeff, ns, seed=111, step=3, **kw)
    for k in ("moments", "samples", "eloc", "term_sums"):
        assert np.array_equal(fused[k], two[k]), k
    s1, _, n, _ = two["moments"]
    g = wf.lstm_gradient(two["samples"], (two["eloc"] - s1 / n) * (1.0 / n), LG.shapes(prm))
    again = wf.lstm_pauli_gradient_step(ham.flip, ham.sign, ham.coeff, ns, 111, 3, LG.shapes(prm), **kw)
    wf.close()
    assert set(g) == set(fused["grads"])
    for k in g:
        assert np.any(g[k] != 0.0), k
        assert np.array_equal(g[k], fused["grads"][k]), k
        assert np.array_equal(again["grads"][k], fused["grads"][k]), k                # a repeated call is bit-identical
    for k in ("moments", "samples", "eloc", "term_sums"):
        assert np.array_equal(again[k], fused[k]), k


def test_fused_gradient_against_float64_autograd():
    shape, units, ns = (4, 3), 20, 200
    prm = LG.parameters(units, sharp=1.5)
    ham = xxz_lattice(*shape)
    wf = handle(shape, units, prm)
    out = wf.lstm_pauli_gradient_step(ham.flip, ham.sign, ham.coeff, ns, 111, 3, LG.shapes(prm), want_samples=True, want_eloc=True)
    wf.close()
    s1, _, n, _ = out["moments"]
    assert out["eloc"].std() > 0.1
    e_ref = PR.local_energy(Q.log_p(prm, *shape), out["samples"], ham.flip, ham.sign, ham.coeff)
    assert np.abs(out["eloc"] - e_ref).max() <= 1e-10
    ref = LG.reference(prm, out["samples"], (out["eloc"] - s1 / n) * (1.0 / n))
    worst, failures = LG.judge("[lstm pauli xxz 4x3-20]", LG.scoped(out["grads"]), ref)
    print("LSTMPAULI fused gradient: worst deviation / bound %.3f (limit %g)" % (worst, A.FACTOR))
    assert not failures, "tensors beyond %g x the bound: %s" % (A.FACTOR, failures)


# ---- 6. training ----------------------------------------------------------------------------------------------------------------------------------

TRAIN = dict(shape=(3, 3), Jxy=-1.0, Jz=0.5, units=10, ns=200, numsteps=300, lr=1e-2, gru_seeds=(333, 334, 335, 336, 337))


def ScheduledAdam():
    """training.Adam at the learning rate of run_2DTFIM_1DRNN_LSTM, 1 / (1 / lr + it / 10): training.minimize_hamiltonian hands every
    iteration the same lr, so the rule is applied here, with it = the updates applied so far"""
    from rnnwavefunctions_amd import training

    class Scheduled(training.Adam):
        def step(self, params, grads, lr):
            return super().step(params, grads, OL.lr_schedule(lr, self.t))
    return Scheduled()


def test_training_closes_the_gap_to_the_ground_energy_as_the_gru_does():
    """3 x 3 raster chain, stoquastic XXZ (Jxy = -1, Jz = 0.5), 10 units, 200 samples, 300 iterations at 1 / (100 + it / 10):
    observables_lstm.minimize_hamiltonian (seed 333) against the one-layer float64 GRU through training.minimize_hamiltonian at the same
    settings (seeds 333..337).  Exact variational energies over all 512 configurations.  The LSTM's final gap to the ED ground energy
    may reach the worst GRU gap times the GRU's seed-to-seed spread (max / min), docs/lstm.md's rule.  The gaps measured on MI355X are in
    docs/pauli_lstm.md."""
    import torch
    from rnnwavefunctions_amd import _lib, training
    Nx, Ny = TRAIN["shape"]
    N = Nx * Ny
    t0 = time.time()
    ham = xxz_lattice(Nx, Ny, TRAIN["Jxy"], TRAIN["Jz"])
    Hd = sum(c * PR.dense_string({i: p for p, i in st}, N).real for c, st in ham.terms)
    assert np.allclose(Hd, Hd.T) and np.all(Hd - np.diag(np.diag(Hd)) <= 0)          # stoquastic: the ground state is positive
    e0 = float(np.linalg.eigvalsh(Hd)[0])
    cfgs = all_configs(N)

    def exact_energy(lp):
        psi = np.exp(0.5 * lp)
        assert abs(psi @ psi - 1.0) < 1e-10
        return float(psi @ Hd @ psi)

    kw = dict(numsteps=TRAIN["numsteps"], numsamples=TRAIN["ns"], learningrate=TRAIN["lr"])
    prm = P.init_lstm_params([TRAIN["units"]], seed=111, scope=SCOPE)
    e_init = exact_energy(LR.lstm_log_probability(prm, cfgs, Nx, Ny))
    wf = handle(TRAIN["shape"], TRAIN["units"])
    mean, var = OL.minimize_hamiltonian(wf, ham, prm, seed=333, **kw)
    wf.close()
    e_lstm = exact_energy(LR.lstm_log_probability(OL.minimize_hamiltonian.last_params, cfgs, Nx, Ny))
    assert len(mean) == len(var) == TRAIN["numsteps"] + 1
    gprm = P.init_gru_params([TRAIN["units"]], seed=111, dtype=np.float64)
    gru_init = exact_energy(A.prnn_log_probability(A.to_torch(gprm, torch.float64), cfgs).numpy())
    gru_gaps = []
    for seed in TRAIN["gru_seeds"]:
        g = _lib.NativeWavefunction(_lib.MODEL_GRU1D_F64, Nx, Ny, (TRAIN["units"],))
        training.minimize_hamiltonian(g, ham, {k: v.copy() for k, v in gprm.items()}, seed=seed, opt=ScheduledAdam(), **kw)
        g.close()
        lp = A.prnn_log_probability(A.to_torch(training.minimize_hamiltonian.last_params, torch.float64), cfgs).numpy()
        gru_gaps.append(exact_energy(lp) - e0)
    spread = max(gru_gaps) / min(gru_gaps)
    print("LSTMPAULITRAIN ED %.6f; LSTM exact energy %.6f -> %.6f (gap %.4e); GRU %.6f -> gaps %s, worst %.4e, spread %.3f; allowed LSTM "
          "gap %.4e; %.1f s" % (e0, e_init, e_lstm, e_lstm - e0, gru_init, " ".join("%.4e" % g for g in gru_gaps), max(gru_gaps), spread,
                               max(gru_gaps) * spread, time.time() - t0))
    assert all(g < gru_init - e0 for g in gru_gaps)               # every GRU seed trained at these settings
    assert e_lstm < e_init
    assert e_lstm - e0 <= max(gru_gaps) * spread


def test_five_iterations_equal_a_hand_written_loop_bit_for_bit():
    from rnnwavefunctions_amd import training
    shape, units, ns = (3, 3), 10, 200
    ham = xxz_lattice(*shape)
    prm = P.init_lstm_params([units], seed=111, scope=SCOPE)
    wf = handle(shape, units)
    mean, var = OL.minimize_hamiltonian(wf, ham, {k: v.copy() for k, v in prm.items()}, numsteps=4, numsamples=ns, learningrate=1e-2, seed=333)
    trained = OL.minimize_hamiltonian.last_params
    wf.close()
    wf = handle(shape, units)
    p = {k: v.copy() for k, v in prm.items()}
    wf.set_params(p, scope=SCOPE)
    opt, mean_h, var_h = training.Adam(), [], []
    for it in range(5):
        out = wf.lstm_pauli_gradient_step(ham.flip, ham.sign, ham.coeff, ns, 333, it, LG.shapes(p))
        s1, s2, n, _ = out["moments"]
        mean_h.append(s1 / n)
        var_h.append(s2 / n - (s1 / n) ** 2)
        p = opt.step(p, LG.scoped(out["grads"]), 1.0 / ((1.0 / 1e-2) + it / 10))
        wf.set_params(p, scope=SCOPE)
    wf.close()
    assert len(mean) == 5 and np.array_equal(mean, mean_h) and np.array_equal(var, var_h)
    assert all(np.array_equal(trained[k], p[k]) and not np.array_equal(trained[k], prm[k]) for k in prm)
