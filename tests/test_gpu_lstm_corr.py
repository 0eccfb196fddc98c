"""GPU tests of the LSTM wave function's all-pair correlation pass (rnnwf_correlations_lstm, csrc/lstm_corr_kernels.h,
observables_lstm.correlation_matrix; docs/correlations_lstm.md).

References: tests/lstm_reference.lstm_log_probability (NumPy float64) under tests/correlations_reference's brute-force estimator - every
flipped configuration written out and scored from site 0 - and its dense-vector values.  Tolerances, the project's own for float64
(docs/correlations.md, docs/pauli_lstm.md): 1e-11 N on a log-ratio, relative 1e-12 on the device sums against math.fsum and on
sum_s P(s) r against dense operators; z and zz sums are integers and compared with ==.  tests/test_lstm_corr_host.py shows on the
reference alone that the log-ratio bound rejects six defects of the trunk / branch bookkeeping on these inputs by factors above 1e9.
"""
import ctypes as C

import numpy as np
import pytest

import correlations_reference as CR
import lstm_corr_reference as LC
import lstm_grad_reference as LG
import lstm_reference as LR
from conftest import all_configs
from rnnwavefunctions_amd import observables as O
from rnnwavefunctions_amd import observables_lstm as OL
from rnnwavefunctions_amd import params as P

pytestmark = pytest.mark.gpu
SCOPE = LC.SCOPE


def handle(shape, units, prm=None):
    from rnnwavefunctions_amd import _lib
    wf = _lib.NativeWavefunction(_lib.MODEL_LSTM1D_F64, shape[0], shape[1], (units,))
    if prm is not None:
        wf.set_params(prm, scope=SCOPE)
    return wf


def evaluations(N):
    return N * (N - 1) // 2 + N * (N - 1) * (N - 2) // 6


def check_sums(out, s, N):
    """the four sums against the returned log-ratios (math.fsum, relative 1e-12) and the spins (integers, ==)"""
    z, zz = CR.diag_sums(s)
    assert np.array_equal(out["z_sums"], z) and np.array_equal(out["zz_sums"], zz)
    x, xx = CR.sums_from_log_ratio(out["log_ratio"], N)
    assert np.allclose(out["x_sums"], x, rtol=1e-12, atol=0)
    assert np.allclose(out["xx_sums"], xx, rtol=1e-12, atol=0)
    assert np.all(out["xx_sums"][np.tril_indices(N)] == 0)


# ---- 1. every log r against explicitly flipped configurations scored in float64 -------------------------------------------------------

@pytest.mark.parametrize("units", LC.WIDTHS)
def test_every_log_ratio_against_flipped_configurations_every_width(units):
    Nx, Ny = LC.ALL_PAIRS
    N = Nx * Ny
    prm = LC.parameters(units)
    s = LC.samples_of(Nx, Ny, units)
    wf = handle(LC.ALL_PAIRS, units, prm)
    out = wf.correlations_lstm(LC.NS, samples=s, want_log_ratio=True)
    lp = wf.log_prob(s)
    wf.close()
    pi, pj = LC.checked_pairs(N)
    assert len(pi) == 66
    ref = LC.brute_force(prm, LC.ALL_PAIRS, s, pi, pj)
    got = out["log_ratio"]
    err = np.abs(got - ref).max()
    print("LSTMCORR %dx%d-%d NFULL %d: %d rows, max |log r - float64| = %.2e = %.2e of the bound (max |log r| %.2f)"
          % (Nx, Ny, units, LG.nfull(units), len(ref), err, err / LC.bound(N), np.abs(ref).max()))
    assert got.shape == (N + 66, LC.NS) == ref.shape
    assert np.abs(ref).max() > 1e-3
    assert np.all(np.abs(got - ref) <= LC.bound(N))
    check_sums(out, s, N)
    assert np.all(np.abs(lp - LR.lstm_log_probability(prm, s, Nx, Ny, scope=SCOPE)) <= LC.bound(N))


CASES = [(shape, units) for shape in LC.LATTICES for units in LC.LATTICE_WIDTHS]


@pytest.mark.parametrize("shape,units", CASES, ids=["%dx%d-%d" % (s[0], s[1], u) for s, u in CASES])
def test_log_ratios_on_one_to_three_spin_words(shape, units):
    Nx, Ny = shape
    N = Nx * Ny
    prm = LC.parameters(units)
    s = LC.samples_of(Nx, Ny, units)
    wf = handle(shape, units, prm)
    out = wf.correlations_lstm(LC.NS, samples=s.reshape(LC.NS, Nx, Ny), want_log_ratio=True)      # the (ns, Nx, Ny) form
    wf.close()
    pi, pj = LC.checked_pairs(N)
    LC.check_subset(N, pi, pj)
    ref = LC.brute_force(prm, shape, s, pi, pj)
    got = out["log_ratio"]
    assert got.shape == (N + N * (N - 1) // 2, LC.NS) and np.all(np.isfinite(got))
    sub = got[LC.rows_of(N, pi, pj)]
    err = np.abs(sub - ref).max()
    print("LSTMCORR %dx%d-%d NFULL %d: %d of %d rows checked, max |log r - float64| = %.2e = %.2e of the bound (max |log r| %.2f)"
          % (Nx, Ny, units, LG.nfull(units), len(ref), len(got), err, err / LC.bound(N), np.abs(ref).max()))
    assert np.abs(ref).max() > 1e-3
    assert np.all(np.abs(sub - ref) <= LC.bound(N))
    check_sums(out, s, N)


# ---- 2. the existing path ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape,units", [((4, 3), 20), ((7, 5), 37), ((11, 3), 68)])
def test_agrees_with_the_pauli_pass_and_log_prob(shape, units):
    Nx, Ny = shape
    N = Nx * Ny
    prm = LC.parameters(units)
    s = LC.samples_of(Nx, Ny, units)
    pi, pj = LC.checked_pairs(N)
    masks = np.zeros((N + len(pi), N), dtype=np.int32)
    masks[np.arange(N), np.arange(N)] = 1
    masks[N + np.arange(len(pi)), pi] = 1
    masks[N + np.arange(len(pi)), pj] = 1
    flipped = s.copy()
    flipped[:, 0] ^= 1
    wf = handle(shape, units, prm)
    out = wf.correlations_lstm(LC.NS, samples=s, want_log_ratio=True)
    ref = wf.pauli_step_lstm(masks, np.zeros_like(masks), np.ones(len(masks)), LC.NS, samples=s, want_log_ratio=True)["log_ratio"]
    lp, lp_f = wf.log_prob(s), wf.log_prob(flipped)
    wf.close()
    err = np.abs(out["log_ratio"][LC.rows_of(N, pi, pj)] - ref).max()
    # bsel summed is log P: log r_0 = 1/2 (both[0] + the trunk's sites - the sum of bsel over the sites above 0), and
    # 1/2 (log_prob(site 0 flipped) - log_prob) is the same quantity from the base pass's own additions
    err_0 = np.abs(out["log_ratio"][0] - 0.5 * (lp_f - lp)).max()
    print("LSTMCORR %dx%d-%d against pauli_step_lstm: max |d log r| = %.2e = %.2e of the bound; log r_0 against log_prob %.2e"
          % (Nx, Ny, units, err, err / LC.bound(N), err_0))
    assert err <= 2 * LC.bound(N) and err_0 <= 2 * LC.bound(N)


# ---- 3. exact enumeration -----------------------------------------------------------------------------------------------------------------
# tests/test_gpu_lstm_pauli.py's EXACT: 3 x 4, 10 units, init_lstm_params(seed 20) with kernels x 3 and biases randomised.  Chosen on
# the CPU by enumeration over seeds 20..23: seed 20 has its largest exact connected xx at (1, 11), 0.0402 (asserted > 0.02 below)
EXACT = dict(shape=(3, 4), units=10, seed=20, floor=0.02)


def exact_case():
    Nx, Ny = EXACT["shape"]
    N = Nx * Ny
    prm = P.randomize_biases(P.scale_kernels(P.init_lstm_params([EXACT["units"]], seed=EXACT["seed"]), 3.0), EXACT["seed"] + 1)
    c = all_configs(N)
    lp = LR.lstm_log_probability(prm, c, Nx, Ny)
    assert abs(np.exp(lp).sum() - 1.0) < 1e-12
    z, zz, x, xx = CR.exact_from_log_probs(lp, N)
    assert (xx - np.outer(x, x))[np.triu_indices(N, 1)].max() > EXACT["floor"]
    return prm, c, lp, dict(z=z, zz=zz, x=x, xx=xx, zz_c=zz - np.outer(z, z), xx_c=xx - np.outer(x, x))


def test_exact_enumeration_against_dense_vector_values():
    prm, c, lp, exact = exact_case()
    N = c.shape[1]
    wf = handle(EXACT["shape"], EXACT["units"], prm)
    out = wf.correlations_lstm(len(c), samples=c, want_log_ratio=True)
    wf.close()
    p = np.exp(lp)
    r = np.exp(out["log_ratio"])
    x = r[:N] @ p
    pi, pj = CR.pair_list(N)
    xx = r[N:] @ p
    rel = max(np.abs(x / exact["x"] - 1.0).max(), np.abs(xx / exact["xx"][pi, pj] - 1.0).max())
    print("LSTMCORR exact 3x4: x %.4f..%.4f, xx %.4f..%.4f, max rel %.2e" % (x.min(), x.max(), xx.min(), xx.max(), rel))
    assert rel <= 1e-12
    check_sums(out, c, N)


def test_device_drawn_samples_within_five_standard_errors():
    prm, c, lp, exact = exact_case()
    N = c.shape[1]
    wf = handle(EXACT["shape"], EXACT["units"], prm)
    got = OL.correlation_matrix(wf, 2 ** 16, seed=111)
    wf.close()
    off = ~np.eye(N, dtype=bool)
    worst = {}
    for k in ("z", "x"):
        assert np.all(got[k + "_err"] > 0)
        worst[k] = (np.abs(got[k] - exact[k]) / got[k + "_err"]).max()
    for k in ("zz", "xx", "zz_c", "xx_c"):
        assert np.all(got[k + "_err"][off] > 0)
        worst[k] = (np.abs(got[k] - exact[k])[off] / got[k + "_err"][off]).max()
    print("LSTMCORR drawn 3x4, 2^16 samples: worst |z| " + ", ".join("%s %.2f" % kv for kv in worst.items()))
    assert max(worst.values()) <= 5.0


def test_zero_kernels_give_the_product_states_closed_form():
    shape, units = (7, 5), 37
    N = 35
    prm = P.randomize_biases(P.scale_kernels(P.init_lstm_params([units], seed=5), 0.0), 6)
    s = LC.samples_of(shape[0], shape[1], units)
    wf = handle(shape, units, prm)
    got = wf.correlations_lstm(LC.NS, samples=s, want_log_ratio=True)["log_ratio"]
    wf.close()
    ref = LC.product_state_log_ratios(prm, s)
    err = np.abs(got - ref).max()
    print("LSTMCORR zero kernels 7x5-37: max |log r - closed form| = %.2e = %.2e of the bound" % (err, err / LC.bound(N)))
    assert np.abs(ref).max() > 1e-3 and err <= LC.bound(N)


# ---- 4. determinism, shards, passes, small batches, short chains ---------------------------------------------------------------------------

KEYS = ("z_sums", "zz_sums", "x_sums", "xx_sums", "log_ratio", "samples")


def test_repeated_call_shards_and_drawn_samples():
    shape, units, ns, cut = (4, 3), 21, 100, 48
    N = 12
    wf = handle(shape, units, LC.parameters(units))
    kw = dict(seed=5, step=2, want_log_ratio=True, want_samples=True)
    a = wf.correlations_lstm(ns, **kw)
    b = wf.correlations_lstm(ns, **kw)
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(a["samples"], wf.sample(ns, seed=5, step=2).reshape(ns, N))
    check_sums(a, a["samples"], N)
    s1 = wf.correlations_lstm(cut, sample_offset=0, **kw)
    s2 = wf.correlations_lstm(ns - cut, sample_offset=cut, **kw)
    wf.close()
    assert np.array_equal(np.concatenate([s1["samples"], s2["samples"]]), a["samples"])
    assert np.array_equal(np.concatenate([s1["log_ratio"], s2["log_ratio"]], axis=1), a["log_ratio"])
    for k in ("z_sums", "zz_sums"):
        assert np.array_equal(s1[k] + s2[k], a[k]), k
    for k in ("x_sums", "xx_sums"):
        assert np.allclose(s1[k] + s2[k], a[k], rtol=1e-12, atol=0), k


def test_several_passes_under_the_state_budget(monkeypatch):
    shape, units, ns = (4, 3), 21, 100
    prm = LC.parameters(units)
    kw = dict(seed=5, step=2, want_log_ratio=True, want_samples=True)
    wf = handle(shape, units, prm)
    a = wf.correlations_lstm(ns, **kw)
    wf.close()
    # per 16-chain block 77 state rows of 9 216 bytes and 312 rows of 128: 0.75 MB - two blocks per pass, four passes
    monkeypatch.setenv("RNNWF_STATE_BUDGET_MB", "2")
    wf1 = handle(shape, units, prm)
    wf1.timing_enable(True)
    wf1.timing_reset()
    m = wf1.correlations_lstm(ns, **kw)
    passes = wf1.timing_get(2)["launches"]
    wf1.close()
    print("LSTMCORR RNNWF_STATE_BUDGET_MB=2: %d passes" % passes)
    assert passes >= 3
    for k in ("samples", "log_ratio", "z_sums", "zz_sums"):
        assert np.array_equal(m[k], a[k]), k
    for k in ("x_sums", "xx_sums"):
        assert np.allclose(m[k], a[k], rtol=1e-12, atol=0), k


@pytest.mark.parametrize("ns", [1, 16, 17])
def test_small_batches(ns):
    shape, units = (3, 3), 53
    N = 9
    prm = LC.parameters(units)
    s = LC.samples_of(3, 3, units)[:ns]
    wf = handle(shape, units, prm)
    out = wf.correlations_lstm(ns, samples=s, want_log_ratio=True)
    wf.close()
    pi, pj = LC.checked_pairs(N)
    ref = LC.brute_force(prm, shape, s, pi, pj)
    assert out["log_ratio"].shape == ref.shape and np.all(np.abs(out["log_ratio"] - ref) <= LC.bound(N))
    check_sums(out, s, N)


@pytest.mark.parametrize("N", [1, 2, 3])
def test_short_chains(N):
    shape, units = (N, 1), 20
    prm = LC.parameters(units)
    s = np.random.RandomState(N).randint(0, 2, size=(LC.NS, N)).astype(np.int32)
    wf = handle(shape, units, prm)
    wf.timing_enable(True)
    wf.timing_reset()
    out = wf.correlations_lstm(LC.NS, samples=s, want_log_ratio=True)
    launches = wf.timing_get(1)["launches"]
    wf.close()
    assert launches == min(N - 1, 2)                          # N = 1: no trunk kernel; N <= 2: no branch kernel
    pi, pj = CR.pair_list(N)
    ref = LC.brute_force(prm, shape, s, pi, pj)
    assert out["log_ratio"].shape == ref.shape == (N + N * (N - 1) // 2, LC.NS)
    assert np.abs(ref).max() > 1e-3 and np.all(np.abs(out["log_ratio"] - ref) <= LC.bound(N))
    check_sums(out, s, N)


# ---- 5. timing, facade, refusals ------------------------------------------------------------------------------------------------------------

def test_timing_ids_and_work():
    shape, units, ns = (4, 3), 20, 40
    N = 12
    wf = handle(shape, units, LC.parameters(units))
    wf.timing_enable(True)
    wf.timing_reset()
    wf.correlations_lstm(ns, samples=LC.samples_of(4, 3, units))
    t = [wf.timing_get(k) for k in range(3)]
    assert [x["launches"] for x in t] == [1, 2, 1]             # base; trunk + branch; the assembly's bracket
    assert all(x["total_ms"] > 0 for x in t)
    assert t[1]["cell_evals"] == ns * evaluations(N) == 40 * 286
    assert t[1]["mfma_flops"] == 3 * evaluations(N) * 5 * 5 * 2048.0          # three blocks; NFULL 1: NT = KT = 5
    wf.timing_reset()
    wf.correlations_lstm(ns, seed=3)
    assert wf.timing_get(0)["launches"] == 2                   # the draw and the teacher-forced base pass
    wf.close()


def test_correlation_matrix_is_correlations_from_sums_of_the_raw_sums():
    shape, units, ns = (3, 3), 20, 300
    wf = handle(shape, units, LC.parameters(units))
    raw = wf.correlations_lstm(ns, seed=111, step=4, want_log_ratio=True, want_samples=True)
    got = OL.correlation_matrix(wf, ns, step=4)
    again = OL.correlation_matrix(wf, ns, samples=raw["samples"].reshape(ns, 3, 3))
    wf.close()
    ref = O.correlations_from_sums(raw["z_sums"], raw["zz_sums"], raw["x_sums"], raw["xx_sums"], ns)
    stats = CR.stats_from_sums(raw["z_sums"], raw["zz_sums"], raw["x_sums"], raw["xx_sums"], ns)
    assert set(got) == set(ref) == set(again)
    for k in ref:
        assert np.array_equal(got[k], ref[k]) and np.array_equal(again[k], ref[k]), k
        assert np.allclose(got[k], stats[k], rtol=1e-9, atol=1e-12), k
    sq = OL.structure_factor(got["zz_c"], [0.0, np.pi], [0.0, np.pi], 3, 3)
    assert sq.shape == (2,) and abs(sq[0] - got["zz_c"].sum() / 9) <= 1e-12


def test_refusals_through_the_c_call_and_the_python_layers():
    from rnnwavefunctions_amd import _lib
    shape, units, N, ns = (3, 2), 10, 6, 32
    prm = LC.parameters(units)
    wf = handle(shape, units, prm)
    s = np.random.RandomState(0).randint(0, 2, size=(ns, N)).astype(np.int32)
    wf.lstm_load_batch(s, np.linspace(-1.0, 1.0, ns))
    assert wf.resident_samples() == ns
    F64P = C.POINTER(C.c_double)
    z, zz, x, xx = np.zeros(N), np.zeros((N, N)), np.zeros((N, 2)), np.zeros((N, N, 5))
    ptr = dict(z=z.ctypes.data_as(F64P), zz=zz.ctypes.data_as(F64P), x=x.ctypes.data_as(F64P), xx=xx.ctypes.data_as(F64P))

    def call(n=ns, offset=0, **null):
        a = dict(ptr, **null)
        return wf.lib.rnnwf_correlations_lstm(wf.h, None, n, 1, 0, offset, a["z"], a["zz"], a["x"], a["xx"], None, None)

    for kwargs, word in [(dict(n=0), "ns must be >= 1"), (dict(n=-5), "ns must be >= 1"), (dict(z=None), "non-null"), (dict(zz=None), "non-null"),
                         (dict(x=None), "non-null"), (dict(xx=None), "non-null"), (dict(offset=-1), "sample_offset must be >= 0")]:
        assert call(**kwargs) == -1, kwargs
        msg = wf.lib.rnnwf_last_error(wf.h).decode()
        assert msg.startswith("rnnwf_correlations_lstm:") and word in msg, (kwargs, msg)
    with pytest.raises(ValueError, match=r"samples must have shape \(ns, 6\)"):
        wf.correlations_lstm(ns, samples=s[:, :5])
    assert wf.resident_samples() == ns                         # the refused calls left the loaded batch resident
    assert call() == 0
    assert wf.resident_samples() == 0                          # a served call overwrites it
    # rnnwf_correlations keeps refusing the LSTM in its own words
    with pytest.raises(ValueError, match="rnnwf_correlations: not implemented for the LSTM cell"):
        wf.correlations(ns)
    wf.close()
    raw = handle(shape, units)
    with pytest.raises(_lib.RnnwfError, match="parameters not committed"):
        raw.correlations_lstm(ns)
    raw.close()
    # every other model, by name, with the entry that serves it - where one does
    gprm = P.init_gru_params([10], seed=1)
    for model, nx, ny, un, p, name, entry, module in [
            (_lib.MODEL_GRU1D, N, 1, (10,), gprm, "GRU1D", "rnnwf_correlations serves the one-layer GRU models", r"observables\.py"),
            (_lib.MODEL_GRU1D_F64, 3, 2, (10,), P.init_gru_params([10], seed=1, dtype=np.float64), "GRU1D_F64",
             "rnnwf_correlations serves the one-layer GRU models", r"observables\.py"),
            (_lib.MODEL_GRU1D, N, 1, (10, 10), P.init_gru_params([10, 10], seed=1), "GRU1D", "no all-pair correlation pass serves stacked",
             "observables_stack"),
            (_lib.MODEL_GRU1D_PARITY, N, 1, (10,), gprm, "GRU1D_PARITY", "no all-pair correlation pass serves this model", "parity"),
            (_lib.MODEL_CRNN_U1, N, 1, (10,), None, "CRNN_U1", "no all-pair correlation pass serves this model", "observables_complex"),
            (_lib.MODEL_MDRNN2D, 3, 2, (10,), None, "MDRNN2D", "no all-pair correlation pass serves this model", "observables_2d")]:
        w = _lib.NativeWavefunction(model, nx, ny, un)
        if p is not None:
            w.set_params(p, scope=SCOPE)
        with pytest.raises(ValueError, match="rnnwf_correlations_lstm: serves the LSTM cell .* this handle's model is %s; .*%s" % (name, entry)):
            w.correlations_lstm(ns)
        with pytest.raises(ValueError, match=module):
            OL.correlation_matrix(w, ns)
        w.close()
