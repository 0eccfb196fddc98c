"""EVERY draw of the HIP samplers against float64 conditionals, at the sizes the project is benchmarked at.

Every other full-size test scores the sample matrix the HIP path drew; none asks whether it was drawn correctly.  Here each drawn
row is fed teacher-forced through the float64 restatement of its family (tests/sampler_reference.py, validated and shown to reject
the defects it is for by tests/test_sampler_reference.py), and the decision of every draw must be  s[b, n] == (u[b, n] >= p0[b, n])
with u = oracle.philox.uniforms(seed, step, sample_offset, ns, N).  A draw is excused only inside the near-tie band computed from the
reference alone (16 x the running maximum of |p0_f32 - p0_f64| along the row, at least 16 x 2^-24; x 2^-29 for the float64
families; none where the U(1) mask forces the spin), and a case must keep at most 1e-3 of its draws and 5 % of its rows in that band
(verified for every case on the CPU oracle's own sampler by test_sampler_reference.py).  Samples come from vmc_step(want_samples=True)
and from sample(); the forward engine is asserted where the case is about one.  Sharpened weights as test_gpu_gradient_full.build
(kernels x 3, every bias randomised), seed 111, with the exceptions the case table of sampler_reference.py states.

Rows checked: all, except a FIXED stride where the table says so (40 000 rows: every 4th; the 32 768-row shard of config 5: every
8th; (64, 20) and the 2D RNN: every 2nd) - rows are never chosen by outcome.

NOT YET RUN ON AN MI355X: no GPU was available while this module was written, so every GPU-side figure (excused shares per family,
engines, reference seconds) is unmeasured.  Each case prints its line (draws, unexcused, excused, shares, reference seconds); the
first run's lines belong in profiles/sampler_full_size.txt, with the largest excused share per family summarised here.  What IS
measured, on the CPU oracle's own sampler for the same parameters and seed, is the table in
test_sampler_reference.py::test_clean_oracle_batches_stay_inside_the_cap (largest share 2.3e-4 of the draws, 4.1 % of the rows,
both at N = 200, 100 units, x 3).
"""
import time

import numpy as np
import pytest

import sampler_reference as R
from lstm_reference import lstm_log_probability
from oracle import models as M

pytestmark = pytest.mark.gpu
SCOPE = R.SCOPE


def model_id(family):
    from rnnwavefunctions_amd import _lib
    return {"gru": _lib.MODEL_GRU1D, "parity": _lib.MODEL_GRU1D_PARITY, "crnn": _lib.MODEL_CRNN_U1, "gru64": _lib.MODEL_GRU1D_F64,
            "mdrnn": _lib.MODEL_MDRNN2D, "lstm": _lib.MODEL_LSTM1D_F64}[family]


def couplings_of(family, N):
    if family == "crnn":
        return np.concatenate([np.ones(N), 0.5 * np.ones(N), np.zeros(N), [0.0, 0.0]])
    return np.append(np.ones(N), 1.0 if family in ("gru", "parity") else 3.0)


def make_wf(family, shape, units, prm, monkeypatch=None, env=None):
    """A fresh handle; `env` is set only while it is created (the library reads its switches once, at rnnwf_create)."""
    from rnnwavefunctions_amd import _lib
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    try:
        wf = _lib.NativeWavefunction(model_id(family), shape[0], shape[1], units)
    finally:
        for k in (env or {}):
            monkeypatch.delenv(k)
    wf.set_params(prm, scope=SCOPE)
    return wf


def verdict(label, res):
    print(R.line(label, res))
    assert res["unexcused"] == 0, "%s %d %s; rows %s; draws %s" % (label, res["unexcused"], R.failure_text(res),
                                                                  res["row_index"][res["wrong_rows"]][:40], res["wrong_draws"][:40])
    assert res["within_cap"], "%s outside the cap: %s" % (label, R.line("", res))


@pytest.mark.parametrize("cid,family,shape,units,ns,sharp,stride,engine,env", R.CASES, ids=[c[0] for c in R.CASES])
def test_every_draw_against_float64_conditionals(cid, family, shape, units, ns, sharp, stride, engine, env, monkeypatch):
    N = shape[0] * shape[1]
    prm = R.build_params(family, units, seed=111, sharp=sharp)
    wf = make_wf(family, shape, units, prm, monkeypatch, env)
    rows = np.arange(0, ns, stride)
    drawn = wf.sample(ns, seed=111, step=0)
    if "RNNWF_STATE_BUDGET_MB" in env:
        # The LSTM's sampler keeps no states, so sample() draws the batch in one pass whatever the budget; the fused step keeps N - 1
        # checkpoints per 16-chain block (1.9 MB here) and refuses a batch beyond the budget: 1 MB leaves one block per call, so the
        # caller's passes are steps of 16 rows at sample_offset = 16 k.  Their rows are judged, and equal sample()'s.
        stepped = drawn.copy()
        for k in range(0, 256, 16):
            stepped[k:k + 16] = wf.vmc_step(16, seed=111, step=0, couplings=couplings_of(family, N), sample_offset=k,
                                            want_samples=True)["samples"]
        with pytest.raises(Exception, match="split the batch"):
            wf.vmc_step(ns, seed=111, step=0, couplings=couplings_of(family, N))
    else:
        stepped = wf.vmc_step(ns, seed=111, step=0, couplings=couplings_of(family, N), want_samples=True)["samples"]
    print("[%s] engine %s, %d of %d rows checked (stride %d)" % (cid, wf.engine_name(), len(rows), ns, stride))
    if engine is not None:
        assert wf.engine_name() == engine
    if family == "crnn":
        assert np.all(stepped.sum(axis=1) == N // 2) and np.all(drawn.sum(axis=1) == N // 2)
    verdict("[%s vmc_step]" % cid, R.check(family, prm, stepped, 111, 0, 0, shape, rows))
    if np.array_equal(drawn, stepped):
        print("[%s sample] bit-identical to vmc_step's rows: the same verdict" % cid)
    else:
        verdict("[%s sample]" % cid, R.check(family, prm, drawn, 111, 0, 0, shape, rows))


# ---- stream edges: every philox_uniform call site, words that are zero everywhere else in the suite ----------------------------------

BIG_SEED = 0x9E3779B97F4A7C15
# family, lattice, units, kernel scale, environment: the one-wave and the cooperative GRU base kernels (gru_kernels.h, both sites), the
# stack (gru_kernels.h), the complex model's two kernels and its stack (crnn_kernels.h), the 2D RNN, the LSTM, and
# the float64 GRU.  Scales as in the table above (2D RNN 1.25).
EDGE_MODELS = [
    ("gru", (40, 1), (50,), 3.0, {}),
    ("gru", (40, 1), (50,), 3.0, {"RNNWF_NO_COOP": "1"}),
    ("gru", (40, 1), (50,), 3.0, {"RNNWF_BASE": "f32"}),
    ("gru", (40, 1), (100,), 3.0, {}),
    ("gru", (40, 1), (20, 20), 3.0, {}),
    ("parity", (40, 1), (50,), 3.0, {}),
    ("crnn", (40, 1), (50,), 3.0, {}),
    ("crnn", (40, 1), (50,), 3.0, {"RNNWF_NO_COOP": "1"}),
    ("crnn", (40, 1), (20, 20), 3.0, {}),
    ("mdrnn", (6, 6), (20,), 1.25, {}),
    ("lstm", (6, 6), (20,), 3.0, {}),
    ("gru64", (6, 6), (20,), 3.0, {}),
]
# seed, step, sample_offset, samples
EDGES = [
    (BIG_SEED, 0, 0, 64),                       # the key word seed >> 32
    (111, 0, 2 ** 32 - 24, 64),                 # the counter word g >> 32 turns 1 inside a 16-chain block (local row 24)
    (111, 0, 2 ** 40 + 5, 64),
    (BIG_SEED, 2 ** 32 + 3, 2 ** 40 + 5, 64),   # all of them; only the low word of the step enters: equals step 3 (asserted below)
    (111, 7, 3, 1),                             # one sample
]


def _edge_id(m):
    return "%s-%dx%d-%s%s" % (m[0], m[1][0], m[1][1], "x".join(map(str, m[2])), "".join("-%s=%s" % kv for kv in sorted(m[4].items())))


@pytest.mark.parametrize("family,shape,units,sharp,env", EDGE_MODELS, ids=[_edge_id(m) for m in EDGE_MODELS])
def test_stream_edges(family, shape, units, sharp, env, monkeypatch):
    prm = R.build_params(family, units, seed=111, sharp=sharp)
    wf = make_wf(family, shape, units, prm, monkeypatch, env)
    label = _edge_id((family, shape, units, sharp, env))
    total = dict(draws=0, excused=0)
    for seed, step, off, ns in EDGES:
        s = wf.sample(ns, seed=seed, step=step, sample_offset=off)
        res = R.check(family, prm, s, seed, step, off, shape)
        tag = "[%s seed %#x step %d offset %d ns %d]" % (label, seed, step, off, ns)
        print(R.line(tag, res))
        assert res["unexcused"] == 0, tag + " " + R.failure_text(res)
        total["draws"] += res["draws"]
        total["excused"] += res["excused"]
        if ns > 1:
            # shard invariance: cut at the 2^32 boundary's row where there is one, and inside a 16-chain block
            for cut in (24, 29):
                a = wf.sample(cut, seed=seed, step=step, sample_offset=off)
                b = wf.sample(ns - cut, seed=seed, step=step, sample_offset=off + cut)
                assert np.array_equal(np.concatenate([a, b]), s), tag + " shards cut at %d" % cut
            one = wf.sample(1, seed=seed, step=step, sample_offset=off + 37)
            assert np.array_equal(one[0], s[37]), tag
    # The cap over the model's edge batches together (a single batch of 64 rows cannot resolve a share of 1e-3)
    assert total["excused"] <= R.CAP_DRAWS * total["draws"], (label, total)
    seed, step, off, ns = EDGES[3]
    assert np.array_equal(wf.sample(ns, seed=seed, step=step, sample_offset=off), wf.sample(ns, seed=seed, step=3, sample_offset=off))
    assert not np.array_equal(wf.sample(ns, seed=seed, step=3, sample_offset=off), wf.sample(ns, seed=seed, step=4, sample_offset=off))
    out = wf.vmc_step(64, seed=BIG_SEED, step=2 ** 32 + 3, couplings=couplings_of(family, shape[0] * shape[1]),
                      sample_offset=2 ** 40 + 5, want_samples=True)
    assert np.array_equal(out["samples"], wf.sample(64, seed=BIG_SEED, step=3, sample_offset=2 ** 40 + 5))


# ---- observables that draw for themselves ----------------------------------------------------------------------------------------------

def _observable_draws(wf, name, N, ns, seed, step, off):
    """(drawn samples (ns, N), global index of row 0) of one self-drawing entry point; ns even."""
    if name == "correlations":
        return wf.correlations(ns, seed=seed, step=step, sample_offset=off, want_samples=True)["samples"], off
    if name == "pauli_step":
        flip, sign = np.zeros((2, N), np.int32), np.zeros((2, N), np.int32)
        flip[0, 3] = 1
        flip[1, N - 2] = sign[1, 1] = 1
        return wf.pauli_step(flip, sign, np.array([1.0, -0.5]), ns, seed=seed, step=step, sample_offset=off, want_samples=True)["samples"], off
    if name == "renyi2_swap":                                # pair p = rows 2p, 2p + 1: pair_offset counts pairs
        return wf.renyi2_swap(ns // 2, seed=seed, step=step, pair_offset=off // 2, want_samples=True)["samples"], 2 * (off // 2)
    masks = np.zeros((2, N), np.int32)
    masks[0, :N // 2] = 1
    masks[1, ::2] = 1
    return wf.renyi2_regions(masks, ns // 2, seed=seed, step=step, pair_offset=off // 2)["samples"], 2 * (off // 2)


@pytest.mark.parametrize("name", ["correlations", "pauli_step", "renyi2_swap", "renyi2_regions"])
@pytest.mark.parametrize("family,shape,units", [("gru", (40, 1), (50,)), ("gru64", (4, 5), (20,))], ids=["gru-f32", "gru-f64"])
def test_observables_draw_the_decisions_of_their_global_indices(name, family, shape, units, monkeypatch):
    """Each entry point draws through Draw{seed, step, sample_offset + s0} per pass.  One handle holds the whole batch, one is created
    under a state budget that forces several passes; both must return the decisions of global indices offset .. offset + ns - 1 -
    judged row by row against the float64 conditionals with the uniforms of those indices, so a pass that restarted at s0 = 0 or
    dropped the offset's high word would show as unexcused draws in its rows."""
    N = shape[0] * shape[1]
    ns, seed, step, off = 1404, BIG_SEED, 5, 2 ** 32 - 700          # the 2^32 boundary falls inside the batch, past the first pass
    prm = R.build_params(family, units, seed=111, sharp=3.0)
    for env in ({}, {"RNNWF_STATE_BUDGET_MB": "1"}):
        wf = make_wf(family, shape, units, prm, monkeypatch, env)
        wf.timing_enable(True)
        wf.timing_reset()
        s, first = _observable_draws(wf, name, N, ns, seed, step, off)
        launches = [wf.timing_get(k)["launches"] for k in range(3)]
        res = R.check(family, prm, s.reshape(ns, N), seed, step, first, shape)
        tag = "[%s %s%s]" % (name, family, " several passes" if env else "")
        print(R.line(tag, res), " launches of timers 0-2:", launches)
        verdict(tag, res)
        assert np.array_equal(s.reshape(ns, N), wf.sample(ns, seed=seed, step=step, sample_offset=first).reshape(ns, N))
        if env:
            assert max(launches) >= 2, "the state budget did not split the batch: %s" % launches


# ---- return_log=True -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("family,shape,units,ns,sharp", [("gru", (80, 1), (50,), 10000, 3.0), ("gru", (80, 1), (50, 50), 4096, 3.0),
                                                          ("gru64", (12, 12), (100,), 1024, 3.0), ("mdrnn", (12, 12), (50,), 1024, 1.25),
                                                          ("lstm", (12, 12), (50,), 1024, 3.0)],
                         ids=["cfg2", "cfg2_l2", "gru64-100", "cfg4", "lstm-50"])
def test_returned_log_probability_of_the_drawn_rows(family, shape, units, ns, sharp):
    """sample(return_log=True): the log-probability that comes back with the rows equals the float64 reference ON those rows, within
    the tolerance tests/test_gpu_prnn.py states: 2e-6 N (x layers, as its stacked tests) + 2e-6 for float32, 1e-11 N for float64."""
    N = shape[0] * shape[1]
    prm = R.build_params(family, units, seed=111, sharp=sharp)
    wf = make_wf(family, shape, units, prm)
    s, lg = wf.sample(ns, seed=111, step=0, return_log=True)
    t0 = time.time()
    if family == "mdrnn":
        ref = M.mdrnn_log_probability(prm, s)
    elif family == "lstm":
        ref = lstm_log_probability(prm, s, shape[0], shape[1])
    else:
        ref = M.prnn_log_probability(R.cast(prm, np.float64), s.reshape(ns, N), dtype=np.float64)
    tol = 1e-11 * N if family in R.FLOAT64_FAMILIES else 2e-6 * N * len(units) + 2e-6
    err = np.abs(lg - ref).max()
    print("[return_log %s %s] %d rows, log P %.1f .. %.1f, max |hip - float64| = %.2e (tolerance %.2e), reference %.1f s" %
          (family, "x".join(map(str, units)), ns, ref.min(), ref.max(), err, tol, time.time() - t0))
    assert np.all(np.isfinite(lg)) and err <= tol
