"""What tests/test_gpu_lstm_grad.py's yardstick is and what its bound rejects, on the reference alone (no GPU).

* tests/lstm_grad_reference.py's torch float64 log P equals tests/lstm_reference.py's NumPy restatement on all 512 configurations of
  3 x 3 to 1e-13, and its reverse-mode gradient passes autograd_reference.fd_check against central differences of that restatement.
* The acceptance bound (lstm_grad_reference.judge: the float64 families' verdict with its rounding floor) REJECTS a gradient with the
  ragged block's last chain dropped, the last site's term dropped, the forget bias left out of sigmoid(f), dc_carry without its factor
  f, the one-hot fed into site 32 taken from site 31, or any one tensor x 1.001 - and ACCEPTS the float64 gradient summed in another
  order.
* Beyond two spin words (13 x 5 at 37 units, 10 x 10 at 17 units) it REJECTS the one-hot fed into site 64 taken from site 31 (bit 31
  of the wrong word), word 0 read as zeros (the refetch at n = 64 skipped) and the wide batch without its ragged block's last chain,
  and ACCEPTS the other summation order; the wide batch's grouped floor is the row-by-row one; BIG_LATTICES holds what it must.
* The new C entries are declared, exported and bound, and the Python wrappers validate shapes and the weights' length before any
  library call.
"""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import autograd_reference as A
import lstm_grad_reference as LG
import lstm_reference as LR
from conftest import ROOT

SCOPE = LG.SCOPE
SHAPE, UNITS = (11, 3), 17


def all_configs(N):
    idx = np.arange(2 ** N)
    return ((idx[:, None] >> (N - 1 - np.arange(N))[None, :]) & 1).astype(np.int64)


def test_torch_log_probability_is_the_numpy_restatement_and_its_gradient_passes_finite_differences():
    prm = LG.parameters(10)
    s = all_configs(9)
    lp_np = LR.lstm_log_probability(prm, s, 3, 3)
    lp_t = LG.lstm_log_probability(A.to_torch(prm), s).numpy()
    assert np.abs(lp_t - lp_np).max() <= 1e-13
    assert abs(np.exp(lp_t).sum() - 1.0) <= 1e-13
    sub = s[np.random.RandomState(3).choice(len(s), size=24, replace=False)]
    w = LG.weights(len(sub))
    g = LG.gradient(prm, sub, w)
    prm64 = {k: np.array(v, dtype=np.float64) for k, v in prm.items()}
    worst = A.fd_check(g, prm64, lambda: float((w * LR.lstm_log_probability(prm64, sub, 3, 3)).sum()), n_per_tensor=12, eps=1e-5,
                       per_tensor=True)
    print("3x3, 10 units: max over tensors of |FD - autograd| / max |autograd| = %.2e" % worst)
    assert worst < 1e-6


@pytest.fixture(scope="module")
def case():
    prm = LG.parameters(UNITS)
    N = SHAPE[0] * SHAPE[1]
    u = np.random.RandomState(5).random_sample((LG.NS, N))
    s = LR.lstm_sample(prm, SHAPE[0], SHAPE[1], u)[0]
    w = LG.weights(LG.NS)
    assert w[-1] != 0.0 and (w == 0.0).sum() == 2 and (w < 0).any() and (w > 0).any()
    return prm, s, w, LG.reference(prm, s, w)


def rejected(label, case, g):
    worst, failures = LG.judge(label, g, case[3], echo=lambda *_: None)
    print("%s: worst deviation / bound %.3g, %d tensors beyond it" % (label, worst, len(failures)))
    return worst > A.FACTOR and failures


def test_the_bound_rejects_wrong_gradients(case):
    prm, s, w, ref = case
    N = s.shape[1]
    assert rejected("last chain of the ragged block dropped", case, LG.gradient(prm, s[:-1], w[:-1]))
    site_weight = np.ones(N)
    site_weight[-1] = 0.0
    assert rejected("last site's term dropped", case, LG.gradient(prm, s, w, site_weight=site_weight))
    assert rejected("forget bias left out of sigmoid(f)", case, LG.gradient(prm, s, w, forget_bias=0.0))
    assert rejected("dc_carry without the factor f", case, LG.gradient(prm, s, w, carry_without_f=True))
    fed = s.copy()
    fed[:, 31] = s[:, 30]                               # what site 32 is fed: site 31's spin, taken from site 30 instead
    assert ((fed[:, 31] != s[:, 31]) & (w != 0.0)).any()
    assert rejected("one-hot fed into site 32 taken from site 31", case, LG.gradient(prm, s, w, inputs=fed))
    for k in ref.g64:
        g = {n: v.copy() for n, v in ref.g64.items()}
        g[k] = g[k] * 1.001
        assert rejected("%s x 1.001" % k, case, g), k


def test_the_bound_accepts_another_summation_order(case):
    prm, s, w, ref = case
    g = {k: np.add.reduce(t[::-1], axis=0) for k, t in ref.terms.items()}            # the samples' terms added last to first
    assert any(not np.array_equal(g[k], ref.g64[k]) for k in g)
    worst, failures = LG.judge("[reversed order]", g, ref)
    assert not failures and worst <= A.FACTOR
    worst, failures = LG.judge("[reference itself]", ref.g64, ref)
    assert worst == 0.0 and not failures


def test_long_batch_floor_equals_the_per_sample_one():
    """the long batch's floor sums the terms per distinct configuration: the same sums as sample by sample"""
    prm = LG.parameters(10)
    s = np.random.RandomState(9).randint(0, 2, size=(300, 4))
    w = LG.weights(300)
    direct = {k: np.abs(t).sum(axis=0) for k, t in LG.per_sample_terms(prm, s, w).items()}
    grouped = LG.abs_term_sums(prm, s, w)
    for k in direct:
        assert np.allclose(grouped[k], direct[k], rtol=1e-12, atol=0.0), k
    a, b = LG.reference(prm, s, w), LG.reference(prm, s, w, keep_terms=False)
    assert all(np.isclose(a.floor[k], b.floor[k], rtol=1e-12) for k in a.floor)


def test_case_table_covers_every_width_class():
    assert sorted({LG.nfull(u) for u in LG.WIDTHS}) == [1, 2, 3, 4]
    assert {16 * nf + 4 for nf in (1, 2, 3, 4)} <= set(LG.WIDTHS)                    # full mixed tile at every NFULL
    assert all(33 <= a * b <= 35 for a, b in LG.LATTICES[:3]) and LG.LATTICES[3] == (2, 1)


# ---- beyond two spin words and one workgroup (BIG_LATTICES, the wide batch) ------------------------------------------------------------

BIG = [((13, 5), 37), ((10, 10), 17)]


@functools.lru_cache(maxsize=None)
def big(shape, units):
    """40 lstm_sample draws at the case table's sharp (10 x 10 / 17: 1, where the draw is not polarised), both spin values at sites 31
    and 63 among the rows with non-zero weight"""
    prm = LG.parameters(units, sharp=LG.big_sharp(shape, units))
    u = np.random.RandomState(5).random_sample((LG.NS, shape[0] * shape[1]))
    s = LR.lstm_sample(prm, shape[0], shape[1], u)[0]
    w = LG.weights(LG.NS)
    assert LG.word_boundaries_mixed(s, w)
    return prm, s, w, LG.reference(prm, s, w)


@pytest.fixture(scope="module", params=BIG, ids=["%dx%d-%d" % (s[0], s[1], u) for s, u in BIG])
def big_case(request):
    return big(*request.param)


def test_the_bound_rejects_a_wrong_word_walk(big_case):
    prm, s, w, ref = big_case
    fed = s.copy()
    fed[:, 63] = s[:, 31]                               # what site 64 is fed: site 63's spin, taken from bit 31 of word 0 instead of word 1
    assert ((fed[:, 63] != s[:, 63]) & (w != 0.0)).sum() >= 2
    assert rejected("one-hot fed into site 64 taken from site 31", big_case, LG.gradient(prm, s, w, inputs=fed))
    low = s.copy()
    low[:, :32] = 0                                     # the refetch at n = 64 skipped: wlow stays 0 and becomes wcur at n = 32
    assert (np.any(low != s, axis=1) & (w != 0.0)).sum() >= 2
    assert rejected("word 0 read as zeros", big_case, LG.gradient(prm, low, w))


def test_the_bound_accepts_another_summation_order_at_these_sizes(big_case):
    prm, s, w, ref = big_case
    g = {k: np.add.reduce(t[::-1], axis=0) for k, t in ref.terms.items()}
    assert any(not np.array_equal(g[k], ref.g64[k]) for k in g)
    worst, failures = LG.judge("[reversed order]", g, ref, echo=lambda *_: None)
    print("reversed order: worst deviation / bound %.3g" % worst)
    assert not failures and worst <= A.FACTOR


def test_the_bound_rejects_the_wide_batch_without_its_last_chain():
    """the wide batch of tests/test_gpu_lstm_grad.py (1 000 rows of 40 configurations, 62 full blocks and a ragged one of 8) on the
    10 x 10 fixture's draws: the ragged block's last chain dropped"""
    prm, configs, _, _ = big(*BIG[1])
    ns = LG.WIDE["ns"]
    s, idx = LG.wide_batch(configs, ns)
    w = LG.weights(ns)
    assert s.shape == (ns, 100) and ns % 16 == 8 and w[-1] != 0.0 and sorted(set(idx)) == list(range(LG.NS))
    wide = prm, s, w, LG.reference(prm, s, w, keep_terms=False)
    assert rejected("last chain of the wide batch's ragged block dropped", wide, LG.gradient(prm, s[:-1], w[:-1]))
    worst, failures = LG.judge("[reference itself]", wide[3].g64, wide[3], echo=lambda *_: None)
    assert worst == 0.0 and not failures


def test_wide_batch_floor_equals_the_per_sample_one():
    """the wide batch's floor sums the terms per distinct configuration, rows with independent weights: the same sums as row by row"""
    prm = LG.parameters(10)
    configs = np.unique(np.random.RandomState(9).randint(0, 2, size=(60, 9)), axis=0)[:20]
    s, idx = LG.wide_batch(configs, 200)
    w = LG.weights(200)
    assert len(configs) == 20 and len(set(idx)) == 20 and np.array_equal(s, configs[idx])
    assert all(len(np.unique(s[b:b + 16], axis=0)) == len(s[b:b + 16]) for b in range(0, 200, 16))
    direct = {k: np.abs(t).sum(axis=0) for k, t in LG.per_sample_terms(prm, s, w).items()}
    grouped = LG.abs_term_sums(prm, s, w)
    for k in direct:
        assert np.allclose(grouped[k], direct[k], rtol=1e-12, atol=0.0), k
    a, b = LG.reference(prm, s, w), LG.reference(prm, s, w, keep_terms=False)
    assert all(np.isclose(a.floor[k], b.floor[k], rtol=1e-12) for k in a.floor)
    assert all(np.array_equal(a.g64[k], b.g64[k]) for k in a.g64)


def test_big_case_table_covers_the_word_walk_at_every_nfull():
    sites = [a * b for a, b in LG.BIG_LATTICES]
    assert {32, 64, 65} <= set(sites)
    assert any(n > 64 and n % 32 == 0 for n in sites)                                # full words above the first refetch
    assert any((n + 31) // 32 >= 5 for n in sites)                                   # refetches at 128, 96 and 64
    cases = LG.big_cases()
    assert len(cases) == len(set(cases)) and {u for _, u in cases} == set(LG.WIDTHS) and {s for s, _ in cases} == set(LG.BIG_LATTICES)
    for n in (65, 100, 144):
        assert {LG.nfull(u) for s, u in cases if s[0] * s[1] == n} == {1, 2, 3, 4}, n
    assert all(key in cases or key == BIG[1] for key in LG.BIG_SHARP)                # no override without its case
    assert {LG.nfull(u) for u in LG.WIDE["widths"]} == {2, 3, 4} and LG.WIDE["ns"] % 16 == 8


# ---- host side of the new entries -------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def built_lib():
    from rnnwavefunctions_amd import build
    return build.build()


ENTRIES = {"rnnwf_lstm_gradient": 4, "rnnwf_lstm_vmc_gradient_step": 9}


def test_new_symbols_resolve(built_lib):
    from rnnwavefunctions_amd import _lib
    header = open(os.path.join(ROOT, "include", "rnnwf.h")).read()
    lib = ctypes.CDLL(built_lib)
    for name, nargs in ENTRIES.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, header)
        assert m and len(m.group(1).split(",")) == nargs == len(_lib.PROTOTYPES[name][1]), name
        assert hasattr(lib, name), name
    assert lib.rnnwf_abi_version() == _lib.ABI_VERSION == 1
    from rnnwavefunctions_amd import build
    assert "lstm_grad.hip" in build.SOURCES


class _Recorder:
    """stands in for the library: records the calls the wrappers make"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append(name)
            return 0
        return fn


def fake_handle(N=6, nx=3, ny=2):
    from rnnwavefunctions_amd import _lib
    wf = object.__new__(_lib.NativeWavefunction)
    wf.lib, wf.h, wf.model, wf.N, wf.nx, wf.ny = _Recorder(), None, _lib.MODEL_LSTM1D_F64, N, nx, ny
    wf._param_layout = [("a", 4), ("b", 2)]
    return wf


def test_wrappers_validate_before_calling_the_library():
    wf = fake_handle()
    shapes = {"a": (2, 2), "b": (2,)}
    with pytest.raises(ValueError, match="6 sites per row"):
        wf.lstm_gradient(np.zeros((4, 5), dtype=np.int32), np.zeros(4), shapes)
    with pytest.raises(ValueError, match="6 sites per row"):
        wf.lstm_gradient(np.zeros((0, 6), dtype=np.int32), np.zeros(0), shapes)
    with pytest.raises(ValueError, match="4 samples but weights of shape"):
        wf.lstm_gradient(np.zeros((4, 6), dtype=np.int32), np.zeros(3), shapes)
    with pytest.raises(ValueError, match="couplings must hold Jz"):
        wf.lstm_vmc_gradient_step(8, 1, 0, np.ones(6), shapes)
    assert wf.lib.calls == []
    with pytest.raises(ValueError, match="shapes must name every tensor"):
        wf.lstm_gradient(np.zeros((4, 3, 2), dtype=np.int32), np.zeros(4), {"a": (2, 2)})
    assert wf.lib.calls == ["rnnwf_lstm_gradient"]
    out = wf.lstm_gradient(np.zeros((4, 3, 2), dtype=np.int32), np.zeros(4), shapes)
    assert out["a"].shape == (2, 2) and out["b"].shape == (2,)
    out = wf.lstm_vmc_gradient_step(8, 1, 0, np.ones(7), shapes, want_samples=True, want_eloc=True)
    assert out["samples"].shape == (8, 6) and out["eloc"].shape == (8,) and set(out["grads"]) == {"a", "b"}
    wf.h = None


def test_training_module_exports():
    from rnnwavefunctions_amd import training, training_lstm
    assert training_lstm.__all__ == ["run_2DTFIM_1DRNN_LSTM", "lstm_training_loop"]
    assert training_lstm.Adam is training.Adam
    with pytest.raises(ValueError, match="one layer"):
        training_lstm.run_2DTFIM_1DRNN_LSTM(numsteps=0, num_layers=2)
