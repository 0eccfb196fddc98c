"""CPU checks of tests/parity_reference.py: the stable combine and shares against numpy.longdouble, the symmetrised reference against
the project's other restatements, the rung tables, the autograd counterpart, and the refusal of every defect model by the judgements
tests/test_gpu_parity_range.py applies."""
import numpy as np
import pytest
import torch

import autograd_reference as A
import flip_rows_reference as F
import parity_reference as PR
from oracle import models as M

LD = np.longdouble


@pytest.fixture(scope="module", params=PR.CASE_IDS)
def table(request):
    return PR.case(request.param), PR.rungs(request.param)


def test_tables_hold_what_they_must(table):
    """`rungs` asserts the conditions when it builds a table; here the counts are printed and the shapes pinned."""
    c, r = table
    d = r.lpF - r.lpR
    print("[%s] %d rungs, log P_sym %.1f .. %.3f; band %d, below -760 %d, above -600 %d, |d| >= 40 %d, deep and |d| < 1 %d, palindromes %d" %
          (c.id, len(r.s), r.sym.min(), r.sym.max(), np.sum((r.sym > PR.BAND[0]) & (r.sym < PR.BAND[1])), np.sum(r.sym < PR.DEEP),
           np.sum(r.sym > PR.ORDINARY), np.sum(np.abs(d) >= PR.SATURATED), np.sum((r.sym < PR.DEEP) & (np.abs(d) < 1)),
           np.sum(r.kind == "palindrome")))
    assert r.s.shape[1] == c.N and r.s.dtype == np.int32 and set(np.unique(r.s)) == {0, 1}
    assert len(r.s) % 32 and len(r.s) % 16
    assert c.N > 64 or c.units > 36                       # three spin words, or the aligned class with padding


def test_combine_equals_the_formula_in_longdouble(table):
    c, r = table
    wide = PR.naive(r.lpF, r.lpR, LD)
    assert np.all(np.isfinite(wide)), "numpy.longdouble does not hold e^-1300 here"
    got = PR.combine(r.lpF, r.lpR)
    assert got.dtype == np.float64
    ratio = np.abs(got.astype(LD) - wide) / (2 * PR.EPS * np.maximum(1.0, np.abs(wide)))
    print("[%s] |combine - longdouble formula| / (2 x 2^-52 x max(1, |value|)): worst %.3f" % (c.id, float(ratio.max())))
    assert np.all(ratio <= 1.0)
    up = r.sym > PR.ORDINARY
    plain = PR.naive(r.lpF, r.lpR)
    assert np.all(np.abs(got[up] - plain[up]) <= 2 * PR.EPS * np.maximum(1.0, np.abs(got[up])))


def test_the_formula_as_written_fails_on_the_table(table):
    """-inf below exp's range; in the band wrong by more than the GPU bound on at least one rung: the table can see the bug."""
    c, r = table
    plain = PR.naive(r.lpF, r.lpR)
    low = np.maximum(r.lpF, r.lpR) < PR.EXP_ZERO
    assert low.sum() >= 8 and np.all(np.isneginf(plain[low]))
    band = (r.sym > PR.BAND[0]) & (r.sym < PR.BAND[1])
    over = PR.over_bound(plain[band], r.sym[band])
    print("[%s] formula as written in the band: error / GPU bound %s" % (c.id, np.array2string(over, precision=2)))
    assert band.sum() >= 4 and over.max() > 1.0


def test_combine_edges():
    inf, nan = np.inf, np.nan
    a = np.array([-3.0, -800.0, -inf, -inf, -5.0, nan, -2.0, 0.0, -1e300])
    b = np.array([-3.0, -800.0, -inf, -7.0, -inf, -1.0, nan, -745.0, -1e300])
    with np.errstate(invalid="ignore"):
        got = PR.combine(a, b)
    assert np.array_equal(got[:3], a[:3])                                       # a == b: exact, -inf without inf - inf
    assert got[3] == -7.0 - np.log(2.0) and got[4] == -5.0 - np.log(2.0)
    assert np.isnan(got[5]) and np.isnan(got[6])
    assert got[7] == -np.log(2.0) and got[8] == -1e300
    with np.errstate(invalid="ignore"):
        assert np.array_equal(PR.combine(b, a), got, equal_nan=True)            # symmetric


def test_palindromes_combine_exactly(table):
    c, r = table
    pal = r.kind == "palindrome"
    assert np.array_equal(r.lpF[pal], r.lpR[pal])
    assert np.array_equal(PR.combine(r.lpF[pal], r.lpR[pal]), r.lpF[pal])
    rng = np.random.RandomState(0)
    x = -rng.uniform(0, 1500, 1000)
    assert np.array_equal(PR.combine(x, x), x)


def test_shares(table):
    c, r = table
    aF, aR = PR.shares(r.lpF, r.lpR)
    wF, wR = PR.shares(r.lpF, r.lpR, LD)
    assert np.all(np.abs(aF + aR - 1.0) <= PR.EPS)
    assert np.all(np.abs(aF.astype(LD) - wF) <= 2 * PR.EPS) and np.all(np.abs(aR.astype(LD) - wR) <= 2 * PR.EPS)
    d = r.lpF - r.lpR
    assert np.all(aF[d >= PR.SATURATED] == 1.0) and np.all(aR[d >= PR.SATURATED] == 0.0)
    assert np.all(aF[d <= -PR.SATURATED] < 2.0 ** -57) and np.all(aR[d <= -PR.SATURATED] == 1.0)
    assert np.sum(np.abs(d) >= PR.SATURATED) >= 4


def test_symmetrised_reference_against_the_other_restatements(table):
    """Above -600 the oracle's formula as written (float64) agrees; everywhere flip_rows_reference's prefix-sharing symmetriser does,
    row by row, far inside its own row bound."""
    c, r = table
    prm = PR.build_params(c)
    up = PR.ordinary(r)
    as_written = M.prnn_paritysym_log_probability(F.R.cast(prm, np.float64), r.s[up], PR.SCOPE, np.float64)
    assert np.all(np.abs(as_written - r.sym[up]) <= 2 * PR.EPS * np.maximum(1.0, np.abs(r.sym[up])))
    assert np.array_equal(PR.sym_log_prob(prm, r.s), r.sym) and np.array_equal(PR.sym_log_prob(prm, r.s[:, ::-1]), r.sym)
    ref = PR.queue_reference(c.id)
    q = PR.sym_queue(prm, r.s)
    assert np.abs(q[0] - r.sym).max() < 1e-10 and np.all(np.isfinite(q))      # another batch size: BLAS may sum in another order
    worst = float((np.abs(q - ref.lp64) / ref.bound).max())
    print("[%s] from-site-0 queue against the prefix-sharing one: worst %.2e of the row bound; yardstick %.1e .. %.1e" %
          (c.id, worst, ref.y.min(), ref.y.max()))
    assert worst < 1e-6 and np.all(np.isfinite(ref.y))
    # the two directions' queues, the second with its rows exchanged, combine to the symmetrised one
    f = F.queue_rows(prm, r.s)
    b = F.queue_rows(prm, r.s[:, ::-1])
    assert np.abs(PR.combine(f, PR.exchange(b)) - q).max() < 1e-9


def test_autograd_counterpart(table):
    """Finite on every rung; on the rungs above -600 the gradient of the formula as written, within 1e-12 relative."""
    c, r = table
    prm = PR.build_params(c)
    e = np.random.RandomState(5).standard_normal(len(r.s))
    leaves = A.to_torch(prm, torch.float64)
    assert np.abs(PR.torch_sym_log_prob(leaves, r.s).numpy() - r.sym).max() < 1e-9
    g = PR.gradient(prm, r.s, e)
    assert all(np.all(np.isfinite(v)) for v in g.values())
    bad = PR.gradient(prm, r.s, e, forward="naive")
    assert not all(np.all(np.isfinite(v)) for v in bad.values())               # what the formula as written does to the whole table
    up = PR.ordinary(r)
    g_up, n_up = PR.gradient(prm, r.s[up], e[up]), PR.gradient(prm, r.s[up], e[up], forward="naive")
    for k in g_up:
        assert np.abs(g_up[k] - n_up[k]).max() <= 1e-12 * np.abs(n_up[k]).max(), k


def test_gradient_reference_accepts_float32_and_refuses_swapped_shares():
    """The gradient bound on the whole ladder of the 10-unit case: the float32 autograd gradient passes, the two directions' shares
    swapped do not."""
    import gradient_classes_reference as G
    c, r = PR.case("10x70"), PR.rungs("10x70")
    prm = PR.build_params(c)
    e = np.random.RandomState(5).standard_normal(len(r.s))
    ref = PR.gradient_reference(c, prm, r.s, e)
    gc = PR.gradient_case(c, len(r.s))
    worst, failures = G.judge("[f32]", gc, ref.g32, ref, echo=lambda *a: None)
    assert not failures and worst <= 1.0 + 1e-9
    aF, aR = PR.shares(r.lpF, r.lpR)
    # d log P_sym = aF d log P_F + aR d log P_R: the per-direction terms with the shares exchanged
    leaves = A.to_torch(prm, torch.float64, requires_grad=True)
    w = torch.as_tensor((e - e.mean()) / len(e))
    lpF = A.prnn_log_probability(leaves, r.s, PR.SCOPE)
    lpR = A.prnn_log_probability(leaves, r.s[:, ::-1], PR.SCOPE)
    (w * (torch.as_tensor(aR) * lpF + torch.as_tensor(aF) * lpR)).sum().backward()
    swapped = {k: v.grad.numpy().reshape(np.shape(prm[k])) for k, v in leaves.items()}
    worst, failures = G.judge("[swapped]", gc, swapped, ref, echo=lambda *a: None)
    assert failures


# ---- the defect models, judged as the GPU test judges the device ----------------------------------------------------------------------

def _queues(c, r):
    prm = PR.build_params(c)
    return prm, F.queue_rows(prm, r.s), F.queue_rows(prm, r.s[:, ::-1])


DEFECTS = ("formula as written", "reversed direction dropped", "factor 0.5 dropped", "reverse map off by one row",
           "spin words reversed in place")


def _defective(name, c, r, prm, f, b):
    """(log_prob (B,), queue (N + 1, B)) of the defective model, the per-direction values being the float64 oracle's f, b (b in the
    reversed chains' own row numbering)."""
    if name == "formula as written":
        return PR.naive(f[0], b[0]), PR.naive(f, PR.exchange(b))
    if name == "reversed direction dropped":
        return f[0], f
    if name == "factor 0.5 dropped":
        return np.logaddexp(f[0], b[0]), np.logaddexp(f, PR.exchange(b))
    if name == "reverse map off by one row":
        shifted = np.concatenate([b[:1], np.roll(b[1:][::-1], 1, axis=0)])          # position n lands in row N - n + 1 (cyclically)
        return PR.combine(f[0], b[0]), PR.combine(f, shifted)
    if name == "spin words reversed in place":
        w = F.queue_rows(prm, PR.word_reversed(r.s))
        return PR.combine(f[0], w[0]), PR.combine(f, PR.exchange(w))
    raise KeyError(name)


@pytest.mark.parametrize("name", DEFECTS)
def test_defect_models_are_refused(table, name):
    """Each defect misses the combine judgement (against the per-direction values) AND the float64 judgement (row bound) - on
    log_prob where it shows there, on the queue in every case."""
    c, r = table
    prm, f, b = _queues(c, r)
    ref = PR.queue_reference(c.id)
    pal = r.kind == "palindrome"
    clean_lp, clean_q = PR.combine(f[0], b[0]), PR.combine(f, PR.exchange(b))
    assert not PR.judge_combine(clean_lp, f[0], b[0], pal)[1] and not PR.judge_combine(clean_q, f, PR.exchange(b))[1]
    assert not PR.judge_rows(clean_q, ref)[1] and not PR.judge_rows(clean_lp, ref, r.sym)[1]
    with np.errstate(invalid="ignore"):
        lp, q = _defective(name, c, r, prm, f, b)
        in_log_prob = name != "reverse map off by one row"                       # log_prob uses no map
        ratio_c, fail_c = PR.judge_combine(q, f, PR.exchange(b))
        ratio_r, fail_r = PR.judge_rows(q, ref)
        assert fail_c and fail_r, (name, ratio_c, ratio_r)
        if in_log_prob:
            assert PR.judge_combine(lp, f[0], b[0], pal)[1] and PR.judge_rows(lp, ref, r.sym)[1], name
        e = F.energies(q, r.s, ref.Jz)
        m = F.measure(q, e, ref)
    print("[%s] %-32s combine judgement %.3g x its bound, rows %.3g x theirs, E_loc %.3g x its bound" % (c.id, name, ratio_c, ratio_r, m["e_over"]))
    assert not m["finite"] or m["row_over"] > 1.0
