"""The parity-symmetric model (MODEL_GRU1D_PARITY) over the whole range of log P, far below the range of float64's exp.

What makes the class a model of its own is a few lines: the reversed packing (pack_bits_kernel, reverse = 1), the reverse map of the
flip queue (prnn.hip: ensure_reverse_map), the combine log(0.5 (P_F + P_R)) of the two directions (util_kernels.h:
parity_combine_kernel, on log_prob / sample's log and on all (N + 1) ns rows of the flip queue) and the shares of the gradient
(parity_share_kernel).  The combine is the only place in the library that handles an ABSOLUTE log-probability, and every other parity
test sits near log P = -30.  tests/parity_reference.py builds, at 10 units on 70 sites and 37 units on 33 sites, 43 and 52 teacher-forced
rungs from log P = -0.01 to -1 270: a ladder, the band (-745, -709) where exp is subnormal, rungs below -760 where it is zero, shares
saturated to exactly 0 and 1, both directions deep and within 1 of each other, six palindromes; the last tile is ragged on either
engine.  Its docstring derives every bound used here; tests/test_parity_reference.py shows on the CPU that each judgement refuses the
formula as written, a dropped direction, a dropped factor 0.5, a reverse map off by one row and a packing that reverses each spin
word in place.

Per case and engine (10 units: f32-input MFMA; 37 units: f32-input MFMA by default and the bf16x3 engine pinned):
  combine     a plain MODEL_GRU1D handle with the same weights, engine and batch gives the two directions (log_prob(s) and
              log_prob(s[:, ::-1]); the queues of s and of s[:, ::-1], the latter with rows k + 1 and N - k exchanged).  The parity
              handle's values must be `combine` of them within 8 x 2^-52 x max(1, |value|), and on the palindromes bit for bit the
              GRU handle's value.  The two handles' per-direction values ARE bit-identical (the palindromes show it: their parity
              value equals the GRU value in every bit), so this test isolates the combine.
  float64     log_prob(s) and log_prob(s[:, ::-1]) against sym_log_prob under flip_rows_reference's row bound; equal to each other
              within the combine bound; every queue row against the symmetrised float64 queue (from site 0, and the prefix-sharing
              one of flip_rows_reference.judge); row 0 equal to log_prob(s) bit for bit; E_loc finite, equal to the float64 assembly
              of the device's own queue within the summation term and to the reference energies within the E_loc bound.
  sampling    vmc_step's energies equal tfim_eloc of its samples bit for bit (unpack_device, then pack_device reversed; three words).
  shares      load_batch(rungs, fixed random E_loc), vmc_gradient: every element of every tensor against the float64 autograd gradient
              of the stable form under gradient_classes_reference.judge's parity bound; once on the whole ladder, once on the rungs
              above -600 alone.
  1 100 sites a user-sized case: initial weights, 32 chains drawn by vmc_step.

On the kernel as it was (log(0.5 (exp(a) + exp(b))); this module run on an MI355X before the fix): 10 failed, 5 passed.  The combine,
float64 and queue tests of all three case/engine rows and the 1 100-site test failed: log_prob was -inf on 11 of 43 and 20 of 52 rungs
(every rung below -745, the deep palindromes among them; the palindrome at -0.009 came out 2.9e-17 off the GRU handle's value), row 0
of the queue was -inf there and E_loc NaN, and at 1 100 sites 2 of the 32 drawn chains had log_prob -inf and NaN energies.  (In the
band the formula as written misses the combine bound by up to 2.6e7 x: test_parity_reference.py, float64 on the CPU.)  The gradient and
the sampling tests passed: parity_share_kernel works on the difference and needed no change.  After the fix all pass; worst ratios to
each bound per case and engine are in profiles/parity_range.txt (combine <= 0.10, rows <= 0.21, E_loc <= 0.04 and <= 0.16 of the
summation term, gradient <= 0.29 of a limit of 16); the module takes 5 s, about 1 s of it the largest case.
"""
import time

import numpy as np
import pytest

import flip_rows_reference as F
import gradient_classes_reference as G
import parity_reference as PR
from oracle import estimators as E
from test_gpu_sampler_full import make_wf

pytestmark = pytest.mark.gpu

# case, RNNWF_ENGINE while the handles are created, the engine the flip pass must report
ROWS = [("10x70", None, "f32mfma"), ("37x33", None, "f32mfma"), ("37x33", "bf16x3", "bf16x3")]
ROW_IDS = ["%s-%s" % (cid, pin or "default") for cid, pin, _ in ROWS]
_device = {}


def handles(cid, pin, monkeypatch):
    c = PR.case(cid)
    prm = PR.build_params(c)
    env = {"RNNWF_ENGINE": pin} if pin else {}
    return [make_wf(family, (c.N, 1), (c.units,), prm, monkeypatch, env) for family in ("parity", "gru")]


def eloc_with_queue(wf, s, Jz):
    lp = np.full((s.shape[1] + 1) * len(s), np.nan)
    e = wf.tfim_eloc(s, Jz, F.BX, log_probs=lp)
    return e, lp.reshape(s.shape[1] + 1, len(s))


def device(cid, pin, engine, monkeypatch):
    """Everything the device computes for a row of ROWS, once per module run."""
    if (cid, pin) not in _device:
        c, r = PR.case(cid), PR.rungs(cid)
        par, gru = handles(cid, pin, monkeypatch)
        s, rev, Jz = r.s, np.ascontiguousarray(r.s[:, ::-1]), F.couplings(c.N)
        d = dict(lp=par.log_prob(s), lp_rev=par.log_prob(rev), a=gru.log_prob(s), b=gru.log_prob(rev))
        d["e"], d["q"] = eloc_with_queue(par, s, Jz)
        d["eF"], d["qF"] = eloc_with_queue(gru, s, Jz)
        d["eR"], d["qR"] = eloc_with_queue(gru, rev, Jz)
        assert par.engine_name() == engine and gru.engine_name() == engine, (par.engine_name(), gru.engine_name())
        par.close()
        gru.close()
        _device[(cid, pin)] = d
    return _device[(cid, pin)]


@pytest.mark.parametrize("cid,pin,engine", ROWS, ids=ROW_IDS)
def test_combine_of_the_two_directions(cid, pin, engine, monkeypatch):
    r, d = PR.rungs(cid), device(cid, pin, engine, monkeypatch)
    pal = r.kind == "palindrome"
    # the palindromes first: both directions are the same chain, so the GRU handle's two values and the parity value are one number
    print("[%s %s] palindromes: GRU handle %s" % (cid, engine, np.array2string(d["a"][pal], precision=3)))
    print("[%s %s]              parity - GRU %s" % (cid, engine, d["lp"][pal] - d["a"][pal]))
    assert np.array_equal(d["a"][pal], d["b"][pal])
    assert np.array_equal(d["lp"][pal], d["a"][pal]), "a palindrome's parity value is not the GRU handle's"
    worst, failures = PR.judge_combine(d["lp"], d["a"], d["b"], pal)
    worst_rev, failures_rev = PR.judge_combine(d["lp_rev"], d["b"], d["a"], pal)
    worst_q, failures_q = PR.judge_combine(d["q"], d["qF"], PR.exchange(d["qR"]))
    print("PARITY-RANGE [%s %s] combine: log_prob %.3f, log_prob(reversed) %.3f, queue (%d rows x %d) %.3f of 8 x 2^-52 x max(1, |value|)" %
          (cid, engine, worst, worst_rev, d["q"].shape[0], d["q"].shape[1], worst_q))
    assert not failures, failures
    assert not failures_rev, failures_rev
    assert not failures_q, failures_q


@pytest.mark.parametrize("cid,pin,engine", ROWS, ids=ROW_IDS)
def test_log_prob_against_float64(cid, pin, engine, monkeypatch):
    r, d, ref = PR.rungs(cid), device(cid, pin, engine, monkeypatch), PR.queue_reference(cid)
    worst, failures = PR.judge_rows(d["lp"], ref, r.sym)
    worst_rev, failures_rev = PR.judge_rows(d["lp_rev"], ref, r.sym)
    both = PR.over_bound(d["lp_rev"], d["lp"])
    print("PARITY-RANGE [%s %s] log_prob against float64: %.3f, reversed %.3f of the row bound (yardstick %.1e .. %.1e); "
          "log_prob(s) against log_prob(reversed s): %.3f of the combine bound; %d of %d values finite" %
          (cid, engine, worst, worst_rev, ref.y.min(), ref.y.max(), both.max(), np.isfinite(d["lp"]).sum(), len(d["lp"])))
    assert np.all(np.isfinite(d["lp"])) and np.all(np.isfinite(d["lp_rev"]))
    assert not failures, failures
    assert not failures_rev, failures_rev
    assert both.max() <= 1.0


@pytest.mark.parametrize("cid,pin,engine", ROWS, ids=ROW_IDS)
def test_queue_and_energies(cid, pin, engine, monkeypatch):
    c, r, d, ref = PR.case(cid), PR.rungs(cid), device(cid, pin, engine, monkeypatch), PR.queue_reference(cid)
    q, e = d["q"], d["e"]
    assert len(r.s) % F.tile_of_engine(engine)                      # the last tile is ragged
    print(F.line("PARITY-RANGE [%s %s] queue" % (cid, engine), F.measure(q, e, ref, d["lp"]), ref.seconds))
    worst_0, failures_0 = PR.judge_rows(q, ref, PR.sym_queue(PR.build_params(c), r.s))
    with np.errstate(over="ignore", invalid="ignore"):
        own = F.energies(q, r.s, ref.Jz)
        term = c.N * F.EPS64 * (np.abs(ref.diag) + F.BX * np.exp(0.5 * (q[1:] - q[0])).sum(axis=0))
        own_over = np.abs(e - own) / term
    own_over = np.where(np.isfinite(own_over), own_over, np.inf)
    print("PARITY-RANGE [%s %s] rows against the from-site-0 float64 queue %.3f of the row bound; E_loc against the float64 assembly of "
          "the device's queue %.3f of the summation term; |E_loc| up to %.2e" % (cid, engine, worst_0, own_over.max(), np.abs(e).max()))
    assert np.all(np.isfinite(q)) and np.all(np.isfinite(e))
    F.judge(q, e, ref, d["lp"], label="[%s %s]" % (cid, engine))
    assert not failures_0, failures_0
    assert np.array_equal(q[0], d["lp"]), "row 0 of the queue is not log_prob(s)"
    assert own_over.max() <= 1.0


def test_fused_step_equals_eloc_of_its_samples(monkeypatch):
    """The drawn spins are unpacked on the device and packed again reversed (prnn.hip: eloc_on_device); tfim_eloc packs the caller's
    upload.  Three spin words."""
    c = PR.case("10x70")
    par, _ = handles("10x70", None, monkeypatch)
    Jz, ns = F.couplings(c.N), 47
    out = par.vmc_step(ns, seed=F.SEED, step=0, couplings=np.append(Jz, F.BX), want_samples=True, want_eloc=True)
    s = out["samples"]
    assert s.shape == (ns, c.N) and np.all(np.isfinite(out["eloc"]))
    assert np.array_equal(out["eloc"], par.tfim_eloc(s, Jz, F.BX))
    assert np.array_equal(par.sample(ns, seed=F.SEED, step=0), s)


def device_gradient(c, prm, s, e, monkeypatch):
    from rnnwavefunctions_amd.training import cost_gradient
    par = make_wf("parity", (c.N, 1), (c.units,), prm, monkeypatch)
    par.load_batch(s, e)
    g = cost_gradient(par, prm, PR.SCOPE, e.mean(), len(s))
    par.close()
    return g


@pytest.mark.parametrize("batch", ["ladder", "ordinary"])
@pytest.mark.parametrize("cid", PR.CASE_IDS)
def test_shares_every_gradient_element(cid, batch, monkeypatch):
    """ladder: every rung in one batch - saturated shares, both directions deep, palindromes.  ordinary: the rungs above -600 alone."""
    t0 = time.time()
    c, r = PR.case(cid), PR.rungs(cid)
    prm = PR.build_params(c)
    idx = np.arange(len(r.s)) if batch == "ladder" else PR.ordinary(r)
    s = np.ascontiguousarray(r.s[idx])
    e = np.random.RandomState(5).standard_normal(len(r.s))[idx]
    g = device_gradient(c, prm, s, e, monkeypatch)
    ref = PR.gradient_reference(c, prm, s, e)
    label = "[%s %s]" % (cid, batch)
    worst, failures = G.judge(label, PR.gradient_case(c, len(s)), g, ref)
    print("PARITY-RANGE %s gradient of %d rungs (log P_sym %.0f .. %.2f): worst deviation / bound %.3f (limit %g), reference %.2f s, case %.2f s" %
          (label, len(s), r.sym[idx].min(), r.sym[idx].max(), worst, G.A.FACTOR, ref.seconds, time.time() - t0))
    assert all(np.all(np.isfinite(v)) for v in g.values())
    assert not failures, "tensors beyond %g x the bound: %s" % (G.A.FACTOR, failures)


def test_eleven_hundred_sites():
    """An untrained chain has log P near -N ln 2 = -762 at 1 100 sites: below exp's range before a single flip row is added."""
    from rnnwavefunctions_amd import _lib, params as P
    N, H, ns = 1100, 10, 32
    prm = P.init_gru_params([H], seed=111)
    wf = _lib.NativeWavefunction(_lib.MODEL_GRU1D_PARITY, N, 1, (H,))
    wf.set_params(prm, scope=PR.SCOPE)
    out = wf.vmc_step(ns, seed=1, step=0, couplings=np.append(np.ones(N), 1.0), want_samples=True, want_eloc=True)
    s, e = out["samples"], out["eloc"]
    lp = wf.log_prob(s)
    print("PARITY-RANGE [1100 sites] log_prob of the drawn chains %.1f .. %.1f, %d of %d below -745; %d energies finite" %
          (lp.min(), lp.max(), np.sum(lp < -745), ns, np.isfinite(e).sum()))
    assert s.shape == (ns, N) and np.all(np.isfinite(e))
    assert np.all(np.isfinite(lp)) and lp.min() < -745
    sub = [0, ns - 1]
    e_ref = E.ising_local_energies(np.ones(N), 1.0, s[sub], lambda x: PR.sym_log_prob(prm, x))
    print("PARITY-RANGE [1100 sites] max |E_loc - oracle| / N = %.2e (limit 1e-5)" % (np.abs(e[sub] - e_ref).max() / N))
    assert np.abs(e[sub] - e_ref).max() / N < 1e-5
