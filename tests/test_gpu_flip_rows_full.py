"""Every row of the f32-family TFIM local-energy (flip) pass against float64, at the sizes the project is benchmarked at: the positive
1D GRU on the bf16x3 engine (every width class, the layer pipeline, the parity-symmetric class) and on the f32-input MFMA (the f32 leg
of the benchmark, above 100 units, unequal stacks, the run script's size).

Every case builds sharpened weights (sampler_reference.build_params: kernels x 3, every bias randomised, seed 111), draws its samples
with sample(ns, seed=111, step=0) - the model's own configurations - takes random bonds Jz and Bx = 1, runs tfim_eloc(s, Jz, Bx,
log_probs=lp) ONCE on the whole batch and hands the queue rows and energies of a fixed set of whole tiles to
flip_rows_reference.judge.  The bounds come from the reference alone (that module's docstring): every row within 16 x the per-chain
float32 yardstick of the float64 reference, E_loc within the first-order propagation of the row bounds plus a float64 summation
term, row 0 within the row bound of wf.log_prob(s), all values finite, the checked batch sharp.  The checked tiles are the first, the
last (ragged where the case is) and fixed positions between, never chosen by outcome; each is checked at every flipped site (200
sites: at the fixed subset SITES_200), so its tiles span the whole walk and the last ones lie beyond the first lap of the persistent
grid - asserted from the CU count (8 waves on a CU: exact for the ping-pong kernels, a lower bound for the others) wherever the case
has more than 8 CUs tiles at all (the case table says which two have not).

test_flip_rows_reference.py shows on the CPU that the prefix-sharing reference equals the from-site-0 oracle, that three honest
float32 evaluations stay inside the bounds on these very sets of whole tiles (f32 C oracle: rows <= 0.40 of the bound, at 200 sites;
the float32 restatement in another summation order: <= 0.29; E_loc <= 0.04) and that every defect model is refused - among them a
bf16 split that lost its third term, which every full-size test before this one lets through.

Further tests on the same references: a state budget that splits config 2 into three passes returns the one-pass queue and energies
bit for bit; 70 copies of one configuration give identical rows in every lane of full and ragged tiles on both engines and on the
layer pipeline; the fused step returns sample()'s rows and tfim_eloc's energies bit for bit.

Measured on an MI355X (profiles/flip_rows_full_size.txt), worst row error / bound per width class and engine (E_loc error / bound
<= 0.06 everywhere; row 0 equals log_prob(s) bit for bit):
  bf16x3   flat 0.26 | aligned 0.11 (config 2: 0.16) | padded 0.09 | riders 0.14, 0.18 | streamed 0.13 | 200 sites, 100 units 0.20
           layer pipeline: two layers 0.16, three 0.14, four 0.32 | parity-symmetric 0.11
  f32mfma  config 2 0.14 | 128 units 0.18, 256 units 0.12 | (64, 20) 0.21 | 20 sites 0.12, one-wave base pass 0.14
bf16x3 is as close to float64 as the f32-input MFMA and as the CPU's honest float32 evaluations are.
The module takes 27 s, almost all of it references (0.1 to 3.8 s per case: the float64 queue and four float32 realisations).
"""
import numpy as np
import pytest

import flip_rows_reference as F
from test_gpu_sampler_full import make_wf

pytestmark = pytest.mark.gpu

NO_LAP = ("wide-256", "script-20", "script-20-nocoop")       # fewer than 8 x 256 tiles at any nearby shape: flip_rows_reference.CASES
_results = {}


def handle(cid, monkeypatch, more_env=None):
    c = F.case(cid)
    family, N, units, pin = c[1], c[2], c[3], c[5]
    env = dict(c[7], **(more_env or {}))
    if pin is not None:
        env["RNNWF_ENGINE"] = pin
    prm = F.build_params(family, units)
    return make_wf(family, (N, 1), units, prm, monkeypatch, env), prm


def eloc_with_queue(wf, s, Jz):
    lp = np.full((s.shape[1] + 1) * len(s), np.nan)
    e = wf.tfim_eloc(s, Jz, F.BX, log_probs=lp)
    return e, lp.reshape(s.shape[1] + 1, len(s))


def judged(ref, e, lp, log_prob, label):
    """`judge` on the checked chains of a whole batch's energies e (ns,) and queue lp (N + 1, ns); returns its figures."""
    lpc = lp[:, ref.chains]
    assembled = None
    if not ref.full:
        with np.errstate(over="ignore", invalid="ignore"):
            assembled = (F.energies(lpc, ref.s, ref.Jz, ref.Bx), np.exp(0.5 * (lpc[1:] - lpc[0])).sum(axis=0))
    return F.judge(lpc[ref.rows], e[ref.chains], ref, log_prob, assembled, label)


def one_pass(cid, monkeypatch):
    """The case's batch, its one-pass energies and queue, and the reference of its checked chains: computed once per module run."""
    if cid in _results:
        return _results[cid]
    _, family, N, units, ns, _, engine, _, count, sites, _ = F.case(cid)
    wf, prm = handle(cid, monkeypatch)
    s = wf.sample(ns, seed=F.SEED, step=0).reshape(ns, N)
    Jz = F.couplings(N)
    e, lp = eloc_with_queue(wf, s, Jz)
    assert wf.engine_name() == engine, "%s ran on %s" % (cid, wf.engine_name())
    tile = F.tile_of_engine(engine)
    chains = F.checked_chains(ns, tile, count)
    # the walk: tile (site k, column c) has index k x columns + c; site N - 1 has no tile (the base pass completes its row).  8 CUs
    # waves is the ping-pong kernels' grid and a lower bound of every other kernel's; 32 CUs is the hardware's ceiling
    cus = wf.device_info()["cu_count"]
    columns = (ns + tile - 1) // tile
    last_site = int(max(k for k in (range(N) if sites is None else sites) if k < N - 1))
    beyond = last_site * columns + int(chains[-1]) // tile
    print("[%s] %d CUs; %d tiles of %d chains; checked columns %s; last checked tile %d: lap %d of 8 waves per CU, lap %d of 32" %
          (cid, cus, (N - 1) * columns, tile, F.checked_tiles(ns, tile, count).tolist(), beyond, beyond // (8 * cus), beyond // (32 * cus)))
    if cid not in NO_LAP:
        assert beyond >= 8 * cus, "%s: no checked tile beyond the first lap (%d < %d)" % (cid, beyond, 8 * cus)
    ref = F.Reference(family, prm, s[chains], Jz, F.BX, sites, chains, ns, tile)
    _results[cid] = (s, Jz, e, lp, ref, wf.log_prob(s[chains]))
    return _results[cid]


@pytest.mark.parametrize("cid", F.CASE_IDS)
def test_queue_rows_and_energies_against_float64(cid, monkeypatch):
    s, Jz, e, lp, ref, log_prob = one_pass(cid, monkeypatch)
    lpc = lp[:, ref.chains]
    with np.errstate(over="ignore", invalid="ignore"):
        assembled = None if ref.full else (F.energies(lpc, ref.s, Jz), np.exp(0.5 * (lpc[1:] - lpc[0])).sum(axis=0))
    # the figures first, so that a failing case still prints them
    print(F.line("[%s %s]" % (cid, F.case(cid)[6]), F.measure(lpc[ref.rows], e[ref.chains], ref, log_prob, assembled), ref.seconds))
    judged(ref, e, lp, log_prob, "[%s: %s]" % (cid, F.case(cid)[-1]))
    assert np.all(np.isfinite(e)) and np.all(np.isfinite(lp))          # the whole batch, not only the checked tiles


def test_several_passes_are_bit_identical(monkeypatch):
    """Config 2, ragged: one 16-chain block keeps (N - 1) sites x 13 rows x 64 lanes x 4 bytes = 262 912 bytes of checkpoints
    (prnn.hip: hck_bytes_per_block, KT = 4 NFULL + 1), so 64 MB hold 255 blocks = 4 080 chains: passes of 4 080, 4 080 and 1 847
    chains, whose boundaries fall inside 32-chain tiles of the one-pass run."""
    cid = "cfg2-ragged"
    s, Jz, e1, lp1, ref, log_prob = one_pass(cid, monkeypatch)
    many, _ = handle(cid, monkeypatch, {"RNNWF_STATE_BUDGET_MB": "64"})
    many.timing_enable(True)
    many.timing_reset()
    e2, lp2 = eloc_with_queue(many, s, Jz)
    launches = [many.timing_get(k)["launches"] for k in range(3)]
    print("[passes] launches of the base, flip and assembly timers: %s" % launches)
    assert many.engine_name() == "bf16x3"
    assert launches[1] == 3
    assert np.array_equal(e1, e2) and np.array_equal(lp1, lp2)
    judged(ref, e2, lp2, many.log_prob(ref.s), "[passes]")


@pytest.mark.parametrize("units,pin,engine", [((50,), "bf16x3", "bf16x3"), ((50,), "f32", "f32mfma"), ((50, 50), "bf16x3", "bf16x3")],
                         ids=["bf16x3", "f32mfma", "pipeline"])
def test_copies_of_one_configuration_give_identical_rows(units, pin, engine, monkeypatch):
    """70 copies: two full 32-chain tiles and a ragged third of 6, or four 16-chain blocks and a ragged fifth: every lane, clamped ones
    included, computes the same.  (70 chains are far below the default's threshold for bf16x3, so the engine is pinned either way.)"""
    N = 80
    prm = F.build_params("gru", units)
    wf = make_wf("gru", (N, 1), units, prm, monkeypatch, {"RNNWF_ENGINE": pin})
    s = np.repeat(wf.sample(3, seed=F.SEED, step=0).reshape(3, N)[2:], 70, axis=0)
    e, lp = eloc_with_queue(wf, s, F.couplings(N))
    assert wf.engine_name() == engine
    assert np.all(np.isfinite(lp)) and np.all(lp == lp[:, :1]) and np.all(e == e[0])


def test_fused_step_equals_sample_and_eloc(monkeypatch):
    N, units, ns = 80, (50,), 10000
    prm = F.build_params("gru", units)
    wf = make_wf("gru", (N, 1), units, prm)
    Jz = F.couplings(N)
    out = wf.vmc_step(ns, seed=F.SEED, step=0, couplings=np.append(Jz, F.BX), want_samples=True, want_eloc=True)
    assert wf.engine_name() == "bf16x3"
    s = wf.sample(ns, seed=F.SEED, step=0)
    assert np.array_equal(out["samples"], s)
    e = wf.tfim_eloc(s, Jz, F.BX)
    assert np.array_equal(out["eloc"], e)
    m = out["moments"]
    assert m[2] == ns and np.isclose(m[0], e.sum(), rtol=1e-12, atol=0) and np.isclose(m[1], (e * e).sum(), rtol=1e-12, atol=0)
