"""CPU validation of tests/flip_rows_reference.py, the reference, yardstick and judge of tests/test_gpu_flip_rows_full.py: no GPU.

The chains are drawn by the CPU oracle's own sampler on the uniforms of (seed 111, step 0) - the rows the HIP sampler draws up to
near-ties (test_gpu_sampler_full.py).  The case of 200 sites keeps its subset of flipped sites.  Two sets of chains per case:
  whole   the whole tiles the GPU test checks (flip_rows_reference.CASES): 134 to 576 chains - what 2. runs on
  cut     of at most four of those tiles (first, last, two between) the first 8 chains, of the last one its last 8 valid chains, so
          that the ragged edge stays in - what 1. and 3. run on

  1. the prefix-sharing evaluation (`queue`) equals the from-site-0 oracle in float64 to rounding: every row of 6 chains of every case
  2. three honest float32 evaluations pass `judge` on the WHOLE set of every case, and their worst deviation / bound is printed:
       the f32 C oracle (oracle.cport, from site 0; one-layer GRU only),
       the NumPy oracle in float32 from site 0 (oracle.models with dtype float32), and
       the prefix-sharing float32 restatement with its hidden units in an order the yardstick does not use (order 7).
     The prefix-sharing restatement in the model's own order is one of the yardstick's realisations and shows nothing (1 / 16 of the
     bound by construction); NumPy from site 0 often repeats it bit for bit (the same products in the same order), so the C oracle
     and order 7 are the independent ones.  The 200-site case runs on a second set as well - the same number of tile columns, each
     moved on by 5 - because that is where the bound was once too tight: with ONE float32 realisation as the yardstick the C
     oracle reached 1.87 x the bound on the whole set (chain 398, row 25), which the 8-chain cut had not shown.  The yardstick now
     takes the maximum over four realisations (flip_rows_reference: ORDERS); FACTOR is unchanged.
     Measured, worst row deviation / bound over the whole sets: C oracle 0.40 (200 sites, chain 398; on
     the other columns 0.21; next case 0.21, 128 units), order 7 0.29 ((64, 20); 200 sites 0.23 and 0.14), NumPy from site 0 0.15
     (two layers); E_loc error / bound <= 0.04.
  3. every defect model (a) - (h) is refused by `judge` on the cut of every case where it can exist: (c) needs more than 32 sites,
     (e) a ragged last tile with at least two chains, (g) a stack.  Measured, as row error / bound: (a) weights cut to two
     bf16 terms 2.0 (wide-256, an f32mfma case) .. 13, at the bf16x3 cases 4.5 (stack-4) .. 13 (flat-36); (b) the state cut likewise
     2.4 (script-20) .. 16; every other defect is beyond its bound by a factor of 700 or more.
     FINDING about the bound: on the four-layer case (33 sites, 4 x 44 units) a cut of 8 chains per tile did NOT refuse (b), the
     hidden state cut to 16 bits (0.74 of the bound under the one-realisation yardstick; the present one is no tighter), and barely (a): four layers' float32 yardstick is the largest of the table over the shortest
     chains.  On whole tiles (128 chains) both are refused, so this case alone runs 3. on whole tiles (WHOLE_TILES): (a) 4.5, (b) 5.6.
     A 16-bit state is seen at four layers only because many chains are checked; confined to few chains of such a stack it would pass.
"""
import functools

import numpy as np
import pytest

import flip_rows_reference as F
import sampler_reference as R
from oracle import philox

PER_TILE = 8
TILES = 4                          # at most: the first, the last and two between
WHOLE_TILES = ("stack-4",)         # see 3. in the module docstring


@functools.lru_cache(maxsize=None)
def drawn(cid, whole=False, shift=0):
    """(family, prm, s, Jz, Reference) of a case's cut, or of the whole tiles the GPU test checks (shift: another set of columns)."""
    _, family, N, units, ns, _, engine, _, count, sites, _ = F.case(cid)
    tile = F.tile_of_engine(engine)
    if whole:
        chains = F.checked_chains(ns, tile, count, shift=shift)
    else:
        chains = F.checked_chains(ns, tile, min(count, TILES), None if cid in WHOLE_TILES else PER_TILE)
    prm = F.build_params(family, units)
    s = R.oracle_draw(family, prm, (N, 1), philox.uniforms(F.SEED, 0, 0, ns, N)[chains]).reshape(len(chains), N)
    Jz = F.couplings(N)
    return family, prm, s, Jz, F.Reference(family, prm, s, Jz, F.BX, sites, chains, ns, tile)


def checked_configurations(ref):
    """((1 + sites) B, N): the configurations of the rows ref.rows of the checked chains, row-major."""
    q = np.repeat(ref.s[None], len(ref.rows), axis=0)
    for j, k in enumerate(ref.sites):
        q[j + 1, :, k] ^= 1
    return q.reshape(-1, ref.N)


@pytest.mark.parametrize("cid", F.CASE_IDS)
def test_sharing_prefixes_equals_the_oracle_from_site_0(cid):
    """float64 to rounding: 1e-15 per site on |log P| of order N (the two sum the same terms; BLAS blocks the products differently)."""
    family, prm, s, Jz, ref = drawn(cid)
    pick = np.r_[0:3, ref.B - 3:ref.B]
    e0, lp0 = F.oracle_reference(family, prm, s[pick], Jz)
    err = np.abs(lp0[ref.rows] - ref.lp64[:, pick]).max()
    tol = 1e-15 * ref.N * np.abs(lp0).max()
    print("[%s] chains %s, %d rows each: max |queue - oracle from site 0| = %.2e (tolerance %.2e)" %
          (cid, ref.chains[pick].tolist(), len(ref.rows), err, tol))
    assert err <= tol
    if ref.full:
        assert np.abs(e0 - ref.e64[pick]).max() <= 1e-13 * np.abs(e0).max()


@pytest.mark.parametrize("cid,shift", [(c, 0) for c in F.CASE_IDS] + [("cfg5-shape", 5)],
                         ids=F.CASE_IDS + ["cfg5-shape-other-columns"])
def test_honest_float32_evaluations_stay_inside_the_bound(cid, shift):
    family, prm, s, Jz, ref = drawn(cid, True, shift)
    units, sites = F.case(cid)[3], F.case(cid)[9]
    x = checked_configurations(ref)
    honest = []
    if family == "gru" and len(units) == 1:
        from oracle import cport
        honest.append(("f32 C oracle", cport.prnn_log_probability(prm, x)))
    with np.errstate(over="ignore"):
        honest.append(("NumPy float32 from site 0", F.log_prob_fn(family, prm, np.float32)(x)))
    honest.append(("prefix-sharing float32, order 7", F.queue(family, prm, s, np.float32, sites, order=7)))
    for name, lp in honest:
        lp = lp.reshape(len(ref.rows), ref.B)
        m = F.judge(lp, F.energies(lp, s, Jz, F.BX) if ref.full else None, ref, label="[%s %s]" % (cid, name))
        print(F.line("[%s%s %s]" % (cid, " columns + %d" % shift if shift else "", name), m, ref.seconds))
    assert 7 not in F.ORDERS
    # the yardstick's own realisations: 1 / FACTOR of the bound by construction
    assert max(F.measure(lp, None, ref)["row_over"] for lp in ref.lp32) <= 1.0 / F.FACTOR


KNOBS = [("a weights16", dict(weights16=True)), ("b state16", dict(state16=True)), ("c word0", dict(word0=True)),
         ("d checkpoint early", dict(checkpoint_shift=1)), ("d checkpoint late", dict(checkpoint_shift=-1)), ("g lagged", dict(lagged=True))]


@pytest.mark.parametrize("cid", F.CASE_IDS)
def test_every_defect_is_refused(cid):
    family, prm, s, Jz, ref = drawn(cid)
    _, _, N, units, _, _, _, _, _, sites, _ = F.case(cid)
    defects = []
    for name, knob in KNOBS:
        if (name[0] == "c" and N <= 32) or (name[0] == "g" and len(units) == 1):
            continue
        defects.append((name, F.queue(family, prm, s, np.float64, sites, **knob)))
    ragged = F.inject_ragged(ref, ref.lp64)
    if ragged is not None:
        defects.append(("e ragged", ragged))
    defects += [("f unwritten", F.inject_unwritten(ref, ref.lp64)), ("h neighbour", F.inject_neighbour(ref, ref.lp64))]
    passed = []
    for name, lp in defects:
        e = F.energies(lp, s, Jz, F.BX) if ref.full else None
        m = F.measure(lp, e, ref)
        print(F.line("[%s %s]" % (cid, name), m))
        try:
            F.judge(lp, e, ref)
            passed.append(name)
        except AssertionError:
            pass
    assert not passed, "%s: judge lets through %s" % (cid, passed)
    # the clean queue passes: what refused the defects is the defects
    F.judge(ref.lp64, ref.e64, ref)


def test_the_edits_touch_what_they_say():
    """(e), (f), (h) on the ragged config-2 case: which entries change, and that a case without a ragged pair has no (e)."""
    _, _, _, _, ref = drawn("cfg2-ragged")
    lp = ref.lp64
    assert ref.chains[-1] == ref.ns - 1 == 10006 and ref.ns % ref.tile == 23
    changed = np.argwhere(F.inject_ragged(ref, lp) != lp)
    assert set(changed[:, 1]) == {ref.B - 1}
    changed = np.argwhere(F.inject_unwritten(ref, lp) != lp)
    assert set(changed[:, 0]) == {ref.N - 1} and set(ref.chains[changed[:, 1]] // ref.tile) == {312}     # site N - 2, the last tile
    changed = np.argwhere(F.inject_neighbour(ref, lp) != lp)
    assert changed.tolist() == [[1 + ref.N // 2, 0]]
    assert F.inject_ragged(drawn("flat-36")[4], drawn("flat-36")[4].lp64) is None


def test_a_failure_names_its_coordinates():
    _, _, _, _, ref = drawn("cfg2-ragged")
    lp = ref.lp64.copy()
    lp[34, ref.B - 1] += 1.0
    with pytest.raises(AssertionError) as err:
        F.judge(lp, None, ref)
    text = str(err.value)
    assert "flipped site 33 (spin word 1, bit 1), chain 10006, tile column 312 of 32 chains = tile %d of the walk" % (33 * 313 + 312) in text
    lp = ref.lp64.copy()
    lp[0, 0] = np.nan
    with pytest.raises(AssertionError, match="non-finite"):
        F.judge(lp, None, ref)
    with pytest.raises(AssertionError, match="row 0 of the queue"):
        F.judge(ref.lp64, None, ref, log_prob=ref.lp64[0] + 2.0 * ref.bound)


def test_glorot_weights_are_not_sharp():
    """The sharpness condition refuses the initialisation every ratio of which is ~1."""
    _, family, N, units, ns, _, engine, _, count, _, _ = F.case("aligned-37")
    prm = R.build_params(family, units, seed=F.SEED, sharp=None)
    s = R.oracle_draw(family, prm, (N, 1), philox.uniforms(F.SEED, 0, 0, 32, N)).reshape(32, N)
    ref = F.Reference(family, prm, s, F.couplings(N))
    with pytest.raises(AssertionError, match="not sharp"):
        F.judge(ref.lp64, ref.e64, ref)
