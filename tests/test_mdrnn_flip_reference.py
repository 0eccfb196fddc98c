"""CPU tests of tests/mdrnn_flip_reference.py, the reference and judge of tests/test_gpu_mdrnn_flip_full.py.

1. The licence of the row bound.  On the checked chains of every GPU case - the model's own draws of those chains, reproduced by the
   CPU oracle's sampler on the same uniforms - two honest float64 realisations of the queue, the prefix-sharing reference (`queue`:
   one stacked product per step) and the from-site-0 oracle (oracle.models.mdrnn_log_probability: four products per step), stay
   within 1/16 of the row bound 1e-11 N of the numpy.longdouble `queue`; the reference is finite on every row and the batch sharp.
   The table is printed.  The restated bookkeeping (`kernel_form`) without a switch reproduces the reference to the same measure.
2. Every defect model is refused by `judge` on at least one GPU case, and is shown BIT-INVISIBLE on the shapes where it cannot show:
   those facts are what justify the case table.  The defect tests run on the first four checked chains of a case (the last block's
   chains where the defect lives in the ragged block): a defect shows on any chain.
"""
import numpy as np
import pytest

import mdrnn_flip_reference as T

WIDTH_CASES = [("7x5-%d" % H, T.WIDTH_LATTICE[0], T.WIDTH_LATTICE[1], H, T.WIDTH_NS, T.width_scale(H), None, "width sweep") for H in T.WIDTHS]
ALL = T.CASES + WIDTH_CASES


def subject(cid, count=4, last_block=False):
    """(prm, s, ref, Jz) of `count` checked chains of a case: the first ones, or the last ones of the last block."""
    _, Nx, Ny, H, ns, scale, blocks, _ = next(c for c in ALL if c[0] == cid)
    prm = T.build_params(H, scale)
    chains = T.checked_chains(ns, blocks)
    chains = chains[-count:] if last_block else chains[:count]
    s = T.oracle_draws(prm, Nx, Ny, chains)
    Jz = T.couplings(Nx, Ny)
    return prm, s, T.Reference(prm, s, Jz, chains=chains, ns=ns), Jz


def small(Nx, Ny, H=20, B=4):
    """A lattice that is no GPU case (the old suite's scale), for an invisibility claim."""
    prm = T.build_params(H, 1.25)
    s = T.oracle_draws(prm, Nx, Ny, np.arange(B))
    return prm, s


@pytest.mark.parametrize("cid,Nx,Ny,H,ns,scale,blocks,why", ALL, ids=[c[0] for c in ALL])
def test_float64_realisations_stay_within_a_sixteenth_of_the_bound_of_longdouble(cid, Nx, Ny, H, ns, scale, blocks, why):
    """Measured here (worst over the cases, as fractions of the row bound 1e-11 N): reference 0.009 (9x11, 17 units), oracle 0.007,
    kernel_form against the reference 0.006 (3x33); config 4 0.001; 16x16 0.002."""
    N = Nx * Ny
    prm = T.build_params(H, scale)
    chains = T.checked_chains(ns, blocks)
    s = T.oracle_draws(prm, Nx, Ny, chains)
    Jz = T.couplings(Nx, Ny)
    ref = T.Reference(prm, s, Jz, chains=chains, ns=ns)
    e_o, lp_o = T.oracle_queue(prm, s, Jz)
    lp_l = T.queue(prm, s, np.longdouble)[0]
    lp_k = T.kernel_form(prm, s)
    bound = T.ROW_TOL * N
    with np.errstate(invalid="ignore"):
        fr = [float(np.nan_to_num(np.abs(a - b), nan=np.inf).max() / bound) for a, b in ((ref.lp, lp_l), (lp_o, lp_l), (lp_k, ref.lp), (lp_o, ref.lp))]
    m = T.judge(lp_o, e_o, ref, label="[%s oracle]" % cid)            # the oracle's queue and energies pass the judge
    print("LICENCE [%s x%.2f] %dx%d %d units, %d checked chains of %d: reference / longdouble %.4f  oracle / longdouble %.4f  "
          "kernel form / reference %.4f  oracle / reference %.4f of the bound %.2e; log r %.1f .. %.1f, std / mean %.2f, %d distinct" %
          (cid, scale, Nx, Ny, H, len(chains), ns, fr[0], fr[1], fr[2], fr[3], bound, 0.5 * (ref.lp[1:] - ref.lp[0]).min(),
           0.5 * (ref.lp[1:] - ref.lp[0]).max(), m["spread"], m["distinct"]))
    assert np.all(np.isfinite(ref.lp)) and np.all(np.isfinite(lp_o)) and np.all(np.isfinite(np.asarray(lp_l, dtype=np.float64)))
    assert fr[0] <= T.LICENCE and fr[1] <= T.LICENCE, "the float64 realisations leave 1/16 of the bound: lower this case's kernel scale"
    assert fr[2] <= T.LICENCE
    assert np.allclose(ref.e, e_o, rtol=1e-12, atol=0)


def test_another_summation_order_is_another_realisation():
    """The hidden units renumbered: the same function, other roundings - and still within the licence of each other."""
    prm, s, ref, _ = subject("13x5-50")
    lp = T.queue(prm, s, order=1)[0]
    d = np.abs(lp - ref.lp).max()
    print("13x5-50: units renumbered, max |difference| %.2e = %.4f of the bound" % (d, d / (T.ROW_TOL * ref.N)))
    assert 0 < d <= T.LICENCE * T.ROW_TOL * ref.N


def test_base_part_is_the_prefix_with_the_flipped_site():
    """baseq: row k's terms up to and including the flipped site - for the last visited site the whole row."""
    prm, s, ref, _ = subject("13x5-50")
    last = (13 - 1) * 5 + 4 + 1                                     # (12, 4): row 4 is even, the path ends at nx = 12
    assert np.array_equal(ref.base[last], ref.lp[last]) and np.array_equal(ref.base[0], ref.lp[0])
    assert np.all(ref.base[1:] >= ref.lp[1:])                        # the continuation only adds log-probabilities


# ---- the defects -------------------------------------------------------------------------------------------------------------------------

def refused(cid, make, last_block=False, count=4):
    """The defective queue of a case is refused by the judge; returns the worst row error / bound."""
    prm, s, ref, Jz = subject(cid, count, last_block)
    bad = make(prm, s, ref)
    assert bad is not None, "%s: the defect does not apply" % cid
    m = T.measure(bad, T.energies(bad, s, Jz), ref)
    with pytest.raises(AssertionError):
        T.judge(bad, T.energies(bad, s, Jz), ref, label=cid)
    assert m["row_over"] > 1.0                                      # and it is the rows that refuse it
    return m


def invisible(prm, s, **switches):
    return np.array_equal(T.kernel_form(prm, s, **switches), T.kernel_form(prm, s))


def knob(**switches):
    return lambda prm, s, ref: T.kernel_form(prm, s, **switches)


@pytest.mark.parametrize("switch", ["le_plus", "lt"])
def test_defect_a_switch_off_by_one(switch):
    """(a) pv <= i + 1 / pv < i.  Shows wherever a site has a vertical neighbour off the row turn: every case with Nx, Ny >= 2 (here
    config 4, 13x5, 5x13, 3x33).  Cannot show on 1x40 (every vertical operand is the row turn's) and 40x1 (none exists)."""
    for cid in ("cfg4", "13x5-50", "5x13-68", "3x33-50"):
        print("(a) %s %s: %.1e bounds" % (switch, cid, refused(cid, knob(switch=switch))["row_over"]))
    for cid in ("1x40-20", "40x1-20"):
        prm, s, _, _ = subject(cid)
        assert invisible(prm, s, switch=switch)


def test_defect_b_slot_not_mirrored():
    """(b) nx = j on odd rows.  Shows on every case with Nx, Ny >= 2; cannot show on 1x40 (one column) and 40x1 (no slot is read)."""
    for cid in ("cfg4", "13x5-50", "5x13-68", "33x3-50"):
        print("(b) %s: %.1e bounds" % (cid, refused(cid, knob(mirror=False))["row_over"]))
    for cid in ("1x40-20", "40x1-20"):
        prm, s, _, _ = subject(cid)
        assert invisible(prm, s, mirror=False)


def test_defect_c_row_turn():
    """(c) the row turn's vertical operand is zero.  Shows wherever there is a second row (here 3x33, 1x40, 13x5, config 4); cannot
    show on 40x1."""
    for cid in ("3x33-50", "1x40-20", "13x5-50", "cfg4"):
        print("(c) %s: %.1e bounds" % (cid, refused(cid, knob(turn="zero"))["row_over"]))
    prm, s, _, _ = subject("40x1-20")
    assert invisible(prm, s, turn="zero")


def test_defect_d_queue_row():
    """(d) Two readings.  Nx taken for Ny in the row index (nx Nx + ny + 1): shows on every non-square lattice (13x5, 5x13), is the
    identity - bit-invisible - on 12x12 and 16x16.  The transposed index ny Nx + nx + 1: a permutation of the rows that differs from
    the identity on every lattice with Nx, Ny >= 2, square ones included, so the rows refuse it on config 4 too; the ENERGY cannot see
    it on any lattice (it sums all rows), which is why the rows are judged."""
    for how in ("stride", "transposed"):
        for cid in ("13x5-50", "5x13-68", "11x3-35"):
            Nx, Ny = T.case(cid)[1:3]
            m = refused(cid, lambda prm, s, ref: T.inject_row_map(ref.lp, Nx, Ny, how))
            print("(d) %s %s: %.1e bounds" % (how, cid, m["row_over"]))
    for cid in ("cfg4", "16x16-50"):
        prm, s, ref, Jz = subject(cid, count=2)
        Nx, Ny = T.case(cid)[1:3]
        assert np.array_equal(T.inject_row_map(ref.lp, Nx, Ny, "stride"), ref.lp)
    m = refused("cfg4", lambda prm, s, ref: T.inject_row_map(ref.lp, 12, 12, "transposed"))
    assert m["e_over"] <= 1.0
    print("(d) transposed cfg4: rows %.1e bounds, E_loc %.1e of its bound" % (m["row_over"], m["e_over"]))
    for cid in ("1x40-20", "40x1-20"):
        prm, s, ref, _ = subject(cid)
        Nx, Ny = T.case(cid)[1:3]
        assert np.array_equal(T.inject_row_map(ref.lp, Nx, Ny, "transposed"), ref.lp)


def test_defect_e_vertical_bit_from_the_word_of_p():
    """(e) Shows where a site and the site above lie in different words (13x5, 11x3 - position 32 alone -, 16x16, config 4).  Cannot
    show up to 32 sites (8x4, one word) and on 40x1."""
    for cid in ("13x5-50", "11x3-35", "16x16-50", "cfg4"):
        print("(e) %s: %.1e bounds" % (cid, refused(cid, knob(vword="p"))["row_over"]))
    assert invisible(*small(8, 4), vword="p")
    prm, s, _, _ = subject("40x1-20")
    assert invisible(prm, s, vword="p")


def test_defect_f_flip_in_word_0():
    """(f) Shows where a flipped position >= 32 has a continuation (13x5, 3x33, config 4).  Cannot show up to 32 sites (8x4), nor on 33
    sites (11x3): position 32 is the last of the path, its row is complete after the base pass and it has no tile."""
    for cid in ("13x5-50", "3x33-50", "cfg4"):
        print("(f) %s: %.1e bounds" % (cid, refused(cid, knob(flip_word0=True))["row_over"]))
    assert invisible(*small(8, 4), flip_word0=True)
    prm, s, _, _ = subject("11x3-35")
    assert invisible(prm, s, flip_word0=True)


def test_defect_g_last_stored_row():
    """(g) Shows wherever there is a second row and more than one column (13x5, 3x33, 33x3, config 4).  Cannot show on 40x1 (no row
    below) and 1x40 (every vertical operand is the row turn's, no slot is read)."""
    for cid in ("13x5-50", "3x33-50", "33x3-50", "cfg4"):
        print("(g) %s: %.1e bounds" % (cid, refused(cid, knob(store_short=True))["row_over"]))
    for cid in ("1x40-20", "40x1-20"):
        prm, s, _, _ = subject(cid)
        assert invisible(prm, s, store_short=True)


@pytest.mark.parametrize("rem", [1, 2, 3, 4])
def test_defect_h_last_remainder_unit(rem):
    """(h) Shows at every width 16 f + rem (here f = 1, the narrowest, where one unit weighs most, and f = 5, where it weighs least).
    Widths at or below 16 have no remainder unit: the defect does not exist there."""
    for f in (1, 5):
        cid = "7x5-%d" % (16 * f + rem)
        print("(h) %s: %.1e bounds" % (cid, refused(cid, knob(drop_last_unit=True))["row_over"]))


def test_defect_i_invalid_lanes_of_a_ragged_block():
    """(i) Shows on every ragged case whose last block is checked (config 4 with 10 007 samples, 13x5 with 2 008, the width sweep's 40
    chains).  Does not exist where the batch is whole blocks (config 4 with 10 000, 16x16 with 528)."""
    for cid in ("cfg4-ragged", "13x5-50", "7x5-50"):
        print("(i) %s: %.1e bounds" % (cid, refused(cid, lambda prm, s, ref: T.inject_ragged(ref, ref.lp), last_block=True)["row_over"]))
    for cid in ("cfg4", "16x16-50"):
        prm, s, ref, _ = subject(cid, count=2, last_block=True)
        assert T.inject_ragged(ref, ref.lp) is None


def test_defect_j_stale_column_slot():
    """(j) Another chain's own state in a column slot.  Shows wherever a slot is read and the chains differ (config 4, 13x5, 5x13).
    Cannot show on 1x40 and 40x1 (no slot is read), nor between copies of one configuration (the lane-independence test's batch)."""
    for cid in ("cfg4", "13x5-50", "5x13-68"):
        print("(j) %s: %.1e bounds" % (cid, refused(cid, knob(stale_first=True))["row_over"]))
    for cid in ("1x40-20", "40x1-20"):
        prm, s, _, _ = subject(cid)
        assert invisible(prm, s, stale_first=True)
    prm, s, _, _ = subject("13x5-50")
    assert invisible(prm, np.repeat(s[:1], 4, axis=0), stale_first=True)
