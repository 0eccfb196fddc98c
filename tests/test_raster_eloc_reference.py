"""CPU validation of tests/raster_eloc_reference.py, the yardstick of tests/test_gpu_raster_eloc_full.py: no GPU.

The samples are the CPU oracle's own draws on the uniforms of (seed 111, step 0) - the rows the HIP samplers draw up to near-ties
(test_gpu_sampler_full.py) - on the sharpened parameters of every case of the table.

  1. the float64 reference against numpy.longdouble: below a tenth of the row bound 1e-11 N on every queue row of every case
  2. the prefix-sharing evaluation (queue_rows) equals the from-site-0 reference, so its knobs model defects of THIS computation
  3. every defect model (a)-(e) is rejected by `judge` on the cases meant to catch it
  4. (f), a wrong small ratio, is rejected by the row bound and accepted by the E_loc bound of the same case
  5. the reference passes `judge` against itself evaluated in other chunks
"""
import functools

import numpy as np
import pytest

import raster_eloc_reference as Q
import sampler_reference as R
from oracle import philox


@functools.lru_cache(maxsize=None)
def drawn(cid, ns=None):
    """(family, prm, s (ns, N), Jz, Nx, Ny) of a case; ns overrides the table's (the draws of chain b do not depend on ns)."""
    _, family, units, Nx, Ny, ns_case, sharp, _ = Q.case(cid)
    ns = ns or ns_case or Q.grid_stride_ns(Q.CUS)
    prm = R.build_params(family, units, seed=111, sharp=sharp)
    s = R.oracle_draw(family, prm, (Nx, Ny), philox.uniforms(111, 0, 0, ns, Nx * Ny)).reshape(ns, Nx * Ny)
    return family, prm, s, Q.couplings(Nx, Ny), Nx, Ny


@functools.lru_cache(maxsize=None)
def scored(cid, ns=None):
    family, prm, s, Jz, Nx, Ny = drawn(cid, ns)
    return Q.reference(family, prm, s, Jz, Q.BX, Nx, Ny)


def rejected(cid, lp=None, e=None, ns=None):
    """The figures of a defective queue (its energies assembled from it) or of defective energies; asserts that judge refuses them."""
    family, prm, s, Jz, Nx, Ny = drawn(cid, ns)
    e_ref, lp_ref = scored(cid, ns)
    if lp is None:
        lp = lp_ref
    elif e is None:
        e = Q.energies(lp, s, Jz, Q.BX, Nx, Ny)
    with pytest.raises(AssertionError):
        Q.judge(lp, e, lp_ref, e_ref, s, Jz, Q.BX, Nx, Ny)
    return Q.measure(lp, e, lp_ref, e_ref, s, Jz, Q.BX, Nx, Ny)


@pytest.mark.parametrize("cid", Q.CASE_IDS)
def test_float64_reference_against_longdouble(cid):
    """Every queue row (0 .. N) of a fixed stride of chains - 4 per case, 2 on the 144-site lattices, never chosen by outcome;
    longdouble NumPy has no BLAS - in 80-bit arithmetic.  Largest |float64 reference - longdouble| over 1e-11 N, kernel scale 3
    everywhere: LSTM 7.2e-4 (53 units, 9x11), one-layer GRU 1.4e-3 (100 units, 12x12), stacks 1.3e-3 (four layers of 20, 3x11).
    No case needed a lower scale."""
    family, prm, s, Jz, Nx, Ny = drawn(cid)
    N, ns = Nx * Ny, len(s)
    chains = np.arange(0, ns, max(1, ns // 4))[:4 if N <= 100 else 2]
    _, lp_ref = Q.reference(family, prm, s[chains], Jz, Q.BX, Nx, Ny)
    exact = Q.yardstick(family, prm, s[chains])
    assert exact.dtype == np.longdouble and np.finfo(np.longdouble).nmant >= 63
    err = float(np.abs(lp_ref - exact).max())
    print("[%s] chains %s: max |float64 reference - longdouble| = %.2e = %.2e of the row bound; log P %.1f .. %.1f" %
          (cid, chains.tolist(), err, err / (Q.ROW_TOL * N), lp_ref.min(), lp_ref.max()))
    assert err <= 0.1 * Q.ROW_TOL * N


def test_sharing_prefixes_changes_nothing():
    """queue_rows against chains scored one by one from site 0 with the same cells (longdouble: the restatements themselves), and
    its float64 run against the oracle-based reference within the yardstick's tenth of the row bound, flip bases included."""
    for cid in ("lstm-10-3x11", "gru64-20x2-5x13"):
        family, prm, s, Jz, Nx, Ny = drawn(cid)
        s, N = s[:5], Nx * Ny
        lpq, base, own = Q.queue_rows(family, prm, s, np.longdouble)
        for k in (0, 1, 31, 32, N - 1):
            flipped = s.copy()
            flipped[:, k] ^= 1
            alone, _, own_flipped = Q.queue_rows(family, prm, flipped, np.longdouble)
            assert np.abs(alone[0] - lpq[k + 1]).max() <= 1e-16 * N
            assert np.abs(own_flipped[k] - base[k]).max() <= 1e-16 * N          # the flip base: sites 0 .. k of the flipped chain
        e_ref, lp_ref = Q.reference(family, prm, s, Jz, Q.BX, Nx, Ny)
        lp64 = Q.queue_rows(family, prm, s)[0]
        assert np.abs(lp64 - lp_ref).max() <= 0.1 * Q.ROW_TOL * N
        assert np.abs(Q.energies(lp_ref, s, Jz, Q.BX, Nx, Ny) - e_ref).max() <= 1e-13 * np.abs(e_ref).max()


@pytest.mark.parametrize("cid", ["lstm-10-3x11", "lstm-21-5x13", "gru64-20-3x11", "gru64-20x2-5x13"])
def test_spins_read_from_word_0_are_rejected(cid):
    """(a) on 33 sites only site 32 is read wrong (as site 0); on 65 sites 33 of them are."""
    family, prm, s, Jz, Nx, Ny = drawn(cid)
    m = rejected(cid, lp=Q.inject_word0(family, prm, s, scored(cid)[1]))
    print(Q.line("[%s word 0]" % cid, m))
    assert m["row_over"] > 1e3


@pytest.mark.parametrize("cid", ["lstm-10-3x11", "lstm-36-8x8", "gru64-36-5x13", "gru64-36x3-3x11"])
def test_a_checkpoint_one_site_early_is_rejected(cid):
    family, prm, s, Jz, Nx, Ny = drawn(cid)
    m = rejected(cid, lp=Q.inject_checkpoint(family, prm, s, scored(cid)[1]))
    print(Q.line("[%s checkpoint]" % cid, m))
    assert m["row_over"] > 1e3


@pytest.mark.parametrize("cid", ["lstm-10-3x11", "lstm-53-9x11", "gru64-68-9x7", "gru64-20x4-3x11"])
def test_a_ragged_block_that_takes_its_last_chain_is_rejected(cid):
    """(c) 37 and 21 chains leave 5 in the last block, 17 and 33 leave one - which IS chain ns - 1, so those two cases can only
    show the defect through a wrong clamp, not through this model: they are asserted to pass it, the others to refuse it."""
    _, _, s, _, _, _ = drawn(cid)
    lp = Q.inject_ragged(scored(cid)[1])
    if len(s) % Q.CHAINS == 1:
        assert np.array_equal(lp, scored(cid)[1])
        return
    m = rejected(cid, lp=lp)
    print(Q.line("[%s ragged]" % cid, m))
    assert m["row_over"] > 1e3


def test_one_grid_stride_only_is_rejected():
    """(d) on the grid-stride case's model and lattice, sized for a device of 32 CUs (96 chains, 384 tiles, 256 waves): the rows of
    tiles 256 .. 383 keep their flip base."""
    cid, cus = "lstm-50-5x13-stride", 32
    ns = Q.grid_stride_ns(cus)
    family, prm, s, Jz, Nx, Ny = drawn(cid, ns)
    N = Nx * Ny
    assert (N - 1) * ((ns + Q.CHAINS - 1) // Q.CHAINS) > 8 * cus
    lp_ref = scored(cid, ns)[1]
    lp = Q.inject_one_stride(family, prm, s, lp_ref, 8 * cus)
    nsb = ns // Q.CHAINS
    touched = np.flatnonzero((lp != lp_ref).any(axis=1))
    assert touched.min() == 1 + (8 * cus) // nsb and touched.max() == N - 1       # row N has no tile: the base pass completes it
    m = rejected(cid, lp=lp, ns=ns)
    print(Q.line("[%s one stride]" % cid, m))
    assert m["row_over"] > 1e3
    # with as many waves as tiles nothing is left out
    assert np.array_equal(Q.inject_one_stride(family, prm, s, lp_ref, (N - 1) * nsb), lp_ref)


@pytest.mark.parametrize("cid", ["lstm-10-3x11", "lstm-37-11x3", "lstm-21-5x13", "gru64-69-11x3", "gru64-68-9x7"])
def test_bonds_on_the_transposed_reshape_are_rejected(cid):
    family, prm, s, Jz, Nx, Ny = drawn(cid)
    assert Nx != Ny
    m = rejected(cid, e=Q.inject_transposed_bonds(scored(cid)[0], s, Jz, Nx, Ny))
    print(Q.line("[%s transposed bonds]" % cid, m))
    assert m["e_over"] > 1e3 and m["row_over"] == 0.0


@pytest.mark.parametrize("cid", ["lstm-53-9x11", "gru64-20x4-3x11", "gru64-100-12x12"])
def test_a_wrong_small_ratio_is_seen_in_its_row_and_not_in_the_energy(cid):
    """(f) the reason for checking rows: E_loc moves by Bx |r' - r|, inside its bound, while the row is off by far more than its own."""
    family, prm, s, Jz, Nx, Ny = drawn(cid)
    e_ref, lp_ref = scored(cid)
    lp, (row, chain), r_true, r_bad = Q.inject_small_ratio(family, prm, s, lp_ref)
    assert r_true < 1e-6 and r_bad < 1e-6
    m = rejected(cid, lp=lp)
    print(Q.line("[%s small ratio %.2e -> %.2e at row %d chain %d]" % (cid, r_true, r_bad, row, chain), m))
    assert m["worst_row"] == (row, chain) and m["row_over"] > 1e3
    assert m["e_over"] <= 1.0                      # the energy bound of the same case lets it through


@pytest.mark.parametrize("cid", ["lstm-10-3x11", "lstm-36-8x8", "gru64-36-5x13", "gru64-20x4-3x11"])
def test_reference_passes_against_itself_in_other_chunks(cid):
    family, prm, s, Jz, Nx, Ny = drawn(cid)
    e_ref, lp_ref = scored(cid)
    e, lp = Q.reference(family, prm, s, Jz, Q.BX, Nx, Ny, chunk=7)
    m = Q.judge(lp, e, lp_ref, e_ref, s, Jz, Q.BX, Nx, Ny)
    print(Q.line("[%s chunks of 7]" % cid, m))
    assert m["row_over"] <= 0.1 and m["e_over"] <= 0.1


def test_every_case_is_sharp():
    """The sharpness condition of `judge` on the oracle's draws of every case (the grid-stride case on its first 96 chains)."""
    for cid in Q.CASE_IDS:
        ns = 96 if Q.case(cid)[5] is None else None
        family, prm, s, Jz, Nx, Ny = drawn(cid, ns)
        e_ref, lp_ref = scored(cid, ns)
        m = Q.judge(lp_ref, e_ref, lp_ref, e_ref, s, Jz, Q.BX, Nx, Ny)
        print(Q.line("[%s]" % cid, m))
