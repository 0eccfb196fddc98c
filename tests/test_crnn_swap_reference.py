"""CPU validation of tests/crnn_swap_reference.py, the reference, yardstick and judges of tests/test_gpu_crnn_swap_full.py: no GPU.

The chains are drawn by the CPU oracle's own sampler (oracle.models.crnn_sample) on the uniforms of (seed 111, step 0) - the rows the
HIP sampler draws up to near-ties (test_gpu_sampler_full.py) - and are the very 16-chain blocks the GPU test checks.

  1. the prefix-sharing restatement (`log_ratios`) equals the from-site-0 oracle (M.crnn_log_amplitude, float64, on written-out
     exchanged rows) to rounding on four chains of every case's shape, all 2 N bonds
  2. `connected` equals oracle.estimators.j1j2_slices row for row, with and without the periodic and Marshall flags, with zero couplings
  3. two honest float32 evaluations pass the probe judge and the energy judge (open; periodic with Marshall) on the WHOLE checked set
     of every case, and their worst deviation / bound is printed: M.crnn_log_amplitude in float32 from site 0 (complex64 terms, summed
     as the oracle sums them) and the float32 restatement with the hidden units in an order the yardstick does not use (order 7).
     Measured, worst deviation / bound over the cases: ratios 0.41 (w69, from site 0; order 7: 0.12) where the ratio term of the
     bound decides; where a ratio lies below the float32 rounding of the complex64 output the bound is that rounding itself and an
     entry reaches 0.77 .. 0.99 of it by construction (it cannot exceed it); energies 0.18 (w69).  Nothing had to be added: four
     realisations and kernels x 3 as flip_rows_reference, FACTOR unchanged.
  4. every defect model (a) - (l) is refused on every case where it can show: (l) needs a stack; (k) a ragged last block whose last
     two chains differ on a bond both have (all but 10 000 samples and the cases that drew the same row twice - printed); (j) a wrap
     bond whose ratio is not negligible - the six cases J_SHOWS (|r| 0.55 .. 9.2); at the others, config 3's shape among them, every
     exchange across the wrap is suppressed below 1e-4 (config 3: 3e-9, under the output's rounding) and nothing about a wrap bond's
     amplitude can show there; (c) exists everywhere (every case has more than 32 sites).  (i) is judged by the energy judge (periodic,
     Marshall on), the others by the probe judge.  Measured: (a) weights cut to two bf16 terms 3.4 (w69) .. 11 x the bound, (b) the state cut
     likewise 5.2 (n66) .. 11 x, every other defect beyond its bound by a factor of 200 or more.
  5. every case is sharp on the oracle's own samples (largest ratio above 3); the glorot initialisation is not.
"""
import functools

import numpy as np
import pytest

import crnn_swap_reference as C
import sampler_reference as R
from crnn_pauli_reference import random_sector_samples
from oracle import estimators as E
from oracle import models as M
from oracle import philox


@functools.lru_cache(maxsize=None)
def drawn(cid):
    """(prm, s, Reference, probed slots) of the blocks the GPU test checks."""
    _, N, units, ns, _, engine, count, slots, _ = C.case(cid)
    chains = C.checked_chains(ns, C.BLOCK, count)
    prm = C.build_params(units)
    s = M.crnn_sample(prm, N, philox.uniforms(C.SEED, 0, 0, ns, N)[chains])
    assert np.all(s.sum(axis=1) == N // 2)
    slots = np.arange(2 * N) if slots is None else np.asarray(slots)
    return prm, s, C.Reference(prm, s, chains, ns, C.tile_of_engine(engine)), slots


def runs(ref):
    """The two energy runs of the GPU test: open; periodic with the Marshall sign."""
    J1, J2, Bz = C.random_couplings(ref.N)
    return [("open", C.connected(ref.s, J1, J2, Bz)), ("periodic, Marshall", C.connected(ref.s, J1, J2, Bz, True, True))]


@pytest.mark.parametrize("cid", C.CASE_IDS)
def test_sharing_prefixes_equals_the_oracle_from_site_0(cid):
    """float64 to rounding: 1e-15 per site on |log psi| (the two sum the same terms; BLAS blocks the products differently)."""
    prm, s, ref, _ = drawn(cid)
    pick = np.r_[0:2, ref.B - 2:ref.B]
    d0 = C.oracle_log_ratios(prm, s[pick], ref.lo, ref.hi)
    _, own = C.log_ratios(prm, s[pick], (ref.lo, ref.hi), return_own=True)
    a = ref.anti[:, pick]
    assert np.all(np.isfinite(d0[a])) and np.all(np.isfinite(ref.d64[ref.anti]))
    err = np.abs(d0 - ref.d64[:, pick])[a].max()
    tol = 1e-15 * ref.N * max(1.0, float(np.abs(own).max()))
    own0 = M.crnn_log_amplitude(R.cast(prm, np.float64), s[pick], dtype=np.float64)
    print("[%s] chains %s, %d ratios: max |restatement - oracle from site 0| = %.2e (tolerance %.2e); log psi itself %.2e" %
          (cid, ref.chains[pick].tolist(), int(a.sum()), err, tol, np.abs(own - own0).max()))
    assert err <= tol and np.abs(own - own0).max() <= tol


@pytest.mark.parametrize("periodic", [False, True])
@pytest.mark.parametrize("marshall", [False, True])
def test_connected_equals_j1j2_slices(periodic, marshall):
    for N in (6, 34, 66):
        s = random_sector_samples(N, 24, N)
        J1, J2, Bz = C.random_couplings(N)
        J1[3], J2[1], J2[N - 2], J1[N - 1] = 0.0, 0.0, 0.0, (0.0 if N == 6 else J1[N - 1])
        con = C.connected(s, J1, J2, Bz, periodic, marshall)
        sig, H, offs = E.j1j2_slices(J1, J2, Bz, s, periodic, marshall)
        assert np.array_equal(np.diff(offs), con.count)
        assert np.all(con.lo < con.hi) and np.array_equal(con.slot, np.sort(con.slot))
        for b in range(len(s)):
            rows, h = sig[offs[b]:offs[b + 1]], H[offs[b]:offs[b + 1]]
            k = np.flatnonzero(con.active[:, b])
            assert np.array_equal(rows[0], s[b]) and h[0] == np.float32(con.diag[b])
            assert np.array_equal(rows[1:], C.swapped_rows(s[b:b + 1], con.lo[k], con.hi[k])[:, 0])
            assert np.array_equal(h[1:], con.coef[k].astype(np.float32))
            assert con.of(b) == [(int(con.slot[j]), int(con.lo[j]), int(con.hi[j]), float(con.coef[j])) for j in k]
    # the slots and their (lo, hi) are those of all_bonds
    lo, hi = C.all_bonds(N)
    assert np.array_equal(lo[con.slot], con.lo) and np.array_equal(hi[con.slot], con.hi)
    assert np.array_equal(con.slot < N, con.dist == 1) and np.array_equal(con.slot % N, con.site)


@pytest.mark.parametrize("cid", C.CASE_IDS)
def test_honest_float32_evaluations_stay_inside_the_bounds(cid):
    prm, s, ref, slots = drawn(cid)
    honest = [("NumPy float32 from site 0", C.oracle_log_ratios(prm, s, ref.lo, ref.hi, np.float32)),
              ("prefix-sharing float32, order 7", C.log_ratios(prm, s, (ref.lo, ref.hi), np.float32, order=7))]
    assert 7 not in C.ORDERS
    for name, d in honest:
        m = C.judge_probes(C.probes_from(d, ref, slots), ref, slots, "[%s %s]" % (cid, name))
        print(C.probe_line("[%s %s]" % (cid, name), m, ref.seconds))
        for run, con in runs(ref):
            print(C.energy_line("[%s %s, %s]" % (cid, name, run), C.judge_energies(C.energies_from(d, ref, con), ref, con, "[%s %s %s]" % (cid, name, run))))
    # the yardstick's own realisations: 1 / FACTOR of the ratio bound by construction (plus the output's rounding)
    assert max(C.measure_probes(C.probes_from(d, ref, slots, False), ref, slots)["over"] for d in ref.d32) <= 1.001 / C.FACTOR + 0.05
    # and the reference passes its own judges
    assert C.judge_probes(C.probes_from(ref.d64, ref, slots), ref, slots)["over"] <= 1.0


KNOBS = [("a weights16", dict(weights16=True)), ("b state16", dict(state16=True)), ("c word0", dict(word0=True)),
         ("d hi not flipped", dict(keep_hi=True)), ("e restart early", dict(restart_shift=1)), ("e restart late", dict(restart_shift=-1)),
         ("f up-count + 1", dict(count_shift=1)), ("f up-count - 1", dict(count_shift=-1)), ("l lagged", dict(lagged=True))]


J_SHOWS = ("w37", "w53", "w68", "wide-128", "cfg3-l2", "stack-3")       # cases whose largest wrap ratio is of order 1


@pytest.mark.parametrize("cid", C.CASE_IDS)
def test_every_defect_is_refused(cid):
    prm, s, ref, slots = drawn(cid)
    units = C.case(cid)[2]
    defects = [(name, C.log_ratios(prm, s, (ref.lo, ref.hi), **knob)) for name, knob in KNOBS if name[0] != "l" or len(units) > 1]
    defects += [("g neighbour", C.inject_neighbour(ref, ref.d64, slots)), ("h zero", C.inject_zero(ref, ref.d64, slots)),
                ("j unwrapped", C.log_ratios(prm, s, C.unwrapped(ref.N), only=ref.anti))]
    ragged = C.inject_ragged(ref, ref.d64)
    assert (ragged is None) == (cid == "cfg3-l2")            # 10 000 samples: the only case without a ragged block
    if ragged is not None:
        # (k) can show only where the last two chains differ on a bond both have (sharp weights draw the same row more than once)
        both = ref.anti[:, -1] & ref.anti[:, -2]
        differ = float(np.abs(ref.r[both, -1] - ref.r[both, -2]).max()) if both.any() else 0.0
        print("[%s] last two chains: largest difference of a ratio both have %.2e" % (cid, differ))
        assert differ > 1e-3 or cid not in ("cfg3-ragged", "cfg3-f32")
        if differ > 1e-3:
            defects.append(("k ragged", ragged))
    # (j) can show only where a wrap bond's ratio is well above the output's rounding (3e-8): crnn_swap_reference's docstring
    wrap = float(np.abs(ref.r[C.wrap_slots(ref.N)]).max())
    print("[%s] largest |ratio| of a wrap bond on the checked chains: %.2e" % (cid, wrap))
    assert wrap > 1e-4 or cid not in J_SHOWS
    passed = []
    for name, d in defects:
        if name[0] == "j" and cid not in J_SHOWS:
            continue
        E_ = C.probes_from(d, ref, slots)
        m = C.measure_probes(E_, ref, slots)
        print(C.probe_line("[%s %s]" % (cid, name), m))
        try:
            C.judge_probes(E_, ref, slots)
            passed.append(name)
        except AssertionError:
            pass
    # (i): the energies of the periodic run with the Marshall sign on the J2 bonds too, against the run's reference
    J1, J2, Bz = C.random_couplings(ref.N)
    con, bad = C.connected(s, J1, J2, Bz, True, True), C.connected(s, J1, J2, Bz, True, True, marshall_j2=True)
    e = C.energies_from(ref.d64, ref, bad)
    print(C.energy_line("[%s i marshall on J2]" % cid, C.measure_energies(e, ref, con)))
    try:
        C.judge_energies(e, ref, con)
        passed.append("i marshall on J2")
    except AssertionError:
        pass
    assert not passed, "%s: the judges let through %s" % (cid, passed)
    C.judge_energies(C.energies_from(ref.d64, ref, con), ref, con)


@pytest.mark.parametrize("cid", C.CASE_IDS)
def test_every_case_is_sharp_on_the_oracles_samples(cid):
    _, _, ref, slots = drawn(cid)
    print("[%s] largest |ratio| of %d checked chains: %.3g; reference %.1f s" % (cid, ref.B, C.assert_sharp(ref), ref.seconds))
    assert float(np.abs(ref.r[slots]).max()) > 3.0           # the probed bonds alone are sharp too


def test_glorot_weights_are_not_sharp():
    _, N, units, ns, _, _, _, _, _ = C.case("w37")
    prm = R.build_params("crnn", units, seed=C.SEED, sharp=None)
    s = M.crnn_sample(prm, N, philox.uniforms(C.SEED, 0, 0, 32, N))
    with pytest.raises(AssertionError, match="not sharp"):
        C.assert_sharp(C.Reference(prm, s))


def test_the_edits_touch_what_they_say_and_a_failure_names_its_coordinates():
    _, _, ref, slots = drawn("n66")
    slots = np.arange(2 * ref.N)
    d = ref.d64
    same = lambda a, b: (a == b) | (np.isnan(a) & np.isnan(b))
    assert ref.chains[-1] == ref.ns - 1 == 1030 and ref.ns % C.BLOCK == 7
    changed = np.argwhere(~same(C.inject_ragged(ref, d), d))
    assert set(changed[:, 1]) == {ref.B - 1}
    for edit in (C.inject_neighbour, C.inject_zero):
        changed = np.argwhere(~same(edit(ref, d, slots), d))
        assert len(changed) == 1 and ref.anti[tuple(changed[0])]
    # a wrong ratio in the second spin word of the last, ragged block
    slot = next(k for k in range(32, 63) if ref.anti[k].any())
    assert ref.lo[slot] == slot and ref.hi[slot] == slot + 1
    b = int(np.flatnonzero(ref.anti[slot])[-1])
    bad = d.copy()
    bad[slot, b] += 1e-2
    with pytest.raises(AssertionError) as err:
        C.judge_probes(C.probes_from(bad, ref, slots), ref, slots)
    text = str(err.value)
    assert ("sample %d, bond slot %d (J1 bond of site %d: lo %d in spin word 1, hi %d in spin word 1), %d ups below lo, tile (lo %d, item >= "
            % (ref.chains[b], slot, slot, slot, slot + 1, ref.s[b, :slot].sum(), slot)) in text
    E_ = C.probes_from(d, ref, slots)
    k, b0 = np.argwhere(~ref.anti[slots])[0]
    E_[k, b0] += 1e-7j
    with pytest.raises(AssertionError, match="not exactly the diagonal"):
        C.judge_probes(E_, ref, slots)
    E_ = C.probes_from(d, ref, slots)
    E_[0, 0] = np.nan
    with pytest.raises(AssertionError, match="non-finite"):
        C.judge_probes(E_, ref, slots)
    # a chain whose float32 realisation is not finite has no yardstick and is refused
    dev = ref.dev.copy()
    try:
        ref.dev[np.flatnonzero(ref.anti[:, 3])[0], 3] = np.nan
        with pytest.raises(AssertionError, match="no yardstick"):
            C.judge_probes(C.probes_from(d, ref, slots), ref, slots)
    finally:
        ref.dev[:] = dev
