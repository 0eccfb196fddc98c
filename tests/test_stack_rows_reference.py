"""The case table and the references of tests/test_gpu_stack_rows.py (tests/stack_rows_reference.py), validated on their own - no GPU:

1. the table reaches every stack row of csrc/shapes.h (27: 15 float32, 12 float64) with the waves per workgroup written there, both
   ends of every width class for each element type, two stacks of unequal widths per type; every case prints its MlSpill value,
   restated from csrc/layout.h, and the values that occur are 0 .. NL - 1 with partial spills (0 < spill < NL - 1) in both types;
2. the masks' and regions' first sites include 0 (Pauli only), 1, 31, 32, 33, one >= 35 short of the last, and N - 1;
3. on EVERY case, on chains drawn by oracle.philox + the oracle's sampler: the brute force equals the site-resolved form of the
   kernels (tail_form) to 1e-11 N in both passes, the judges' non-triviality conditions hold, and two honest float32 evaluations - the
   float32 stack in another summation order, and the float64 form restarted from states rounded through float32 - stay inside the
   float32 bound 16 x dev32 capped at 2 (2e-6 N + 2e-6) (a float32 case's seed is the first at which they stay below HALF of it);
4. every defect model is REFUSED by the case's bound, at one case per (element type, layer count), in both passes where it applies:
   renyi_stack_reference.DEFECTS and the two of stack_rows_reference.DEFECTS.  Not claimed, because void there: layer_image_swapped on
   two layers (one upper image: nothing to swap); own_on_A and partner_checkpoint in the Pauli pass (no partner).  tail_form's Renyi
   defects are renyi_stack_reference.stack_form's to 1e-10 (asserted on one case).

The module takes about 70 s on 8 CPU cores, nearly all of it NumPy GRU steps (31 cases x two passes x up to five evaluations).
"""
import os

import numpy as np
import pytest

import stack_rows_reference as W

S = W.S
SHAPES_H = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rnnwavefunctions_amd", "csrc", "shapes.h")


def test_the_table_reaches_every_stack_row_and_prints_every_spill_value():
    with open(SHAPES_H) as f:
        rows = W.shapes_h_stack_rows(f.read())
    assert len(rows) == 27 and sum(1 for r in rows if r[0] == "float") == 15 and sum(1 for r in rows if r[0] == "double") == 12
    equal = [c for c in W.CASES if len(set(c.units)) == 1]
    assert {(c.T, c.NL, c.NFULL): c.WAVES for c in equal} == rows and len(equal) == 27
    assert {k for k, w in rows.items() if w == 8} == set(W.ROW_WAVES)
    for c in W.CASES:
        assert c.shape[0] * c.shape[1] == W.N and (c.T, c.NL, c.NFULL) in rows and c.WAVES == rows[c.T, c.NL, c.NFULL]
        assert 16 * c.NFULL + 4 >= max(c.units) and (c.NFULL == 1 or max(c.units) > 16 * W.NFULLS[c.T][W.NFULLS[c.T].index(c.NFULL) - 1] + 4)
        assert c.spill == W.spill_of(c.T, c.NL, c.NFULL) and 0 <= c.spill <= c.NL - 1
        print(W.row_label(c) + (" (partial)" if 0 < c.spill < c.NL - 1 else ""))
    for T in ("float", "double"):
        mine = [c for c in W.CASES if c.T == T]
        # both ends of every width class, and over the layer counts
        for nf in W.NFULLS[T]:
            assert {W.GC.CLASS_WIDTHS[nf].index(c.units[0]) for c in mine if c.NFULL == nf and len(set(c.units)) == 1} == {0, 1}
        for NL in (2, 3, 4):
            ends = {W.GC.CLASS_WIDTHS[c.NFULL].index(c.units[0]) for c in mine if c.NL == NL and len(set(c.units)) == 1}
            assert ends == {0, 1}
            assert {0, NL - 1} <= {c.spill for c in mine if c.NL == NL}, (T, NL)         # nothing and everything out of LDS
        assert {c.spill for c in mine} == {0, 1, 2, 3}
        assert len([c for c in mine if len(set(c.units)) > 1]) == 2
        # partial spills: with three layers and with four, in both types; float32 (3, 3) has 8 waves
        assert {c.NL for c in mine if 0 < c.spill < c.NL - 1} == {3, 4}
    assert W.case_of(False, 3, 3).spill == 1 and W.case_of(False, 3, 3).WAVES == 8
    # layout.h's own words: three float32 layers of 50 units leave the top image out (171 KB); at 100 units every upper image is out
    assert W.spill_of("float", 3, 3) == 1 and all(W.spill_of("float", NL, 6) == NL - 1 for NL in (2, 3, 4))
    assert 240e3 < W.upper_layout_bytes(4, 6) < 250e3 and W.gru_layout_bytes(4, 6) <= W.LDS and W.gru_layout_bytes(8, 4) <= W.LDS
    assert W.upper_layout_bytes(4, 3) == 67392 and 170e3 < W.gru_layout_bytes(4, 3) + 2 * W.upper_layout_bytes(4, 3) < 172e3


def test_first_sites_of_the_masks_and_regions():
    ham = W.hamiltonian()
    masks = W.flip_masks(ham)
    firsts = set(W.first_sites(masks, False))
    assert {0, 1, 31, 32, 33, W.N - 1} <= firsts and any(35 <= f < W.N - 1 for f in firsts)
    as_sites = [tuple(np.flatnonzero(m)) for m in masks]
    assert (35, 38) in as_sites and (32,) in as_sites and (33, 37) in as_sites and any(m.all() for m in masks)
    for f64 in (False, True):
        names, reg = W.regions(W.SHAPE[f64])
        firsts = set(W.first_sites(reg, True))
        assert {1, 31, 32, 33, W.N - 1} <= firsts and any(35 <= f < W.N - 1 for f in firsts) and 0 not in firsts
        assert S.word_boundaries_covered(W.N, reg) and any(m[0] for m in reg) and len(names) == len(reg)


@pytest.fixture(scope="module")
def refs():
    """per case, once: weights, oracle-drawn chains, operators, the float64 brute force of both passes and the float32 bounds"""
    cache = {}

    def get(c):
        if c not in cache:
            prm = W.weights(c)
            chains = W.oracle_chains(c, prm)
            masks = W.flip_masks(W.hamiltonian())
            names, reg = W.regions(c.shape)
            lp64 = W.scorer(prm)
            d = dict(prm=prm, chains=chains, masks=masks, reg=reg, names=names)
            d["pauli"] = dict(paired=False, x=chains[:W.NS], m=masks, ref=W.pauli_log_ratio(lp64, chains[:W.NS], masks), brute=W.pauli_log_ratio)
            d["renyi"] = dict(paired=True, x=chains, m=reg, ref=W.renyi_log_ratio(lp64, chains, reg), brute=W.renyi_log_ratio)
            lp32 = W.scorer(prm, np.float32)
            for p in (d["pauli"], d["renyi"]):
                p["dev32"] = float(np.abs(p["brute"](lp32, p["x"], p["m"]) - p["ref"]).max())
                p["b32"] = S.f32_bound(p["dev32"], W.N)[0]
                p["bound"] = S.f64_bound(W.N) if c.f64 else p["b32"]
            cache[c] = d
        return cache[c]
    return get


@pytest.mark.parametrize("c", W.CASES, ids=W.case_id)
def test_every_case_brute_force_site_form_and_honest_float32(c, refs):
    d = refs(c)
    assert d["chains"].shape == (2 * W.NPAIRS, W.N) and np.any(d["chains"][0::2, 32:] != d["chains"][1::2, 32:])
    sp = W.spread(d["pauli"]["ref"])
    mx, share = S.nontrivial(d["renyi"]["ref"])
    print("%s seed %d: ratios std/mean %.2f, log r in [%.1f, %.1f]; Renyi max |log r| %.2f, %.0f %% above 0.01"
          % (W.row_label(c), c.seed, sp, d["pauli"]["ref"].min(), d["pauli"]["ref"].max(), mx, 100 * share))
    assert sp > 0.2 and mx > 0.1 and share >= 0.25
    for name in ("pauli", "renyi"):
        p = d[name]
        form = W.tail_form(d["prm"], p["x"], p["m"], p["paired"])
        assert np.abs(form - p["ref"]).max() <= S.f64_bound(W.N), name
        # honest float32 evaluations against the float32 bound (of a float64 case too: the bound is the reference's own)
        other = p["brute"](W.other_order_scorer(d["prm"]), p["x"], p["m"])
        rounded = W.tail_form(d["prm"], p["x"], p["m"], p["paired"], round_restart=True)
        a, b = float(np.abs(other - p["ref"]).max()), float(np.abs(rounded - p["ref"]).max())
        print("  %s: dev32 %.2e, float32 bound %.2e; other summation order %.2f, float32-rounded restart %.3f of it" % (name, p["dev32"], p["b32"], a / p["b32"], b / p["b32"]))
        assert a <= p["b32"] and b <= p["b32"], name
        assert b > S.f64_bound(W.N)                                   # ... and the rounding is seen: not the float64 form again


DEFECT_CASES = [W.case_of(f64, NL, 3) for f64 in (False, True) for NL in (2, 3, 4)]
VOID = {(NL, "layer_image_swapped", name) for NL in (2,) for name in ("pauli", "renyi")}


@pytest.mark.parametrize("defect", sorted(W.DEFECTS))
@pytest.mark.parametrize("c", DEFECT_CASES, ids=W.case_id)
def test_every_defect_is_refused_by_the_bounds(c, defect, refs):
    d = refs(c)
    assert len(set(c.units)) == 1
    for name in ("pauli", "renyi"):
        if name == "pauli" and defect not in W.PAULI_DEFECTS:
            continue
        p = d[name]
        if (c.NL, defect, name) in VOID:
            with pytest.raises(AssertionError, match="nothing to swap"):
                W.tail_form(d["prm"], p["x"], p["m"], p["paired"], defect=defect)
            print("%s %s %s: void here, not claimed" % (W.case_id(c), name, defect))
            continue
        err = float(np.abs(W.tail_form(d["prm"], p["x"], p["m"], p["paired"], defect=defect) - p["ref"]).max())
        print("%s %s: %s: max |d log r| = %.3e = %.3g x the case's bound (%.3g x float64, %.3g x float32)"
              % (W.case_id(c), name, W.DEFECTS[defect], err, err / p["bound"], err / S.f64_bound(W.N), err / p["b32"]))
        assert err > 10.0 * p["bound"]


def test_the_renyi_defects_are_those_of_renyi_stack_reference(refs):
    c = W.case_of(False, 3, 3)
    d = refs(c)
    for defect in [None] + sorted(S.DEFECTS):
        mine, theirs = W.tail_form(d["prm"], d["chains"], d["reg"], True, defect=defect), S.stack_form(d["prm"], d["chains"], d["reg"], defect=defect)
        assert np.allclose(mine, theirs, rtol=1e-10, atol=1e-10), defect                                 # other batch sizes: not to the bit
