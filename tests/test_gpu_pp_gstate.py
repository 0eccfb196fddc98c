"""The one-layer ping-pong flip kernel (37..50 units) carries its state as g = (h + 1) / 2 and reads the g-state form of the bf16x3
image (csrc/split_pp.h: SplitPP<.., GSTATE>; csrc/pack_split.h: gstate_word): every weight that multiplies the state doubled, every
constant such a row starts from less the row's weight sum.  Not bit-identical to the h form: the claim is float32 equivalence at the
suite's own yardstick.

CPU half (no GPU): rnnwf_host_split_images packs both forms at 37 and 50 units; NumPy decodes them (three bf16 parts per weight, the
accumulator start table, the VALU head's tables) and applies them in float64 to random h and to g = (h + 1) / 2.  All pre-activations
of r, u, q, the lagged head rows and the VALU head's logit agree to 1e-6 (the fold's one float32 rounding of a constant of size <= 8);
the input-side table is equal bit for bit, every part is doubled exactly, and a padded unit's rows, columns and constants are zero.

GPU half: every row of tfim_eloc's log-probability queue against float64 from site 0 (oracle.estimators.ising_local_energies on
oracle.models.prnn_log_probability), bound = 16 x the float32 restatement's own deviation on the same inputs
(flip_rows_reference.Reference / judge, as tests/test_gpu_pp_fragment_order.py), engine pinned to bf16x3, kernels x 3:
  widths 37, 38, 44, 49, 50 (both parities, 13 .. 0 padded units; the class has ONE kernel row, <NF32, RJ> = <1, 9>) on 33 sites,
      40 samples (one spin word; a full 32-chain tile and a ragged one of 8);
  widths 37 and 50 on 65 sites, 33 samples (three spin words; a full tile and a ragged one of 1);
  width 49, row 0 of the queue against log_prob - a padded unit that leaked into the head or a gate would show on every row, row 0
      is the base pass's, untouched: the two must still agree within the row bound (asserted by judge in every case; named here);
  width 50, kernels x 0.01 and zero biases: |h| <~ 1e-3 in every checkpoint, so g = 0.5 + h / 2 rounds h to 2^-25 absolute where
      the tile begins.  The yardstick has its floor at one float32 rounding of the value itself, the same bound.
Measured on an MI355X (profiles/pp_gstate.txt), worst row deviation / bound, this kernel | the parent's h form on the same inputs:
  33 sites: w37 0.263 | 0.078, w38 0.174 | 0.143, w44 0.089 | 0.065, w49 0.141 | 0.081, w50 0.116 | 0.081;
  65 sites: w37 0.235 | 0.094, w50 0.257 | 0.109;   tiny 0.027 | 0.024;
  E_loc <= 0.022 of its bound and row 0 = log_prob to 0.000 everywhere.  Under 1 throughout, but up to 3.4 x the h form's: a finding,
  reported in that file, not tuned away.  The GPU half takes 3 s, the CPU half 8 s (most of it the library's load).
"""
import ctypes as C

import numpy as np
import pytest

import flip_rows_reference as F

PIN = {"RNNWF_ENGINE": "bf16x3"}
SCOPE = F.SCOPE


# ---- CPU half -------------------------------------------------------------------------------------------------------------------------

def _bf16(a):
    return (a.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def _images(units, prm):
    from rnnwavefunctions_amd import _lib
    lib = _lib.load_library()
    flat = np.concatenate([np.asarray(prm[k], dtype=np.float64).ravel() for k in sorted(prm, key=lambda s: s.encode())])
    cap = 1 << 18
    ih, ig = np.zeros(cap, dtype=np.uint8), np.zeros(cap, dtype=np.uint8)
    lay = np.zeros(10, dtype=np.int32)
    rc = lib.rnnwf_host_split_images(units, flat.ctypes.data_as(C.POINTER(C.c_double)), flat.size, ih.ctypes.data, ig.ctypes.data, cap,
                                     lay.ctypes.data_as(C.POINTER(C.c_int32)))
    assert rc == 0, lib.rnnwf_last_error(None).decode()
    names = ("NT", "NQ", "NUP", "NOUT", "OFF_ASP", "OFF_CI", "OFF_XC", "OFF_WD", "OFF_BD", "BYTES")
    L = dict(zip(names, (int(v) for v in lay)))
    return ih[:L["BYTES"]].copy(), ig[:L["BYTES"]].copy(), L


def _decode(img, L):
    """W (NT, 32 rows, 2 K halves, NU entries) float64 and its three parts, CI (2, NT, 32 rows), XC, WD (2, NUP), BD"""
    NT, NQ, NUP = L["NT"], L["NQ"], L["NUP"]
    NU = 8 * NQ + 1
    A = _bf16(img[:L["OFF_ASP"]].view(np.uint16).reshape(NT, 3, NQ, 64, 8))
    SP = _bf16(img[L["OFF_ASP"]:L["OFF_CI"]].view(np.uint16).reshape(NT, 64, 8))
    assert np.array_equal(SP[..., 0], SP[..., 1]) and np.array_equal(SP[..., 0], SP[..., 2]) and np.array_equal(SP[..., 3], SP[..., 4])
    assert not SP[..., 6:].any()
    parts = np.zeros((3, NT, 32, 2, NU))
    for hhk in range(2):
        lanes = slice(32 * hhk, 32 * hhk + 32)
        for a in range(3):
            parts[a, :, :, hhk, :NU - 1] = A[:, a, :, lanes, :].transpose(0, 2, 1, 3).reshape(NT, 32, 8 * NQ)
            parts[a, :, :, hhk, NU - 1] = SP[:, lanes, (0, 3, 5)[a]]
    ci = img[L["OFF_CI"]:L["OFF_XC"]].view(np.float32).astype(np.float64).reshape(2, NT, 2, 16)
    r32 = np.arange(32)
    CI = ci[:, :, (r32 >> 2) & 1, (r32 & 3) + 4 * (r32 >> 3)]
    XC = img[L["OFF_XC"]:L["OFF_WD"]].view(np.uint32)
    WD = img[L["OFF_WD"]:L["OFF_BD"]].view(np.float32).astype(np.float64).reshape(2, NUP)
    BD = float(img[L["OFF_BD"]:L["OFF_BD"] + 4].view(np.float32)[0])
    return parts.sum(axis=0), parts, CI, XC, WD, BD


@pytest.mark.parametrize("units", [37, 50])
def test_both_image_forms_give_the_same_preactivations(units):
    import sampler_reference as R
    prm = R.build_params("gru", (units,), seed=F.SEED, sharp=1.0)          # glorot kernels, random biases
    ih, ig, L = _images(units, prm)
    Wh, Ph, CIh, XCh, WDh, BDh = _decode(ih, L)
    Wg, Pg, CIg, XCg, WDg, BDg = _decode(ig, L)
    NU = Wh.shape[-1]
    assert np.array_equal(Pg, 2.0 * Ph), "a weight part is not exactly doubled"
    assert np.array_equal(WDg, 2.0 * WDh) and np.array_equal(XCg, XCh)
    assert np.abs(Wh).max() > 0.1 and np.abs(CIh).max() > 0.1 and np.abs(WDh).max() > 0.01
    # rows and K entries in use: 3 x units gate rows + the head row (both lane halves of a tile hold it); units K entries
    used_rows = np.abs(Wh).sum(axis=(2, 3)) > 0
    used_k = np.abs(Wh).sum(axis=(0, 1)) > 0
    assert int(used_k.sum()) == units and int(used_rows.sum()) == 3 * units + 2, (int(used_k.sum()), int(used_rows.sum()))
    assert not CIh[:, ~used_rows].any() and not CIg[:, ~used_rows].any(), "a padded row's constant is not zero"
    assert not WDh[:, :NU][~used_k].any() and not WDg[:, :NU][~used_k].any() and not WDg[:, NU:].any()
    rng = np.random.RandomState(units)
    worst = 0.0
    for trial in range(8):
        h = rng.uniform(-1.0, 1.0, (2, NU)) * (1.0 if trial < 6 else 1e-3)
        g = 0.5 * (h + 1.0)
        for sgm in range(2):
            pre_h = CIh[sgm] + np.einsum("trke,ke->tr", Wh, h)
            pre_g = CIg[sgm] + np.einsum("trke,ke->tr", Wg, g)
            worst = max(worst, float(np.abs(pre_h - pre_g).max()))
        z_h = BDh + (WDh[:, :NU] * h).sum()
        z_g = BDg + (WDg[:, :NU] * g).sum()
        worst = max(worst, abs(z_h - z_g))
    print("[g-state images, %d units] max |pre(h form, h) - pre(g form, (h + 1) / 2)| = %.2e, max |constant| %.2f" %
          (units, worst, max(np.abs(CIg).max(), abs(BDg))))
    assert worst <= 1e-6


# ---- GPU half -------------------------------------------------------------------------------------------------------------------------

CASES = [("w37", 37, 33, 40), ("w38", 38, 33, 40), ("w44", 44, 33, 40), ("w49", 49, 33, 40), ("w50", 50, 33, 40),
         ("w37-n65", 37, 65, 33), ("w50-n65", 50, 65, 33)]
_RESULTS = {}


def _run(cid, units, N, ns, prm, monkeypatch):
    """(lp, e, ref, log_prob) of the case, computed once per module; the reference's float64 queue is the from-site-0 oracle's"""
    if cid not in _RESULTS:
        from test_gpu_sampler_full import make_wf
        wf = make_wf("gru", (N, 1), (units,), prm, monkeypatch, PIN)
        s = wf.sample(ns, seed=F.SEED, step=0).reshape(ns, N)
        Jz = F.couplings(N)
        lp = np.full((N + 1) * ns, np.nan)
        e = wf.tfim_eloc(s, Jz, F.BX, log_probs=lp)
        assert wf.engine_name() == "bf16x3", "%s ran on %s" % (cid, wf.engine_name())
        ref = F.Reference("gru", prm, s, Jz, F.BX, None, np.arange(ns), ns, 32)
        e0, lp0 = F.oracle_reference("gru", prm, s, Jz)
        assert np.abs(lp0 - ref.lp64).max() <= 1e-9 * max(1.0, np.abs(lp0).max())      # the shared-prefix queue IS the oracle's
        ref.lp64, ref.e64 = lp0, e0
        _RESULTS[cid] = (lp.reshape(N + 1, ns), e, ref, wf.log_prob(s))
    return _RESULTS[cid]


@pytest.mark.gpu
@pytest.mark.parametrize("cid,units,N,ns", CASES, ids=[c[0] for c in CASES])
def test_queue_rows_against_float64(cid, units, N, ns, monkeypatch):
    lp, e, ref, log_prob = _run(cid, units, N, ns, F.build_params("gru", (units,)), monkeypatch)
    label = "[pp g-state, %s]" % cid
    print(F.line(label, F.measure(lp, e, ref, log_prob), ref.seconds))     # the figures first, so that a failing case still prints them
    F.judge(lp, e, ref, log_prob, None, label)


@pytest.mark.gpu
def test_padded_units_do_not_leak_into_row_0(monkeypatch):
    cid, units, N, ns = CASES[3]
    lp, e, ref, log_prob = _run(cid, units, N, ns, F.build_params("gru", (units,)), monkeypatch)
    over = np.abs(lp[0] - log_prob) / ref.bound
    print("[pp g-state, %s] row 0 vs log_prob / bound %.3f" % (cid, over.max()))
    assert np.all(over <= 1.0)
    # and the last flipped site's row, one step of the flip kernel behind a checkpoint, against float64
    assert np.all(np.abs(lp[N - 1] - ref.lp64[N - 1]) <= ref.bound)


@pytest.mark.gpu
def test_tiny_checkpoints(monkeypatch):
    from rnnwavefunctions_amd import params as P
    units, N, ns = 50, 33, 40
    prm = P.scale_kernels(P.init_gru_params([units], seed=F.SEED), 0.01)
    lp, e, ref, log_prob = _run("tiny", units, N, ns, prm, monkeypatch)
    m = F.measure(lp, e, ref, log_prob)
    print(F.line("[pp g-state, tiny checkpoints]", m, ref.seconds))
    assert m["finite"] and np.all(np.isfinite(ref.y))
    assert m["row_over"] <= 1.0 and m["e_over"] <= 1.0 and m["row0_over"] <= 1.0, m
