"""GPU tests of the second Renyi entropy of arbitrary regions for the LSTM wave function (rnnwf_renyi2_regions_lstm:
csrc/lstm_renyi.hip, csrc/lstm_pauli_kernels.h PAIRED, observables_lstm; docs/renyi_lstm.md).

The device's log r is compared, every region on every pair, with the float64 brute force of tests/lstm_renyi_reference.py (both swapped
configurations scored from site 0 by tests/lstm_reference's NumPy LSTM) under the project's float64 bound 1e-11 N; the sums against
math.fsum of the device's own log r to relative 1e-12.  Everything else is an identity under np.array_equal (draws, repeats, shards,
passes, complements, duplicates, permutations, self pairs), an exact purity from the dense state vector, the agreement with the Pauli
pass on pairs that differ exactly on A, a refusal, or a five-sigma statement on 2^14 pairs.  tests/test_lstm_renyi_host.py shows on the
reference alone that the bound rejects six defects of the kernel's bookkeeping.  docs/renyi_lstm.md has the measured table.
"""
import re

import numpy as np
import pytest

import lstm_grad_reference as LG
import lstm_renyi_reference as Z
import renyi_stack_reference as S
from conftest import all_configs
from rnnwavefunctions_amd import observables as O
from rnnwavefunctions_amd import observables_lstm as OL
from rnnwavefunctions_amd import params as P

pytestmark = pytest.mark.gpu

SCOPE = Z.SCOPE
ENTRY = "rnnwf_renyi2_regions_lstm"
NPAIRS = Z.NPAIRS
BIG = 4379                       # 8758 chains: 547 full 16-chain blocks and a ragged one of 6


def handle(shape, units, prm=None):
    from rnnwavefunctions_amd import _lib
    wf = _lib.NativeWavefunction(_lib.MODEL_LSTM1D_F64, shape[0], shape[1], (units,))
    if prm is not None:
        wf.set_params(prm, scope=SCOPE)
    return wf


def call(wf, masks, npairs, **kw):
    return wf.renyi2_regions_lstm(masks, npairs, log_ratio=True, **kw)


# ---- 1. values ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape,units", Z.CASES, ids=["%dx%d-%d" % (s[0], s[1], u) for s, u in Z.CASES])
def test_log_ratios_against_float64(shape, units):
    Nx, Ny = shape
    N = Nx * Ny
    prm = Z.parameters(units)
    names, masks = Z.regions_of(Nx, Ny)
    assert any(m[0] for m in masks) and (N <= 33 or S.word_boundaries_covered(N, masks))
    s = Z.pairs_of(Nx, Ny, units)
    wf = handle(shape, units, prm)
    out = call(wf, masks, NPAIRS, samples=s)
    assert "samples" not in out and out["log_ratio"].shape == (len(masks), NPAIRS) and wf.resident_samples() == 0
    wf.close()
    label = "[LSTMRENYI %dx%d-%d NFULL %d]" % (Nx, Ny, units, LG.nfull(units))
    S.judge(label, out["log_ratio"], Z.log_ratio(prm, Nx, Ny, s, masks), None, True, N)
    rel = S.judge_sums(label, out["sums"], out["log_ratio"])
    print("%s sums: relative %.1e of the exactly rounded sums" % (label, rel))


def test_exact_purity_from_all_pairs_of_configurations():
    """3 x 2, 10 units: all 64 x 64 pairs as samples, weighted with P(sigma) P(tau) from the reference - Tr rho_A^2 of the dense vector to
    relative 1e-12, for a bulk interval, a two-piece region and a single site"""
    shape, units, N = (3, 2), 10, 6
    prm = Z.parameters(units)
    c = all_configs(N).astype(np.int32)
    lp = Z.log_p(prm, *shape)(c)
    i, j, pairs = S.all_pairs(c)
    masks = np.stack([S.mask_of(N, [2, 3]), S.mask_of(N, [1, 4]), S.mask_of(N, [5])])
    wf = handle(shape, units, prm)
    lr = call(wf, masks, len(i), samples=pairs)["log_ratio"]
    wf.close()
    purity = (np.exp(lp[i] + lp[j])[None, :] * np.exp(lr)).sum(axis=1)
    exact = np.array([S.purity_of_region(np.exp(0.5 * lp), N, m) for m in masks])
    print("[LSTMRENYI exact] Tr rho_A^2 = %s, device/exact - 1 = %s" % (exact, purity / exact - 1.0))
    assert -np.log(exact.min()) > 0.05 and np.abs(purity / exact - 1.0).max() <= 1e-12


def grid_regions(Nx, Ny):
    """17 regions on 4 x 3, none empty after normalisation: small_regions, the single sites 2..10 and a checkerboard"""
    N = Nx * Ny
    masks = [m for _, m in S.small_regions(Nx, Ny)] + [S.mask_of(N, [n]) for n in range(2, N - 1)] + [S.mask_of(N, range(1, N, 2))]
    return np.stack(masks)


@pytest.mark.parametrize("units", [37, 68])
def test_grid_stride_loop_on_the_8_wave_rows(units):
    """4 379 pairs x 17 regions = 17 x 548 = 9 316 tiles, more than the 8 waves per workgroup on each of 256 CUs: first, middle and last
    full blocks and the ragged block against brute force"""
    shape, N = (4, 3), 12
    prm = Z.parameters(units)
    masks = grid_regions(*shape)
    assert len(masks) == 17 and all(np.any(m != m[0]) for m in masks) and len({m.tobytes() for m in masks}) == 17
    wf = handle(shape, units, prm)
    wf.timing_enable(True)
    wf.timing_reset()
    out = call(wf, masks, BIG, seed=111, step=0)
    t = wf.timing_get(1)
    wf.close()
    assert t["launches"] == 1 and -(-2 * BIG // 16) * len(masks) == 9316
    idx = S.choose_pairs(BIG)
    S.check_subset(BIG, N, idx, masks)
    s = out["samples"].reshape(2 * BIG, N)
    ref = Z.log_ratio(prm, 4, 3, s, masks, pair_idx=idx)
    S.judge("[LSTMRENYI grid-stride 4x3-%d, %d of %d pairs]" % (units, len(idx), BIG), out["log_ratio"][:, idx], ref, None, True, N)
    S.judge_sums("grid-stride %d" % units, out["sums"], out["log_ratio"])


# ---- 2. identities -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape,units", [((3, 2), 10), ((7, 5), 21), ((3, 22), 68)], ids=["3x2-10", "7x5-21", "3x22-68"])
def test_bit_exact_identities(shape, units):
    Nx, Ny = shape
    N = Nx * Ny
    npairs = 300
    prm = Z.parameters(units)
    masks = Z.regions_of(Nx, Ny)[1]
    R = len(masks)
    wf = handle(shape, units, prm)
    # drawn samples are rnnwf_sample's at the same (seed, step, offset), and the call on them as supplied samples is the same call
    drawn = call(wf, masks, npairs, seed=5, step=3, pair_offset=7)
    s = wf.sample(2 * npairs, seed=5, step=3, sample_offset=14).reshape(2 * npairs, N)
    assert np.array_equal(drawn["samples"].reshape(2 * npairs, N), s)
    one, again = call(wf, masks, npairs, samples=s), call(wf, masks, npairs, samples=s)
    for k in ("sums", "log_ratio"):
        assert np.array_equal(one[k], drawn[k]) and np.array_equal(one[k], again[k]), k
    assert np.abs(one["log_ratio"]).max() > 0.1 and wf.resident_samples() == 0
    # (R, Nx, Ny) masks and (..., Nx, Ny) samples are the flat forms
    lat = call(wf, masks.reshape(R, Nx, Ny), npairs, samples=s.reshape(2 * npairs, Nx, Ny))
    assert np.array_equal(lat["log_ratio"], one["log_ratio"]) and np.array_equal(lat["sums"], one["sums"])
    # shards by pair_offset: bit-identical per pair, additive sums
    half = npairs // 2
    a, b = call(wf, masks, half, seed=5, step=3, pair_offset=7), call(wf, masks, npairs - half, seed=5, step=3, pair_offset=7 + half)
    assert np.array_equal(np.concatenate([a["log_ratio"], b["log_ratio"]], axis=1), one["log_ratio"])
    assert np.allclose(a["sums"] + b["sums"], one["sums"], rtol=1e-13, atol=0)
    # region and complement bit-equal; duplicates equal; a permuted list gives permuted rows; empty and full exactly 0
    comp = call(wf, 1 - masks, npairs, samples=s)
    assert np.array_equal(comp["log_ratio"], one["log_ratio"]) and np.array_equal(comp["sums"], one["sums"])
    perm = np.random.RandomState(1).permutation(R)
    ext = np.concatenate([masks[perm], masks[:2], np.zeros((1, N), dtype=np.int32), np.ones((1, N), dtype=np.int32)])
    e = call(wf, ext, npairs, samples=s)
    assert np.array_equal(e["log_ratio"][:R], one["log_ratio"][perm]) and np.array_equal(e["sums"][:R], one["sums"][perm])
    assert np.array_equal(e["log_ratio"][R:R + 2], one["log_ratio"][:2])
    assert np.all(e["log_ratio"][R + 2:] == 0.0) and np.all(e["sums"][R + 2:] == float(npairs))
    # self pairs: sigma = tau swaps nothing, and the mixed chain's terms are the chain's own bit for bit
    twin = np.repeat(s[0::2], 2, axis=0)
    self_lr = call(wf, masks, npairs, samples=twin)["log_ratio"]
    wf.close()
    assert np.all(self_lr == 0.0)


def test_several_passes_under_a_small_state_budget(monkeypatch):
    """RNNWF_STATE_BUDGET_MB=1 on 7 x 5 with 1 000 pairs: more than one pass; bit-equal per pair, the sums the per-pass sums in order"""
    shape, units, N, npairs = (7, 5), 21, 35, 1000
    prm = Z.parameters(units)
    masks = Z.regions_of(*shape)[1]
    R = len(masks)
    wf = handle(shape, units, prm)
    s = wf.sample(2 * npairs, seed=5, step=3).reshape(2 * npairs, N)
    one = call(wf, masks, npairs, samples=s)
    monkeypatch.setenv("RNNWF_STATE_BUDGET_MB", "1")
    many = handle(shape, units, prm)
    monkeypatch.delenv("RNNWF_STATE_BUDGET_MB")
    kt = 4 * LG.nfull(units) + 1                              # k-steps of a hidden vector: (h, c) rows of a checkpoint are 2 kt
    per_block = (N - 1) * 2 * kt * 64 * 8 + N * 16 * 8 + 16 * 8 + R * 16 * 8 + R * 8 * 8
    pairs_per_pass = max(1, (1 << 20) // per_block) * 8
    many.timing_enable(True)
    many.timing_reset()
    multi = call(many, masks, npairs, samples=s)
    passes = many.timing_get(1)["launches"]
    many.close()
    print("[LSTMRENYI passes] %d bytes per block: %d pairs per pass, %d passes" % (per_block, pairs_per_pass, passes))
    assert passes > 1 and passes == -(-npairs // pairs_per_pass)
    assert np.array_equal(multi["log_ratio"], one["log_ratio"])
    sums = np.zeros_like(one["sums"])
    for k in range(0, npairs, pairs_per_pass):
        part = s[2 * k:2 * (k + pairs_per_pass)]
        sums += call(wf, masks, len(part) // 2, samples=part)["sums"]
    wf.close()
    assert np.array_equal(multi["sums"], sums) and np.allclose(sums, one["sums"], rtol=1e-13, atol=0)


def test_work_counter_is_exact_and_tiny_lattices_run_every_subset():
    units = 10
    prm = Z.parameters(units)
    for shape in [(2, 1), (3, 1)]:
        N = shape[0] * shape[1]
        wf = handle(shape, units, prm)
        masks = np.array([[(k >> n) & 1 for n in range(N)] for k in range(2 ** N)], dtype=np.int32)
        s = wf.sample(2 * NPAIRS, seed=3, step=0).reshape(2 * NPAIRS, N)
        wf.timing_enable(True)
        wf.timing_reset()
        lr = call(wf, masks, NPAIRS, samples=s)["log_ratio"]
        t = wf.timing_get(1)
        wf.close()
        assert t["launches"] == 1
        steps = sum(N - int(np.flatnonzero(m ^ m[0])[0]) for m in masks if np.any(m != m[0]))
        assert t["cell_evals"] == 2 * NPAIRS * steps, (t["cell_evals"], steps)
        ref = Z.log_ratio(prm, shape[0], shape[1], s, masks)
        assert np.abs(lr - ref).max() <= Z.bound(N) and np.abs(ref).max() > 0.01
        assert np.all(lr[0] == 0.0) and np.all(lr[-1] == 0.0)
    # 1 x 1: every region is empty after normalisation - zeros, sums = npairs, no recurrent kernel
    wf = handle((1, 1), units, prm)
    wf.timing_enable(True)
    wf.timing_reset()
    both = np.array([[0], [1]], dtype=np.int32)
    given = call(wf, both, NPAIRS, samples=np.random.RandomState(3).randint(0, 2, (2 * NPAIRS, 1)).astype(np.int32))
    assert wf.timing_get(0)["launches"] == 0 and wf.timing_get(1)["launches"] == 0 and wf.timing_get(2)["launches"] == 1
    out = call(wf, both, NPAIRS, seed=3)                          # the draw is the only recurrent kernel
    assert wf.timing_get(1)["launches"] == 0 and wf.timing_get(1)["cell_evals"] == 0
    wf.close()
    for o in (given, out):
        assert np.all(o["log_ratio"] == 0.0) and o["log_ratio"].shape == (2, NPAIRS) and np.all(o["sums"] == float(NPAIRS))
    assert out["samples"].shape == (2 * NPAIRS, 1)


# ---- 3. consistency with the Pauli pass ----------------------------------------------------------------------------------------------

def test_pairs_that_differ_exactly_on_a_agree_with_the_pauli_pass():
    """7 x 5, 53 units.  tau = sigma with the sites of A flipped: the PAIRED tail of chain 2p under the region A is the computation of
    pauli_step_lstm's !PAIRED tail of that chain under the flip mask A, and likewise for 2p + 1, so log r = 1/2 (the sum of the two
    chains' Pauli log-ratios) within the bound.  (Both are 0 analytically - the swap exchanges the two chains - while each chain's
    log-ratio is of order 1: a wrong partner word or checkpoint leaves a term of that size.)"""
    shape, units, N = (7, 5), 53, 35
    prm = Z.parameters(units)
    masks = np.unique(Z.regions_of(*shape)[1], axis=0)
    masks = masks[masks[:, 0] == 0]                               # site 0 not in A: the region as given is the region the kernel runs
    R = len(masks)
    assert R >= 10 and {1, 32} <= {int(np.flatnonzero(m)[0]) for m in masks}
    sigma = np.random.RandomState(7).randint(0, 2, (R, NPAIRS, N)).astype(np.int32)
    pairs = np.empty((R, NPAIRS, 2, N), dtype=np.int32)
    pairs[:, :, 0], pairs[:, :, 1] = sigma, sigma ^ masks[:, None, :]
    chains = pairs.reshape(2 * R * NPAIRS, N)
    wf = handle(shape, units, prm)
    lr = call(wf, masks, R * NPAIRS, samples=chains)["log_ratio"]
    pauli = wf.pauli_step_lstm(masks, np.zeros_like(masks), np.ones(R), len(chains), samples=chains, want_log_ratio=True)["log_ratio"]
    wf.close()
    assert pauli.shape == (R, len(chains))                        # distinct masks, in order
    worst, size = 0.0, np.inf
    for k in range(R):
        cols = slice(k * NPAIRS, (k + 1) * NPAIRS)
        p = pauli[k, 2 * k * NPAIRS:2 * (k + 1) * NPAIRS]
        worst = max(worst, np.abs(lr[k, cols] - 0.5 * (p[0::2] + p[1::2])).max())
        size = min(size, np.abs(p).max())
    print("[LSTMRENYI vs Pauli 7x5-53] %d regions: max |log r - 1/2 sum| = %.2e = %.2e of the bound; smallest max |Pauli log r| %.2f"
          % (R, worst, worst / Z.bound(N), size))
    assert size > 0.1 and worst <= Z.bound(N)


# ---- 4. statistics -----------------------------------------------------------------------------------------------------------------

def test_entropies_and_mutual_information_within_five_standard_errors():
    shape, units, N, npairs = (3, 2), 10, 6, 1 << 14
    prm = Z.parameters(units)
    lp = Z.log_p(prm, *shape)(all_configs(N).astype(np.int32))
    psi = np.exp(0.5 * lp)
    exact_s2 = lambda m: -np.log(S.purity_of_region(psi, N, m))
    wf = handle(shape, units, prm)
    Sl, el = OL.renyi2_entropy(wf, npairs, seed=7, step=1)
    cuts = np.array([exact_s2(S.mask_of(N, range(l))) if 0 < l < N else 0.0 for l in range(N + 1)])
    print("[LSTMRENYI stat] S2(l) = %s +- %s, exact %s" % (np.round(Sl, 4), np.round(el, 4), np.round(cuts, 4)))
    assert Sl[0] == 0.0 and Sl[N] == 0.0 and el[0] == 0.0 and el[N] == 0.0
    assert np.all(el[1:N] > 0.0) and cuts[1:N].max() > 0.05 and np.all(np.abs(Sl - cuts) <= 5.0 * el)
    masks = Z.regions_of(*shape)[1]
    S2, err = OL.renyi2_regions(wf, masks, npairs, seed=7, step=1)
    want = np.array([exact_s2(m) for m in masks])
    assert np.all(err > 0.0) and np.all(np.abs(S2 - want) <= 5.0 * err)
    ma, mb = S.mask_of(N, [1, 2]), S.mask_of(N, [4, 5])
    exact = exact_s2(ma) + exact_s2(mb) - exact_s2(ma | mb)
    i2, e2 = OL.renyi2_mutual_information(wf, ma, mb, npairs, seed=7, step=1)
    wf.close()
    print("[LSTMRENYI stat] I2({1,2}:{4,5}) = %.4f +- %.4f, exact %.4f" % (i2, e2, exact))
    assert e2 > 0.0 and abs(i2 - exact) <= 5.0 * e2


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------

def test_refusals_happen_before_any_work():
    from rnnwavefunctions_amd import _lib
    shape, units, N = (3, 2), 10, 6
    prm = Z.parameters(units)
    masks = Z.regions_of(*shape)[1]
    wf = handle(shape, units, prm)
    bad = masks.copy()
    bad[1, 3] = 2
    for fn, word in [(lambda: wf.renyi2_regions_lstm(masks, 0), "npairs must be >= 1"),
                     (lambda: wf.renyi2_regions_lstm(masks, NPAIRS, pair_offset=-1), "pair_offset must be >= 0"),
                     (lambda: wf.renyi2_regions_lstm(bad, NPAIRS), r"regions\[1\]\[3\] = 2")]:
        with pytest.raises(ValueError, match=ENTRY + ": .*" + word):
            fn()
    # null pointers and nregions out of range through the C entry
    I32P, F64P = _lib._I32P, _lib._F64P
    reg = np.ascontiguousarray(masks, dtype=np.int32)
    sums = np.zeros((len(reg), 2))
    full = [reg.ctypes.data_as(I32P), len(reg), None, NPAIRS, 1, 0, 0, sums.ctypes.data_as(F64P), None, None]
    for idx, value, word in [(0, None, "regions and sums must be non-null"), (7, None, "regions and sums must be non-null"),
                             (1, 0, "nregions must be in 1.."), (1, -3, "nregions must be in 1..")]:
        a = list(full)
        a[idx] = value
        assert wf.lib.rnnwf_renyi2_regions_lstm(wf.h, *a) == -1
        msg = wf.lib.rnnwf_last_error(wf.h).decode()
        assert msg.startswith(ENTRY + ": ") and word in msg, msg
    assert wf.resident_samples() == 0
    # the five existing entries keep refusing the LSTM, in their present words
    for fn, words in [(lambda: wf.renyi2_swap(NPAIRS), "rnnwf_renyi2_swap: not implemented for the LSTM cell"),
                      (lambda: wf.renyi2_regions(masks, NPAIRS), "rnnwf_renyi2_regions: not implemented for the LSTM cell"),
                      (lambda: wf.renyi2_regions_stack(masks, NPAIRS), "rnnwf_renyi2_regions_stack: not implemented for the LSTM cell"),
                      (lambda: wf.renyi2_regions_2d(masks, NPAIRS),
                       r"rnnwf_renyi2_regions_2d: serves the 2D RNN \(MDRNN2D\) only, this handle's model is LSTM1D_F64"),
                      (lambda: wf.renyi2_regions_complex(masks, NPAIRS),
                       r"rnnwf_renyi2_regions_complex: serves the complex RNN \(CRNN_U1\) only, this handle's model is LSTM1D_F64")]:
        with pytest.raises(ValueError, match=words):
            fn()
    with pytest.raises(ValueError, match="LSTM"):
        O.renyi2_regions(wf, masks[0], NPAIRS)
    # a served call after all the refusals
    assert np.abs(call(wf, masks, NPAIRS, seed=1)["log_ratio"]).max() > 0.01
    wf.close()
    # parameters not committed: RNNWF_ERR_STATE
    raw = handle(shape, units)
    with pytest.raises(_lib.RnnwfError, match="parameters not committed") as e:
        raw.renyi2_regions_lstm(masks, NPAIRS)
    assert not isinstance(e.value, ValueError)
    raw.close()
    # every other model: RNNWF_ERR_INVALID by name, with the region entry that serves it; the module without a library call
    gprm = P.init_gru_params([10], seed=1)
    for model, nx, ny, un, p, name, entry in [
            (_lib.MODEL_GRU1D, N, 1, (10,), gprm, "GRU1D", "rnnwf_renyi2_regions serves the GRU models"),
            (_lib.MODEL_GRU1D_F64, 3, 2, (10,), P.init_gru_params([10], seed=1, dtype=np.float64), "GRU1D_F64",
             "rnnwf_renyi2_regions serves the GRU models"),
            (_lib.MODEL_GRU1D, N, 1, (10, 10), P.init_gru_params([10, 10], seed=1), "GRU1D", "rnnwf_renyi2_regions_stack serves stacked GRU layers"),
            (_lib.MODEL_GRU1D_PARITY, N, 1, (10,), gprm, "GRU1D_PARITY", "no region-Renyi pass serves the parity model"),
            (_lib.MODEL_CRNN_U1, N, 1, (10,), None, "CRNN_U1", "rnnwf_renyi2_regions_complex serves the complex RNN"),
            (_lib.MODEL_MDRNN2D, 3, 2, (10,), None, "MDRNN2D", "rnnwf_renyi2_regions_2d serves the 2D RNN")]:
        w = _lib.NativeWavefunction(model, nx, ny, un)
        if p is not None:
            w.set_params(p, scope=SCOPE)
        with pytest.raises(ValueError, match=ENTRY + ": serves the LSTM cell .* this handle's model is %s; %s" % (name, entry)):
            w.renyi2_regions_lstm(masks, NPAIRS)
        touched = []
        w.renyi2_regions_lstm = lambda *a, **k: touched.append(1)
        for fn in (lambda: OL.renyi2_regions(w, masks, NPAIRS), lambda: OL.renyi2_entropy(w, NPAIRS),
                   lambda: OL.renyi2_mutual_information(w, S.mask_of(N, [1]), S.mask_of(N, [4]), NPAIRS)):
            with pytest.raises(ValueError, match="observables_lstm serves the LSTM wave function"):
                fn()
        assert not touched
        w.close()
