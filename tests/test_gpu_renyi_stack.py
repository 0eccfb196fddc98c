"""GPU tests of the second Renyi entropy of arbitrary regions for STACKED GRU layers (rnnwf_renyi2_regions_stack:
csrc/renyi_stack.hip, csrc/stack_chain_kernels.h PAIRED; docs/renyi_stack.md).

The device's log r is compared, every region on every pair, with the float64 brute force of tests/renyi_stack_reference.py (both
swapped configurations scored from site 0 by the oracle's stacked GRU) on caller-supplied samples drawn with `sample`; the bounds are
tests/renyi_reference.py's: float64 1e-11 N, float32 16 x the float32 NumPy oracle's deviation from float64 on the same pairs and
regions (computed here), capped at 2 (2e-6 N + 2e-6); the sums against math.fsum of the device's own log r to relative 1e-12.
Everything else is an identity under np.array_equal (draws, repeats, shards, passes, complements, duplicates, permutations), an exact
purity from the dense state vector, a refusal, or a five-sigma statement on 2^14 pairs.  docs/renyi_stack.md has the measured table.
"""
import re

import numpy as np
import pytest

import renyi_stack_reference as S
from conftest import all_configs
from oracle import models as M
from rnnwavefunctions_amd import observables as O
from rnnwavefunctions_amd import observables_stack as OS
from rnnwavefunctions_amd import training as T

pytestmark = pytest.mark.gpu

SCOPE = S.SCOPE
ENTRY = "rnnwf_renyi2_regions_stack"
NPAIRS = 19                      # 38 chains: two full 16-chain blocks and a ragged one
BIG = 2003                       # 4006 chains: 250 full blocks and a ragged one
# weight seeds chosen on the CPU from the reference alone (oracle-drawn chains), so that the case is not trivial: 111 unless listed
WSEED = {(100, 100): 113, (37, 20): 112, (10, 20): 112}


def make_wf(f64, shape, units, prm):
    from rnnwavefunctions_amd import _lib
    wf = _lib.NativeWavefunction(_lib.MODEL_GRU1D_F64 if f64 else _lib.MODEL_GRU1D, shape[0], shape[1], tuple(units))
    wf.set_params(prm, scope=SCOPE)
    return wf


def weights(f64, units):
    return S.weights(f64, units, seed=WSEED.get(tuple(units), 111))


def regions_of(shape, kind):
    N = shape[0] * shape[1]
    names, masks = zip(*(S.boundary_regions(N) if kind == "boundary" else S.small_regions(*shape)))
    return list(names), np.stack(masks)


# (float64, lattice, units, pairs, region set)
SMALL = [(False, (6, 1), u, NPAIRS, "small") for u in [(10, 10), (10, 10, 10), (10, 10, 10, 10), (36, 36), (50, 50), (68, 68), (100, 100),
                                                       (10, 20), (37, 20)]] + \
        [(True, (3, 2), u, NPAIRS, "small") for u in [(10, 10), (10, 10, 10, 10), (36, 36), (52, 52), (68, 68)]]
BOUNDARY = [(False, (34, 1), (10, 10), NPAIRS, "boundary"), (True, (17, 2), (10, 10), NPAIRS, "boundary")]
MULTI = [(False, (34, 1), (10, 10), BIG, "boundary")]


def case_id(c):
    return "%s-%dx%d-%s-np%d" % ("f64" if c[0] else "f32", c[1][0], c[1][1], "x".join(str(u) for u in c[2]), c[3])


@pytest.mark.parametrize("case", SMALL + BOUNDARY + MULTI, ids=case_id)
def test_log_ratios_against_float64(case):
    f64, shape, units, npairs, kind = case
    N = shape[0] * shape[1]
    prm = weights(f64, units)
    wf = make_wf(f64, shape, units, prm)
    names, masks = regions_of(shape, kind)
    if kind == "boundary":
        assert S.word_boundaries_covered(N, masks) and any(m[0] for m in masks)
    s = wf.sample(2 * npairs, seed=111, step=0).reshape(2 * npairs, N)
    out = wf.renyi2_regions_stack(masks, npairs, samples=s, log_ratio=True)
    assert "samples" not in out and out["log_ratio"].shape == (len(masks), npairs) and wf.resident_samples() == 0
    idx = np.arange(npairs)
    if npairs == BIG:
        idx = S.choose_pairs(npairs)
        S.check_subset(npairs, N, idx, masks)
    ref = S.log_ratio(prm, s, masks, pair_idx=idx)
    ref32 = None if f64 else S.log_ratio(prm, s, masks, dtype=np.float32, pair_idx=idx)
    S.judge("[%s]" % case_id(case), out["log_ratio"][:, idx], ref, ref32, f64, N)
    rel = S.judge_sums(case_id(case), out["sums"], out["log_ratio"])
    print("[%s] sums: relative %.1e of the exactly rounded sums" % (case_id(case), rel))


def test_exact_purity_from_all_pairs_of_configurations():
    """N = 6, two float64 layers of 10 units: all 64 x 64 pairs as samples, weighted with P(sigma) P(tau) from the reference - Tr rho_A^2
    of the dense vector to relative 1e-12"""
    units, shape, N = (10, 10), (6, 1), 6
    prm = weights(True, units)
    wf = make_wf(True, shape, units, prm)
    c = all_configs(N).astype(np.int32)
    lp = M.prnn_log_probability(prm, c, dtype=np.float64)
    i, j, pairs = S.all_pairs(c)
    masks = np.stack([S.mask_of(N, [2, 3]), S.mask_of(N, [1, 4]), S.mask_of(N, [5])])
    lr = wf.renyi2_regions_stack(masks, len(i), samples=pairs, log_ratio=True)["log_ratio"]
    purity = (np.exp(lp[i] + lp[j])[None, :] * np.exp(lr)).sum(axis=1)
    exact = np.array([S.purity_of_region(np.exp(0.5 * lp), N, m) for m in masks])
    print("[exact] Tr rho_A^2 = %s, device/exact - 1 = %s" % (exact, purity / exact - 1.0))
    assert -np.log(exact.min()) > 0.05 and np.abs(purity / exact - 1.0).max() <= 1e-12


@pytest.mark.parametrize("f64,shape,units", [(True, (3, 2), (10, 10)), (False, (34, 1), (10, 10)), (False, (10, 1), (68, 68))],
                         ids=["f64-3x2-10x10", "f32-34-10x10", "f32-10-68x68"])
def test_bit_exact_identities(f64, shape, units, monkeypatch):
    N = shape[0] * shape[1]
    npairs = 300
    prm = weights(f64, units)
    names, masks = regions_of(shape, "boundary" if N > 33 else "small")
    if N == 10:
        masks = np.stack([S.mask_of(N, range(3, 6)), S.mask_of(N, [1, 8]), S.mask_of(N, [9]), S.mask_of(N, [0, 7, 8])])
    R = len(masks)
    wf = make_wf(f64, shape, units, prm)
    call = lambda w, m, n, **k: w.renyi2_regions_stack(m, n, log_ratio=True, **k)
    # drawn samples are rnnwf_sample's at the same (seed, step, offset), and the call on them as supplied samples is the same call
    drawn = call(wf, masks, npairs, seed=5, step=3, pair_offset=7)
    s = wf.sample(2 * npairs, seed=5, step=3, sample_offset=14).reshape(2 * npairs, N)
    assert np.array_equal(drawn["samples"].reshape(2 * npairs, N), s)
    one, again = call(wf, masks, npairs, samples=s), call(wf, masks, npairs, samples=s)
    for k in ("sums", "log_ratio"):
        assert np.array_equal(one[k], drawn[k]) and np.array_equal(one[k], again[k]), k
    assert np.abs(one["log_ratio"]).max() > 0.1 and wf.resident_samples() == 0
    # shards by pair_offset: bit-identical per pair, additive sums
    half = npairs // 2
    a, b = call(wf, masks, half, seed=5, step=3, pair_offset=7), call(wf, masks, npairs - half, seed=5, step=3, pair_offset=7 + half)
    assert np.array_equal(np.concatenate([a["log_ratio"], b["log_ratio"]], axis=1), one["log_ratio"])
    assert np.allclose(a["sums"] + b["sums"], one["sums"], rtol=1e-13, atol=0)
    # several passes under a small state budget: bit-equal per pair, the sums the per-pass sums added in order
    monkeypatch.setenv("RNNWF_STATE_BUDGET_MB", "1")
    many = make_wf(f64, shape, units, prm)
    monkeypatch.delenv("RNNWF_STATE_BUDGET_MB")
    kt = 4 * next(nf for nf in (1, 2, 3, 4, 6) if 16 * nf + 4 >= max(units)) + 1          # k-steps of a hidden vector: 4 NFULL + 1
    per_block = N * len(units) * kt * 64 * (8 if f64 else 4) + N * 16 * 8 + R * 16 * 8 + R * 8 * 8
    pairs_per_pass = max(1, (1 << 20) // per_block) * 8
    print("[passes %s] %d bytes per block: %d pairs per pass, %d passes" % (units, per_block, pairs_per_pass, -(-npairs // pairs_per_pass)))
    assert pairs_per_pass < npairs
    multi = call(many, masks, npairs, samples=s)
    assert np.array_equal(multi["log_ratio"], one["log_ratio"])
    sums = np.zeros_like(one["sums"])
    for k in range(0, npairs, pairs_per_pass):
        part = s[2 * k:2 * (k + pairs_per_pass)]
        sums += call(wf, masks, len(part) // 2, samples=part)["sums"]
    assert np.array_equal(multi["sums"], sums) and np.allclose(sums, one["sums"], rtol=1e-13, atol=0)
    # region and complement bit-equal; duplicates equal; a permuted list gives permuted rows; empty and full exactly 0
    comp = call(wf, 1 - masks, npairs, samples=s)
    assert np.array_equal(comp["log_ratio"], one["log_ratio"]) and np.array_equal(comp["sums"], one["sums"])
    perm = np.random.RandomState(1).permutation(R)
    ext = np.concatenate([masks[perm], masks[:2], np.zeros((1, N), dtype=np.int32), np.ones((1, N), dtype=np.int32)])
    e = call(wf, ext, npairs, samples=s)
    assert np.array_equal(e["log_ratio"][:R], one["log_ratio"][perm]) and np.array_equal(e["sums"][:R], one["sums"][perm])
    assert np.array_equal(e["log_ratio"][R:R + 2], one["log_ratio"][:2])
    assert np.all(e["log_ratio"][R + 2:] == 0.0) and np.all(e["sums"][R + 2:] == float(npairs))
    # self pairs: sigma = tau swaps nothing
    twin = np.repeat(s[0::2], 2, axis=0)
    self_lr = call(wf, masks, npairs, samples=twin)["log_ratio"]
    print("[self pairs %s] max |log r| = %.2e" % (units, np.abs(self_lr).max()))
    assert np.abs(self_lr).max() <= (1e-11 * N if f64 else 2e-6 * N)


def test_work_counter_is_exact_and_tiny_lattices_run_every_subset():
    for f64, shape in [(False, (2, 1)), (False, (3, 1)), (True, (2, 1)), (True, (3, 1))]:
        N = shape[0] * shape[1]
        units = (10, 10)
        prm = weights(f64, units)
        wf = make_wf(f64, shape, units, prm)
        masks = np.array([[(k >> n) & 1 for n in range(N)] for k in range(2 ** N)], dtype=np.int32)
        s = wf.sample(2 * NPAIRS, seed=3, step=0).reshape(2 * NPAIRS, N)
        wf.timing_enable(True)
        wf.timing_reset()
        lr = wf.renyi2_regions_stack(masks, NPAIRS, samples=s, log_ratio=True)["log_ratio"]
        t = wf.timing_get(1)
        work = t["cell_evals"]
        assert t["launches"] == 1
        steps = sum(N - int(np.flatnonzero(m ^ m[0])[0]) for m in masks if np.any(m != m[0]))
        assert work == 2 * NPAIRS * steps, (work, steps)
        ref = S.log_ratio(prm, s, masks)
        tol = S.f64_bound(N) if f64 else S.f32_bound(float(np.abs(S.log_ratio(prm, s, masks, dtype=np.float32) - ref).max()), N)[0]
        assert np.abs(lr - ref).max() <= tol and np.all(lr[0] == 0.0) and np.all(lr[-1] == 0.0)


def test_refusals_happen_before_any_work_and_leave_the_batch_usable():
    from rnnwavefunctions_amd import _lib
    N, units = 6, (10, 10)
    prm = weights(False, units)
    wf = make_wf(False, (N, 1), units, prm)
    masks = regions_of((N, 1), "small")[1]
    ham = O.xxz_hamiltonian(N, -1.0, 0.5)
    ns = 37
    m = wf.pauli_step_stack(ham.flip, ham.sign, ham.coeff, ns, seed=1, step=2)["moments"]     # leaves its batch resident
    g0 = T.cost_gradient(wf, prm, SCOPE, m[0] / m[2], m[2])

    def untouched():
        g1 = T.cost_gradient(wf, prm, SCOPE, m[0] / m[2], m[2])
        return wf.resident_samples() == ns and all(np.array_equal(g0[k], g1[k]) for k in g0)
    bad = masks.copy()
    bad[1, 3] = 2
    for call, word in [(lambda: wf.renyi2_regions_stack(masks, 0), "npairs must be"),
                       (lambda: wf.renyi2_regions_stack(masks, NPAIRS, pair_offset=-1), "pair_offset"),
                       (lambda: wf.renyi2_regions_stack(bad, NPAIRS), r"regions\[1\]\[3\] = 2")]:
        with pytest.raises(ValueError, match=ENTRY + ": .*" + word):
            call()
        assert untouched()
    # null pointers and nregions out of range through the C entry
    I32P, F64P = _lib._I32P, _lib._F64P
    reg = np.ascontiguousarray(masks, dtype=np.int32)
    sums = np.zeros((len(reg), 2))
    full = [reg.ctypes.data_as(I32P), len(reg), None, NPAIRS, 1, 0, 0, sums.ctypes.data_as(F64P), None, None]
    for idx, value, word in [(0, None, "non-null"), (7, None, "non-null"), (1, 0, "nregions"), (1, 65536, "nregions")]:
        a = list(full)
        a[idx] = value
        assert wf.lib.rnnwf_renyi2_regions_stack(wf.h, *a) == -1
        msg = wf.lib.rnnwf_last_error(wf.h).decode()
        assert msg.startswith(ENTRY + ": ") and re.search(word, msg), msg
        assert untouched()
    # the one-layer entry keeps refusing the stack, in its present words
    with pytest.raises(ValueError, match="rnnwf_renyi2_regions: not implemented for stacked layers"):
        wf.renyi2_regions(masks, NPAIRS)
    assert untouched()
    # the vmc_step batch still serves vmc_gradient after a refused call; after a served call no batch is resident
    wf.vmc_step(ns, seed=1, step=0, couplings=np.append(np.ones(N), 1.0))
    with pytest.raises(ValueError, match=ENTRY):
        wf.renyi2_regions_stack(bad, NPAIRS)
    assert wf.resident_samples() == ns
    wf.vmc_gradient(0.0, ns, {nm: (cnt,) for nm, cnt in wf._layout()})
    wf.renyi2_regions_stack(masks, NPAIRS)
    assert wf.resident_samples() == 0
    # one-layer handles, with the pointer to the entry that serves them
    for model, nx, ny in [(_lib.MODEL_GRU1D, N, 1), (_lib.MODEL_GRU1D_F64, 3, 2)]:
        w = _lib.NativeWavefunction(model, nx, ny, (10,))
        w.init_params(1)
        with pytest.raises(ValueError, match=ENTRY + ": serves stacked layers .*one layer; rnnwf_renyi2_regions serves it"):
            w.renyi2_regions_stack(masks, NPAIRS)
        with pytest.raises(ValueError, match="one layer; observables.py"):
            OS.renyi2_regions(w, masks, NPAIRS)
    # the other models, in the existing entries' words
    for model, nx, ny, un, word in [(_lib.MODEL_GRU1D_PARITY, N, 1, (10,), "parity"), (_lib.MODEL_CRNN_U1, N, 1, (10, 10), "complex RNN"),
                                    (_lib.MODEL_MDRNN2D, 3, 2, (10,), "MDRNN"), (_lib.MODEL_LSTM1D_F64, 3, 2, (10,), "LSTM")]:
        w = _lib.NativeWavefunction(model, nx, ny, un)
        w.init_params(1)
        with pytest.raises(ValueError, match=ENTRY + ": .*" + word):
            w.renyi2_regions_stack(masks, NPAIRS)
        with pytest.raises(ValueError, match="positive GRU models"):
            OS.renyi2_entropy(w, NPAIRS)
    fresh = _lib.NativeWavefunction(_lib.MODEL_GRU1D, N, 1, units)
    with pytest.raises(_lib.RnnwfError, match="not committed") as e:
        fresh.renyi2_regions_stack(masks, NPAIRS)
    assert not isinstance(e.value, ValueError)


# exact values at the weights of seed 111 (the same numbers in float32 and float64 to the digits shown), from the dense state vector
# on the CPU: I2({1} : {4}) = 0.0560, I2({1, 2} : {4, 5}) = 0.0997 - both >= 0.05
EXACT_I2 = {"sites": 0.0560, "blocks": 0.0997}


@pytest.mark.parametrize("f64,shape", [(False, (6, 1)), (True, (3, 2))], ids=["f32-6", "f64-3x2"])
def test_entropies_and_mutual_information_within_five_standard_errors(f64, shape):
    N, units, npairs = 6, (10, 10), 1 << 14
    prm = S.weights(f64, units, seed=111)
    wf = make_wf(f64, shape, units, prm)
    lp = M.prnn_log_probability(S.R.to64(prm), all_configs(N), dtype=np.float64)
    psi = np.exp(0.5 * lp)
    exact_s2 = lambda m: -np.log(S.purity_of_region(psi, N, m))
    names, masks = regions_of(shape, "small")
    S2, err = OS.renyi2_regions(wf, masks, npairs, seed=7, step=1)
    want = np.array([exact_s2(m) for m in masks])
    print("[stat %s] S2 = %s +- %s, exact %s" % ("f64" if f64 else "f32", np.round(S2, 4), np.round(err, 4), np.round(want, 4)))
    assert np.all(err > 0.0) and np.all(np.abs(S2 - want) <= 5.0 * err)
    Sl, el = OS.renyi2_entropy(wf, npairs, seed=7, step=1)
    cuts = np.array([exact_s2(S.mask_of(N, range(l))) if 0 < l < N else 0.0 for l in range(N + 1)])
    assert Sl[0] == 0.0 and Sl[N] == 0.0 and el[0] == 0.0 and el[N] == 0.0 and np.all(np.abs(Sl - cuts) <= 5.0 * el)
    for key, (a, b) in [("sites", ([1], [4])), ("blocks", ([1, 2], [4, 5]))]:
        ma, mb = S.mask_of(N, a), S.mask_of(N, b)
        exact = exact_s2(ma) + exact_s2(mb) - exact_s2(ma | mb)
        assert exact >= 0.05 and abs(exact - EXACT_I2[key]) < 5e-4
        i2, e2 = OS.renyi2_mutual_information(wf, ma, mb, npairs, seed=7, step=1)
        print("[stat %s] I2 %s = %.4f +- %.4f, exact %.4f" % ("f64" if f64 else "f32", key, i2, e2, exact))
        assert e2 > 0.0 and abs(i2 - exact) <= 5.0 * e2
