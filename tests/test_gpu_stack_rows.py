"""GPU tests of the Pauli and region-Renyi passes of STACKED GRU layers on EVERY row of the kernel table (rnnwf_pauli_step_stack,
rnnwf_pauli_train_steps_stack, rnnwf_renyi2_regions_stack: csrc/stack_chain_kernels.h, prnn_ml_masked_tail_kernel plain and PAIRED,
prnn_ml_site_terms_kernel; one instantiation per stack row of csrc/shapes.h, each with its waves per workgroup and its MlSpill value).

tests/stack_rows_reference.py has the case table (27 rows and two stacks of unequal widths per element type), the shapes (N = 40: two
words of packed spins; 37 samples, 19 pairs), the operators (first sites 0, 1, 31, 32, 33, 35, 36, N - 1 among them) and the bounds -
float64 1e-11 N, float32 16 x the float32 NumPy oracle's deviation from the float64 brute force on the same chains and masks, capped at
2 (2e-6 N + 2e-6), in BOTH passes; tests/test_stack_rows_reference.py shows on the CPU what these bounds accept and refuse.

  a. Pauli pass, every row: log-ratios, E_loc and per-term sums against the float64 brute force.
  b. Renyi pass, every row: log r of every region on every pair; the sums against math.fsum of the device's own log r.
  c. the grid-stride loop on 8-wave rows (float32 (3, 2), float64 (2, 2)): more tiles than 32 waves on every CU, each pass run once on the
     whole batch, the reference on whole 16-chain blocks at asserted positions (first, two between, the last full, the ragged last).
  d. lane identity on a partially spilled row per element type: 19 identical pairs give identical columns, ragged block included.
  e. pauli_train_steps_stack, three iterations, against the host loop bit for bit on a partially spilled row per element type.

Measured on an MI355X (profiles/stack_rows.txt has every row): float32 log-ratios at most 0.717 of the bound in the Pauli pass
((float, 3, 6), 100 units: 1.18e-04 of 1.64e-04) and 0.465 in the Renyi pass ((float, 2, 6)); float64 at most 5.4e-13 of 4.0e-10; E_loc at
most 0.011 of its bound, per-term sums 0.100.  No row failed.  The module takes 13 s, its slowest case 0.6 s.
"""
import numpy as np
import pytest

import pauli_stack_reference as SR
import stack_rows_reference as W
from rnnwavefunctions_amd import training as T

pytestmark = pytest.mark.gpu

S = W.S
SCOPE = W.SCOPE
N, NS, NPAIRS = W.N, W.NS, W.NPAIRS


def make_wf(c, prm, shape=None):
    from rnnwavefunctions_amd import _lib
    shape = shape or c.shape
    wf = _lib.NativeWavefunction(_lib.MODEL_GRU1D_F64 if c.f64 else _lib.MODEL_GRU1D, shape[0], shape[1], tuple(c.units))
    wf.set_params(prm, scope=SCOPE)
    return wf


# ---- a, b: every row -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", W.CASES, ids=W.case_id)
def test_pauli_pass_on_every_row_against_float64(c):
    prm = W.weights(c)
    wf = make_wf(c, prm)
    ham = W.hamiltonian()
    s = wf.sample(NS, seed=W.SEED, step=0).reshape(NS, N)
    out = wf.pauli_step_stack(ham.flip, ham.sign, ham.coeff, NS, samples=s, want_eloc=True, want_log_ratio=True)
    ref = SR.reference(prm, s, ham)
    lr32 = None if c.f64 else W.pauli_log_ratio(W.scorer(prm, np.float32), s, W.flip_masks(ham))
    tol, dev32, how = W.pauli_tol(c, ref["log_ratio"], lr32)
    SR.judge("%s Pauli, bound %s" % (W.row_label(c), how), out, ref, tol)
    assert out["moments"][2] == NS and wf.resident_samples() == NS
    assert W.spread(ref["log_ratio"]) > 0.2                      # the weights are sharp: the ratios spread


@pytest.mark.parametrize("c", W.CASES, ids=W.case_id)
def test_renyi_pass_on_every_row_against_float64(c):
    prm = W.weights(c)
    wf = make_wf(c, prm)
    names, reg = W.regions(c.shape)
    s = wf.sample(2 * NPAIRS, seed=W.SEED, step=0).reshape(2 * NPAIRS, N)
    out = wf.renyi2_regions_stack(reg, NPAIRS, samples=s, log_ratio=True)
    assert out["log_ratio"].shape == (len(reg), NPAIRS)
    ref = S.log_ratio(prm, s, reg)
    ref32 = None if c.f64 else S.log_ratio(prm, s, reg, dtype=np.float32)
    W.judge_renyi("%s Renyi" % W.row_label(c), out["log_ratio"], ref, ref32, c, names)
    rel = S.judge_sums(W.case_id(c), out["sums"], out["log_ratio"])
    print("%s sums: relative %.1e of the exactly rounded sums" % (W.row_label(c), rel))


# ---- c: the grid-stride loop on 8-wave rows ----------------------------------------------------------------------------------------------
STRIDE_NS = 2693                                   # 168 blocks and a ragged one of 5 x 49 masks = 8 281 tiles > 32 waves on each of 256 CUs
STRIDE_NPAIRS = 4379                               # 8 758 chains: 547 blocks and a ragged one of 6 x 15 distinct regions (17 listed) = 8 220 tiles
STRIDE_BLOCKS = {STRIDE_NS: [0, 56, 112, 167, 168], 2 * STRIDE_NPAIRS: [0, 182, 365, 546, 547]}
STRIDE_ROWS = [(False, 3, 2), (True, 2, 2)]


def checked_columns(ns, rows):
    """the chains of the 16-chain blocks STRIDE_BLOCKS[ns] and the least tile index of the last row of each; positions only"""
    nsb = (ns + 15) // 16
    blocks = STRIDE_BLOCKS[ns]
    assert blocks[0] == 0 and blocks[-1] == nsb - 1 and blocks[-2] == nsb - 2 and ns % 16 != 0 and sorted(set(blocks)) == blocks
    cols = np.concatenate([np.arange(16 * b, min(16 * b + 16, ns)) for b in blocks])
    return cols, [(rows - 1) * nsb + b for b in blocks], nsb


@pytest.mark.parametrize("row", STRIDE_ROWS, ids=lambda r: "%s-%dx%d" % ("f64" if r[0] else "f32", r[1], r[2]))
def test_grid_stride_on_8_wave_rows(row):
    c = W.case_of(*row)
    assert c.WAVES == 8
    prm = W.weights(c)
    wf = make_wf(c, prm)
    cus = wf.device_info()["cu_count"]
    s = wf.sample(2 * STRIDE_NPAIRS, seed=W.SEED, step=0).reshape(2 * STRIDE_NPAIRS, N)
    # Pauli: the first STRIDE_NS chains, one call
    ham = W.hamiltonian()
    masks = W.flip_masks(ham)
    cols, last_tiles, nsb = checked_columns(STRIDE_NS, len(masks))
    print("%s: %d CUs; Pauli %d tiles, last tiles of the checked blocks %s" % (W.row_label(c), cus, len(masks) * nsb, last_tiles))
    assert len(masks) * nsb > 32 * cus and last_tiles[2] >= 32 * cus and last_tiles[-1] >= 32 * cus        # beyond the first lap
    out = wf.pauli_step_stack(ham.flip, ham.sign, ham.coeff, STRIDE_NS, samples=s[:STRIDE_NS], want_eloc=True, want_log_ratio=True)
    assert wf.resident_samples() == STRIDE_NS                                                               # one pass
    assert np.all(np.isfinite(out["log_ratio"])) and np.all(np.isfinite(out["eloc"]))
    ref = SR.reference(prm, s[cols], ham)
    lr32 = None if c.f64 else W.pauli_log_ratio(W.scorer(prm, np.float32), s[cols], masks)
    tol, dev32, how = W.pauli_tol(c, ref["log_ratio"], lr32)
    d = np.abs(out["log_ratio"][:, cols] - ref["log_ratio"])
    r, k = np.unravel_index(int(np.argmax(d)), d.shape)
    e_over = float((np.abs(out["eloc"][cols] - ref["eloc"]) / SR.eloc_bound(ref, tol)).max())
    print("%s grid-stride Pauli: max |d log r| %.3e = %.3f x tol %.3e (%s; mask row %d, chain %d, block %d) over %d chains; E_loc %.3f x bound"
          % (W.row_label(c), d[r, k], d[r, k] / tol, tol, how, r, cols[k], cols[k] // 16, len(cols), e_over))
    assert d[r, k] <= tol, "%s: mask row %d, chain %d (block %d): |log r - ref| = %.3e > %.3e" % (W.row_label(c), r, cols[k], cols[k] // 16, d[r, k], tol)
    assert e_over <= 1.0 and W.spread(ref["log_ratio"]) > 0.2
    # PAIRED: all pairs, one call
    names, reg = W.regions(c.shape)
    distinct = len({W.G.normalise(m)[0].tobytes() for m in reg})
    cols, last_tiles, nsb = checked_columns(2 * STRIDE_NPAIRS, distinct)
    print("%s: Renyi %d tiles of %d distinct regions, last tiles of the checked blocks %s" % (W.row_label(c), distinct * nsb, distinct, last_tiles))
    assert distinct * nsb > 32 * cus and last_tiles[-2] >= 32 * cus and last_tiles[-1] >= 32 * cus
    wf.timing_enable(True)
    wf.timing_reset()
    out = wf.renyi2_regions_stack(reg, STRIDE_NPAIRS, samples=s, log_ratio=True)
    assert wf.timing_get(1)["launches"] == 1                                                                # one pass
    assert np.all(np.isfinite(out["log_ratio"]))
    pairs = cols[0::2] // 2
    ref = S.log_ratio(prm, s, reg, pair_idx=pairs)
    ref32 = None if c.f64 else S.log_ratio(prm, s, reg, dtype=np.float32, pair_idx=pairs)
    bound = S.f64_bound(N) if c.f64 else S.f32_bound(float(np.abs(ref32 - ref).max()), N)[0]
    d = np.abs(out["log_ratio"][:, pairs] - ref)
    r, k = np.unravel_index(int(np.argmax(d)), d.shape)
    assert d[r, k] <= bound, "%s: region %d (%s), pair %d (chains %d, %d; block %d): |log r - ref| = %.3e > %.3e" % (
        W.row_label(c), r, names[r], pairs[k], 2 * pairs[k], 2 * pairs[k] + 1, pairs[k] // 8, d[r, k], bound)
    S.judge("%s grid-stride Renyi, %d pairs" % (W.row_label(c), len(pairs)), out["log_ratio"][:, pairs], ref, ref32, c.f64, N)
    S.judge_sums(W.case_id(c), out["sums"], out["log_ratio"])


# ---- d: lane identity ------------------------------------------------------------------------------------------------------------------
PARTIAL_ROWS = [(False, 3, 3), (True, 3, 2)]


@pytest.mark.parametrize("row", PARTIAL_ROWS, ids=lambda r: "%s-%dx%d" % ("f64" if r[0] else "f32", r[1], r[2]))
def test_identical_pairs_give_identical_columns(row):
    c = W.case_of(*row)
    assert 0 < c.spill < c.NL - 1
    prm = W.weights(c)
    wf = make_wf(c, prm)
    two = np.random.RandomState(7).randint(0, 2, size=(2, N)).astype(np.int32)
    assert np.any(two[0, 32:] != two[1, 32:]) and np.any(two[0, :32] != two[1, :32])
    s = np.tile(two, (NPAIRS, 1))                                 # 38 chains: two full 16-chain blocks and a ragged one of 6
    ham = W.hamiltonian()
    lr = wf.pauli_step_stack(ham.flip, ham.sign, ham.coeff, 2 * NPAIRS, samples=s, want_log_ratio=True)["log_ratio"]
    assert np.all(np.isfinite(lr)) and np.abs(lr).max() > 0.1
    for k in (0, 1):
        assert np.array_equal(lr[:, k::2], np.repeat(lr[:, k:k + 1], NPAIRS, axis=1)), "Pauli: lanes %d, %d, ... differ" % (k, k + 2)
    assert not np.array_equal(lr[:, 0], lr[:, 1])
    names, reg = W.regions(c.shape)
    lr = wf.renyi2_regions_stack(reg, NPAIRS, samples=s, log_ratio=True)["log_ratio"]
    assert np.all(np.isfinite(lr)) and np.abs(lr).max() > 0.1
    assert np.array_equal(lr, np.repeat(lr[:, :1], NPAIRS, axis=1)), "Renyi: pair columns differ"
    # ... and they are the right numbers
    ref = S.log_ratio(prm, two, reg)
    bound = S.f64_bound(N) if c.f64 else S.f32_bound(float(np.abs(S.log_ratio(prm, two, reg, dtype=np.float32) - ref).max()), N)[0]
    print("%s identical pairs: max |d log r| %.3e, bound %.3e" % (W.row_label(c), np.abs(lr[:, :1] - ref).max(), bound))
    assert np.abs(lr[:, :1] - ref).max() <= bound


# ---- e: training -------------------------------------------------------------------------------------------------------------------------
K = 3
LRS = [5e-3, 2e-2, 1e-3]
TRAIN_NS = 64
TRAIN_CASES = [(False, (10, 1), (50, 50, 50)), (True, (5, 2), (36, 36, 36, 36))]


@pytest.mark.parametrize("f64,shape,units", TRAIN_CASES, ids=["f32-10-50x50x50", "f64-5x2-36x36x36x36"])
def test_device_resident_training_equals_the_host_loop_on_partially_spilled_rows(f64, shape, units, monkeypatch):
    c = W.row_case(f64, units)
    assert 0 < c.spill < c.NL - 1
    prm = S.weights(f64, units, seed=5, sharp=2.0)
    ham = SR.hamiltonian("mixed", shape[0] * shape[1])
    args = (ham.flip, ham.sign, ham.coeff)
    # the host loop pauli_step_stack -> cost_gradient -> training.Adam -> set_params.  Its handle keeps the one-wave base kernel, as the
    # stack entries always do (test_gpu_pauli_stack.test_bit_exact_identities: float32 stacks of up to 52 units)
    if not f64 and max(units) <= 52:
        monkeypatch.setenv("RNNWF_NO_COOP", "1")
    host = make_wf(c, prm, shape)
    monkeypatch.delenv("RNNWF_NO_COOP", raising=False)
    opt = T.Adam()
    params = {k: np.array(v) for k, v in prm.items()}
    moms, sums = [], []
    for k, lr in enumerate(LRS):
        out = host.pauli_step_stack(*args, TRAIN_NS, seed=11, step=k)
        s1, s2, n, _ = out["moments"]
        moms.append(out["moments"].copy())
        sums.append(out["term_sums"].copy())
        params = opt.step(params, T.cost_gradient(host, params, SCOPE, s1 / n, n), lr)
        host.set_params(params, scope=SCOPE)
    moms, sums = np.array(moms), np.array(sums)
    assert np.all(np.isfinite(moms)) and moms[:, 1].min() > 0.0 and not np.array_equal(moms[0], moms[-1])
    wf = make_wf(c, prm, shape)
    out = wf.pauli_train_steps_stack(*args, TRAIN_NS, 11, 0, LRS, want_term_sums=True)
    assert np.array_equal(out["moments"], moms) and np.array_equal(out["term_sums"], sums)
    got = wf.get_params_dict(prm, SCOPE)
    for k in params:
        assert got[k].dtype == params[k].dtype and np.array_equal(got[k], params[k]), k
    assert any(not np.array_equal(params[k], prm[k]) for k in prm)
    m, v, t = wf.adam_get_state()
    m0, v0 = opt.to_flat(wf, params, SCOPE)
    assert t == opt.t == K and np.array_equal(m, m0) and np.array_equal(v, v0) and np.abs(m).max() > 0.0
