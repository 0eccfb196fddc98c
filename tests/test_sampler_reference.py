"""The sampler check of tests/sampler_reference.py on the CPU oracle alone: (1) its conditionals agree with the restatements that
exist and are normalised, (2) oracle-drawn batches of every case of tests/test_gpu_sampler_full.py pass it inside the cap, (3) it
rejects the defects it is for, each applied to an oracle-drawn batch at config 2's size, (4) Philox known answers for the 64-bit
words of the stream.  No GPU.
"""
import numpy as np
import pytest

import sampler_reference as R
from conftest import all_configs
from lstm_reference import lstm_log_probability
from oracle import models as M
from oracle import philox

BIG_SEED = 0x9E3779B97F4A7C15


# ---- 1. the conditionals ------------------------------------------------------------------------------------------------------------

def _log_p(dec, p0):
    p1 = 1.0 - p0
    with np.errstate(divide="ignore"):
        return np.where(dec == 0, np.log(p0), np.log(p1)).sum(axis=1)


@pytest.mark.parametrize("family,shape,units", [("gru", (17, 1), (12,)), ("gru", (9, 1), (7, 5)), ("gru64", (3, 4), (9,)),
                                                ("parity", (11, 1), (6,)), ("mdrnn", (3, 4), (7,)), ("lstm", (3, 4), (6,))])
def test_conditionals_multiply_to_the_existing_log_probabilities(family, shape, units):
    N = shape[0] * shape[1]
    prm = R.build_params(family, units, seed=5, sharp=1.25 if family == "mdrnn" else 2.0)      # the elu cell saturates at x 2
    rng = np.random.RandomState(3)
    s = rng.randint(0, 2, (50, shape[0], shape[1]) if family == "mdrnn" else (50, N))
    p64, p32, forced, dec = R.conditionals(family, prm, s, shape)
    if family == "mdrnn":
        ref = M.mdrnn_log_probability(prm, s)
    elif family == "lstm":
        ref = lstm_log_probability(prm, s, shape[0], shape[1])
    else:       # the parity class draws from the forward chain: its conditionals multiply to the UNsymmetrised probability
        ref = M.prnn_log_probability(R.cast(prm, np.float64), s, dtype=np.float64)
    assert np.abs(_log_p(dec, p64) - ref).max() < 1e-12 * N
    assert p32.shape == p64.shape == dec.shape == (50, N) and 1e-9 < np.abs(p32 - p64).max() < 1e-4
    if family not in R.FLOAT64_FAMILIES and family != "parity":
        ref32 = M.prnn_log_probability(prm, s)
        assert np.abs(_log_p(dec, p32) - ref32).max() < 2e-6 * N


def test_mdrnn_uniforms_and_conditionals_are_in_path_order():
    prm = R.build_params("mdrnn", (6,), seed=2, sharp=1.25)
    u = philox.uniforms(7, 0, 0, 40, 12)
    s, _ = M.mdrnn_sample(prm, 3, 4, u)
    p64, p32, _, dec = R.conditionals("mdrnn", prm, s)
    assert np.array_equal(dec, (u >= p64).astype(np.int64))              # column k of u: the k-th visited site
    assert not np.array_equal(s.reshape(40, 12), dec)                     # ... which is not the flat site index


@pytest.mark.parametrize("layers", [1, 2])
def test_complex_conditionals_against_the_amplitude_and_the_mask(layers):
    N = 10
    prm = R.build_params("crnn", (8,) * layers, seed=4, sharp=2.0)
    s = M.crnn_sample(prm, N, philox.uniforms(1, 0, 0, 200, N))
    assert np.all(s.sum(axis=1) == N // 2)
    p64, p32, forced, dec = R.conditionals("crnn", prm, s)
    la = M.crnn_log_amplitude(R.cast(prm, np.float64), s, dtype=np.float64)
    assert np.abs(_log_p(dec, p64) - 2.0 * la.real).max() < 1e-11          # |psi|^2
    assert forced.any() and not forced[:, :N // 2].any()
    assert np.all((p64[forced] == 0.0) | (p64[forced] == 1.0)) and np.all((p64[~forced] > 0) & (p64[~forced] < 1))
    # every configuration: the conditionals are normalised, and all the weight lies in the sector of N / 2 up spins
    cfg = all_configs(N)
    p, _, _, d = R.conditionals("crnn", prm, cfg)
    w = np.exp(_log_p(d, p))
    assert abs(w.sum() - 1.0) < 1e-12 and abs(w[cfg.sum(axis=1) == N // 2].sum() - 1.0) < 1e-12


@pytest.mark.parametrize("family,shape,units", [("gru", (10, 1), (6,)), ("gru", (8, 1), (5, 4)), ("gru64", (2, 5), (6,)),
                                                ("mdrnn", (3, 3), (5,)), ("lstm", (3, 3), (5,))])
def test_normalisation_over_all_configurations(family, shape, units):
    N = shape[0] * shape[1]
    prm = R.build_params(family, units, seed=8, sharp=1.25 if family == "mdrnn" else 2.0)
    cfg = all_configs(N)
    s = cfg.reshape(-1, shape[0], shape[1]) if family == "mdrnn" else cfg
    p64, p32, _, dec = R.conditionals(family, prm, s, shape)
    assert abs(np.exp(_log_p(dec, p64)).sum() - 1.0) < 1e-12
    assert abs(np.exp(_log_p(dec, p32)).sum() - 1.0) < 1e-5


# ---- 2. clean oracle batches of every GPU case stay inside the cap -----------------------------------------------------------------------

def _distinct_cases():
    seen, out = set(), []
    for c in R.CASES:
        key = (c[1], c[2], c[3], c[5])
        if key not in seen:
            seen.add(key)
            out.append(c)
    return out


@pytest.mark.parametrize("cid,family,shape,units,ns,sharp,stride,engine,env", _distinct_cases(), ids=[c[0] for c in _distinct_cases()])
def test_clean_oracle_batches_stay_inside_the_cap(cid, family, shape, units, ns, sharp, stride, engine, env):
    """The oracle's own sampler (float32 cell for the float32 families), seed 111, on the parameters of every distinct case of the GPU
    module; config 2 on all 10 000 rows, the others on min(samples, 2 048) rows (the share is a rate per draw).  Recorded here:

        case              draws    excused  share    rows with one          case              draws    excused  share    rows
        cfg2-x3           800 000  1        1.3e-6   1                      stack-64-20        81 920  0
        cfg2-glorot       163 840  0                                        stack-3-layers     81 920  1        1.2e-5   1
        cfg5-x1.5         409 600  1        2.4e-6   1                      parity-40          81 920  1        1.2e-5   1
        cfg5-x3           409 600  95       2.3e-4   84 (4.1 %)             cfg3               81 920  1        1.2e-5   1
        width-36 .. -96    81 920  0                                        cfg3_l2            81 920  1        1.2e-5   1
        wide-128           81 920  2        2.4e-5   2                      cfg4-x1.25        294 912  0
        long-1000 x 2      96 000  0                                        gru64, lstm       294 912  0
        cfg2_l2           163 840  3        1.8e-5   3
        long-1000 at x 3: 29 draws in 17 of 96 rows (17.7 %) - outside the cap, so the case runs at x 2 (x 1.5: 1 draw).
    The oracle sampler disagreed with the float64 decision on 0 draws outside the band in every case."""
    rows = ns if cid == "cfg2-x3" else min(ns, 2048)
    N = shape[0] * shape[1]
    prm = R.build_params(family, units, seed=111, sharp=sharp)
    s = R.oracle_draw(family, prm, shape, philox.uniforms(111, 0, 0, rows, N))
    res = R.check(family, prm, s, 111, 0, 0, shape)
    print(R.line("[%s oracle]" % cid, res))
    assert res["unexcused"] == 0, R.failure_text(res)
    assert res["within_cap"]
    if family in R.FLOAT64_FAMILIES:
        assert res["excused"] == 0


# ---- 3. the defects -------------------------------------------------------------------------------------------------------------------

N2, H2, NS2, SEED, STEP = 80, 50, 10000, 111, 0


@pytest.fixture(scope="module")
def cfg2():
    """Config 2's size on sharpened weights: parameters, the stream's uniforms, the oracle's draws and their conditionals."""
    prm = R.build_params("gru", (H2,), seed=111, sharp=3.0)
    u = philox.uniforms(SEED, STEP, 0, NS2, N2)
    s = M.prnn_sample(prm, N2, u)[0]
    p64, p32, _, dec = R.conditionals("gru", prm, s)
    clean = R.judge(dec, u, p64, p32)
    assert clean["unexcused"] == 0 and clean["within_cap"] and clean["excused"] <= 2
    return dict(prm=prm, u=u, s=s, p64=p64, p32=p32)


def _rejudge(c, s_new, rows, u=None):
    """Judge the batch with rows `rows` replaced by s_new (conditionals recomputed for those rows only) against the TRUE uniforms."""
    p64, p32, s = c["p64"].copy(), c["p32"].copy(), c["s"].copy()
    a, b, _, _ = R.conditionals("gru", c["prm"], s_new)
    p64[rows], p32[rows], s[rows] = a, b, s_new
    return R.judge(s, c["u"] if u is None else u, p64, p32)


def _drawn_with(c, u_wrong, rows):
    """What a sampler that read u_wrong for `rows` would have drawn there, judged against the true stream."""
    return _rejudge(c, M.prnn_sample(c["prm"], N2, u_wrong[rows])[0], rows)


def test_rejects_one_chain_drawn_with_another_chains_uniforms(cfg2):
    u = cfg2["u"].copy()
    u[7321] = cfg2["u"][7322]
    res = _drawn_with(cfg2, u, np.array([7321]))
    assert res["unexcused"] > 0 and set(res["wrong_rows"]) == {7321}


def test_rejects_the_site_index_shifted_by_one(cfg2):
    rows = np.arange(0, NS2, 5)
    res = _drawn_with(cfg2, np.roll(cfg2["u"], -1, axis=1), rows)
    assert len(res["wrong_rows"]) > 0.5 * len(rows)        # sharp conditionals: many decisions hold for any uniform


def test_rejects_permuted_philox_lanes(cfg2):
    rows = np.arange(0, NS2, 5)
    u = cfg2["u"].reshape(NS2, N2 // 4, 4)[:, :, [1, 0, 2, 3]].reshape(NS2, N2)      # lanes n & 3 = 0 and 1 exchanged
    res = _drawn_with(cfg2, u, rows)
    assert len(res["wrong_rows"]) > 0.5 * len(rows)        # sharp conditionals: many decisions hold for any uniform
    assert set(res["wrong_draws"] % 4) == {0, 1}              # teacher-forced: the lanes that kept their place still decide correctly


def test_rejects_the_step_replaced_by_the_next(cfg2):
    rows = np.arange(0, NS2, 5)
    res = _drawn_with(cfg2, philox.uniforms(SEED, STEP + 1, 0, NS2, N2), rows)
    assert len(res["wrong_rows"]) > 0.5 * len(rows)        # sharp conditionals: many decisions hold for any uniform


def test_rejects_the_comparison_inverted_at_one_site_of_one_row(cfg2):
    r = 4242
    p = cfg2["p64"][r]
    n = int(np.flatnonzero((p > 0.05) & (p < 0.95) & (np.abs(cfg2["u"][r] - p) > 0.01))[0])      # chosen from the reference alone
    u = cfg2["u"].copy()
    u[r, n] = 0.0 if cfg2["s"][r, n] == 1 else 1.0 - 2.0 ** -24                                     # forces the other spin there
    res = _drawn_with(cfg2, u, np.array([r]))
    assert res["unexcused"] >= 1 and (r, n) == res["mismatches"][0][:2]


def test_rejects_a_block_that_reuses_block_zeros_hidden_state(cfg2):
    """Chains 16 b + c of block b = 300 decide with the conditionals of chain c of block 0 (its state), on their own uniforms."""
    b = 300
    rows = np.arange(16 * b, 16 * b + 16)
    s_new = (cfg2["u"][rows] >= cfg2["p32"][:16]).astype(np.int64)
    res = _rejudge(cfg2, s_new, rows)
    assert res["unexcused"] >= 8 and set(res["wrong_rows"]) <= set(rows) and len(res["wrong_rows"]) >= 8


def test_rejects_dropped_high_words_of_seed_and_sample_index():
    """A seed >= 2^32 and a batch whose global indices cross 2^32: a sampler that drops seed >> 32, or g >> 32, draws another stream."""
    ns, off = 2000, 2 ** 32 - 1000
    prm = R.build_params("gru", (H2,), seed=111, sharp=3.0)
    u = philox.uniforms(BIG_SEED, STEP, off, ns, N2)
    s = M.prnn_sample(prm, N2, u)[0]
    clean = R.check("gru", prm, s, BIG_SEED, STEP, off)
    assert clean["unexcused"] == 0 and clean["within_cap"]
    low_seed = M.prnn_sample(prm, N2, philox.uniforms(BIG_SEED & 0xFFFFFFFF, STEP, off, ns, N2))[0]
    res = R.check("gru", prm, low_seed, BIG_SEED, STEP, off)
    assert len(res["wrong_rows"]) > 0.9 * ns
    u_low_g = np.concatenate([u[:1000], philox.uniforms(BIG_SEED, STEP, 0, 1000, N2)])      # g & 0xFFFFFFFF past the boundary
    low_g = M.prnn_sample(prm, N2, u_low_g)[0]
    res = R.check("gru", prm, low_g, BIG_SEED, STEP, off)
    assert len(res["wrong_rows"]) > 900 and res["wrong_rows"].min() >= 1000


def _crnn_sample_mask_late(prm, N, u, scope=R.SCOPE):
    """M.crnn_sample with the defect: site n is masked with the counts of site n - 1."""
    ns = u.shape[0]
    Wa, ba = prm[scope + "/wf_dense_ampl/kernel"], prm[scope + "/wf_dense_ampl/bias"]
    x = np.zeros((ns, 2), np.float32)
    states = M._zero_states(prm, scope, ns, np.float32)
    s = np.empty((ns, N), np.int64)
    for n in range(N):
        out, states = M.multi_gru(x, states, prm, scope)
        ampl = M._crnn_masked_ampl(out, Wa, ba, n - 1, N, s[:, :max(n - 1, 0)].sum(axis=1).astype(np.float32))
        with np.errstate(divide="ignore"):
            s[:, n] = M.multinomial_2(np.log(ampl ** 2), u[:, n])
        x = M._one_hot(s[:, n], np.float32)
    return s


def test_rejects_the_complex_mask_applied_one_site_late():
    N, ns = 40, 2000
    prm = R.build_params("crnn", (50,), seed=111, sharp=3.0)
    u = philox.uniforms(SEED, STEP, 0, ns, N)
    clean = R.check("crnn", prm, M.crnn_sample(prm, N, u), SEED, STEP)
    assert clean["unexcused"] == 0 and clean["within_cap"]
    res = R.check("crnn", prm, _crnn_sample_mask_late(prm, N, u), SEED, STEP)
    assert res["unexcused"] > 0 and res["wrong_draws"].min() >= N // 2
    # the knob of the restatement itself reproduces the defective sampler: the check is about the mask, nothing else
    p64, p32, forced, dec = R.conditionals("crnn", prm, _crnn_sample_mask_late(prm, N, u), mask_delay=1)
    assert R.judge(dec, u, p64, p32, forced=forced)["unexcused"] == 0


def test_forced_draws_admit_no_band():
    N, ns = 40, 500
    prm = R.build_params("crnn", (50,), seed=111, sharp=3.0)
    u = philox.uniforms(SEED, STEP, 0, ns, N)
    s = M.crnn_sample(prm, N, u)
    p64, p32, forced, dec = R.conditionals("crnn", prm, s)
    band, _ = R.band_of(p64, p32, forced=forced)
    assert forced.any() and np.all(band[forced] == 0.0) and np.all(band[~forced] >= R.FACTOR * R.FLOOR)
    r, n = np.argwhere(forced)[0]
    dec[r, n] ^= 1
    assert R.judge(dec, u, p64, p32, forced=forced)["unexcused"] == 1


# ---- 4. Philox: the 64-bit words ------------------------------------------------------------------------------------------------------

def _direct(seed, step_word, g, site):
    out = philox.philox4x32_10(g & 0xFFFFFFFF, g >> 32, site // 4, step_word, seed & 0xFFFFFFFF, seed >> 32)
    return (int(np.asarray(out[site % 4])) >> 8) * 2.0 ** -24


def test_philox_known_answers_for_64_bit_words():
    """uniforms() places (g_lo, g_hi, site // 4, step_lo) in the counter and (seed_lo, seed_hi) in the key: checked against the
    block function called word by word (itself pinned to Random123's vectors by tests/test_oracle.py), and against recorded values."""
    seed, step, g = BIG_SEED, 2 ** 32 + 3, 2 ** 40 + 5
    u = philox.uniforms(seed, step, g, 3, 11)
    for b in range(3):
        for n in range(11):
            assert u[b, n] == _direct(seed, 3, g + b, n)
    assert np.array_equal(u, philox.uniforms(seed, 3, g, 3, 11))                     # only the low 32 bits of the step enter
    assert not np.array_equal(u, philox.uniforms(seed, 4, g, 3, 11))
    assert not np.array_equal(u, philox.uniforms(seed & 0xFFFFFFFF, step, g, 3, 11))  # seed >> 32 enters
    assert not np.array_equal(u, philox.uniforms(seed, step, g & 0xFFFFFFFF, 3, 11))  # g >> 32 enters
    words = [int(round(x * 2 ** 24)) for x in u[0, :4]]
    print("recorded:", words)
    assert words == KNOWN_WORDS
    across = philox.uniforms(111, 0, 2 ** 32 - 2, 4, 4)                               # the carry into g >> 32 inside one call
    assert np.array_equal(across[2:], philox.uniforms(111, 0, 2 ** 32, 2, 4))
    assert across[2, 0] == _direct(111, 0, 2 ** 32, 0) and across[1, 3] == _direct(111, 0, 2 ** 32 - 1, 3)


KNOWN_WORDS = [6588322, 5603836, 1675713, 14176600]      # 24-bit words of sample 2^40 + 5, sites 0..3, seed 0x9E3779B97F4A7C15, step 2^32 + 3
