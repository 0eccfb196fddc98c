"""CPU validation of tests/crnn_renyi_reference.py, the float64 reference of the complex RNN's Renyi-2 swap estimator
(docs/renyi_complex.md): kernel_form against brute force, the defect study, and the exact identities over all 252^2 pairs of the
N = 10 sector against the dense reduced density matrix.  No GPU."""
import numpy as np
import pytest

import crnn_pauli_reference as CR
import crnn_renyi_reference as RR

TOL = 1e-12


@pytest.fixture(scope="module")
def big():
    """N = 40 / 20 units, 24 in-sector pairs and regions that reach both mask words."""
    N, H = 40, 20
    prm = CR.weights(H, seed=11, scale=2.0)
    regions = np.stack([RR.sites(N, g) for g in (range(10, 30), range(30, 36), range(33, 40), [5, 6, 34, 35], range(0, 34), range(3, 40, 3))])
    seed, s = RR.pick_seed(N, 24, regions, lo=3)
    return N, prm, s, regions, RR.explicit_log_ratio(prm, s, regions)


def test_kernel_form_meets_brute_force(big):
    N, prm, s, regions, brute = big
    assert RR.max_abs_diff(RR.kernel_form(prm, s, regions), brute) <= TOL
    # both outcomes of the survivor rule occur in every region, and the rule is the sector membership of the mixed chains
    for m, row in zip(regions, brute):
        alive = ~np.isneginf(row.real)
        assert 3 <= alive.sum() <= len(row) - 3
        assert np.array_equal(alive, RR.popcount_rule(s, m)) and np.array_equal(alive, RR.survives(s, m))
    # small case, the empty and the full region: exactly (0, 0)
    prm10 = CR.weights(12)
    s10 = CR.random_sector_samples(10, 40, 3)
    reg10 = np.stack([RR.sites(10, g) for g in RR.EXACT_REGIONS] + [RR.sites(10, []), RR.sites(10, range(10))])
    a, b = RR.kernel_form(prm10, s10, reg10), RR.explicit_log_ratio(prm10, s10, reg10)
    assert RR.max_abs_diff(a, b) <= TOL and np.all(a[-2:] == 0.0) and np.all(np.abs(b[-2:]) <= TOL)


@pytest.mark.parametrize("defect", RR.DEFECTS)
def test_every_defect_moves_log_r_far_beyond_the_f32_bound(big, defect):
    N, prm, s, regions, brute = big
    bad = RR.kernel_form(prm, s, regions, defect=defect)
    fin = ~np.isneginf(brute.real)                       # a finite log r turned into -inf has moved by infinity
    with np.errstate(invalid="ignore"):
        moved = np.where(np.isneginf(bad.real[fin]), np.inf, np.abs(bad[fin] - brute[fin])).max()
    flipped = np.isneginf(bad.real) != np.isneginf(brute.real)
    print("[crnn renyi defect %s] max |d log r| %.3e on %d finite entries, %d entries changed sector" % (defect, moved, fin.sum(), flipped.sum()))
    assert moved >= 1e3 * CR.F32_BOUND * N


def test_the_complement_survivor_rule_differs_only_outside_the_sector(big):
    """Counting the ups over the complement of the normalised mask instead of the mask: for two chains of the sector the two counts
    differ by the same total, so the rule is the same to the bit and this is NOT a defect on the chains the entry point accepts.  It
    is one as soon as a chain leaves the sector - which is why caller-supplied samples are checked on the host."""
    N, prm, s, regions, brute = big
    assert np.array_equal(RR.kernel_form(prm, s, regions, rule="complement").view(np.float64), RR.kernel_form(prm, s, regions).view(np.float64))
    out = s.copy()
    out[1] = out[0]                                                  # pair 0 = (sigma, sigma), then
    out[0, np.flatnonzero(out[0] == 0)[0]] = 1                       # sigma with N/2 + 1 ups: exactly one of the two counts still agrees
    differs = False
    for m in regions:
        mm = RR.normalised(m)
        qa, qc = out[:2][:, mm == 1].sum(axis=1), out[:2][:, mm == 0].sum(axis=1)
        differs = differs or ((qa[0] == qa[1]) != (qc[0] == qc[1]))
    assert differs


@pytest.fixture(scope="module")
def exact():
    """N = 10 / 12 units / weights(12): all 252^2 pairs of the sector, their weights and their brute-force log r."""
    N = 10
    prm = CR.weights(12)
    psi, idx = CR.dense_state(prm, N)
    assert abs(np.vdot(psi, psi).real - 1.0) <= TOL
    cfg = CR.sector(N)
    n = len(cfg)
    ia, ib = np.repeat(np.arange(n), n), np.tile(np.arange(n), n)
    pairs = np.empty((2 * n * n, N), dtype=np.int32)
    pairs[0::2], pairs[1::2] = cfg[ia], cfg[ib]
    P = np.abs(psi[idx]) ** 2
    regions = np.stack([RR.sites(N, g) for g in RR.EXACT_REGIONS])
    return N, prm, psi, pairs, P[ia] * P[ib], regions, RR.explicit_log_ratio(prm, pairs, regions)


def test_exact_identities_over_all_sector_pairs(exact):
    N, prm, psi, pairs, w, regions, lr = exact
    r = RR.ratio(lr)
    for k, m in enumerate(regions):
        trace, sectors = RR.dense_renyi2(psi, N, m)
        est = np.sum(w * r[k])
        match = np.sum(w * (r[k] != 0.0))
        print("[crnn renyi exact] region %-18s Tr rho^2 %.6f S2 %.6f P(match) %.4f | est %.12f%+.2ei" % (RR.EXACT_REGIONS[k], trace, -np.log(trace), match, est.real, est.imag))
        assert trace >= RR.FLOOR
        assert abs(est.real - trace) <= TOL and abs(est.imag) <= TOL
        assert abs(trace - RR.EXACT_TRACE[k]) <= 5e-5 and abs(match - RR.EXACT_MATCH[k]) <= 1e-3      # the table's digits
        # symmetry-resolved: the sector traces and the charge distribution against the dense blocks, and their sum is the total
        q = pairs[0::2][:, m == 1].sum(axis=1)
        total = 0.0
        for c, (p_q, t_q) in sectors.items():
            assert abs(np.sum(w * r[k].real * (q == c)) - t_q) <= TOL and abs(np.sum(w * (q == c)) - p_q) <= TOL
            total += t_q
        assert abs(total - trace) <= TOL


def test_region_and_complement_give_the_same_ratio(exact):
    N, prm, psi, pairs, w, regions, lr = exact
    sub = slice(0, 4000)
    comp = RR.explicit_log_ratio(prm, pairs[sub], 1 - regions)
    assert RR.max_abs_diff(comp, lr[:, :2000]) <= TOL
    assert RR.max_abs_diff(RR.kernel_form(prm, pairs[sub], regions), lr[:, :2000]) <= TOL


def test_mutual_information_values(exact):
    N, prm, psi, pairs, w, regions, lr = exact
    for (a, b), want in RR.EXACT_I2:
        ta, tb, tab = (RR.dense_renyi2(psi, N, RR.sites(N, g))[0] for g in (a, b, a + b))
        i2 = -np.log(ta) - np.log(tb) + np.log(tab)
        print("[crnn renyi exact] I2(%s : %s) = %.6f" % (a, b, i2))
        assert i2 >= RR.FLOOR and abs(i2 - want) <= 5e-4
