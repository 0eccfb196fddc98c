"""Float64 reference of the complex RNN's Renyi-2 swap estimator for arbitrary regions (docs/renyi_complex.md), independent of the
library: plain NumPy on the oracle's complex RNN.  TEST INFRASTRUCTURE ONLY; validated by tests/test_crnn_renyi_reference.py.

    pair p = chains (2p, 2p + 1) = (sigma, tau),   mixed_s = (own & ~A) | (partner & A)
    log r_A = [log psi(mixed_sigma) - log psi(sigma)] + [log psi(mixed_tau) - log psi(tau)]   (complex; no factor 1/2)
    exp(-S2(A)) = E[Re r_A],   E[Im r_A] = 0;   r_A = 0, log r_A = (-inf, 0), where a mixed chain leaves the sector

explicit_log_ratio is brute force: both mixed configurations are written out in full and scored from site 0 with
crnn_pauli_reference.log_amp; the sector is decided by counting the ups of the mixed chains; the masks are NOT normalised.

kernel_form restates what crnn_renyi_kernels.h computes - the mask normalised to site 0 not in A, the restart from the chain's own
state after site f - 1 with its own spin f - 1 as input, the up-count restarted from the own prefix, the suffix from the own terms,
the survivor rule popcount(sigma & A) = popcount(tau & A) - with switches for the defects whose rejection the CPU test shows.
"""
import numpy as np

import crnn_pauli_reference as CR
from oracle import models as M

SCOPE = CR.SCOPE
NEG = complex(-np.inf, 0.0)


def mixed(samples, mask):
    """(2n, N): every chain with the partner's spins on the sites of the mask."""
    s = np.asarray(samples)
    partner = s.reshape(-1, 2, s.shape[1])[:, ::-1].reshape(s.shape)
    return np.where(np.asarray(mask, dtype=bool)[None, :], partner, s)


def survives(samples, mask):
    """(n,) bool: both mixed chains of the pair lie in the zero-magnetisation sector (by counting their ups)."""
    ok = CR.in_sector(mixed(samples, mask))
    return ok[0::2] & ok[1::2]


def popcount_rule(samples, mask):
    """(n,) bool: sigma and tau carry the same number of ups in the region - the device's survivor rule."""
    s = np.asarray(samples)
    q = s[:, np.asarray(mask, dtype=bool)].sum(axis=1)
    return q[0::2] == q[1::2]


def explicit_log_ratio(prm, samples, regions, score=None):
    """(R, n) complex128 log r_A, brute force; (-inf + 0j) where a mixed chain leaves the sector.  score: log psi of in-sector rows
    (default the float64 oracle)."""
    score = score or (lambda x: CR.log_amp(prm, x))
    samples = np.asarray(samples)
    assert np.all(CR.in_sector(samples)) and len(samples) % 2 == 0
    own = score(samples)
    out = np.full((len(regions), len(samples) // 2), NEG, dtype=np.complex128)
    for k, m in enumerate(regions):
        x = mixed(samples, m)
        ok = np.repeat(survives(samples, m), 2)
        if ok.any():
            d = score(x[ok]) - own[ok]
            out[k, ok[0::2]] = d[0::2] + d[1::2]
    return out


def explicit_log_ratio_f32(prm, samples, regions):
    """explicit_log_ratio on the FLOAT32 oracle: the yardstick of the full-size test."""
    return explicit_log_ratio(prm, samples, regions,
                              score=lambda x: M.crnn_log_amplitude(prm, x, SCOPE, dtype=np.float32).astype(np.complex128))


def ratio(d):
    return CR.ratio(d)


# ---- the site-resolved form of the kernels, with defects ------------------------------------------------------------------------------

DEFECTS = ("mask_shifted", "own_spins", "mask_word_0", "partner_checkpoint", "num_up_no_prefix", "half")


def normalised(mask):
    m = np.asarray(mask).astype(np.int64)
    return m ^ m[0]


def kernel_form(prm, samples, regions, defect=None, rule="region"):
    """(R, n) complex128 log r_A as the paired tail pass computes it.  defect names one deliberate error:
      "mask_shifted"        every mask shifted by one site (site n swapped where n - 1 was asked; the last site drops out)
      "own_spins"           the sites of A keep the chain's own spins (nothing is swapped)
      "mask_word_0"         the mask word of sites >= 32 read from word 0 (mask[n & 31] for mask[n])
      "partner_checkpoint"  restart from the PARTNER's state after site f - 1, with the partner's spin f - 1 as input
      "num_up_no_prefix"    the up-count of the restarted chain starts at 0 instead of the ups of the own sites below f
      "half"                the factor 1/2 of the positive models' estimator applied to log r
    rule: which sites the survivor rule counts the ups of - "region" (the normalised mask, the device's rule) or "complement"."""
    assert defect is None or defect in DEFECTS
    prm = CR.to64(prm)
    samples = np.asarray(samples)
    B, N = samples.shape
    rows = np.arange(B)
    one_hot = lambda s: np.eye(2)[s]
    partner_row = rows ^ 1

    def run(state, x, spins, n0, num_up):
        re, im, states = [], [], []
        num_up = num_up.copy()
        for n in range(n0, N):
            state = M.gru_cell(x, state, prm, SCOPE, 0)
            la, ph = CR._site_terms(prm, state, n, N, num_up)
            re.append(la[rows, spins[:, n]])
            im.append(ph[rows, spins[:, n]])
            states.append(state)
            num_up += spins[:, n]
            x = one_hot(spins[:, n])
        return np.stack(re, axis=1), np.stack(im, axis=1), states

    H = prm[SCOPE + "/" + M.GRU % 0 + "candidate/hidden_projection/kernel"].shape[0]
    own_re, own_im, hs = run(np.zeros((B, H)), np.zeros((B, 2)), samples, 0, np.zeros(B, dtype=np.int64))
    out = np.empty((len(regions), B // 2), dtype=np.complex128)
    for k, mask in enumerate(regions):
        m = normalised(mask)
        if not m.any():
            out[k] = 0.0
            continue
        f = int(np.flatnonzero(m)[0])                  # of the region that was asked for: the restart point
        counted = m if rule == "region" else 1 - m
        q = samples[:, counted == 1].sum(axis=1)
        alive = q[0::2] == q[1::2]
        if defect == "mask_shifted":
            m = np.concatenate([[0], m[:-1]])
        elif defect == "mask_word_0":
            m = m[np.arange(N) & 31]
        elif defect == "own_spins":
            m = np.zeros_like(m)
        x = np.where(m[None, :] == 1, samples[partner_row], samples)
        src = partner_row if defect == "partner_checkpoint" else rows
        state, inp = hs[f - 1][src], one_hot(samples[src, f - 1])
        nu = np.zeros(B, dtype=np.int64) if defect == "num_up_no_prefix" else samples[:, :f].sum(axis=1).astype(np.int64)
        re, im, _ = run(state, inp, x, f, nu)
        with np.errstate(invalid="ignore"):
            d = (re.sum(axis=1) - own_re[:, f:].sum(axis=1)) + 1j * (im.sum(axis=1) - own_im[:, f:].sum(axis=1))
            lr = d[0::2] + d[1::2]
        if defect == "half":
            lr = 0.5 * lr.real + 0.5j * lr.imag
        dead = ~alive | np.isneginf(re.sum(axis=1)[0::2]) | np.isneginf(re.sum(axis=1)[1::2])
        out[k] = np.where(dead, NEG, lr)
    return out


def max_abs_diff(a, b):
    return CR.max_abs_diff(a, b)


# ---- dense values -------------------------------------------------------------------------------------------------------------------

def dense_blocks(psi, N, mask):
    """{q: the rows of psi reshaped to (configurations of A, configurations of B) whose A part carries q ups} of a state over
    crnn_pauli_reference.all_configs(N) (site 0 = the most significant bit)."""
    m = np.asarray(mask, dtype=bool)
    a_sites, b_sites = np.flatnonzero(m), np.flatnonzero(~m)
    mat = psi.reshape((2,) * N).transpose(list(a_sites) + list(b_sites)).reshape(2 ** len(a_sites), 2 ** len(b_sites))
    charge = np.array([bin(i).count("1") for i in range(2 ** len(a_sites))])
    return {q: mat[charge == q] for q in range(len(a_sites) + 1)}


def dense_renyi2(psi, N, mask):
    """(Tr rho_A^2, {q: (p_q, Tr rho_A(q)^2)}) of a normalised state; rho_A is block-diagonal in the charge of A for a U(1) state."""
    sectors = {}
    for q, mq in dense_blocks(psi, N, mask).items():
        rho = mq @ mq.conj().T
        sectors[q] = (float(np.trace(rho).real), float(np.sum(np.abs(rho) ** 2)))
    return sum(t for _, t in sectors.values()), sectors


# ---- the regions of the tests ---------------------------------------------------------------------------------------------------------

def sites(N, which):
    m = np.zeros(N, dtype=np.int32)
    m[list(which)] = 1
    return m


# N = 10 / 12 units / weights(12): regions and their exact values (float64, this file's dense_renyi2): Tr rho_A^2, S2, P(match)
EXACT_REGIONS = [list(range(0, 5)), [3, 4, 5, 6], [2], [1, 2, 6, 7], [0, 2, 4, 6, 8], list(range(0, 8))]
EXACT_TRACE = [0.2303, 0.1664, 0.5027, 0.1324, 0.0950, 0.3887]
EXACT_MATCH = [0.286, 0.333, 0.503, 0.379, 0.358, 0.402]
EXACT_I2 = [(([1, 2], [6, 7]), 0.448), (([0, 1], [8, 9]), 0.156)]
FLOOR = 0.05


def case_regions(N):
    """The regions of the GPU log-ratio test: a bulk interval, a single site, every third site, a two-piece region, a region with site
    0, intervals ending on, starting on and straddling every 32-site boundary, the empty and the full region."""
    groups = [range(N // 3, (2 * N) // 3), [N // 2], range(1, N, 3), list(range(1, 3)) + list(range(N - 3, N - 1)), range(0, N // 2 + 1)]
    for w in range(32, N, 32):
        groups += [range(w - 3, w), range(w, min(w + 3, N)), range(w - 2, min(w + 2, N))]
    groups += [[], range(N)]
    return np.stack([sites(N, g) for g in groups])


def pick_seed(N, npairs, regions, lo=3):
    """The first seed whose random_sector_samples give every non-trivial region at least `lo` and at most npairs - lo survivors by
    the NumPy rule alone: both branches of the device's rule then provably run."""
    for seed in range(1000):
        s = CR.random_sector_samples(N, 2 * npairs, seed)
        ok = True
        for m in regions:
            if 0 < m.sum() < N:
                k = int(survives(s, m).sum())
                ok = ok and lo <= k <= npairs - lo
        if ok:
            return seed, s
    raise AssertionError("no seed below 1000 gives every region both outcomes")
