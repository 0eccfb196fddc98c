"""What tests/test_lstm_renyi_host.py and tests/test_gpu_lstm_renyi.py share: the cases of the LSTM's region-Renyi pass
(rnnwf_renyi2_regions_lstm, docs/renyi_lstm.md) and a NumPy float64 restatement of the bookkeeping of csrc/lstm_pauli_kernels.h's
PAIRED tail - checkpoints (h, c) after every site, packed spin and mask words, normalisation of the mask, restart at f - 1, the mixed
word (own & ~mask) | (partner & mask) - with switches for six deliberate defects.  TEST INFRASTRUCTURE ONLY.

The yardstick itself is brute force: renyi_regions_reference.log_ratio_regions on lstm_pauli_reference.log_p, both swapped
configurations of every (pair, region) written out in full and scored from site 0 in NumPy float64.

    log r_A(sigma, tau) = 1/2 [log P(tau_A sigma_B) + log P(sigma_A tau_B) - log P(sigma) - log P(tau)]

Bounds: the project's float64 bound 1e-11 N on a log-ratio (docs/renyi_regions.md); the sums against math.fsum of the device's own
log r, relative 1e-12.
"""
import numpy as np

import lstm_pauli_reference as Q
import lstm_reference as LR
import renyi_regions_reference as G
import renyi_stack_reference as S

SCOPE = Q.SCOPE
NPAIRS = 19                                               # 38 chains: two full 16-chain blocks and a ragged one of 6
WIDTHS = Q.WIDTHS                                         # NFULL 1, 1, 2, 2, 3, 3, 4, 4
LATTICES = ((3, 2), (4, 3), (11, 3), (7, 5), (3, 22))     # 6, 12, 33, 35, 66 sites: one, two and three spin words
CASES = [(shape, units) for shape in LATTICES for units in WIDTHS]
DEFECTS = {"own_on_A": "own instead of the partner's spins on A", "partner_checkpoint": "restart from the partner's checkpoint",
           "c_from_h": "the cell state restored from h's rows of the checkpoint", "checkpoint_f": "restart from row f instead of f - 1",
           "mask_shifted": "mask shifted by one site", "mask_word_0": "mask words of sites >= 32 read from word 0"}
# the lattices (by their number of sites) on which a defect changes some log r of the cases' regions
SHOWS = {"own_on_A": lambda N: N >= 2,                    # some region is not empty after normalisation
         "partner_checkpoint": lambda N: N >= 3,          # some region has f >= 2: hck[f - 1] has seen the spins 0..f-2
         "c_from_h": lambda N: N >= 2,                    # some region has f >= 1
         "checkpoint_f": lambda N: N >= 3,                # f - 1 and f name different checkpoints for some region with 1 <= f <= N - 2
         "mask_shifted": lambda N: N >= 2,
         "mask_word_0": lambda N: N > 32}                 # some region has a site in a second word


def bound(N):
    return Q.bound(N)


def parameters(units):
    return Q.parameters(units)


def log_p(prm, Nx, Ny):
    return Q.log_p(prm, Nx, Ny)


def pairs_of(Nx, Ny, units):
    N = Nx * Ny
    return np.random.RandomState(2000 * N + units).randint(0, 2, (2 * NPAIRS, N)).astype(np.int32)


def regions_of(Nx, Ny):
    """(names, (R, N) masks): renyi_stack_reference.small_regions, plus boundary_regions beyond one word and a site"""
    N = Nx * Ny
    named = S.small_regions(Nx, Ny) + (S.boundary_regions(N) if N > 33 else [])
    names, masks = zip(*named)
    return list(names), np.stack(masks)


def log_ratio(prm, Nx, Ny, pairs, masks, pair_idx=None):
    """the yardstick: (R, len(pair_idx)) log r_A by brute force"""
    pairs, masks = np.asarray(pairs), np.asarray(masks)
    return G.log_ratio_regions(log_p(prm, Nx, Ny), pairs.reshape(len(pairs), -1), masks.reshape(len(masks), -1), pair_idx)


def kernel_form(prm, pairs, masks, defect=None):
    """log r_A = 1/2 [(tail_sigma - suffix_sigma) + (tail_tau - suffix_tau)], (R, npairs), as lstm_site_terms_kernel, the PAIRED
    lstm_masked_tail_kernel and renyi_region_assemble_kernel compute it: the mask normalised (site 0 not in A), f its first site, the
    chain's own (h, c) of checkpoint f - 1 restored, its own spin f - 1 fed, the sites f..N-1 teacher-forced on the word
    (own & ~mask) | (partner & mask) with the partner the chain s ^ 1; suffix = the chain's own terms from f.  An empty region gives 0.
    defect names one deliberate error (DEFECTS)."""
    assert defect is None or defect in DEFECTS
    K, b, Wd, bd = LR._unpack(prm, SCOPE)
    s = np.asarray(pairs).astype(np.int64)
    B, N = s.shape
    assert B % 2 == 0
    H = b.size // 4
    eye = np.eye(2)
    rows = np.arange(B)
    partner = rows ^ 1
    x, c, h = np.zeros((B, 2)), np.zeros((B, H)), np.zeros((B, H))
    ck_h, ck_c, terms = [], [], np.zeros((N, B))
    for n in range(N):
        c, h = LR.lstm_step(x, c, h, K, b)
        terms[n] = LR._log_softmax(h @ Wd + bd)[rows, s[:, n]]
        ck_h.append(h)
        ck_c.append(c)
        x = eye[s[:, n]]
    own_words = Q._words(s)
    par_words = own_words[partner]
    one = np.uint64(1)
    out = np.zeros((len(masks), B // 2))
    for k, mask in enumerate(np.asarray(masks)):
        m, f = G.normalise(mask)
        if f == 0:
            continue
        if defect == "mask_shifted":
            m = np.concatenate([[0], m[:-1]])
        elif defect == "own_on_A":
            m = np.zeros(N, dtype=np.int64)
        mw = Q._words(m[None, :])[0]
        if defect == "mask_word_0":
            mw = np.full_like(mw, mw[0])
        g = min(f, N - 2) if defect == "checkpoint_f" else f - 1
        src = partner if defect == "partner_checkpoint" else rows
        h = ck_h[g][src]
        c = (ck_h[f - 1] if defect == "c_from_h" else ck_c[g])[src]
        x = eye[s[:, f - 1]]
        tail = np.zeros(B)
        for n in range(f, N):
            w = n >> 5
            word = (own_words[:, w] & ~mw[w]) | (par_words[:, w] & mw[w])
            spin = ((word >> np.uint64(n & 31)) & one).astype(np.int64)
            c, h = LR.lstm_step(x, c, h, K, b)
            tail += LR._log_softmax(h @ Wd + bd)[rows, spin]
            x = eye[spin]
        own = np.zeros(B)
        for n in range(f, N):
            own += terms[n]
        d = tail - own
        out[k] = 0.5 * (d[0::2] + d[1::2])
    return out
