"""What tests/test_lstm_corr_host.py and tests/test_gpu_lstm_corr.py share: the cases of the LSTM's all-pair correlation pass
(rnnwf_correlations_lstm, docs/correlations_lstm.md) and a NumPy float64 restatement of the bookkeeping of csrc/lstm_corr_kernels.h and
corr_assemble_kernel - checkpoints (h, c) after every site, packed spin words, trunk states kept per (i, n), the branch restarted
from the trunk, the assembly formula - with switches for six deliberate defects.  TEST INFRASTRUCTURE ONLY.  The yardstick itself is
brute force: tests/correlations_reference.log_ratio_entries on tests/lstm_reference's log P, every flipped configuration written out
and scored from site 0.
"""
import numpy as np

import correlations_reference as CR
import lstm_grad_reference as LG
import lstm_pauli_reference as Q
import lstm_reference as LR

SCOPE = LG.SCOPE
NS = Q.NS                                                 # 40: two full 16-chain blocks and a ragged one of 8
WIDTHS = Q.WIDTHS                                         # both ends of every NFULL
ALL_PAIRS = (4, 3)                                        # every width: all 12 + 66 rows against brute force
LATTICES = ((2, 1), (3, 3), (11, 3), (7, 5), (3, 22))     # 2 .. 66 sites: one, two and three spin words
LATTICE_WIDTHS = (20, 68)
DEFECTS = ("trunk_from_base", "branch_from_hck", "c_from_h", "j_plus_one", "word_0", "dropped_tail")
N_RANDOM_PAIRS = 32

bound = Q.bound
parameters = Q.parameters
samples_of = Q.samples_of
log_p = Q.log_p
pair_list, row_of = CR.pair_list, CR.row_of


def pair_index(i, n, N):
    return i * (2 * N - i - 1) // 2 + (n - i - 1)


def checked_pairs(N, seed=0):
    """(i, j) arrays.  N <= 12: every pair.  Larger: distance 1 at both ends, (0, N-1), each pair straddling a word boundary
    (31|32, 63|64), (0, 32), and N_RANDOM_PAIRS more drawn with a fixed seed."""
    pi, pj = pair_list(N)
    if N <= 12:
        return pi, pj
    pairs = {(0, 1), (N - 2, N - 1), (0, N - 1)}
    pairs |= {(w - 1, w) for w in (32, 64) if w < N}
    if N > 32:
        pairs.add((0, 32))
    rest = [p for p in zip(pi.tolist(), pj.tolist()) if p not in pairs]
    pick = np.random.RandomState(seed).choice(len(rest), size=N_RANDOM_PAIRS, replace=False)
    pairs |= {rest[k] for k in pick}
    p = np.array(sorted(pairs), dtype=np.int64)
    return p[:, 0], p[:, 1]


def check_subset(N, i, j):
    """what a case's pairs must contain, asserted (not only intended)"""
    have = set(zip(np.asarray(i).tolist(), np.asarray(j).tolist()))
    assert len(have) == len(i) and all(0 <= a < b < N for a, b in have)
    if N >= 2:
        assert {(0, 1), (N - 2, N - 1), (0, N - 1)} <= have
    for w in (32, 64):
        assert w >= N or (w - 1, w) in have
    assert N <= 32 or (0, 32) in have
    assert N <= 12 or len(have) >= N_RANDOM_PAIRS + 3


def brute_force(prm, shape, samples, i, j):
    """(N + len(i), ns): log r of every single flip, then of the pairs (i, j), each flipped configuration scored from site 0"""
    s = np.asarray(samples)
    ns, N = s.shape
    ii = np.concatenate([np.arange(N), np.asarray(i, dtype=np.int64)])
    jj = np.concatenate([np.full(N, -1), np.asarray(j, dtype=np.int64)])
    c, r = np.meshgrid(np.arange(ns), np.arange(len(ii)), indexing="xy")
    return CR.log_ratio_entries(log_p(prm, *shape), s, c.ravel(), ii[r.ravel()], jj[r.ravel()]).reshape(len(ii), ns)


def rows_of(N, i, j):
    """the rows of a full (N + N(N-1)/2, ns) log-ratio array that brute_force(.., i, j) restates"""
    return np.concatenate([np.arange(N), row_of(np.asarray(i), np.asarray(j), N)])


def kernel_form(prm, samples, defect=None):
    """(N + N(N-1)/2, ns) log-ratios as lstm_corr_base_kernel, lstm_trunk_kernel, lstm_branch_kernel, corr_suffix_kernel and
    corr_assemble_kernel compute them.  defect names one deliberate error:
      "trunk_from_base"  sites i+1..j-1 taken from the base chain (tsel = bsel)
      "branch_from_hck"  the branch restored from hck[j] instead of tck[p(i, j)] (the first flip lost)
      "c_from_h"         the cell state restored from h's rows, in trunk and branch
      "j_plus_one"       the branch of (i, j) restored from tck[p(i, j + 1)] (where j + 1 <= N - 2)
      "word_0"           the spins of sites >= 32 read from word 0 in trunk and branch
      "dropped_tail"     the tail term left out of the assembly
    """
    assert defect in (None,) + DEFECTS
    K, b, Wd, bd = LR._unpack(prm, SCOPE)
    s = np.asarray(samples).astype(np.int64)
    B, N = s.shape
    H = b.size // 4
    eye = np.eye(2)
    rows = np.arange(B)
    NP = N * (N - 1) // 2
    words = Q._words(s)

    def spin(n):
        w = 0 if defect == "word_0" else n >> 5
        return ((words[:, w] >> np.uint64(n & 31)) & np.uint64(1)).astype(np.int64)

    def both_terms(h, sig):
        ls = LR._log_softmax(h @ Wd + bd)
        return ls[rows, sig], ls[rows, 1 - sig]

    # base pass: checkpoints after every site, bsel and both
    x, c, h = np.zeros((B, 2)), np.zeros((B, H)), np.zeros((B, H))
    hck, bsel, both = [], np.zeros((N, B)), np.zeros((N, B))
    for n in range(N):
        c, h = LR.lstm_step(x, c, h, K, b)
        sel, oth = both_terms(h, s[:, n])
        bsel[n], both[n] = sel, oth - sel
        hck.append((h, c))
        x = eye[s[:, n]]
    # trunks: states kept per (i, n)
    tck, tsel, toth, tail = [None] * max(NP, 1), np.zeros((max(NP, 1), B)), np.zeros((max(NP, 1), B)), np.zeros((max(NP, 1), B))
    for i in range(N - 1):
        h, c = hck[i]
        if defect == "c_from_h":
            c = h
        x = eye[1 - s[:, i]]
        for n in range(i + 1, N):
            p = pair_index(i, n, N)
            sig = spin(n)
            c, h = LR.lstm_step(x, c, h, K, b)
            tck[p] = (h, c)
            tsel[p], toth[p] = both_terms(h, sig)
            x = eye[sig]
    if defect == "trunk_from_base":
        for i in range(N - 1):
            for n in range(i + 1, N):
                tsel[pair_index(i, n, N)] = bsel[n]
    # branches
    for j in range(1, N - 1):
        for i in range(j):
            p = pair_index(i, j, N)
            src = tck[pair_index(i, j + 1, N)] if defect == "j_plus_one" and j + 1 <= N - 2 else tck[p]
            h, c = hck[j] if defect == "branch_from_hck" else src
            if defect == "c_from_h":
                c = h
            x = eye[1 - s[:, j]]
            lp = np.zeros(B)
            for n in range(j + 1, N):
                sig = spin(n)
                c, h = LR.lstm_step(x, c, h, K, b)
                lp += both_terms(h, sig)[0]
                x = eye[sig]
            tail[p] = lp
    # corr_suffix_kernel and corr_assemble_kernel, in their order of additions
    suf, acc = np.zeros((N, B)), np.zeros(B)
    for j in range(N - 1, -1, -1):
        suf[j] = acc
        acc = acc + bsel[j]
    lr = np.zeros((N + NP, B))
    for i in range(N):
        xb, mid = both[i], np.zeros(B)
        for j in range(i + 1, N):
            p = pair_index(i, j, N)
            v = (xb + mid) + (toth[p] - bsel[j])
            if j < N - 1 and defect != "dropped_tail":
                v = v + (tail[p] - suf[j])
            lr[N + p] = 0.5 * v
            mid = mid + (tsel[p] - bsel[j])
        lr[i] = 0.5 * (xb + mid)
    return lr


def product_state_log_ratios(prm, samples):
    """closed form with every kernel zero: the sites are independent, log p(s_n) = log_softmax(h0 Wd + bd) of the state h0 the biases
    alone produce - which still depends on how many steps the constant input has run, so the closed form is per site:
    log r_i = 1/2 [t_i(1-s_i) - t_i(s_i)], log r_ij = log r_i + log r_j"""
    K, b, Wd, bd = LR._unpack(prm, SCOPE)
    assert not K.any()
    s = np.asarray(samples).astype(np.int64)
    B, N = s.shape
    H = b.size // 4
    c, h = np.zeros((1, H)), np.zeros((1, H))
    d = np.zeros((N, B))
    for n in range(N):
        c, h = LR.lstm_step(np.zeros((1, 2)), c, h, K, b)
        ls = LR._log_softmax(h @ Wd + bd)[0]
        d[n] = 0.5 * (ls[1 - s[:, n]] - ls[s[:, n]])
    pi, pj = pair_list(N)
    return np.concatenate([d, d[pi] + d[pj]]) if N > 1 else d
