"""What tests/test_lstm_pauli_host.py and tests/test_gpu_lstm_pauli.py share: the cases of the LSTM's Pauli pass (rnnwf_pauli_step_lstm,
docs/pauli_lstm.md) and a NumPy float64 restatement of the bookkeeping of csrc/lstm_pauli_kernels.h - checkpoints (h, c) after every
site, packed spin and mask words, restart at the first flipped site - with switches for three deliberate defects.  TEST
INFRASTRUCTURE ONLY.  The yardstick itself is brute force: tests/pauli_reference.log_ratio_masks on tests/lstm_reference's log P, every
flipped configuration scored from site 0.
"""
import numpy as np

import lstm_grad_reference as LG
import lstm_reference as LR
import pauli_reference as PR

SCOPE = LG.SCOPE
NS = 40                                                   # two full 16-chain blocks and a ragged one of 8
WIDTHS = (10, 17, 21, 36, 37, 52, 53, 68)                 # NFULL 1, 1, 2, 2, 3, 3, 4, 4
LATTICES = ((2, 1), (3, 3), (4, 3), (11, 3), (7, 5), (3, 22))      # 2 .. 66 sites: one, two and three spin words
DEFECTS = ("checkpoint_f", "c_from_h", "mask_word_0")


def bound(N):
    """the project's float64 bound on a log-ratio (docs/pauli.md, docs/renyi_regions.md)"""
    return 1e-11 * N


def parameters(units):
    return LG.parameters(units)


def log_p(prm, Nx, Ny):
    return lambda s: LR.lstm_log_probability(prm, s, Nx, Ny, scope=SCOPE)


def site_mask(N, sites):
    m = np.zeros(N, dtype=np.int32)
    m[list(sites)] = 1
    return m


def masks_of(Nx, Ny):
    """pauli_reference.mask_set plus, by hand: site 0 alone, site N-1 alone, {31, 32} and {63, 64} where they exist, all sites"""
    N = Nx * Ny
    # mask_set names sites up to N // 2 + 1: on two sites the three masks by hand are every non-empty mask
    out = [m for _, m in PR.mask_set(Nx, Ny)] if N >= 3 else []
    out += [site_mask(N, [0]), site_mask(N, [N - 1]), site_mask(N, range(N))]
    out += [site_mask(N, [w - 1, w]) for w in (32, 64) if w < N]
    seen, distinct = set(), []
    for m in out:
        if m.tobytes() not in seen:
            seen.add(m.tobytes())
            distinct.append(m)
    return np.stack(distinct)


def samples_of(Nx, Ny, units):
    return np.random.RandomState(1000 * Nx * Ny + units).randint(0, 2, size=(NS, Nx * Ny)).astype(np.int32)


def _words(rows):
    """(B, N) 0 / 1 -> (B, W) packed words: site n = bit n & 31 of word n >> 5"""
    rows = np.asarray(rows, dtype=np.uint64)
    B, N = rows.shape
    W = (N + 31) // 32
    out = np.zeros((B, W), dtype=np.uint64)
    for n in range(N):
        out[:, n >> 5] |= rows[:, n] << np.uint64(n & 31)
    return out


def kernel_form(prm, samples, masks, defect=None):
    """1/2 (tail - suffix), (M, ns), as lstm_site_terms_kernel, lstm_masked_tail_kernel and pauli_log_ratio_kernel compute it.
    defect names one deliberate error:
      "checkpoint_f"   restart from the checkpoint of site f instead of f - 1 (the chain's own spin f - 1 still fed)
      "c_from_h"       the cell state restored from h's rows of the checkpoint
      "mask_word_0"    the mask words of sites >= 32 read from word 0
    """
    assert defect in (None,) + DEFECTS
    K, b, Wd, bd = LR._unpack(prm, SCOPE)
    s = np.asarray(samples).astype(np.int64)
    B, N = s.shape
    H = b.size // 4
    eye = np.eye(2)
    rows = np.arange(B)
    # base pass: checkpoints after every site, the site terms
    x, c, h = np.zeros((B, 2)), np.zeros((B, H)), np.zeros((B, H))
    ck_h, ck_c, terms = [], [], np.zeros((N, B))
    for n in range(N):
        c, h = LR.lstm_step(x, c, h, K, b)
        terms[n] = LR._log_softmax(h @ Wd + bd)[rows, s[:, n]]
        ck_h.append(h)
        ck_c.append(c)
        x = eye[s[:, n]]
    own_words = _words(s)
    out = np.zeros((len(masks), B))
    for k, mask in enumerate(np.asarray(masks)):
        f = int(np.flatnonzero(mask)[0])
        mw = _words(mask[None, :])[0]
        if defect == "mask_word_0":
            mw = np.full_like(mw, mw[0])
        if f > 0:
            g = min(f, N - 2) if defect == "checkpoint_f" else f - 1
            h = ck_h[g]
            c = ck_h[f - 1] if defect == "c_from_h" else ck_c[g]
            x = eye[s[:, f - 1]]
        else:
            x, c, h = np.zeros((B, 2)), np.zeros((B, H)), np.zeros((B, H))
        tail = np.zeros(B)
        for n in range(f, N):
            spin = (((own_words[:, n >> 5] ^ mw[n >> 5]) >> np.uint64(n & 31)) & np.uint64(1)).astype(np.int64)
            c, h = LR.lstm_step(x, c, h, K, b)
            tail += LR._log_softmax(h @ Wd + bd)[rows, spin]
            x = eye[spin]
        own = np.zeros(B)
        for n in range(f, N):
            own += terms[n]
        out[k] = 0.5 * (tail - own)
    return out
