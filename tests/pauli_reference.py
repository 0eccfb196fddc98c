"""Float64 / float32 reference of the Pauli-string estimator (docs/pauli.md), independent of the library: plain NumPy on the oracle's
GRU (oracle.models.prnn_log_probability).  TEST INFRASTRUCTURE ONLY; validated by tests/test_pauli_reference.py.

    O = (prod_{i in S} sz_i)(prod_{i in F} sx_i),   v(sigma) = prod_{i in S} (2 sigma_i - 1) * exp(1/2 [log P(sigma ^ F) - log P(sigma)])

Brute force on purpose: every flipped configuration is written out in full and scored from site 0 - no first site, no checkpoint, no
grouping by mask, no packed words.  Dense operators are Kronecker products over conftest.all_configs's basis (site 0 most
significant, sigma = 0 <-> s = -1), for N <= 10.

Also here: the mask set and chain subset of a full-size case (mask_set, choose_chains, check_subset), and the site-resolved form the
kernels use, restated with switches for the defects tests/test_pauli_reference.py shows the bounds to reject (kernel_form).  Bounds,
comparator and the other-order float32 evaluation are those of tests/renyi_reference.py / tests/correlations_reference.py.
"""
import math

import numpy as np

import correlations_reference as C
import renyi_reference as R

BLOCK = R.BLOCK

I2 = np.eye(2)
SX = np.array([[0.0, 1.0], [1.0, 0.0]])
SZ = np.array([[-1.0, 0.0], [0.0, 1.0]])          # sigma = 0 <-> s = -1
SY = -1j * SZ @ SX
PAULI = {"I": I2, "X": SX, "Y": SY, "Z": SZ}


def dense_string(letters, N):
    """The 2^N x 2^N matrix of a Pauli string given as {site: letter} or a dense "XZIY..." (complex when it holds a Y)."""
    if isinstance(letters, str):
        letters = {i: c for i, c in enumerate(letters) if c != "I"}
    out = np.ones((1, 1), dtype=np.complex128)
    for i in range(N):
        out = np.kron(out, PAULI[letters.get(i, "I")])
    return out


def dense_term(flip, sign):
    """(prod_{sign} sz)(prod_{flip} sx) as a real dense matrix, sz to the left."""
    N = len(flip)
    z = dense_string({i: "Z" for i in range(N) if sign[i]}, N).real
    x = dense_string({i: "X" for i in range(N) if flip[i]}, N).real
    return z @ x


def log_ratio_masks(log_p, samples, masks, idx=None):
    """(len(masks), len(idx)) 1/2 [log P(sigma ^ F) - log P(sigma)], float64; samples (ns, N), masks (M, N) of 0 / 1."""
    samples, masks = np.asarray(samples), np.asarray(masks)
    idx = np.arange(len(samples)) if idx is None else np.asarray(idx, dtype=np.int64)
    assert masks.ndim == 2 and masks.shape[1] == samples.shape[1] and np.all((masks == 0) | (masks == 1))
    x = samples[idx]
    own = R._chunked(log_p, x)
    return np.stack([0.5 * (R._chunked(log_p, x ^ m[None, :].astype(x.dtype)) - own) for m in masks]) if len(masks) else np.zeros((0, len(idx)))


def log_ratio(prm, samples, masks, dtype=np.float64, idx=None):
    prm = R.to64(prm) if dtype == np.float64 else R.to32(prm)
    return log_ratio_masks(R._scorer(prm, dtype), samples, masks, idx)


def signs(samples, sign):
    """(K, ns) prod_{i in S_k} (2 sigma_i - 1) of the SAMPLED configurations."""
    s = 2.0 * np.asarray(samples, dtype=np.float64) - 1.0
    return np.stack([np.prod(np.where(np.asarray(m, dtype=bool)[None, :], s, 1.0), axis=1) for m in sign])


def local_values(log_p, samples, flip, sign):
    """(K, ns) v_k(sigma), every term on its own (no grouping)."""
    return signs(samples, sign) * np.exp(log_ratio_masks(log_p, samples, flip))


def local_energy(log_p, samples, flip, sign, coeff):
    return np.asarray(coeff, dtype=np.float64) @ local_values(log_p, samples, flip, sign)


def sums_from_values(v):
    """(K, 2): exactly rounded sums of v and v^2 per row."""
    return np.array([[math.fsum(row), math.fsum(row * row)] for row in np.asarray(v, dtype=np.float64)])


# ---- masks and chains of a full-size case -----------------------------------------------------------------------------------------

def _sites(N, sites):
    m = np.zeros(N, dtype=np.int32)
    m[list(sites)] = 1
    return m


def mask_set(Nx, Ny):
    """[(name, mask)] of a full-size case on Nx x Ny raster sites (Ny = 1: a chain): single sites, nearest-neighbour and long-range
    pairs, a five-site string straddling each 32-site word boundary, a checkerboard, site 0 and the full mask."""
    N = Nx * Ny
    out = [("site 0", _sites(N, [0])), ("site %d" % (N - 1), _sites(N, [N - 1])), ("site %d" % (N // 2), _sites(N, [N // 2])),
           ("site 1", _sites(N, [1])), ("pair 0,1", _sites(N, [0, 1])), ("pair %d,%d" % (N // 2, N // 2 + 1), _sites(N, [N // 2, N // 2 + 1])),
           ("pair %d,%d" % (N - 2, N - 1), _sites(N, [N - 2, N - 1])), ("pair 0,%d" % (N - 1), _sites(N, [0, N - 1])),
           ("pair 1,%d" % (N - 2), _sites(N, [1, N - 2])), ("pair %d,%d" % (N // 4, (3 * N) // 4), _sites(N, [N // 4, (3 * N) // 4]))]
    for w in range(32, N, 32):
        lo, hi = w - 2, min(N, w + 3)
        out.append(("string %d..%d (straddles word boundary %d)" % (lo, hi - 1, w), _sites(N, range(lo, hi))))
        out.append(("site %d (last of a word)" % (w - 1), _sites(N, [w - 1])))
        out.append(("site %d (first of a word)" % w, _sites(N, [w])))
    if Ny > 1:
        yy, xx = np.divmod(np.arange(N), Nx)
        out.append(("checkerboard", ((xx + yy) & 1).astype(np.int32)))
        out.append(("pair above / below", _sites(N, [N // 2, N // 2 - Nx])))
    else:
        out.append(("checkerboard", (np.arange(N) & 1).astype(np.int32)))
    out.append(("checkerboard with site 0", ((np.arange(N) + 1) & 1).astype(np.int32)))
    out.append(("full", np.ones(N, dtype=np.int32)))
    seen, distinct = set(), []                       # small lattices repeat a mask under two names: the first stays
    for name, m in out:
        if m.tobytes() not in seen:
            seen.add(m.tobytes())
            distinct.append((name, m))
    return distinct


def word_boundaries_covered(N, masks):
    """Every 32-site word boundary w < N has a mask that is one run of sites with both w - 1 and w in it."""
    ok = []
    for w in range(32, N, 32):
        hit = False
        for m in np.asarray(masks):
            nz = np.flatnonzero(m)
            if len(nz) >= 2 and nz[-1] - nz[0] + 1 == len(nz) and len(nz) < N and nz[0] < w <= nz[-1]:
                hit = True
        ok.append(hit)
    return all(ok)


def choose_chains(ns):
    """All 16 chains of the first, a middle and the last full 16-chain block and every chain of the ragged last block; filled up at
    random (fixed seed) to at least 32."""
    nfull = ns // BLOCK
    assert nfull >= 3
    idx = set(range(nfull * BLOCK, ns))
    for b in (0, nfull // 2, nfull - 1):
        idx.update(range(b * BLOCK, (b + 1) * BLOCK))
    free = np.array(sorted(set(range(ns)) - idx))
    need = max(0, 32 - len(idx))
    idx.update(np.random.RandomState(0).choice(free, size=need, replace=False).tolist())
    return np.array(sorted(idx), dtype=np.int64)


def check_subset(ns, N, idx, masks):
    """The conditions a case's subset must meet, asserted (not only intended): >= 32 chains, each checked on every mask."""
    nfull = ns // BLOCK
    idx = np.asarray(idx)
    assert len(set(idx.tolist())) == len(idx) >= 32 and idx.min() >= 0 and idx.max() < ns
    have = set(idx.tolist())
    for b in (0, nfull - 1):
        assert set(range(b * BLOCK, (b + 1) * BLOCK)) <= have, "block %d is not complete" % b
    blk = idx // BLOCK
    assert [b for b in range(1, nfull - 1) if np.sum(blk == b) == BLOCK], "no complete middle block"
    assert set(range(nfull * BLOCK, ns)) <= have, "a chain of the ragged last block is missing"
    masks = np.asarray(masks)
    assert word_boundaries_covered(N, masks), "a word boundary has no string straddling it"
    firsts = {int(np.flatnonzero(m)[0]) for m in masks}
    assert 0 in firsts and N - 1 in firsts and np.any(masks.sum(axis=1) == N), "site 0, site N-1 or the full mask is missing"


# ---- the site-resolved form of the kernels, with defects -----------------------------------------------------------------------------

def kernel_form(prm, samples, masks, defect=None, dtype=np.float64):
    """1/2 (tail - suffix) as pauli_kernels.h computes it: f = the first flipped site, tail = sum_{n >= f} log p((sigma ^ F)_n | ...),
    suffix the chain's own terms from f.  (M, ns).  defect names one deliberate error:
      "mask_shifted"   every mask shifted by one site (site n flipped where n - 1 was asked; the last site drops out)
      "mask_word_0"    the mask word of sites >= 32 read from word 0 (mask[n & 31] for mask[n])
      "checkpoint_f"   restart from the state before site f + 1 (the chain's own spins 0..f-1 AND f fed), then the flipped spins f..
    """
    samples = np.asarray(samples)
    N = samples.shape[1]
    prm = R.to64(prm) if dtype == np.float64 else R.to32(prm)
    own = R.site_log_probs(prm, samples, dtype)
    out = np.zeros((len(masks), len(samples)))
    for k, mask in enumerate(masks):
        m = np.asarray(mask).astype(samples.dtype)
        f = int(np.flatnonzero(m)[0])                  # of the mask that was asked for: the restart point
        if defect == "mask_shifted":
            m = np.concatenate([[0], m[:-1]]).astype(samples.dtype)
        elif defect == "mask_word_0":
            m = m[np.arange(N) & 31]
        x = samples ^ m[None, :]
        if defect == "checkpoint_f" and f < N - 1:
            # inputs: own spins 0..f (state before site f + 1), then spin f - 1's slot is taken by the flipped chain from f on
            y = np.concatenate([samples[:, :f + 1], x[:, f:]], axis=1)          # N + 1 sites; its sites f+1.. are the chain's f..
            tail = R.site_log_probs(prm, y, dtype)[:, f + 1:].sum(axis=1)
        else:
            tail = R.site_log_probs(prm, x, dtype)[:, f:].sum(axis=1)
        out[k] = 0.5 * (tail - own[:, f:].sum(axis=1))
    return out


def log_ratio_other_order(prm, samples, masks):
    """float32, every gate sum in another order (renyi_reference.log_prob_other_order): what the bound must accept."""
    samples = np.asarray(samples)
    p32 = R.to32(prm)
    own = R.log_prob_other_order(p32, samples)
    return np.stack([0.5 * (R.log_prob_other_order(p32, samples ^ np.asarray(m).astype(samples.dtype)[None, :]) - own) for m in masks])


f32_ceiling = C.f32_ceiling
f32_bound = C.f32_bound
f64_bound = C.f64_bound
