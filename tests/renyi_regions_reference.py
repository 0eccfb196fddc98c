"""Float64 reference of the swap estimator of the second Renyi entropy for ARBITRARY regions (docs/renyi_regions.md), independent of
the library: plain NumPy on the oracle's GRU (oracle.models.prnn_log_probability).  TEST INFRASTRUCTURE ONLY; validated by
tests/test_renyi_regions_reference.py.

    log r_A(sigma, tau) = 1/2 [log P(tau_A sigma_B) + log P(sigma_A tau_B) - log P(sigma) - log P(tau)],   A = any set of sites (a mask)

Brute force on purpose: both swapped configurations of every (pair, region) are written out in full and scored from site 0 - no
normalisation to "site 0 not in A", no first site, no prefix reuse, no checkpoint, no pairing by lane, no packed words.

Also here: the exact purity of a region from the dense state vector (purity_of_region), the region set and the chain subset a
full-size case checks (region_set, choose_pairs, check_subset), and the site-resolved form the kernels use, restated with switches
for the defects tests/test_renyi_regions_reference.py shows the bound to reject (mixed_chain_form).  The bounds, the comparator and the
sums are those of tests/renyi_reference.py.
"""
import numpy as np

import renyi_reference as R

BLOCK = R.BLOCK


def log_ratio_regions(log_p, pairs, masks, pair_idx=None):
    """(len(masks), len(pair_idx)) log r_A, float64.  pairs: (2 npairs, N) spins, pair p = rows 2p, 2p + 1; masks: (R, N) of 0 / 1;
    log_p scores (B, N) configurations.  Every region, the empty and the full one included, takes the same path."""
    pairs, masks = np.asarray(pairs), np.asarray(masks)
    pair_idx = np.arange(len(pairs) // 2) if pair_idx is None else np.asarray(pair_idx, dtype=np.int64)
    assert masks.ndim == 2 and masks.shape[1] == pairs.shape[1] and np.all((masks == 0) | (masks == 1))
    sigma, tau = pairs[2 * pair_idx], pairs[2 * pair_idx + 1]
    own = R._chunked(log_p, sigma) + R._chunked(log_p, tau)
    out = np.empty((len(masks), len(pair_idx)))
    for k, m in enumerate(masks):
        in_a = m.astype(bool)[None, :]
        a = np.where(in_a, tau, sigma)               # tau_A sigma_B
        b = np.where(in_a, sigma, tau)               # sigma_A tau_B
        lp = R._chunked(log_p, np.concatenate([a, b]))
        out[k] = 0.5 * (lp[:len(a)] + lp[len(a):] - own)
    return out


def log_ratio(prm, pairs, masks, dtype=np.float64, pair_idx=None):
    prm = R.to64(prm) if dtype == np.float64 else R.to32(prm)
    return log_ratio_regions(R._scorer(prm, dtype), pairs, masks, pair_idx)


def purity_of_region(psi, N, mask):
    """Tr rho_A^2 of the state psi over conftest.all_configs(N) (site 0 most significant), normalised here, for the sites with
    mask = 1: A's axes moved to the front, the matrix reshaped to (2^|A|, 2^|B|), rho_A = M M^T taken directly."""
    sites = [n for n in range(N) if mask[n]]
    rest = [n for n in range(N) if not mask[n]]
    psi = np.asarray(psi, dtype=np.float64)
    t = (psi / np.linalg.norm(psi)).reshape((2,) * N).transpose(sites + rest).reshape(2 ** len(sites), -1)
    rho = t @ t.T
    return float(np.sum(rho * rho))


# ---- regions and chains of a full-size case ------------------------------------------------------------------------------------------

def _interval(N, a, b):
    m = np.zeros(N, dtype=np.int32)
    m[a:b] = 1
    return m


def _rect(Nx, Ny, x0, x1, y0, y1):
    m = np.zeros((Ny, Nx), dtype=np.int32)
    m[y0:y1, x0:x1] = 1
    return m.reshape(-1)


def region_set(Nx, Ny):
    """[(name, mask)] of a full-size case on Nx x Ny raster sites (Ny = 1: a chain), masks written out here (not by the library's
    builders): all column cuts and corner / bulk squares (2D); bulk intervals; intervals that end or start on each 32-site word
    boundary of the packed spins; a two-piece region; a checkerboard."""
    N = Nx * Ny
    out = []
    if Ny > 1:
        for c in range(1, Nx):
            out.append(("columns < %d" % c, _rect(Nx, Ny, 0, c, 0, Ny)))
        L = max(2, min(Nx, Ny) // 2)
        out.append(("corner %dx%d at (0,0)" % (L, L), _rect(Nx, Ny, 0, L, 0, L)))
        out.append(("corner %dx%d at the far end" % (L, L), _rect(Nx, Ny, Nx - L, Nx, Ny - L, Ny)))
        out.append(("corner %dx%d top right" % (L, L), _rect(Nx, Ny, Nx - L, Nx, 0, L)))
        if Nx >= 4 and Ny >= 4:
            out.append(("bulk 2x2", _rect(Nx, Ny, Nx // 2 - 1, Nx // 2 + 1, Ny // 2 - 1, Ny // 2 + 1)))
        out.append(("two blocks", _rect(Nx, Ny, 0, 1, 0, 2) | _rect(Nx, Ny, Nx - 1, Nx, Ny - 2, Ny)))
        yy, xx = np.divmod(np.arange(N), Nx)
        out.append(("checkerboard", ((xx + yy) & 1).astype(np.int32)))
    else:
        out.append(("checkerboard", (np.arange(N) & 1).astype(np.int32)))
    out.append(("every third site", (np.arange(N) % 3 == 1).astype(np.int32)))
    out.append(("interval N/4..N/2", _interval(N, N // 4, N // 2)))
    out.append(("interval 1..N-1", _interval(N, 1, N - 1)))
    out.append(("interval N/2..N/2+3", _interval(N, N // 2, min(N, N // 2 + 3))))
    out.append(("site N-1", _interval(N, N - 1, N)))
    for w in range(32, N, 32):                                  # word boundaries of the packed spins and masks
        out.append(("interval %d..%d (ends on a word)" % (w - 5, w), _interval(N, w - 5, w)))
        out.append(("interval %d..%d (starts on a word)" % (w, min(N, w + 5)), _interval(N, w, min(N, w + 5))))
        out.append(("interval %d..%d (across a word)" % (w - 1, w + 1), _interval(N, w - 1, w + 1)))
    out.append(("two pieces", _interval(N, 1, max(2, N // 5)) | _interval(N, (3 * N) // 4, N - 1)))
    out.append(("site 0 and the last third", _interval(N, 0, 1) | _interval(N, (2 * N) // 3, N)))     # normalised by the library
    return out


def word_boundaries_covered(N, masks):
    """Every 32-site word boundary w < N has an interval (one run of sites) that ends at w and one that starts at w."""
    runs = set()
    for m in np.asarray(masks):
        nz = np.flatnonzero(m)
        if len(nz) and nz[-1] - nz[0] + 1 == len(nz):
            runs.add((int(nz[0]), int(nz[-1]) + 1))
    return all(any(b == w for _, b in runs) and any(a == w for a, _ in runs) for w in range(32, N, 32))


def choose_pairs(npairs):
    """All 8 pairs of the first, a middle and the last full 16-chain block and every pair of the ragged last block; filled up at
    random (fixed seed) to at least 32."""
    per = BLOCK // 2
    nfull = (2 * npairs) // BLOCK
    assert nfull >= 3
    idx = set(range(nfull * per, npairs))
    for b in (0, nfull // 2, nfull - 1):
        idx.update(range(b * per, (b + 1) * per))
    free = np.array(sorted(set(range(npairs)) - idx))
    need = max(0, 32 - len(idx))
    idx.update(np.random.RandomState(0).choice(free, size=need, replace=False).tolist())
    return np.array(sorted(idx), dtype=np.int64)


def check_subset(npairs, N, pair_idx, masks):
    """The conditions a case's subset must meet, asserted (not only intended)."""
    per, nfull = BLOCK // 2, (2 * npairs) // BLOCK
    pair_idx = np.asarray(pair_idx)
    assert len(set(pair_idx.tolist())) == len(pair_idx) >= 32 and pair_idx.min() >= 0 and pair_idx.max() < npairs
    have = set(pair_idx.tolist())
    for b in (0, nfull - 1):
        assert set(range(b * per, (b + 1) * per)) <= have, "block %d is not complete" % b
    blk = pair_idx // per
    middle = [b for b in range(1, nfull - 1) if np.sum(blk == b) == per]
    assert middle, "no complete middle block"
    assert set(range(nfull * per, npairs)) <= have, "a pair of the ragged last block is missing"
    assert word_boundaries_covered(N, masks), "a word boundary has no interval ending or starting on it"


# ---- the site-resolved form of the kernels, with defects -----------------------------------------------------------------------------

def normalise(mask):
    """(mask with site 0 not in A - complemented when mask[0] == 1; f = its first site, 0 when it is empty)."""
    m = np.asarray(mask).astype(np.int64)
    m = m ^ m[0]
    nz = np.flatnonzero(m)
    return m, (int(nz[0]) if len(nz) else 0)


def mixed_chain_form(prm, pairs, masks, defect=None, dtype=np.float64):
    """log r_A = 1/2 [(tail_sigma - suffix_sigma) + (tail_tau - suffix_tau)] as renyi_region_kernels.h computes it: the mask
    normalised, f its first site, the mixed chain m_n = (n in A ? partner : own), tail = sum_{n >= f} log p(m_n | m_<n), suffix the
    chain's own terms from f.  (R, npairs).  defect names one deliberate error:
      "own_on_A"            own instead of the partner's spins on A
      "partner_after_f"     the partner's spins taken at every site >= f
      "mask_word_0"         the mask word of sites >= 32 read from word 0 (mask[n & 31] for mask[n])
      "partner_checkpoint"  restart from the PARTNER's state before site f (its spins 0..f-2), fed the chain's own spin f-1
    """
    pairs = np.asarray(pairs)
    sigma, tau = pairs[0::2], pairs[1::2]
    N = pairs.shape[1]
    prm = R.to64(prm) if dtype == np.float64 else R.to32(prm)
    own_s, own_t = R.site_log_probs(prm, sigma, dtype), R.site_log_probs(prm, tau, dtype)
    out = np.zeros((len(masks), len(sigma)))
    for k, mask in enumerate(masks):
        m, f = normalise(mask)
        if f == 0:
            continue
        if defect == "partner_after_f":
            m = (np.arange(N) >= f).astype(np.int64)
        elif defect == "mask_word_0":
            m = m[np.arange(N) & 31]
        elif defect == "own_on_A":
            m = np.zeros(N, dtype=np.int64)
        in_a = m.astype(bool)[None, :]
        mix_s, mix_t = np.where(in_a, tau, sigma), np.where(in_a, sigma, tau)
        if defect == "partner_checkpoint":
            mix_s[:, :f - 1], mix_t[:, :f - 1] = tau[:, :f - 1], sigma[:, :f - 1]
        ts = R.site_log_probs(prm, mix_s, dtype)[:, f:].sum(axis=1)
        tt = R.site_log_probs(prm, mix_t, dtype)[:, f:].sum(axis=1)
        out[k] = 0.5 * ((ts - own_s[:, f:].sum(axis=1)) + (tt - own_t[:, f:].sum(axis=1)))
    return out
