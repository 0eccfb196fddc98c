"""Float64 reference of the correlation estimators of rnnwf_correlations (docs/correlations.md), independent of the library: plain
NumPy on the oracle's GRU (oracle.models.prnn_log_probability).  TEST INFRASTRUCTURE ONLY; validated by
tests/test_correlations_reference.py.

    log r_i  = 1/2 [log P(sigma with i flipped)       - log P(sigma)]
    log r_ij = 1/2 [log P(sigma with i and j flipped) - log P(sigma)],   i < j

Brute force on purpose: every flipped configuration is written out in full and scored from site 0 - no prefix cancellation, no
checkpoint, no trunk shared between branches.  For the raster model the rows are raster-ordered spins.  Row order of a log-ratio
array everywhere: N rows log r_i, then log r_ij in lexicographic order of (i, j) (row_of).

Also here: the exact values from the dense vector of all 2^N amplitudes (exact_from_log_probs), the sums and statistics restated
(sums_from_log_ratio, stats_from_sums), the bounds of tests/test_gpu_correlations_full.py (f32_bound, f64_bound), the choice of the
checked chains and pairs (choose_subset, check_subset, subset_entries), the comparator, and the site-resolved form trunk / branch
with its defects (site_resolved), which only tests/test_correlations_reference.py uses to show what the bound rejects.
"""
import math

import numpy as np

from oracle import models as M
from renyi_reference import CHUNK, log_prob_other_order, site_log_probs, to32, to64

SCOPE = "RNNwavefunction"
FACTOR = 16.0          # f32: max |d log r| <= FACTOR x (f32 oracle's deviation from f64), the rule of test_gpu_gradient_full.py
BLOCK = 16             # chains per block of the kernels


def scorer(prm, dtype=np.float64):
    prm = to64(prm) if dtype == np.float64 else to32(prm)
    return lambda x: M.prnn_log_probability(prm, x, dtype=dtype)


def _chunked(log_p, x):
    return np.concatenate([log_p(x[k:k + CHUNK]) for k in range(0, len(x), CHUNK)]) if len(x) else np.zeros(0)


def pair_list(N):
    """(i, j) of every pair i < j, lexicographic: two int arrays of length N (N - 1) / 2."""
    i, j = np.triu_indices(N, 1)
    return i.astype(np.int64), j.astype(np.int64)


def row_of(i, j, N):
    """Row of log r_ij (j >= 0) or log r_i (j < 0) in a (N + N(N-1)/2, ns) log-ratio array."""
    i, j = np.asarray(i, dtype=np.int64), np.asarray(j, dtype=np.int64)
    return np.where(j < 0, i, N + i * (2 * N - i - 1) // 2 + (j - i - 1))


def log_ratio_entries(log_p, samples, chain, i, j):
    """log r of the entries e = (chain[e], i[e], j[e]); j[e] < 0: the single flip of site i[e].  float64 (E,)."""
    samples = np.asarray(samples)
    chain, i, j = (np.asarray(a, dtype=np.int64) for a in (chain, i, j))
    assert chain.shape == i.shape == j.shape and np.all((j < 0) | (j > i)) and np.all(i >= 0) and np.all(j < samples.shape[1])
    used = np.unique(chain)
    own = np.zeros(len(samples))
    own[used] = _chunked(log_p, samples[used])           # log P(sigma) of every chain that occurs, scored in full as well
    out = np.empty(len(chain))
    for k0 in range(0, len(chain), CHUNK):
        e = slice(k0, k0 + CHUNK)
        x = samples[chain[e]].copy()
        r = np.arange(len(x))
        x[r, i[e]] = 1 - x[r, i[e]]
        two = j[e] >= 0
        x[r[two], j[e][two]] = 1 - x[r[two], j[e][two]]
        out[e] = 0.5 * (log_p(x) - own[chain[e]])
    return out


def log_ratio_all(prm, samples, dtype=np.float64):
    """(N + N(N-1)/2, ns): every log r_i and log r_ij of every chain, cell arithmetic in `dtype`."""
    samples = np.asarray(samples)
    ns, N = samples.shape
    pi, pj = pair_list(N)
    ii = np.concatenate([np.arange(N), pi])
    jj = np.concatenate([np.full(N, -1), pj])
    c, r = np.meshgrid(np.arange(ns), np.arange(len(ii)), indexing="xy")
    return log_ratio_entries(scorer(prm, dtype), samples, c.ravel(), ii[r.ravel()], jj[r.ravel()]).reshape(len(ii), ns)


# ---- exact values from the dense vector --------------------------------------------------------------------------------------

def exact_from_log_probs(lp, N):
    """z (N,), zz (N, N), x (N,), xx (N, N) of psi = sqrt(P) / |sqrt(P)| from lp = log P over conftest.all_configs(N) (site 0 most
    significant): <psi| O |psi> with O written out on the basis states, sx flipping a bit of the configuration index."""
    psi = np.exp(0.5 * np.asarray(lp, dtype=np.float64))
    psi = psi / np.linalg.norm(psi)
    k = np.arange(2 ** N)
    s = 2.0 * ((k[:, None] >> np.arange(N)[::-1]) & 1) - 1.0
    p = psi * psi
    z = p @ s
    zz = (s * p[:, None]).T @ s
    mask = 1 << np.arange(N)[::-1]
    x = np.array([psi @ psi[k ^ mask[i]] for i in range(N)])
    xx = np.eye(N)
    for i in range(N):
        for j in range(i + 1, N):
            xx[i, j] = xx[j, i] = psi @ psi[k ^ mask[i] ^ mask[j]]
    return z, zz, x, xx


# ---- sums and statistics, written out again ----------------------------------------------------------------------------------

def sums_from_log_ratio(lr, N):
    """x_sums (N, 2) and xx_sums (N, N, 5) from a (N + N(N-1)/2, ns) log-ratio array, exactly rounded sums (math.fsum)."""
    r = np.exp(np.asarray(lr, dtype=np.float64))
    x = np.array([[math.fsum(r[i]), math.fsum(r[i] * r[i])] for i in range(N)])
    xx = np.zeros((N, N, 5))
    for i, j in zip(*pair_list(N)):
        q = r[row_of(i, j, N)]
        xx[i, j] = [math.fsum(q), math.fsum(q * q), math.fsum(q * r[i]), math.fsum(q * r[j]), math.fsum(r[i] * r[j])]
    return x, xx


def diag_sums(samples):
    """z_sums (N,), zz_sums (N, N) of s = 2 sigma - 1, in integers."""
    s = 2 * np.asarray(samples, dtype=np.int64) - 1
    return s.sum(axis=0).astype(np.float64), (s.T @ s).astype(np.float64)


def stats_from_sums(z_sums, zz_sums, x_sums, xx_sums, n):
    """The statistics of observables.correlations_from_sums, element by element from the per-chain definitions: the mean of a
    quantity q is sum q / n, its error sqrt((mean q^2 - (mean q)^2) / n); the connected functions are the means of
    g = a - mean(c) b - mean(b) c (a = the product, b and c = the factors) to first order, so their errors are those of g."""
    N = len(z_sums)
    n = float(n)
    out = {k: np.zeros((N, N)) for k in ("zz", "zz_err", "xx", "xx_err", "zz_c", "zz_c_err", "xx_c", "xx_c_err")}
    out.update({k: np.zeros(N) for k in ("z", "z_err", "x", "x_err")})

    def err(m1, m2):
        return math.sqrt(max(m2 - m1 * m1, 0.0) / n)

    for i in range(N):
        out["z"][i] = z_sums[i] / n
        out["z_err"][i] = err(out["z"][i], 1.0)
        out["x"][i] = x_sums[i][0] / n
        out["x_err"][i] = err(out["x"][i], x_sums[i][1] / n)
    for i in range(N):
        for j in range(N):
            zi, zj, xi, xj = out["z"][i], out["z"][j], out["x"][i], out["x"][j]
            zz = zz_sums[i][j] / n
            out["zz"][i, j] = zz
            out["zz_err"][i, j] = err(zz, 1.0)
            out["zz_c"][i, j] = zz - zi * zj
            if i == j:
                out["xx"][i, j] = 1.0
                out["xx_c"][i, j] = 1.0 - xi * xi
                out["zz_c_err"][i, j] = 2.0 * abs(zi) * out["z_err"][i]
                out["xx_c_err"][i, j] = 2.0 * abs(xi) * out["x_err"][i]
                continue
            # g = s_i s_j - z_j s_i - z_i s_j: g^2 expanded with s^2 = 1
            g1 = zz - 2.0 * zi * zj
            g2 = 1.0 + zj * zj + zi * zi - 2.0 * zj * zj - 2.0 * zi * zi + 2.0 * zi * zj * zz
            out["zz_c_err"][i, j] = err(g1, g2)
            a, b = min(i, j), max(i, j)
            m = [v / n for v in xx_sums[a][b]]
            xa, xb = out["x"][a], out["x"][b]
            ra2, rb2 = x_sums[a][1] / n, x_sums[b][1] / n
            out["xx"][i, j] = m[0]
            out["xx_err"][i, j] = err(m[0], m[1])
            out["xx_c"][i, j] = m[0] - xa * xb
            g1 = m[0] - 2.0 * xa * xb
            g2 = m[1] + xb * xb * ra2 + xa * xa * rb2 - 2.0 * xb * m[2] - 2.0 * xa * m[3] + 2.0 * xa * xb * m[4]
            out["xx_c_err"][i, j] = err(g1, g2)
    return out


# ---- bounds ------------------------------------------------------------------------------------------------------------------

def f32_ceiling(N):
    """log r is half the difference of two partial log-probabilities of at most N sites, each held to 2e-6 N + 2e-6 by
    tests/test_gpu_prnn.py: 1/2 x 2 x that."""
    return 2e-6 * N + 2e-6


def f32_bound(dev32, N):
    """(bound, capped): FACTOR x dev32, capped at f32_ceiling(N) - unless the f32 oracle itself (dev32) is beyond the ceiling, where
    FACTOR x dev32 stands uncapped."""
    cap = f32_ceiling(N)
    if dev32 > cap:
        return FACTOR * dev32, False
    return min(FACTOR * dev32, cap), FACTOR * dev32 > cap


def f64_bound(N):
    return 1e-11 * N


# ---- which chains and pairs a case checks ----------------------------------------------------------------------------------------

def boundary_pairs(N):
    """The pairs the `rest` chains are checked at: distance 1, distance N - 1, and pairs straddling each 32-site word boundary of
    the packed spins (i < 32 k <= j): (32k-1, 32k), (32k-2, 32k+1), (0, 32k), (32k-1, N-1), where they exist."""
    pairs = {(i, i + 1) for i in range(N - 1)}
    pairs.add((0, N - 1))
    for w in range(32, N, 32):
        for i, j in ((w - 1, w), (w - 2, w + 1), (0, w), (w - 1, N - 1)):
            if 0 <= i < w <= j < N:
                pairs.add((i, j))
    p = np.array(sorted(pairs), dtype=np.int64).reshape(-1, 2)
    return p[:, 0], p[:, 1]


def choose_subset(ns, n_all=32, n_rest=32, seed=0):
    """(chains checked at every pair, chains checked at the boundary pairs), disjoint.  The first list holds >= n_all chains: eight
    from each of the first, a middle and the last full 16-chain block (lanes 0, 1, 5, 6, 10, 11, 14, 15), every chain of the ragged
    last block, the rest at random; the second n_rest further chains at random."""
    nfull = ns // BLOCK
    assert nfull >= 3
    blocks = [0, nfull // 2, nfull - 1]
    every = [b * BLOCK + k for b in blocks for k in (0, 1, 5, 6, 10, 11, 14, 15)] + list(range(nfull * BLOCK, ns))
    free = np.array(sorted(set(range(ns)) - set(every)))
    need = max(0, n_all - len(every))
    n_rest = min(n_rest, len(free) - need)
    extra = np.random.RandomState(seed).choice(free, size=need + n_rest, replace=False).tolist()
    every += extra[:need]
    return np.array(sorted(every), dtype=np.int64), np.array(sorted(extra[need:]), dtype=np.int64)


def check_subset(ns, N, every, rest, rest_i, rest_j):
    """The conditions a case's subset must meet, asserted (not only intended)."""
    nfull = ns // BLOCK
    both = np.concatenate([every, rest])
    assert len(set(both.tolist())) == len(both) and both.min() >= 0 and both.max() < ns
    assert len(every) >= 32
    blk = every // BLOCK
    for b in (0, nfull - 1):
        assert np.any(blk == b), "no chain from block %d" % b
    assert np.any((blk > 0) & (blk < nfull - 1)), "no chain from a middle block"
    assert set(range(nfull * BLOCK, ns)) <= set(every.tolist()), "a chain of the ragged last block is missing"
    have = set(zip(np.asarray(rest_i).tolist(), np.asarray(rest_j).tolist()))
    assert {(i, i + 1) for i in range(N - 1)} <= have and (0, N - 1) in have
    for w in range(32, N, 32):
        assert any(i < w <= j for i, j in have), "no pair straddles the word boundary at %d" % w
        assert (w - 1, w) in have


def subset_entries(N, every, rest):
    """Entry lists (chain, i, j): `every` x (all singles and pairs), then `rest` x (all singles and boundary_pairs(N))."""
    pi, pj = pair_list(N)
    bi, bj = boundary_pairs(N)
    one = np.arange(N)
    ii1, jj1 = np.concatenate([one, pi]), np.concatenate([np.full(N, -1), pj])
    ii2, jj2 = np.concatenate([one, bi]), np.concatenate([np.full(N, -1), bj])
    c1, r1 = np.meshgrid(every, np.arange(len(ii1)), indexing="ij")
    c2, r2 = np.meshgrid(rest, np.arange(len(ii2)), indexing="ij")
    return (np.concatenate([c1.ravel(), c2.ravel()]), np.concatenate([ii1[r1.ravel()], ii2[r2.ravel()]]),
            np.concatenate([jj1[r1.ravel()], jj2[r2.ravel()]]))


def compare(label, got, ref, chain, i, j, bound, echo=print):
    """max |got - ref| over the entries, where it occurs and its ratio to `bound`."""
    d = np.abs(np.asarray(got) - np.asarray(ref))
    k = int(np.argmax(d))
    res = dict(err=float(d[k]), chain=int(chain[k]), i=int(i[k]), j=int(j[k]), block=int(chain[k]) // BLOCK, bound=float(bound),
               ratio=float(d[k] / bound), entries=len(d), finite=bool(np.all(np.isfinite(got))))
    echo("%s max |d log r| = %.3e at (i, j) = (%d, %d), chain %d (block %d, lane %d) over %d entries; bound %.3e; ratio %.3f"
         % (label, res["err"], res["i"], res["j"], res["chain"], res["block"], res["chain"] % BLOCK, res["entries"], bound, res["ratio"]))
    return res


def nontrivial(ref):
    """(max |log r|, share of entries with |log r| > 0.01): a case requires > 0.1 and >= 1/4."""
    a = np.abs(ref)
    return float(a.max()), float(np.mean(a > 0.01))


# ---- the site-resolved form and its defects, for tests/test_correlations_reference.py -----------------------------------------------

def site_resolved(prm, samples, i, j, dtype=np.float64, defect=None):
    """log r_ij of every chain by the kernels' decomposition (docs/correlations.md), from three teacher-forced evaluations: the
    base chain t, trunk i (spin i flipped) t', branch (i, j) (both flipped) t'':
        2 log r_ij = [t_i(1-s_i) - t_i(s_i)] + sum_{i<n<j} [t'_n - t_n] + [t'_j(1-s_j) - t_j(s_j)] + sum_{n>j} [t''_n - t_n]
    defect: None, or one mistake a kernel could make -
        "trunk_from_base": sites i+1..j-1 taken from the base chain (the middle sum dropped);
        "dropped_tail":    the sum over n > j dropped;
        "word0":           the teacher-forced spins of sites n >= 32 read from the first spin word (spin n & 31) in trunk and branch."""
    x = np.asarray(samples)
    r = np.arange(len(x))
    fed = x.copy()
    if defect == "word0":
        fed[:, 32:] = x[:, np.arange(32, x.shape[1]) & 31]
    xi = fed.copy()
    xi[:, i] = 1 - x[:, i]
    xij = xi.copy()
    xij[:, j] = 1 - x[:, j]
    prm = to64(prm) if dtype == np.float64 else to32(prm)
    p0 = np.log(M.prnn_site_probs(prm, x, SCOPE, dtype).astype(np.float64))
    p1 = np.log(M.prnn_site_probs(prm, xi, SCOPE, dtype).astype(np.float64))
    p2 = np.log(M.prnn_site_probs(prm, xij, SCOPE, dtype).astype(np.float64))
    sel = lambda p, n, v: p[r, n, v]
    out = sel(p0, i, 1 - x[:, i]) - sel(p0, i, x[:, i])
    if defect != "trunk_from_base":
        for n in range(i + 1, j):
            out += sel(p1, n, x[:, n]) - sel(p0, n, x[:, n])
    out += sel(p1, j, 1 - x[:, j]) - sel(p0, j, x[:, j])
    if defect != "dropped_tail":
        for n in range(j + 1, x.shape[1]):
            out += sel(p2, n, x[:, n]) - sel(p0, n, x[:, n])
    return 0.5 * out


def log_ratio_other_order(prm, samples, i, j):
    """log r_ij of every chain from a float32 GRU whose gate sums run in another order (renyi_reference.log_prob_other_order)."""
    x = np.asarray(samples)
    y = x.copy()
    y[:, i] = 1 - y[:, i]
    y[:, j] = 1 - y[:, j]
    return 0.5 * (log_prob_other_order(prm, y) - log_prob_other_order(prm, x))
