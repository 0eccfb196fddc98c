"""Float64 reference of the swap estimator of the second Renyi entropy (docs/renyi.md), independent of the library: plain NumPy on
the oracle's GRU (oracle.models.prnn_log_probability).  TEST INFRASTRUCTURE ONLY; validated by tests/test_renyi_reference.py.

    log r_l(sigma, tau) = 1/2 [log P(tau_A sigma_B) + log P(sigma_A tau_B) - log P(sigma) - log P(tau)],   A = the first l sites

Brute force on purpose: both swapped configurations of every (pair, cut) are written out in full and scored from site 0 - no prefix
reuse, no checkpoint, no pairing by lane, none of the kernels' shortcuts.  For the raster model the rows are raster-ordered spins and
the cut counts raster sites.  The scoring is chunked (CHUNK configurations at a time), so peak memory stays at a few dozen MB.

Also here: the sums and statistics restated (sums_from_log_ratio, entropy_from_sums), the bounds of tests/test_gpu_renyi_full.py
(f32_bound, f64_bound), the choice of the checked pairs and cuts (choose_subset), the comparator (compare), and two further
restatements that only tests/test_renyi_reference.py uses to show what the bound rejects and accepts: the site-resolved form
tail - suffix (tails_and_suffixes) and a float32 GRU whose gate and candidate sums run in another order (log_prob_other_order).
"""
import math

import numpy as np

from oracle import models as M
from test_renyi_host import swap_log_ratio

SCOPE = "RNNwavefunction"
CHUNK = 4096           # configurations scored per call of the oracle
FACTOR = 16.0          # f32: max |d log r| <= FACTOR x (f32 oracle's deviation from f64), the rule of test_gpu_gradient_full.py
BLOCK = 16             # chains per block of the kernels; pair p = chains 2p, 2p + 1 sits in block p // 8


def to64(prm):
    return {k: np.asarray(v, dtype=np.float64) for k, v in prm.items()}


def to32(prm):
    return {k: np.asarray(v, dtype=np.float32) for k, v in prm.items()}


def _scorer(prm, dtype):
    return lambda x: M.prnn_log_probability(prm, x, dtype=dtype)


def _chunked(log_p, x):
    return np.concatenate([log_p(x[k:k + CHUNK]) for k in range(0, len(x), CHUNK)]) if len(x) else np.zeros(0)


def log_ratio_entries(log_p, pairs, pair_idx, cut):
    """log r of the entries e = (pair pair_idx[e], cut cut[e]): float64 (E,).  pairs: (2 npairs, N) spins, pair p = rows 2p, 2p + 1;
    log_p scores (B, N) configurations.  Cuts 0 and N swap nothing: exactly 0."""
    pairs = np.asarray(pairs)
    N = pairs.shape[1]
    pair_idx, cut = np.asarray(pair_idx, dtype=np.int64), np.asarray(cut, dtype=np.int64)
    assert pair_idx.shape == cut.shape and np.all((cut >= 0) & (cut <= N))
    out = np.zeros(len(cut))
    own = {}                                         # log P(sigma), log P(tau) of every pair that occurs, scored in full as well
    used = np.unique(pair_idx)
    lp_own = _chunked(log_p, np.concatenate([pairs[2 * used], pairs[2 * used + 1]]))
    for k, p in enumerate(used):
        own[int(p)] = lp_own[k] + lp_own[len(used) + k]
    inner = np.flatnonzero((cut > 0) & (cut < N))
    for k0 in range(0, len(inner), CHUNK // 2):
        e = inner[k0:k0 + CHUNK // 2]
        sigma, tau = pairs[2 * pair_idx[e]], pairs[2 * pair_idx[e] + 1]
        in_a = np.arange(N)[None, :] < cut[e][:, None]
        a = np.where(in_a, tau, sigma)               # tau_A sigma_B
        b = np.where(in_a, sigma, tau)               # sigma_A tau_B
        lp = log_p(np.concatenate([a, b]))
        out[e] = 0.5 * (lp[:len(e)] + lp[len(e):] - np.array([own[int(p)] for p in pair_idx[e]]))
    return out


def log_ratio(prm, pairs, cuts, dtype=np.float64, pair_idx=None):
    """(len(cuts), len(pair_idx)) log r of the pairs pair_idx (default: all) at every cut of `cuts`, cell arithmetic in `dtype`."""
    pairs = np.asarray(pairs)
    pair_idx = np.arange(len(pairs) // 2) if pair_idx is None else np.asarray(pair_idx)
    cuts = np.asarray(cuts, dtype=np.int64)
    pp, cc = np.meshgrid(pair_idx, cuts, indexing="xy")
    prm = to64(prm) if dtype == np.float64 else to32(prm)
    return log_ratio_entries(_scorer(prm, dtype), pairs, pp.ravel(), cc.ravel()).reshape(len(cuts), len(pair_idx))


def log_ratio_f64(prm, pairs, cuts):
    """The reference: log r of every pair (rows 2p, 2p + 1 of `pairs`) at the cuts `cuts`, float64, (len(cuts), npairs)."""
    return log_ratio(prm, pairs, cuts, dtype=np.float64)


def log_ratio_one_cut(prm, pairs, l, dtype=np.float64):
    """One cut through test_renyi_host.swap_log_ratio, the formula as that module states it (a cross-check of log_ratio_entries)."""
    prm = to64(prm) if dtype == np.float64 else to32(prm)
    pairs = np.asarray(pairs)
    return swap_log_ratio(lambda x: _chunked(_scorer(prm, dtype), x), pairs[0::2], pairs[1::2], l)


# ---- sums and statistics, written out again ----------------------------------------------------------------------------------

def sums_from_log_ratio(log_ratio_rows):
    """(rows, 2): [sum_p r, sum_p r^2] per row of log r, r = exp(log r), exactly rounded sums (math.fsum)."""
    r = np.exp(np.asarray(log_ratio_rows, dtype=np.float64))
    return np.array([[math.fsum(row), math.fsum(row * row)] for row in r])


def entropy_from_sums(sums, npairs):
    """S2 = -log(mean r) and sigma = std(r) / (sqrt(n) mean r), std^2 = mean r^2 - (mean r)^2 (docs/renyi.md), per cut."""
    n = float(npairs)
    S2, err = np.empty(len(sums)), np.empty(len(sums))
    for l, (s1, s2) in enumerate(np.asarray(sums, dtype=np.float64)):
        mean = s1 / n
        S2[l] = -math.log(mean)
        err[l] = math.sqrt(max(s2 / n - mean * mean, 0.0)) / (math.sqrt(n) * mean)
    return S2, err


# ---- bounds ------------------------------------------------------------------------------------------------------------------

def f32_ceiling(N):
    """log r = 1/2 (tail_sigma + tail_tau - suffix_sigma - suffix_tau), four partial log-probabilities of at most N sites, each
    held to 2e-6 N + 2e-6 by tests/test_gpu_prnn.py: 1/2 x 4 x that."""
    return 2.0 * (2e-6 * N + 2e-6)


def f32_bound(dev32, N):
    """(bound, capped): FACTOR x dev32, capped at f32_ceiling(N) - unless the f32 oracle itself (dev32) is beyond the ceiling (config 5's
    precedent in tests/test_gpu_sharpened.py: 200 steps through x 3 kernels), where FACTOR x dev32 stands uncapped."""
    cap = f32_ceiling(N)
    if dev32 > cap:
        return FACTOR * dev32, False
    return min(FACTOR * dev32, cap), FACTOR * dev32 > cap


def f64_bound(N):
    return 1e-11 * N


# ---- which pairs and cuts a case checks ----------------------------------------------------------------------------------------

def boundary_cuts(N):
    """1, N - 1 and both sides of every 32-site word boundary of the packed spins: 31, 32, 33, 63, 64, 65, ... (those in 1..N-1)."""
    cuts = {1, N - 1}
    for w in range(32, N + 1, 32):
        cuts.update((w - 1, w, w + 1))
    return np.array(sorted(c for c in cuts if 1 <= c <= N - 1), dtype=np.int64)


def choose_subset(npairs, n_min=64, n_all=16, seed=0):
    """(pairs checked at every cut, pairs checked at the boundary cuts), disjoint, together >= n_min, the first >= n_all.  All 8 pairs
    of the first, a middle and the last full 16-chain block and every pair of the ragged last block are in; four pairs of each of
    those blocks (lanes 0/1, 6/7, 12/13, 14/15) and the ragged block go to the first list; the rest are spread at random."""
    per = BLOCK // 2
    nfull = (2 * npairs) // BLOCK
    assert nfull >= 3 and npairs >= n_min
    blocks = [0, nfull // 2, nfull - 1]
    every = list(range(nfull * per, npairs)) + [b * per + k for b in blocks for k in (0, 3, 6, 7)]
    rest = [b * per + k for b in blocks for k in (1, 2, 4, 5)]
    free = np.array(sorted(set(range(npairs)) - set(every) - set(rest)))
    need_every = max(0, n_all - len(every))
    need = need_every + max(0, n_min - len(every) - need_every - len(rest))
    extra = np.random.RandomState(seed).choice(free, size=need, replace=False).tolist()
    every += extra[:need_every]
    rest += extra[need_every:]
    return np.array(sorted(every), dtype=np.int64), np.array(sorted(rest), dtype=np.int64)


def check_subset(npairs, N, every, rest, cuts_rest):
    """The conditions a case's subset must meet, asserted (not only intended)."""
    per, nfull = BLOCK // 2, (2 * npairs) // BLOCK
    both = np.concatenate([every, rest])
    assert len(set(both.tolist())) == len(both) >= 64 and both.min() >= 0 and both.max() < npairs
    assert len(every) >= 16
    blk = both // per
    for b in (0, nfull - 1):
        assert np.any(blk == b), "no pair from block %d" % b
    assert np.any((blk > 0) & (blk < nfull - 1)), "no pair from a middle block"
    assert set(range(nfull * per, npairs)) <= set(both.tolist()), "a pair of the ragged last block is missing"
    assert set(boundary_cuts(N).tolist()) <= set(np.asarray(cuts_rest).tolist())


def subset_entries(N, every, rest):
    """Entry lists (pair_idx, cut): `every` x cuts 1..N-1, then `rest` x boundary_cuts(N)."""
    p1, c1 = np.meshgrid(every, np.arange(1, N), indexing="ij")
    p2, c2 = np.meshgrid(rest, boundary_cuts(N), indexing="ij")
    return np.concatenate([p1.ravel(), p2.ravel()]), np.concatenate([c1.ravel(), c2.ravel()])


# ---- comparator ----------------------------------------------------------------------------------------------------------------

def compare(label, got, ref, pair_idx, cut, bound, echo=print):
    """max |got - ref| over the entries, where it occurs (cut, pair, 16-chain block, lane pair) and its ratio to `bound`."""
    d = np.abs(np.asarray(got) - np.asarray(ref))
    k = int(np.argmax(d))
    res = dict(err=float(d[k]), cut=int(cut[k]), pair=int(pair_idx[k]), block=int(pair_idx[k]) // (BLOCK // 2), bound=float(bound),
               ratio=float(d[k] / bound), entries=len(d), finite=bool(np.all(np.isfinite(got))))
    echo("%s max |d log r| = %.3e at cut %d, pair %d (block %d, lanes %d/%d) over %d entries; bound %.3e; ratio %.3f"
         % (label, res["err"], res["cut"], res["pair"], res["block"], 2 * res["pair"] % BLOCK, 2 * res["pair"] % BLOCK + 1, res["entries"],
            bound, res["ratio"]))
    return res


def nontrivial(ref):
    """(max |log r|, share of entries with |log r| > 0.01): a case requires > 0.1 and >= 1/4."""
    a = np.abs(ref)
    return float(a.max()), float(np.mean(a > 0.01))


# ---- further restatements, for tests/test_renyi_reference.py ---------------------------------------------------------------------

def site_log_probs(prm, x, dtype=np.float64):
    """(B, N) log p(x_n | x_<n) of the oracle, cell arithmetic in `dtype`."""
    x = np.asarray(x)
    out = []
    for k in range(0, len(x), CHUNK):
        p = M.prnn_site_probs(prm, x[k:k + CHUNK], SCOPE, dtype).astype(np.float64)
        out.append(np.log(np.take_along_axis(p, x[k:k + CHUNK, :, None].astype(np.int64), axis=2)[:, :, 0]))
    return np.concatenate(out)


def tails_and_suffixes(prm, pairs, cuts, fed_prefix=None, dtype=np.float64):
    """The site-resolved form the kernels use: for every pair and cut l, tail_s(l) = the log-probability of chain s's own spins
    l..N-1 after the PARTNER's first l spins, and suffix_s(l) the same after its own; log r = 1/2 (tail_sigma + tail_tau -
    suffix_sigma - suffix_tau).  Returns four (len(cuts), npairs) arrays.  fed_prefix(partner, own, l) -> the l spins fed before
    site l (default: the partner's; a defect may say otherwise)."""
    pairs = np.asarray(pairs)
    sigma, tau = pairs[0::2], pairs[1::2]
    N = pairs.shape[1]
    prm = to64(prm) if dtype == np.float64 else to32(prm)
    own_s, own_t = site_log_probs(prm, sigma, dtype), site_log_probs(prm, tau, dtype)
    fed_prefix = fed_prefix or (lambda partner, own, l: partner[:, :l])
    out = [np.zeros((len(cuts), len(sigma))) for _ in range(4)]
    for k, l in enumerate(cuts):
        a = np.concatenate([fed_prefix(tau, sigma, l), sigma[:, l:]], axis=1)
        b = np.concatenate([fed_prefix(sigma, tau, l), tau[:, l:]], axis=1)
        assert a.shape == b.shape == (len(sigma), N)
        out[0][k] = site_log_probs(prm, a, dtype)[:, l:].sum(axis=1)
        out[1][k] = site_log_probs(prm, b, dtype)[:, l:].sum(axis=1)
        out[2][k], out[3][k] = own_s[:, l:].sum(axis=1), own_t[:, l:].sum(axis=1)
    return out


def log_prob_other_order(prm, x, dtype=np.float32, parts=3):
    """log P of a one-layer GRU wave function restated with every gate and candidate sum accumulated in ANOTHER order than
    oracle.models.gru_cell: the input and hidden products separately (no concatenation), the hidden one in `parts` slices of the
    hidden index added last to first, sigmoid as 1/2 (1 + tanh(x/2)), log-softmax as z - logaddexp.  The same function of the
    parameters; in float32 a second, differently rounded evaluation."""
    pre = SCOPE + "/" + M.GRU % 0
    p = {k: np.asarray(v, dtype=dtype) for k, v in prm.items()}
    Wg, bg = p[pre + "gates/kernel"], p[pre + "gates/bias"]
    Wci, bci = p[pre + "candidate/input_projection/kernel"], p[pre + "candidate/input_projection/bias"]
    Wch, bch = p[pre + "candidate/hidden_projection/kernel"], p[pre + "candidate/hidden_projection/bias"]
    Wd, bd = p[SCOPE + "/wf_dense/kernel"], p[SCOPE + "/wf_dense/bias"]
    x = np.asarray(x)
    B, N = x.shape
    H = Wch.shape[0]
    cutsH = np.linspace(0, H, parts + 1).astype(int)
    half, one = dtype(0.5), dtype(1)

    def hidden(h, W):
        acc = np.zeros((B, W.shape[1]), dtype=dtype)
        for k in range(parts - 1, -1, -1):
            acc = acc + h[:, cutsH[k]:cutsH[k + 1]] @ W[cutsH[k]:cutsH[k + 1]]
        return acc

    h = np.zeros((B, H), dtype=dtype)
    inp = np.zeros((B, 2), dtype=dtype)
    lp = np.zeros(B)
    for n in range(N):
        g = (bg + hidden(h, Wg[2:])) + inp @ Wg[:2]
        g = half * (one + np.tanh(half * g))
        r, u = g[:, :H], g[:, H:]
        c = np.tanh(r * (bch + hidden(h, Wch)) + (inp @ Wci + bci))
        h = u * h + (one - u) * c
        z = (h @ Wd + bd).astype(np.float64)
        lp += z[np.arange(B), x[:, n]] - np.logaddexp(z[:, 0], z[:, 1])
        inp = np.eye(2, dtype=dtype)[x[:, n]]
    return lp
