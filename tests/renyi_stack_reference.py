"""Float64 reference of the swap estimator of the second Renyi entropy of arbitrary regions for STACKED GRU layers
(docs/renyi_stack.md), independent of the library: a thin layer over tests/renyi_regions_reference.py, whose log_ratio scores with
oracle.models.prnn_log_probability - over multi_gru, layers of unequal width included.  TEST INFRASTRUCTURE ONLY; validated by
tests/test_renyi_stack_reference.py.

    log r_A(sigma, tau) = 1/2 [log P(tau_A sigma_B) + log P(sigma_A tau_B) - log P(sigma) - log P(tau)],   A = any set of sites (a mask)

Brute force on purpose, as that module: both swapped configurations of every (pair, region) are written out in full and scored from
site 0.  Weights: sampler_reference.build_params(family, units, seed, sharp=3).

Bounds, none taken from a kernel under test (tests/renyi_reference.py):
  float64   |log r - ref| <= 1e-11 N                                                                     (f64_bound)
  float32   16 x the float32 NumPy oracle's deviation from float64 on the same pairs and regions, capped at 2 (2e-6 N + 2e-6)
            (f32_bound)
  sums      against math.fsum of the device's own log r: relative 1e-12

Also here: the site-resolved form the stack kernels use (stack_form: every layer restarted from the chain's own states before site f),
restated with switches for the defects tests/test_renyi_stack_reference.py shows the bounds to reject.
"""
import numpy as np

import renyi_reference as R
import renyi_regions_reference as G
import sampler_reference as SR
from oracle import models as M

SCOPE = R.SCOPE
SUM_RTOL = 1e-12
f64_bound, f32_bound, nontrivial = R.f64_bound, R.f32_bound, R.nontrivial
word_boundaries_covered, choose_pairs, check_subset = G.word_boundaries_covered, G.choose_pairs, G.check_subset
purity_of_region = G.purity_of_region


def weights(f64, units, seed=111, sharp=3.0):
    return SR.build_params("gru64" if f64 else "gru", units, seed=seed, sharp=sharp)


def log_ratio(prm, pairs, masks, dtype=np.float64, pair_idx=None):
    """(R, len(pair_idx)) log r_A, cell arithmetic in `dtype`; pairs (2 npairs, N) in the model's site order"""
    pairs = np.asarray(pairs).reshape(len(pairs), -1)
    return G.log_ratio(prm, pairs, np.asarray(masks).reshape(len(masks), -1), dtype=dtype, pair_idx=pair_idx)


def judge(label, got, ref, ref32, f64, N, echo=print):
    """asserts the device's log r (R, n) against the float64 reference `ref`; ref32: the float32 oracle on the same entries (None for
    float64).  Returns dict(err, bound, ratio, dev32)."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and np.all(np.isfinite(got))
    mx, share = nontrivial(ref)
    assert mx > 0.1 and share >= 0.25, "%s: the reference is trivial (max |log r| %.3f, %.0f %% above 0.01)" % (label, mx, 100 * share)
    if f64:
        dev32, bound, how = 0.0, f64_bound(N), "1e-11 N"
    else:
        dev32 = float(np.abs(np.asarray(ref32) - ref).max())
        bound, capped = f32_bound(dev32, N)
        how = "capped" if capped else "16 x dev32 %.2e" % dev32
    d = np.abs(got - ref)
    r, p = np.unravel_index(int(np.argmax(d)), d.shape)
    err = float(d[r, p])
    echo("%s max |d log r| = %.3e (region %d, pair column %d) over %d entries; bound %.3e (%s); ratio %.3f; max |log r| %.2f, %.0f %% above 0.01"
         % (label, err, r, p, d.size, bound, how, err / bound, mx, 100 * share))
    assert err <= bound, "%s: region %d, pair column %d: |log r - ref| = %.3e > %.3e" % (label, r, p, err, bound)
    return dict(err=err, bound=bound, ratio=err / bound, dev32=dev32)


def judge_sums(label, sums, log_ratio_rows):
    want = R.sums_from_log_ratio(log_ratio_rows)
    rel = np.abs(np.asarray(sums) / want - 1.0).max()
    assert rel <= SUM_RTOL, "%s: sums off the exactly rounded sums of the device's own log r by %.2e" % (label, rel)
    return float(rel)


# ---- regions of the tests ------------------------------------------------------------------------------------------------------------

def mask_of(N, sites):
    m = np.zeros(N, dtype=np.int32)
    m[list(sites)] = 1
    return m


def small_regions(Nx, Ny):
    """[(name, mask)] on Nx x Ny raster sites (site ny Nx + nx; Ny = 1: a chain) of at least 6: a bulk interval, a two-piece region,
    single sites, a suffix, a column cut (every other site of a chain), a region containing site 0 (normalised by the library)"""
    N = Nx * Ny
    col = mask_of(N, [n for n in range(N) if n % Nx == 0]) if Ny > 1 else mask_of(N, range(0, N, 2))
    return [("interval 2..4", mask_of(N, range(2, 4))), ("two pieces", mask_of(N, [1, N - 2])), ("site N-1", mask_of(N, [N - 1])),
            ("site 1", mask_of(N, [1])), ("suffix N/2..", mask_of(N, range(N // 2, N))), ("column 0" if Ny > 1 else "even sites", col),
            ("site 0 and the last two", mask_of(N, [0, N - 2, N - 1]))]


def boundary_regions(N):
    """[(name, mask)] of a case beyond one 32-site word of packed spins (N > 33): intervals ending on, starting on and straddling
    every word boundary; a checkerboard; every third site; a single site; a two-piece region; a region containing site 0"""
    out = []
    for w in range(32, N, 32):
        out += [("interval %d..%d (ends on a word)" % (w - 5, w), mask_of(N, range(w - 5, w))),
                ("interval %d..%d (starts on a word)" % (w, min(N, w + 5)), mask_of(N, range(w, min(N, w + 5)))),
                ("interval %d..%d (across a word)" % (w - 1, w + 1), mask_of(N, range(w - 1, w + 1)))]
    out += [("checkerboard", mask_of(N, range(1, N, 2))), ("every third site", mask_of(N, range(1, N, 3))), ("site N-1", mask_of(N, [N - 1])),
            ("two pieces", mask_of(N, list(range(1, max(2, N // 5))) + list(range((3 * N) // 4, N - 1)))),
            ("site 0 and the last third", mask_of(N, [0] + list(range((2 * N) // 3, N))))]
    return out


def all_pairs(configs):
    """(i, j, pairs): every ordered pair of the rows of `configs`, pair p = rows 2p, 2p + 1 = configs[i[p]], configs[j[p]]"""
    n = len(configs)
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    pairs = np.empty((2 * i.size, configs.shape[1]), dtype=np.int32)
    pairs[0::2], pairs[1::2] = configs[i.ravel()], configs[j.ravel()]
    return i.ravel(), j.ravel(), pairs


# ---- the site-resolved form of the stack kernels, with defects -------------------------------------------------------------------------

def run_stack(prm, x, dtype, states=None, spin_in=None, n0=0):
    """Sites n0..N-1 of the chains x (B, N) teacher-forced from the layer states `states` (None: zero) and the input spin spin_in
    (B,) (None: the zero input): (log p(x_n | ...) (B, N - n0) float64, [the layer states after each of these steps])."""
    x = np.asarray(x)
    B, N = x.shape
    Wd, bd = M._p(prm, SCOPE, "wf_dense/kernel"), M._p(prm, SCOPE, "wf_dense/bias")
    states = M._zero_states(prm, SCOPE, B, dtype) if states is None else [np.array(s) for s in states]
    inp = np.zeros((B, 2), dtype=dtype) if spin_in is None else M._one_hot(np.asarray(spin_in), dtype)
    lp, kept = np.empty((B, N - n0)), []
    for n in range(n0, N):
        out, states = M.multi_gru(inp, states, prm, SCOPE)
        p = M.softmax(out @ Wd + bd).astype(np.float64)
        lp[:, n - n0] = np.log(p[np.arange(B), x[:, n]])
        kept.append(states)
        inp = M._one_hot(x[:, n], dtype)
    return lp, kept


DEFECTS = {"own_on_A": "own instead of the partner's spins on A", "mask_shifted": "mask shifted by one site",
           "partner_checkpoint": "restart from the partner's checkpoint", "layer_below": "layer l restored from layer l-1's state",
           "mask_word_0": "mask words of sites >= 32 read from word 0"}


def stack_form(prm, pairs, masks, defect=None, dtype=np.float64):
    """log r_A = 1/2 [(tail_sigma - suffix_sigma) + (tail_tau - suffix_tau)] as stack_chain_kernels.h computes it: the mask normalised,
    f its first site, EVERY layer's state restored from the chain's own states before site f, the chain's own spin f - 1 fed, the
    mixed chain m_n = (n in A ? partner : own) teacher-forced from f; suffix = the chain's own terms from f.  (R, npairs).  defect
    names one deliberate error (DEFECTS; "layer_below" needs layers of equal width)."""
    pairs = np.asarray(pairs)
    sigma, tau = pairs[0::2], pairs[1::2]
    N = pairs.shape[1]
    prm = R.to64(prm) if dtype == np.float64 else R.to32(prm)
    (own_s, st_s), (own_t, st_t) = run_stack(prm, sigma, dtype), run_stack(prm, tau, dtype)
    out = np.zeros((len(masks), len(sigma)))
    for k, mask in enumerate(masks):
        m, f = G.normalise(mask)
        if f == 0:
            continue
        if defect == "mask_shifted":
            m = np.concatenate([[0], m[:-1]])
        elif defect == "mask_word_0":
            m = m[np.arange(N) & 31]
        elif defect == "own_on_A":
            m = np.zeros(N, dtype=np.int64)
        in_a = m.astype(bool)[None, :]

        def tail(own, partner, st_own, st_partner):
            start = (st_partner if defect == "partner_checkpoint" else st_own)[f - 1]
            if defect == "layer_below":
                start = [start[0]] + [start[l - 1] for l in range(1, len(start))]
            return run_stack(prm, np.where(in_a, partner, own), dtype, states=start, spin_in=own[:, f - 1], n0=f)[0].sum(axis=1)
        ts, tt = tail(sigma, tau, st_s, st_t), tail(tau, sigma, st_t, st_s)
        out[k] = 0.5 * ((ts - own_s[:, f:].sum(axis=1)) + (tt - own_t[:, f:].sum(axis=1)))
    return out
