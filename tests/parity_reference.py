"""The parity-symmetric model over the whole range of log P: the stable combine and shares, the symmetrised float64 reference and queue,
the autograd counterpart, the table of rungs and the judgements of tests/test_gpu_parity_range.py.  TEST INFRASTRUCTURE ONLY.

log P_sym = log(0.5 (P(s) + P(reversed s))) is the one place where the library turns an ABSOLUTE log-probability into a probability
(util_kernels.h: parity_combine_kernel; every estimator works on differences).  In float64 exp leaves the normal range below -708.4
and is zero below -745.1, so the formula as written loses a bit per 0.69 below -708.4 and returns -inf below -745.1.  Here it is

    combine(a, b) = max(a, b) + log(0.5 (1 + exp(-|a - b|)))            shares  aF = 1 / (1 + exp(b - a)),  aR = 1 - aF

which needs the difference alone.  `naive` is the formula as written, in any float type: numpy.longdouble (x87: the exponent range
of the whole table) is what test_parity_reference.py checks `combine` against.

The symmetrised reference (sym_log_prob, sym_queue) combines oracle.models.prnn_log_probability in float64, every chain from site 0,
on s and on s[:, ::-1]; the autograd counterpart is torch.logaddexp(lp1, lp2) - log 2 on autograd_reference.prnn_log_probability.
The symmetriser of flip_rows_reference.queue (prefix-sharing, float64 and float32: the yardstick) and the formula as written in
oracle/models.py and autograd_reference.py stay as they are; test_parity_reference.py ties this module to each.

The rungs.  Small shapes reach the whole range: kernels x 3, every bias randomised (flip_rows_reference.build_params) and the head
bias set to (+head, -head) make a 1 as unlikely as a few e^-head per site, so a teacher-forced configuration with k ones has
log P about -k x (2 head + a few).  CASES: 10 units on 70 sites (three spin words, the last ragged; head 6: to -1 300) and 37 units on
33 sites (another kernel class, two words, a padded width; 33 sites reach -760 only with a stronger head, 16: to -1 100).  A case's
rungs come from three fixed pools - random configurations of k ones (eight per k, seeded), contiguous blocks of ones (every length
and start: these carry the large |log P_F - log P_R|), palindromes (a seeded half of j ones, mirrored) - scored in float64 by the
oracle and taken in pool order:
    ladder      the first configuration of k ones, for every k of the case's ladder (k = 0 and k = N are palindromes)
    band        the first six with log P_sym in (-745, -709): the formula as written is silently inexact
    saturated   the first two with log P_F - log P_R >= 40 and the first two with <= -40: a share is exactly 0 or 1 in float64
    close       the first four below -760 with |log P_F - log P_R| < 1 that are no palindromes: both directions deep
    palindrome  six, j evenly spaced from 0 to N // 2: a = b, so combine(a, a) == a bit for bit
`rungs` asserts what the table must hold (conditions on the inputs, read off the float64 oracle, never off a kernel): at least four
rungs in the band, eight below -760, eight above -600, four saturated, four close and deep, six palindromes of which two below -760,
and a rung count that is no multiple of 32 (ragged last tile on either engine).

Bounds, none taken from a kernel:
    combine     |got - combine(a, b)| <= 8 x 2^-52 x max(1, |value|), a and b the DEVICE's per-direction values (a plain GRU handle
                with the same weights, engine and batch size): the maximum is exact, the correction lies in [-0.70, 0] with an
                absolute error of a few 1e-16, the sum rounds once; 8 leaves room for the device's exp and log.  On a palindrome:
                bit equality with the GRU handle's value.
    float64     flip_rows_reference's row bound, 16 x the per-chain float32 yardstick (its Reference of the parity family), for
                log_prob as for every queue row; its E_loc bound and summation term for the energies.
    gradient    gradient_classes_reference.judge on its parity family (16 x the float32 autograd deviation, its rounding floor), the
                float64 and float32 autograd gradients being those of the stable form.

Defect models, each refused on the CPU by the judgement the GPU test applies (test_parity_reference.py), the device's per-direction
values played by the float64 oracle's: the formula as written; the reversed direction dropped; the factor 0.5 dropped; the reverse map
(prnn.hip: ensure_reverse_map) off by one row; a reversed packing (pack.h: pack_bits_kernel, reverse = 1) that reverses each 32-site
spin word in place instead of the chain.
"""
import collections
import functools
import time

import numpy as np
import torch

import autograd_reference as A
import flip_rows_reference as F
import gradient_classes_reference as G
from oracle import models as M

SCOPE = F.SCOPE
LN2 = float(np.log(2.0))
ULPS = 8.0
EPS = 2.0 ** -52
EXP_ZERO = -745.2                  # below it exp(x) is 0 in float64 (the smallest subnormal is e^-744.44, half of it e^-745.13)
BAND = (-745.0, -709.0)            # exp(x) is subnormal
DEEP = -760.0
ORDINARY = -600.0
SATURATED = 40.0                   # 1 + e^-40 == 1 in float64 (e^-40 < 2^-53)
SEED = F.SEED
PER_K = 8                          # random configurations per number of ones in the pool


# ---- the combine and the shares ----------------------------------------------------------------------------------------------------

def combine(a, b):
    """log(0.5 (e^a + e^b)) from the difference alone, in the type of the inputs (float64 unless they are wider)."""
    a, b = np.asarray(a), np.asarray(b)
    a, b = (a, b) if a.dtype == np.longdouble else (a.astype(np.float64), b.astype(np.float64))
    with np.errstate(invalid="ignore"):
        d = np.where(a == b, 0.0, np.abs(a - b))           # a == b = -inf: no inf - inf
    return np.maximum(a, b) + np.log(0.5 * (1.0 + np.exp(-d)))


def naive(a, b, dtype=np.float64):
    """The formula as written (RNNwavefunction_paritysym.py:145, oracle/models.py), evaluated in `dtype`."""
    a, b = np.asarray(a, dtype=dtype), np.asarray(b, dtype=dtype)
    with np.errstate(divide="ignore", under="ignore"):
        return np.log(dtype(0.5) * (np.exp(a) + np.exp(b)))


def shares(a, b, dtype=np.float64):
    """(aF, aR) = (P_F, P_R) / (P_F + P_R) from the difference (util_kernels.h: parity_share_kernel)."""
    a, b = np.asarray(a, dtype=dtype), np.asarray(b, dtype=dtype)
    with np.errstate(over="ignore", under="ignore"):
        aF = dtype(1) / (dtype(1) + np.exp(b - a))
    return aF, dtype(1) - aF


def bound(value):
    """The combine bound of the module docstring."""
    return ULPS * EPS * np.maximum(1.0, np.abs(value))


def over_bound(got, want):
    """|got - want| / bound(want) per entry; inf where got is not finite."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        r = np.abs(got - want) / bound(want)
    return np.where(np.isfinite(got) & np.isfinite(r), r, np.inf)


# ---- the float64 reference ---------------------------------------------------------------------------------------------------------

def directions(prm, s):
    """(log P(s), log P(reversed s)), float64, every chain from site 0 by the oracle."""
    p = F.R.cast(prm, np.float64)
    s = np.asarray(s).reshape(len(s), -1)
    return M.prnn_log_probability(p, s, SCOPE, np.float64), M.prnn_log_probability(p, s[:, ::-1], SCOPE, np.float64)


def sym_log_prob(prm, s):
    return combine(*directions(prm, s))


def flipped(s):
    """(N + 1, B, N): row 0 is s, row k + 1 is s flipped at site k."""
    s = np.asarray(s).reshape(len(s), -1)
    q = np.repeat(s[None], s.shape[1] + 1, axis=0)
    k = np.arange(s.shape[1])
    q[k + 1, :, k] = 1 - q[k + 1, :, k]
    return q


def sym_queue(prm, s):
    """(N + 1, B) float64: sym_log_prob of every row of `flipped`."""
    q = flipped(s)
    return sym_log_prob(prm, q.reshape(-1, q.shape[2])).reshape(q.shape[:2])


def exchange(q):
    """The queue (N + 1, B) of the reversed configurations in the numbering of the unreversed ones: the reversed chain flipped at its
    position n is the chain flipped at site N - 1 - n, so rows k + 1 and N - k change places."""
    return np.concatenate([q[:1], q[1:][::-1]])


def word_reversed(s):
    """Defect model: every 32-site spin word reversed in place (the last one over its valid sites), the words left in order."""
    s = np.asarray(s)
    return np.concatenate([s[:, lo:lo + 32][:, ::-1] for lo in range(0, s.shape[1], 32)], axis=1)


# ---- autograd ----------------------------------------------------------------------------------------------------------------------

def torch_sym_log_prob(params, samples, scope=SCOPE):
    s = np.asarray(samples)
    lp1 = A.prnn_log_probability(params, s, scope)
    lp2 = A.prnn_log_probability(params, s[:, ::-1], scope)
    return torch.logaddexp(lp1, lp2) - LN2


FORWARDS = {"stable": torch_sym_log_prob, "naive": A.prnn_paritysym_log_probability}


def gradient(prm, s, e, dtype=torch.float64, forward="stable"):
    """{scoped tf name: float64 ndarray}: d cost_real / d parameter (autograd_reference.gradient with the chosen combine)."""
    leaves = A.to_torch(prm, dtype, requires_grad=True)
    A.cost_real(FORWARDS[forward](leaves, s, SCOPE), e).backward()
    return {k: v.grad.detach().to(torch.float64).numpy().reshape(np.shape(prm[k])) for k, v in leaves.items()}


def per_sample_gradients(prm, s, e):
    """gradient_classes_reference.per_sample_gradients on the stable form: {name: (ns,) + shape}, float64."""
    leaves = A.to_torch(prm, torch.float64, requires_grad=True)
    e = np.asarray(e)
    L = torch_sym_log_prob(leaves, s, SCOPE) * torch.as_tensor((e - e.mean()) / len(e))
    order = sorted(leaves)
    g = torch.autograd.grad(L, [leaves[k] for k in order], grad_outputs=torch.eye(len(L), dtype=L.dtype), is_grads_batched=True)
    return {k: v.detach().numpy().reshape((len(L),) + np.shape(prm[k])) for k, v in zip(order, g)}


def gradient_case(case, ns):
    return G.Case("parity", (case.N, 1), (case.units,), ns, F.SHARP)


def gradient_reference(case, prm, s, e):
    """gradient_classes_reference.reference with the stable form in the place of autograd_reference's parity forward."""
    t0 = time.time()
    g64, g32 = gradient(prm, s, e, torch.float64), gradient(prm, s, e, torch.float32)
    terms = per_sample_gradients(prm, s, e)
    return G.Reference(g64, g32, terms, G.rounding_floor(gradient_case(case, len(s)), terms, g64), time.time() - t0)


# ---- the table ---------------------------------------------------------------------------------------------------------------------

Case = collections.namedtuple("Case", "id units N head ladder")
CASES = [
    Case("10x70", 10, 70, 6.0, tuple(range(1, 70, 3))),               # three spin words, the last holds 6 sites
    Case("37x33", 37, 33, 16.0, tuple(range(1, 33))),                 # NFULL 3, 11 padded units; the second word holds one site
]
CASE_IDS = [c.id for c in CASES]

Rungs = collections.namedtuple("Rungs", "s kind lpF lpR sym")


def case(cid):
    return CASES[CASE_IDS.index(cid)]


def build_params(c):
    prm = F.build_params("parity", (c.units,))
    prm[SCOPE + "/wf_dense/bias"] = np.array([c.head, -c.head], dtype=np.float32)
    return prm


def _pools(c):
    rng = np.random.RandomState(SEED + c.N)
    N = c.N
    random_k = np.zeros((N + 1, PER_K, N), dtype=np.int32)
    for k in range(N + 1):
        for j in range(PER_K):
            random_k[k, j, rng.permutation(N)[:k]] = 1
    blocks = []
    for k in range(1, N):
        for lo in range(N - k + 1):
            b = np.zeros(N, dtype=np.int32)
            b[lo:lo + k] = 1
            blocks.append(b)
    palindromes = np.zeros((N // 2 + 1, N), dtype=np.int32)
    for j in range(N // 2 + 1):
        half = np.zeros(N // 2, dtype=np.int32)
        half[rng.permutation(N // 2)[:j]] = 1
        palindromes[j, :N // 2], palindromes[j, N - N // 2:] = half, half[::-1]          # odd N: the centre stays 0
    return random_k, np.array(blocks), palindromes


@functools.lru_cache(maxsize=None)
def rungs(cid):
    """The rungs of a case, in the order ladder, band, saturated, close, palindrome, with the float64 oracle's per-direction values.
    The search is the pool order above; what it must find is asserted."""
    c = case(cid)
    prm = build_params(c)
    random_k, blocks, pal = _pools(c)
    pool = np.concatenate([random_k.reshape(-1, c.N), blocks])
    a, b = directions(prm, pool)
    sym, d, ones = combine(a, b), a - b, pool.sum(axis=1)
    taken = np.all(pool == pool[:, ::-1], axis=1)                              # palindromes have a pool of their own
    taken[np.setdiff1d(np.arange(len(pool)), np.unique(pool, axis=0, return_index=True)[1])] = True     # held twice: the first counts

    def first(mask, count):
        idx = np.flatnonzero(mask & ~taken)[:count]
        assert len(idx) == count, "%s: the pools hold %d of %d such rungs" % (cid, len(idx), count)
        taken[idx] = True
        return pool[idx]

    ladder = np.concatenate([first(ones == k, 1) for k in c.ladder])
    band = first((sym > BAND[0]) & (sym < BAND[1]), 6)
    saturated = np.concatenate([first(d >= SATURATED, 2), first(d <= -SATURATED, 2)])
    close = first((sym < DEEP) & (np.abs(d) < 1.0), 4)
    pals = pal[np.round(np.linspace(0, len(pal) - 1, 6)).astype(np.int64)]
    parts = [("ladder", ladder), ("band", band), ("saturated", saturated), ("close", close), ("palindrome", pals)]
    s = np.ascontiguousarray(np.concatenate([p for _, p in parts]))
    kind = np.concatenate([[name] * len(p) for name, p in parts])
    lpF, lpR = directions(prm, s)
    r = Rungs(s, kind, lpF, lpR, combine(lpF, lpR))
    d = r.lpF - r.lpR
    is_pal = np.all(s == s[:, ::-1], axis=1)
    assert 40 <= len(s) <= 60 and len(s) % 32 != 0 and len(s) % 16 != 0, len(s)
    assert len(np.unique(s, axis=0)) == len(s)
    assert np.sum((r.sym > BAND[0]) & (r.sym < BAND[1])) >= 4
    assert np.sum(r.sym < DEEP) >= 8 and np.sum(r.sym > ORDINARY) >= 8
    assert np.sum(np.abs(d) >= SATURATED) >= 4 and np.sum(d >= SATURATED) >= 2 and np.sum(d <= -SATURATED) >= 2
    assert np.sum((r.sym < DEEP) & (np.abs(d) < 1.0) & ~is_pal) >= 4
    assert np.array_equal(is_pal, kind == "palindrome") and is_pal.sum() == 6 and np.sum(r.sym[is_pal] < DEEP) >= 2
    assert np.all(d[is_pal] == 0.0)
    return r


def ordinary(r):
    """indices of the rungs above -600"""
    return np.flatnonzero(r.sym > ORDINARY)


@functools.lru_cache(maxsize=None)
def queue_reference(cid):
    """flip_rows_reference.Reference of the case's rungs in the parity family (the float64 queue with shared prefixes, the four
    float32 realisations, the per-chain yardstick and the energies), random bonds, Bx = 1, for the tile of the f32-input MFMA."""
    c, r = case(cid), rungs(cid)
    return F.Reference("parity", build_params(c), r.s, F.couplings(c.N), F.BX, tile=16)


# ---- the judgements of the GPU test ------------------------------------------------------------------------------------------------

def judge_combine(got, a, b, palindrome=None, equal_to=None):
    """got (...,) against combine(a, b) of the per-direction values under the combine bound; where `palindrome` (a mask over the last
    axis) bit equality with equal_to (default a).  Returns (worst ratio to the bound, [failure texts])."""
    got, want = np.asarray(got, dtype=np.float64), combine(a, b)
    r = over_bound(got, want)
    failures = []
    if palindrome is not None:
        ref = np.asarray(a if equal_to is None else equal_to)
        bad = np.flatnonzero(~(got[..., palindrome] == ref[..., palindrome]).reshape(-1, int(np.sum(palindrome))).all(axis=0))
        if len(bad):
            failures.append("palindromes %s differ from the one-direction value" % np.flatnonzero(palindrome)[bad].tolist())
    if not np.all(r <= 1.0):
        w = np.unravel_index(int(np.argmax(r)), r.shape)
        failures.append("entry %s: %r against %r, %.3g x the bound; %d entries beyond it, %d not finite" %
                        (tuple(int(i) for i in w), float(got[w]), float(want[w]), float(r[w]), int(np.sum(~(r <= 1.0))),
                         int(np.sum(~np.isfinite(got)))))
    return float(r.max()), failures


def judge_rows(got, ref, want=None):
    """got (N + 1, B) against the float64 queue (default ref.lp64) under flip_rows_reference's row bound: (worst ratio, failures)."""
    got = np.asarray(got, dtype=np.float64)
    want = ref.lp64 if want is None else want
    with np.errstate(invalid="ignore"):
        r = np.abs(got - want) / ref.bound
    r = np.where(np.isfinite(got) & np.isfinite(r), r, np.inf)
    failures = []
    if not np.all(r <= 1.0):
        w = np.unravel_index(int(np.argmax(r)), r.shape)
        failures.append("%s: %r against %r, %.3g x the row bound %.3e; %d entries beyond it, %d not finite" %
                        (F.where(ref, int(w[0]), int(w[1])) if r.ndim == 2 else "chain %d" % w[0], float(got[w]), float(want[w]),
                         float(r[w]), float(np.broadcast_to(ref.bound, r.shape)[w]), int(np.sum(~(r <= 1.0))),
                         int(np.sum(~np.isfinite(got)))))
    return float(r.max()), failures
