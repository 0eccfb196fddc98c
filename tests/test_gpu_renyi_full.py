"""The swap pass of the second Renyi entropy (rnnwf_renyi2_swap: csrc/renyi.hip, csrc/renyi_kernels.h, observables.renyi2_entropy)
against an independent float64 reference, at the sizes the library is used and measured at.

Each case draws its chains on the device from SHARPENED weights (kernels x 3, x 2 above 60 units, every bias randomised, as
tests/test_gpu_sharpened.py and tests/test_gpu_renyi.py), takes log r of every pair and cut, the sums and the samples, and checks

  * log r per pair and cut against tests/renyi_reference.py (brute force in float64 NumPy on the oracle's GRU, scoring the very
    chains the device drew; validated by tests/test_renyi_reference.py) on a subset that the test asserts to contain: all 8 pairs
    of the first, a middle and the last full 16-chain block, EVERY pair of the ragged last block, >= 16 of those pairs at all cuts
    1..N-1, the others at 1, N-1 and both sides of every 32-site word boundary of the packed spins (31, 32, 33, 63, ...); >= 64 pairs;
  * sums against an exactly rounded float64 re-summation of the device's OWN log r array, all pairs: relative 1e-12 (sums of
    positive doubles in another order), and S2, sigma of observables.renyi2_from_sums against the formula written out again;
  * rows 0 and N exactly 0, everything finite, and the inputs non-trivial: max |log r| > 0.1 and at least a quarter of the checked
    entries above 0.01.

No pair is skipped or excluded.  Bounds - derived from tolerances the project already holds, never from the kernels:
  * float32, the bound that decides: 16 x dev32, dev32 = the largest deviation of the FLOAT32 NumPy oracle from the float64
    reference on the same pairs and cuts, computed here at run time - the rule (and the factor) of tests/test_gpu_gradient_full.py.
    The kernels sum in another order and use another exp / tanh than NumPy: a small multiple of one float32 evaluation's error is
    expected, two orders are not.
  * float32, the ceiling: log r = 1/2 (tail_sigma + tail_tau - suffix_sigma - suffix_tau), four partial log-probabilities of at most
    N sites, each held to 2e-6 N + 2e-6 by tests/test_gpu_prnn.py, so 16 x dev32 is capped at 2 (2e-6 N + 2e-6); today's
    tests/test_gpu_renyi.py allows 1e-5 N.  Where dev32 itself is beyond the cap (config 5's precedent in test_gpu_sharpened.py),
    the case says so and 16 x dev32 stands uncapped.
  * float64: 1e-11 N.

Measured on MI355X: profiles/renyi_full_size.txt.
"""
import time

import numpy as np
import pytest

import renyi_reference as R
from rnnwavefunctions_amd import params as P

pytestmark = pytest.mark.gpu

SCOPE = "RNNwavefunction"


def sharpened(H, f64, seed=111):
    prm = P.init_gru_params([H], seed=seed, dtype=np.float64 if f64 else np.float32)
    return P.randomize_biases(P.scale_kernels(prm, 2.0 if H > 60 else 3.0), seed + 1)


def make_wf(f64, Nx, Ny, H, prm):
    from rnnwavefunctions_amd import _lib
    wf = _lib.NativeWavefunction(_lib.MODEL_GRU1D_F64 if f64 else _lib.MODEL_GRU1D, Nx, Ny, (H,))
    wf.set_params(prm, scope=SCOPE)
    return wf


def check(label, f64, prm, N, npairs, out, n_all=32, n_min=128):
    """Everything a case asserts about one renyi2_swap result with log_ratio and samples.  Returns the comparator's record."""
    from rnnwavefunctions_amd.observables import renyi2_from_sums
    t0 = time.time()
    lr, sums, s = out["log_ratio"], out["sums"], out["samples"]
    assert lr.shape == (N + 1, npairs) and sums.shape == (N + 1, 2) and s.shape == (2 * npairs, N)
    assert np.all(np.isfinite(lr)) and np.all(np.isfinite(sums)) and np.all((s == 0) | (s == 1))
    assert np.all(lr[0] == 0.0) and np.all(lr[N] == 0.0)
    assert np.all(sums[[0, N]] == float(npairs))

    # log r per pair and cut
    every, rest = R.choose_subset(npairs, n_min=n_min, n_all=n_all)
    R.check_subset(npairs, N, every, rest, R.boundary_cuts(N))
    pi, ci = R.subset_entries(N, every, rest)
    ref = R.log_ratio_entries(R._scorer(R.to64(prm), np.float64), s, pi, ci)
    mx, share = R.nontrivial(ref)
    if f64:
        bound, dev32, how = R.f64_bound(N), float("nan"), "1e-11 N"
    else:
        r32 = R.log_ratio_entries(R._scorer(R.to32(prm), np.float32), s, pi, ci)
        dev32 = float(np.abs(r32 - ref).max())
        bound, capped = R.f32_bound(dev32, N)
        how = "capped at 2 (2e-6 N + 2e-6)" if capped else "16 x dev32"
        if dev32 > R.f32_ceiling(N):
            how = "16 x dev32 UNCAPPED: the float32 oracle itself is beyond the ceiling %.2e" % R.f32_ceiling(N)
    print("%s %d pairs, %d at all cuts + %d at cuts %s; max |log r| = %.2f, %.0f %% of %d entries above 0.01; dev32 = %.2e; bound %.3e (%s)"
          % (label, npairs, len(every), len(rest), R.boundary_cuts(N).tolist(), mx, 100 * share, len(pi), dev32, bound, how))
    res = R.compare(label, lr[ci, pi], ref, pi, ci, bound)

    # sums: the device's own log r, re-summed exactly
    resum = R.sums_from_log_ratio(lr)
    rel = float(np.abs(sums / resum - 1.0).max())
    S2, err = renyi2_from_sums(sums, npairs)
    S2r, errr = R.entropy_from_sums(sums, npairs)
    S2s, _ = R.entropy_from_sums(resum, npairs)
    dS = float(np.abs(S2 - S2r).max())
    with np.errstate(invalid="ignore", divide="ignore"):
        dE = float(np.nanmax(np.abs(err / errr - 1.0)[1:N]))
    seconds = time.time() - t0
    print("%s sums vs float64 re-summation: max rel %.2e; S2 %.4f .. %.4f; |S2 - restated| %.1e, sigma rel %.1e; host reference %.1f s"
          % (label, rel, S2[1:N].min(), S2[1:N].max(), dS, dE, seconds))
    print("RENYI_FULL %-44s err %.3e cut %3d pair %5d block %4d | bound %.3e ratio %6.3f | dev32 %.2e | sums rel %.1e | ref %.1f s"
          % (label, res["err"], res["cut"], res["pair"], res["block"], bound, res["ratio"], dev32, rel, seconds))
    assert mx > 0.1 and share >= 0.25, "bland inputs: max |log r| %.3f, share above 0.01 %.2f" % (mx, share)
    assert rel <= 1e-12
    assert dS <= 1e-13 and np.all(err[[0, N]] == 0.0) and dE <= 1e-12 and np.abs(S2 - S2s).max() <= 2e-12
    assert res["finite"] and res["err"] <= bound, "%s: |d log r| %.3e > bound %.3e at cut %d, pair %d (block %d)" % (
        label, res["err"], bound, res["cut"], res["pair"], res["block"])
    return res


# f64, (Nx, Ny), units, pairs, what the case is for
CASES = [
    (False, (80, 1), 50, 5000, "the size docs/renyi.md measures (config 2)"),
    (False, (80, 1), 50, 5003, "ns = 10 006: ragged last block of 6 chains, the clamped lane and its partner"),
    (False, (33, 1), 20, 500, "word boundary of the packed spins: one site in the second word"),
    (False, (33, 1), 36, 500, "word boundary of the packed spins: one site in the second word"),
    (False, (64, 1), 20, 500, "two full spin words"),
    (False, (64, 1), 36, 500, "two full spin words"),
    (False, (65, 1), 20, 500, "one site in the third word"),
    (False, (65, 1), 36, 500, "one site in the third word"),
    (False, (200, 1), 100, 1001, "config 5's chain: 7 spin words, the longest tails"),
    (False, (40, 1), 128, 203, "image read from global memory, more than a few steps per tail"),
    (False, (40, 1), 256, 203, "image read from global memory, more than a few steps per tail"),
    (False, (12, 1), 10, 65536 + 4099, "second iteration of renyi_sums_kernel's stride loop, ragged assembly block"),
    (True, (6, 6), 50, 1003, "raster model at a lattice size"),                       # weight seed 36, see WEIGHT_SEED
    (True, (4, 8), 53, 301, "the 4-wave instantiations"),
    (True, (4, 8), 68, 301, "the 4-wave instantiations"),
    (True, (10, 10), 100, 301, "the widest f64 model, 4 spin words"),
]


# Weight seed 111 (biases 112) as tests/test_gpu_sharpened.py, with one exception found on the reference alone, with oracle-drawn pairs:
# at 6 x 6, 50 units, float64, seed 111 gives conditionals so flat that only 17 - 29 % of the entries have |log r| > 0.01, short of
# the quarter a case requires; seed 36 gives 53 - 60 % (max |log r| 5 .. 9).  Sharper inputs, the same share.
WEIGHT_SEED = {(True, (6, 6), 50): 36}


def _id(c):
    return "%s-%dx%d-%d-%d" % ("f64" if c[0] else "f32", c[1][0], c[1][1], c[2], c[3])


@pytest.mark.parametrize("f64,shape,H,npairs,why", CASES, ids=[_id(c) for c in CASES])
def test_log_ratio_and_sums_against_the_float64_reference(f64, shape, H, npairs, why):
    N = shape[0] * shape[1]
    prm = sharpened(H, f64, seed=WEIGHT_SEED.get((f64, shape, H), 111))
    wf = make_wf(f64, shape[0], shape[1], H, prm)
    out = wf.renyi2_swap(npairs, seed=111, step=0, want_log_ratio=True, want_samples=True)
    if N == 12:
        assert (npairs + 255) // 256 > 256 and npairs % 256 != 0          # the stride loop's second round; a ragged assembly block
    check("[%s]" % _id((f64, shape, H, npairs)), f64, prm, N, npairs, out)


def test_three_passes_equal_one_pass_and_the_reference(monkeypatch):
    """N = 80, 50 units, 5 003 pairs under a 30 MB state budget: at least three passes of whole 16-chain blocks, the last one partial
    (pairs per pass are a multiple of 8, 5 003 is not) and ragged.  Bit-equal to the one-pass call, and checked against the
    reference - the last full block and the ragged block lie in the last pass."""
    f64, N, H, npairs = False, 80, 50, 5003
    prm = sharpened(H, f64)

    def run(wf):
        wf.timing_enable(True)
        wf.timing_reset()
        out = wf.renyi2_swap(npairs, seed=111, step=0, want_log_ratio=True, want_samples=True)
        return out, wf.timing_get(2)["launches"]                           # one assembly launch per pass

    one, passes_one = run(make_wf(f64, N, 1, H, prm))
    monkeypatch.setenv("RNNWF_STATE_BUDGET_MB", "30")
    many, passes = run(make_wf(f64, N, 1, H, prm))
    print("[f32-80x1-50-5003 passes] %d pass(es) by default, %d under RNNWF_STATE_BUDGET_MB=30" % (passes_one, passes))
    assert passes_one == 1 and passes >= 3 and npairs % 8 != 0
    assert np.array_equal(many["samples"], one["samples"]) and np.array_equal(many["log_ratio"], one["log_ratio"])
    assert np.allclose(many["sums"], one["sums"], rtol=1e-13, atol=0)
    check("[f32-80x1-50-5003 passes]", f64, prm, N, npairs, many)


def test_facade_gives_the_restated_statistics_of_a_direct_call():
    """observables.renyi2_entropy on the reference-named facade at N = 80, 50 units = S2, sigma by the formula written out again from
    a direct renyi2_swap call with the same seed."""
    from rnnwavefunctions_amd.observables import renyi2_entropy
    from rnnwavefunctions_amd.TFIM1D.RNNwavefunction import RNNwavefunction
    N, H, npairs, seed = 80, 50, 5003, 2024
    prm = sharpened(H, False)
    facade = RNNwavefunction(N, units=[H])
    facade.set_params(prm)
    S2, err = renyi2_entropy(facade, npairs, seed=seed)
    out = make_wf(False, N, 1, H, prm).renyi2_swap(npairs, seed=seed, step=0, want_log_ratio=True)
    S2r, errr = R.entropy_from_sums(R.sums_from_log_ratio(out["log_ratio"]), npairs)
    print("facade N=80: S2 %.4f .. %.4f, sigma up to %.4f; max |S2 - restated| = %.1e, sigma rel %.1e"
          % (S2[1:N].min(), S2[1:N].max(), err.max(), np.abs(S2 - S2r).max(), np.abs(err[1:N] / errr[1:N] - 1).max()))
    assert S2.shape == err.shape == (N + 1,) and S2[0] == 0.0 and S2[N] == 0.0 and err[0] == 0.0 and err[N] == 0.0
    assert S2[1:N].max() > 0.01 and err[1:N].min() > 0
    assert np.abs(S2 - S2r).max() <= 2e-12
    # sigma = sqrt(mean r^2 - (mean r)^2) / (sqrt(n) mean r): the difference under the root amplifies the sums' 1e-12 by
    # mean r^2 / var r, which is below 1e3 at every cut here (asserted)
    sums = R.sums_from_log_ratio(out["log_ratio"])
    amp = (sums[1:N, 1] / npairs) / ((sums[1:N, 1] / npairs) - (sums[1:N, 0] / npairs) ** 2)
    assert amp.max() < 1e3
    assert np.abs(err[1:N] / errr[1:N] - 1).max() <= 1e-9


def test_hand_fed_pairs_that_differ_in_one_spin_word_only():
    """N = 65 (three spin words), 36 units, hand-fed pairs.  Pairs whose halves differ only at sites >= 32 agree on A for every cut
    l <= 32: log r = 0 there; pairs that differ only at sites < 32 agree on B for every cut l >= 32: the swapped chains are tau and
    sigma themselves, log r = 0.  Asserted to the case's bound (and printed whether it is exactly 0); every cut of every pair against
    the reference."""
    N, H, npairs = 65, 36, 64
    prm = sharpened(H, False)
    wf = make_wf(False, N, 1, H, prm)
    base = wf.sample(2 * npairs, 7, 0).reshape(2 * npairs, N).astype(np.int32)       # sigma from the model, tau = sigma with one side redrawn
    rng = np.random.RandomState(65)
    s = base.copy()
    high, low = np.arange(0, npairs // 2), np.arange(npairs // 2, npairs)
    s[2 * high + 1, :32] = s[2 * high, :32]                                          # differ at sites >= 32 only
    s[2 * low + 1, 32:] = s[2 * low, 32:]                                            # differ at sites < 32 only
    s[2 * low + 1, :32] = rng.randint(0, 2, size=(len(low), 32))
    assert np.all((s[2 * high] != s[2 * high + 1])[:, 32:].sum(axis=1) > 0) and np.all((s[2 * low] != s[2 * low + 1])[:, :32].sum(axis=1) > 0)
    out = wf.renyi2_swap(npairs, samples=s, want_log_ratio=True)
    lr = out["log_ratio"]
    cuts = np.arange(1, N)
    ref = R.log_ratio_f64(prm, s, cuts)
    dev32 = float(np.abs(R.log_ratio(prm, s, cuts, dtype=np.float32) - ref).max())
    bound, capped = R.f32_bound(dev32, N)
    assert dev32 <= R.f32_ceiling(N)
    pi, ci = np.meshgrid(np.arange(npairs), cuts, indexing="xy")
    free = np.concatenate([ref[32:][:, high].ravel(), ref[:31][:, low].ravel()])      # the entries that are not 0 by construction
    mx, share = R.nontrivial(free)
    print("[hand-fed N=65] dev32 = %.2e, bound %.3e (%s); max |log r| = %.2f, %.0f %% of the entries that are not 0 by construction above 0.01"
          % (dev32, bound, "capped" if capped else "16 x dev32", mx, 100 * share))
    res = R.compare("[hand-fed N=65]", lr[1:N].ravel(), ref.ravel(), pi.ravel(), ci.ravel(), bound)
    zero_a, zero_b = lr[1:33][:, high], lr[32:N][:, low]
    assert np.abs(ref[:32][:, high]).max() <= 1e-12 and np.abs(ref[31:][:, low]).max() <= 1e-12     # the structure, in the reference
    print("[hand-fed N=65] halves agree on A (cuts 1..32): max |log r| = %.2e (%s); agree on B (cuts 32..64): %.2e (%s)"
          % (np.abs(zero_a).max(), "exactly 0" if not zero_a.any() else "not exactly 0",
             np.abs(zero_b).max(), "exactly 0" if not zero_b.any() else "not exactly 0"))
    print("RENYI_FULL %-44s err %.3e cut %3d pair %5d block %4d | bound %.3e ratio %6.3f | dev32 %.2e |" %
          ("[hand-fed N=65, 36 units, 64 pairs]", res["err"], res["cut"], res["pair"], res["block"], bound, res["ratio"], dev32))
    assert mx > 0.1 and share >= 0.25                       # among the cuts that are not zero by construction
    assert np.abs(zero_a).max() <= bound and np.abs(zero_b).max() <= bound
    assert np.all(np.isfinite(lr)) and res["err"] <= bound
    assert np.all(lr[[0, N]] == 0.0)
    assert np.abs(out["sums"] / R.sums_from_log_ratio(lr) - 1.0).max() <= 1e-12
