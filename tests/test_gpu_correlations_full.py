"""The correlation pass (rnnwf_correlations: csrc/corr.hip, csrc/corr_kernels.h) against an independent float64 reference, at the
sizes the library is used and measured at.

Each case draws its chains on the device from SHARPENED weights (kernels x 3, x 2 above 60 units, every bias randomised, as
tests/test_gpu_sharpened.py and tests/test_gpu_renyi_full.py), takes every log r_i and log r_ij of every chain, the sums and the
samples, and checks

  * log r against tests/correlations_reference.py (brute force in float64 NumPy on the oracle's GRU, every flipped configuration
    scored from site 0; validated by tests/test_correlations_reference.py) on a subset that the test asserts to contain: >= 32
    chains at EVERY single flip and pair, among them eight of the first, a middle and the last full 16-chain block and every chain
    of the ragged last block; 32 further chains at every single flip and at the pairs of distance 1, of distance N - 1 and
    straddling each 32-site word boundary of the packed spins;
  * every *_sums array against an exactly rounded float64 re-summation (math.fsum) of the device's OWN log-ratio array over all
    chains, relative 1e-12, and the diagonal sums against integer sums of the samples (exact);
  * everything finite, and the inputs non-trivial: max |log r| > 0.1 and at least a quarter of the checked entries above 0.01.

Bounds - derived from tolerances the project already holds, never from the kernels:
  * float32: 16 x dev32, dev32 = the largest deviation of the FLOAT32 NumPy oracle from the float64 reference on the same entries,
    computed here at run time - the rule (and the factor) of tests/test_gpu_gradient_full.py - capped at 2e-6 N + 2e-6: log r is
    half the difference of two partial log-probabilities of at most N sites, each held to that by tests/test_gpu_prnn.py.  Where
    dev32 itself is beyond the cap the case says so and 16 x dev32 stands uncapped.
  * float64: 1e-11 N.

Batches are sized so that a case's host reference stays within a few minutes on 16 cores.  Measured on MI355X:
profiles/corr_full_size.txt.
"""
import time

import numpy as np
import pytest

import correlations_reference as R
from rnnwavefunctions_amd import params as P

pytestmark = pytest.mark.gpu

SCOPE = "RNNwavefunction"
KEYS = ("z_sums", "zz_sums", "x_sums", "xx_sums")


def sharpened(H, f64, seed=111):
    prm = P.init_gru_params([H], seed=seed, dtype=np.float64 if f64 else np.float32)
    return P.randomize_biases(P.scale_kernels(prm, 2.0 if H > 60 else 3.0), seed + 1)


def make_wf(f64, Nx, Ny, H, prm):
    from rnnwavefunctions_amd import _lib
    wf = _lib.NativeWavefunction(_lib.MODEL_GRU1D_F64 if f64 else _lib.MODEL_GRU1D, Nx, Ny, (H,))
    wf.set_params(prm, scope=SCOPE)
    return wf


def check(label, f64, prm, N, ns, out):
    """Everything a case asserts about one correlations result with log_ratio and samples.  Returns the comparator's record."""
    t0 = time.time()
    lr, s = out["log_ratio"], out["samples"]
    rows = N + N * (N - 1) // 2
    assert lr.shape == (rows, ns) and s.shape == (ns, N) and np.all((s == 0) | (s == 1))
    assert np.all(np.isfinite(lr)) and all(np.all(np.isfinite(out[k])) for k in KEYS)

    every, rest = R.choose_subset(ns)
    bi, bj = R.boundary_pairs(N)
    R.check_subset(ns, N, every, rest, bi, bj)
    ci, ii, jj = R.subset_entries(N, every, rest)
    ref = R.log_ratio_entries(R.scorer(prm, np.float64), s, ci, ii, jj)
    mx, share = R.nontrivial(ref)
    if f64:
        bound, dev32, how = R.f64_bound(N), float("nan"), "1e-11 N"
    else:
        r32 = R.log_ratio_entries(R.scorer(prm, np.float32), s, ci, ii, jj)
        dev32 = float(np.abs(r32 - ref).max())
        bound, capped = R.f32_bound(dev32, N)
        how = "capped at 2e-6 N + 2e-6" if capped else "16 x dev32"
        if dev32 > R.f32_ceiling(N):
            how = "16 x dev32 UNCAPPED: the float32 oracle itself is beyond the ceiling %.2e" % R.f32_ceiling(N)
    print("%s %d chains, %d at every pair + %d at %d boundary pairs; max |log r| = %.2f, %.0f %% of %d entries above 0.01; dev32 = %.2e; "
          "bound %.3e (%s)" % (label, ns, len(every), len(rest), len(bi), mx, 100 * share, len(ci), dev32, bound, how))
    res = R.compare(label, lr[R.row_of(ii, jj, N), ci], ref, ci, ii, jj, bound)

    xs, xxs = R.sums_from_log_ratio(lr, N)
    zs, zzs = R.diag_sums(s)
    iu = np.triu_indices(N, 1)
    rel = max(float(np.abs(out["x_sums"] / xs - 1.0).max()), float(np.abs(out["xx_sums"][iu] / xxs[iu] - 1.0).max()) if N > 1 else 0.0)
    seconds = time.time() - t0
    print("CORR_FULL %-40s err %.3e pair (%3d,%3d) chain %5d block %4d | bound %.3e ratio %6.3f | dev32 %.2e | sums rel %.1e | ref %.1f s"
          % (label, res["err"], res["i"], res["j"], res["chain"], res["block"], bound, res["ratio"], dev32, rel, seconds))
    assert mx > 0.1 and share >= 0.25, "bland inputs: max |log r| %.3f, share above 0.01 %.2f" % (mx, share)
    assert rel <= 1e-12
    assert np.all(out["xx_sums"][np.tril_indices(N)] == 0.0)
    assert np.array_equal(out["z_sums"], zs) and np.array_equal(out["zz_sums"], zzs)
    assert res["finite"] and res["err"] <= bound, "%s: |d log r| %.3e > bound %.3e at pair (%d, %d), chain %d (block %d)" % (
        label, res["err"], bound, res["i"], res["j"], res["chain"], res["block"])
    return res


# f64, (Nx, Ny), units, chains, what the case is for
CASES = [
    (False, (80, 1), 50, 1000, "the size docs/correlations.md measures"),
    (False, (80, 1), 50, 1003, "ragged last block of 11 chains, the clamped lanes"),
    (False, (33, 1), 20, 203, "word boundary of the packed spins: one site in the second word"),
    (False, (33, 1), 36, 203, "word boundary of the packed spins: one site in the second word"),
    (False, (64, 1), 20, 203, "two full spin words"),
    (False, (64, 1), 36, 203, "two full spin words"),
    (False, (65, 1), 20, 203, "one site in the third word"),
    (False, (65, 1), 36, 203, "one site in the third word"),
    (False, (40, 1), 128, 107, "image read from global memory"),
    (False, (40, 1), 256, 107, "image read from global memory"),
    (False, (100, 1), 100, 107, "four spin words, the longest tails, a small batch"),
    (True, (6, 6), 50, 203, "raster model at a lattice size"),                        # weight seed 36, see WEIGHT_SEED
    (True, (4, 8), 53, 107, "the 4-wave instantiations"),
    (True, (4, 8), 68, 107, "the 4-wave instantiations"),
    (True, (8, 8), 100, 107, "the widest f64 model, two full spin words"),
]

# Weight seed 111 (biases 112) as tests/test_gpu_sharpened.py; 6 x 6, 50 units, float64 takes seed 36 as in
# tests/test_gpu_renyi_full.py (seed 111 gives conditionals so flat there that the share of non-trivial entries is marginal).
WEIGHT_SEED = {(True, (6, 6), 50): 36}


def _id(c):
    return "%s-%dx%d-%d-%d" % ("f64" if c[0] else "f32", c[1][0], c[1][1], c[2], c[3])


@pytest.mark.parametrize("f64,shape,H,ns,why", CASES, ids=[_id(c) for c in CASES])
def test_log_ratio_and_sums_against_the_float64_reference(f64, shape, H, ns, why):
    N = shape[0] * shape[1]
    prm = sharpened(H, f64, seed=WEIGHT_SEED.get((f64, shape, H), 111))
    wf = make_wf(f64, shape[0], shape[1], H, prm)
    out = wf.correlations(ns, seed=111, step=0, want_log_ratio=True, want_samples=True)
    check("[%s]" % _id((f64, shape, H, ns)), f64, prm, N, ns, out)


@pytest.mark.parametrize("ns", [1000, 1003])
def test_several_passes_equal_one_pass_and_the_reference(ns, monkeypatch):
    """N = 80, 50 units under a 64 MB state budget: a 16-chain block needs about 12.4 MB (3 160 trunk states and 79 checkpoints of
    3 328 bytes, 12 960 doubles per chain), so a pass holds 5 blocks and the call takes 13 passes, the last one partial (and, at
    1 003 chains, ragged).  Per-chain log-ratios bit-equal to the one-pass call; checked against the reference as well."""
    f64, N, H = False, 80, 50
    prm = sharpened(H, f64)

    def run(wf):
        wf.timing_enable(True)
        wf.timing_reset()
        out = wf.correlations(ns, seed=111, step=0, want_log_ratio=True, want_samples=True)
        return out, wf.timing_get(2)["launches"]                           # one assembly bracket per pass

    one, passes_one = run(make_wf(f64, N, 1, H, prm))
    monkeypatch.setenv("RNNWF_STATE_BUDGET_MB", "64")
    many, passes = run(make_wf(f64, N, 1, H, prm))
    print("[f32-80x1-50-%d passes] %d pass(es) by default, %d under RNNWF_STATE_BUDGET_MB=64" % (ns, passes_one, passes))
    assert passes_one == 1 and passes >= 3
    assert np.array_equal(many["samples"], one["samples"]) and np.array_equal(many["log_ratio"], one["log_ratio"])
    assert np.array_equal(many["z_sums"], one["z_sums"]) and np.array_equal(many["zz_sums"], one["zz_sums"])
    assert np.allclose(many["x_sums"], one["x_sums"], rtol=1e-12, atol=0) and np.allclose(many["xx_sums"], one["xx_sums"], rtol=1e-12, atol=0)
    check("[f32-80x1-50-%d passes]" % ns, f64, prm, N, ns, many)


def test_facade_gives_the_restated_statistics_of_a_direct_call():
    """observables.correlations on the reference-named facade at N = 80, 50 units = the statistics written out again
    (correlations_reference.stats_from_sums) from the exactly re-summed log-ratios of a direct call with the same seed."""
    from rnnwavefunctions_amd.observables import correlations
    from rnnwavefunctions_amd.TFIM1D.RNNwavefunction import RNNwavefunction
    N, H, ns, seed = 80, 50, 1003, 2024
    prm = sharpened(H, False)
    facade = RNNwavefunction(N, units=[H])
    facade.set_params(prm)
    c = correlations(facade, ns, seed=seed)
    out = make_wf(False, N, 1, H, prm).correlations(ns, seed=seed, step=0, want_log_ratio=True, want_samples=True)
    xs, xxs = R.sums_from_log_ratio(out["log_ratio"], N)
    zs, zzs = R.diag_sums(out["samples"])
    ref = R.stats_from_sums(zs, zzs, xs, xxs, ns)
    for k in ("z", "zz", "x", "xx", "zz_c", "xx_c"):
        assert np.abs(c[k] - ref[k]).max() <= 1e-11, k
    for k in ("z_err", "zz_err", "zz_c_err"):
        assert np.allclose(c[k], ref[k], rtol=1e-9, atol=1e-12), k
    # errors of x and xx: a difference under the root amplifies the sums' 1e-12 by mean q^2 / var q
    for k in ("x_err", "xx_err", "xx_c_err"):
        assert np.allclose(c[k], ref[k], rtol=1e-6, atol=1e-9), k
    assert np.abs(c["xx_c"][np.triu_indices(N, 1)]).max() > 1e-3
