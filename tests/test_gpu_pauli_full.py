"""The flip-mask pass of rnnwf_pauli_step (csrc/pauli.hip, csrc/pauli_kernels.h) against an independent float64 reference, at the
sizes the library is used and measured at: the case list and the chain-subset rule of tests/test_gpu_renyi_regions_full.py.

Each case draws its chains on the device from SHARPENED weights (kernels x 3, x 2 above 60 units, every bias randomised), takes log r
of every chain and mask, the per-term sums and the samples, and checks

  * log r per chain and mask against tests/pauli_reference.py (brute force in float64 NumPy on the oracle's GRU, scoring the very
    chains the device drew; validated by tests/test_pauli_reference.py) for EVERY mask of the case's set - single sites,
    nearest-neighbour and long-range pairs, a five-site string straddling each 32-site word boundary, checkerboards, site 0, the full
    mask - on a chain subset that the test asserts (check_subset) to contain all 16 chains of the first, a middle and the last full
    16-chain block and EVERY chain of the ragged last block; >= 32 chains on every mask;
  * sums against an exactly rounded float64 re-summation (math.fsum) of the device's OWN log r array, all chains: relative 1e-12;
  * everything finite and the inputs non-trivial: max |log r| > 0.1 and at least a quarter of the checked entries above 0.01.

Bounds - never derived from the kernels:
  * float32: 16 x dev32, dev32 = the largest deviation of the FLOAT32 NumPy oracle from the float64 reference on the same chains and
    masks, computed here at run time; capped at f32_ceiling(N) = 2e-6 N + 2e-6, the rule of tests/correlations_reference.py.  Where
    dev32 itself is beyond the cap, the case says so and 16 x dev32 stands uncapped.
  * float64: 1e-11 N.

Every case prints one PAULI_FULL line with its error, bound and ratio; docs/pauli.md says which figures have been recorded.
"""
import time

import numpy as np
import pytest

import pauli_reference as PR
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


def mask_set(shape):
    names, masks = zip(*PR.mask_set(*shape))
    return list(names), np.stack(masks)


def run(wf, masks, ns):
    return wf.pauli_step(masks, np.zeros_like(masks), np.ones(len(masks)), ns, seed=111, step=0, want_log_ratio=True, want_samples=True)


def check(label, f64, prm, shape, ns, names, masks, out):
    """Everything a case asserts about one pauli_step result with log_ratio and samples.  Returns the comparator's record."""
    t0 = time.time()
    N = shape[0] * shape[1]
    lr, sums, s = out["log_ratio"], out["term_sums"], out["samples"]
    assert lr.shape == (len(masks), ns) and sums.shape == (len(masks), 2) and s.shape == (ns, N)
    assert np.all(np.isfinite(lr)) and np.all(np.isfinite(sums)) and np.all((s == 0) | (s == 1))

    idx = PR.choose_chains(ns)
    PR.check_subset(ns, N, idx, masks)
    ref = PR.log_ratio(prm, s, masks, dtype=np.float64, idx=idx)
    assert ref.shape == (len(masks), len(idx)) and len(idx) >= 32           # every mask on every chosen chain
    mx, share = R.nontrivial(ref)
    if f64:
        bound, dev32, how = PR.f64_bound(N), float("nan"), "1e-11 N"
    else:
        dev32 = float(np.abs(PR.log_ratio(prm, s, masks, dtype=np.float32, idx=idx) - ref).max())
        bound, capped = PR.f32_bound(dev32, N)
        how = "capped at 2e-6 N + 2e-6" if capped else "16 x dev32"
        if dev32 > PR.f32_ceiling(N):
            how = "16 x dev32 UNCAPPED: the float32 oracle itself is beyond the ceiling %.2e" % PR.f32_ceiling(N)
    print("%s %d chains, %d checked x %d masks; max |log r| = %.2f, %.0f %% of %d entries above 0.01; dev32 = %.2e; bound %.3e (%s)"
          % (label, ns, len(idx), len(masks), mx, 100 * share, ref.size, dev32, bound, how))
    d = np.abs(lr[:, idx] - ref)
    k, c = np.unravel_index(int(np.argmax(d)), d.shape)
    err, ratio = float(d[k, c]), float(d[k, c] / bound)
    resum = R.sums_from_log_ratio(lr)                                       # the device's own log r, re-summed exactly
    rel = float(np.abs(sums / resum - 1.0).max())
    print("PAULI_FULL %-28s err %.3e mask %2d (%s) chain %5d block %4d | bound %.3e ratio %6.3f | dev32 %.2e | sums rel %.1e | ref %.1f s"
          % (label, err, k, names[k], idx[c], idx[c] // 16, bound, ratio, dev32, rel, time.time() - t0))
    assert mx > 0.1 and share >= 0.25, "bland inputs: max |log r| %.3f, share above 0.01 %.2f" % (mx, share)
    assert rel <= 1e-12
    assert err <= bound, "%s: |d log r| %.3e > bound %.3e at mask %d (%s), chain %d" % (label, err, bound, k, names[k], idx[c])
    return ratio


# f64, (Nx, Ny), units, chains, what the case is for
CASES = [
    (False, (80, 1), 50, 10006, "the size docs/pauli.md measures; ragged last block of 6 chains"),
    (False, (33, 1), 20, 1000, "one site in the second word of spins and masks"),
    (False, (33, 1), 36, 1000, "one site in the second word of spins and masks"),
    (False, (64, 1), 20, 1000, "two full words"),
    (False, (64, 1), 36, 1000, "two full words"),
    (False, (65, 1), 20, 1000, "one site in the third word"),
    (False, (65, 1), 36, 1000, "one site in the third word"),
    (False, (40, 1), 128, 406, "image read from global memory"),
    (False, (40, 1), 256, 406, "image read from global memory"),
    (False, (100, 1), 100, 602, "four words, the widest LDS-resident f32 image"),
    (True, (6, 6), 50, 2006, "raster model at a lattice size"),                       # weight seed 36, see WEIGHT_SEED
    (True, (4, 8), 53, 602, "the 4-wave instantiations"),
    (True, (4, 8), 68, 602, "the 4-wave instantiations"),
    (True, (8, 8), 100, 602, "the widest f64 model, two words"),
]

# Weight seed 111 (biases 112), with the exception tests/test_gpu_renyi_full.py makes and explains: 6 x 6, 50 units, float64 uses 36.
WEIGHT_SEED = {(True, (6, 6), 50): 36}


def _id(c):
    return "%s-%dx%d-%d-%d" % ("f64" if c[0] else "f32", c[1][0], c[1][1], c[2], c[3])


@pytest.mark.parametrize("f64,shape,H,ns,why", CASES, ids=[_id(c) for c in CASES])
def test_log_ratio_and_sums_against_the_float64_reference(f64, shape, H, ns, why):
    prm = sharpened(H, f64, seed=WEIGHT_SEED.get((f64, shape, H), 111))
    wf = make_wf(f64, shape[0], shape[1], H, prm)
    names, masks = mask_set(shape)
    check("[%s]" % _id((f64, shape, H, ns)), f64, prm, shape, ns, names, masks, run(wf, masks, ns))


def test_several_passes_equal_one_pass_and_the_reference(monkeypatch):
    """N = 80, 50 units, 10 006 chains under a 30 MB state budget: at least three passes of whole 16-chain blocks, the last one partial
    and ragged.  Bit-equal per chain to the one-pass call, and checked against the reference."""
    f64, shape, H, ns = False, (80, 1), 50, 10006
    prm = sharpened(H, f64)
    names, masks = mask_set(shape)

    def timed(wf):
        wf.timing_enable(True)
        wf.timing_reset()
        return run(wf, masks, ns), wf.timing_get(1)["launches"]             # one flip-mask launch per pass

    one, passes_one = timed(make_wf(f64, 80, 1, H, prm))
    monkeypatch.setenv("RNNWF_STATE_BUDGET_MB", "30")
    many, passes = timed(make_wf(f64, 80, 1, H, prm))
    print("[f32-80x1-50-10006 passes] %d pass(es) by default, %d under RNNWF_STATE_BUDGET_MB=30" % (passes_one, passes))
    assert passes_one == 1 and passes >= 3 and ns % 16 != 0
    assert np.array_equal(many["samples"], one["samples"]) and np.array_equal(many["log_ratio"], one["log_ratio"])
    assert np.allclose(many["term_sums"], one["term_sums"], rtol=1e-13, atol=0)
    check("[f32-80x1-50-10006 passes]", f64, prm, shape, ns, names, masks, many)
