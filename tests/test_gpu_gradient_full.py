"""EVERY element of the VMC-cost gradient against exact float64 autograd, at the sizes the project is benchmarked at.

Each case draws its batch with vmc_step on SHARPENED weights (kernels x 3, every bias randomised, as tests/test_gpu_sharpened.py),
takes cost_gradient(...) and compares every element of every tensor with the gradient one reverse-mode pass of the float64 torch
restatement (tests/autograd_reference.py, validated by tests/test_autograd_reference.py) gives for the same samples and local
energies.  Per tensor, normalised by that tensor alone:  max |g_hip - g_ref| / max |g_ref|  and  ||g_hip - g_ref||_2 / ||g_ref||_2.

Bounds - measured against the reference, never against the kernel:
  * float32 families: the yardstick of each case and tensor is the deviation of the FLOAT32 torch restatement from the float64 one
    on the same batch, computed here, so the bound follows the case's conditioning.  The HIP gradient must stay within 16 x the
    yardstick in both norms, every tensor.  (16: the yardstick is one realisation of f32 rounding; the kernels sum 1e5 - 1e6 rows in
    other block shapes and orders and start from checkpoints the bf16x3 base pass wrote.)
  * float64 families: the same yardstick scaled by the ratio of the unit round-offs, 16 x 2^-29 x (f32-vs-f64 deviation).
  * a tensor whose reference is zero to rounding: absolute, against 16 x max |g32 - g64| of that tensor.
test_autograd_reference.py shows on the reference alone that this bound rejects one chain of 10 000 dropped, one input of 80 shifted
by a site, and one tensor scaled by 1.001.

Which path ran.  The handle exposes the forward engine (engine_name), the device's CU count and, per gradient, the number of
backward passes and weight-gradient products (timers 3 and 4).  Those are asserted.  Whether a one-layer float32 batch took the
two-waves-per-block GradPair kernel or the four-wave persistent one is NOT observable: it follows the documented threshold - pair
while ceil(ns / 16) <= 2 x CUs (8 192 chains on 256 CUs) and the width fits - so each case asserts on which side of that threshold
it stands, the 8 192 / 8 208 cases bracket it, and RNNWF_NO_COOP=1 on a fresh handle sends the run-script batch down the four-wave
kernel.

Largest ratio deviation / yardstick observed on MI355X per family (profiles/gradient_full_size.txt; bound 16; the whole module takes
about 20 s there, the references 0.1 - 2.2 s each):
    GRU f32, one layer        3.5 at config 2's size (ragged batch); 11.0 on the run-script batch under RNNWF_NO_COOP=1, where the
                              two-element wf_dense/bias is one float32 ulp (9.9e-8) from float64 and its yardstick happens to be 9.0e-9
    GRU f32, stacks           8.2 (units (64, 20): layer 0's candidate biases, 1.1e-5 against a yardstick of 1.4e-6); cfg2_l2 1.8
    parity-symmetric          1.2
    complex U(1)              1.4 (one layer 1.3)
    GRU f64 on the raster     2.6 (100 units; the stack 0.8)
    MDRNN f64                 2.1
No case exceeded the bound; no kernel defect was found at these sizes and paths.
"""
import os
import time

import numpy as np
import pytest
import torch

import autograd_reference as A
from rnnwavefunctions_amd import params as P

pytestmark = pytest.mark.gpu
SCOPE = A.SCOPE
HEADS = ("wf_dense_ampl", "wf_dense_phase")


def build(family, shape, units, seed, sharp=3.0):
    """(model id, sharpened parameters: kernels x sharp and every bias randomised, couplings of the family's Hamiltonian)."""
    from rnnwavefunctions_amd import _lib
    N = shape[0] * shape[1]

    def sharpened(prm, seed):
        return P.randomize_biases(P.scale_kernels(prm, sharp), seed)

    if family == "mdrnn":
        return _lib.MODEL_MDRNN2D, sharpened(P.init_mdrnn_params(units[0], seed=seed), seed + 1), np.append(np.ones(N), 3.0)
    if family == "crnn":
        prm = sharpened(P.init_gru_params(list(units), seed=seed, heads=HEADS), seed + 1)
        return _lib.MODEL_CRNN_U1, prm, np.concatenate([np.ones(N), 0.5 * np.ones(N), np.zeros(N), [0.0, 0.0]])
    if family == "gru64":
        return _lib.MODEL_GRU1D_F64, sharpened(P.init_gru_params(list(units), seed=seed, dtype=np.float64), seed + 1), np.append(np.ones(N), 3.0)
    mid = _lib.MODEL_GRU1D_PARITY if family == "parity" else _lib.MODEL_GRU1D
    return mid, sharpened(P.init_gru_params(list(units), seed=seed), seed + 1), np.append(np.ones(N), 1.0)


def hip_gradient(wf, prm, e, ns):
    """cost_gradient with the timers on: (gradient, backward passes, weight-gradient products)."""
    from rnnwavefunctions_amd.training import cost_gradient
    wf.timing_enable(True)
    wf.timing_reset()
    g = cost_gradient(wf, prm, SCOPE, e.mean(), ns)
    return g, wf.timing_get(3)["launches"], wf.timing_get(4)["launches"]


def reference(family, prm, s, e):
    """(float64 autograd gradient, float32 autograd gradient, seconds)."""
    t0 = time.time()
    fam = "gru" if family == "gru64" else family
    g64 = A.gradient(fam, prm, s, e, dtype=torch.float64)
    g32 = A.gradient(fam, prm, s, e, dtype=torch.float32)
    return g64, g32, time.time() - t0


def judge(label, family, prm, grads, g64, g32):
    assert set(grads) == set(prm)
    for k in prm:
        assert grads[k].shape == prm[k].shape, k
        assert np.all(np.isfinite(grads[k])), k
    scale = A.F64_OVER_F32 if family in ("gru64", "mdrnn") else 1.0
    worst, failures = A.verdict(grads, g64, g32, unit_roundoff_ratio=scale, label=label)
    print("%s worst ratio deviation / yardstick = %.3f (bound %g)" % (label, worst, A.FACTOR))
    return worst, failures


# family, lattice, units, samples, kernel scale, side of the pair threshold the batch must stand on ("pair": ceil(ns / 16) <= 2 CUs,
# "persistent": above it, None: the width has no pair kernel or the model no such choice), forward engine.  Reference time: both
# autograd passes (float64 + float32) on 16 threads, as measured next to the MI355X; the largest keeps 11 GB of activations.
# Kernel scale: 3 as in tests/test_gpu_sharpened.py, with two exceptions that are stated, not fitted.  (a) The 2D RNN's elu cell is
# unbounded: at x 3 (even x 1.5) its state grows along the 23-site diagonals until every conditional past the first row is exactly
# 0 or 1 - the reference gradient of Wv / Uv is then exactly ZERO and the float32 restatement overflows, which tests nothing; x 1.25
# keeps the conditionals sharp (log P of a 144-site sample -5 .. -28) and every tensor's gradient alive.  (b) At N = 200, 100 units,
# x 3 the recurrence amplifies rounding so much (test_gpu_sharpened.py: config 5) that float32 itself is off by percents and the
# yardstick is loose; the case runs as specified AND at x 1.5, where the float32 yardstick is back at 4e-7 and the bound is tight.
CASES = [
    # BASELINE config 2: the four-wave persistent kernel over 625 blocks of 16 chains, bf16x3 checkpoints                  [ref 1.6 s]
    ("gru", (80, 1), (50,), 10000, 3.0, "persistent", "bf16x3"),
    # ... and a ragged last block (10 007 = 625 x 16 + 7)                                                               [ref 1.2 s]
    ("gru", (80, 1), (50,), 10007, 3.0, "persistent", "bf16x3"),
    # the last batch of the pair path (512 blocks on 256 CUs) and the first of the persistent one (513)                   [ref 1.0 s, 0.8 s]
    ("gru", (80, 1), (50,), 8192, 3.0, "pair", "bf16x3"),
    ("gru", (80, 1), (50,), 8208, 3.0, "persistent", "bf16x3"),
    # N = 200, 100 units: 7 spin words per chain, the backward operand read through L2 (GradStream; no pair kernel at this width) [ref 2.2 s, 1.7 s]
    ("gru", (200, 1), (100,), 4096, 3.0, None, "bf16x3"),
    ("gru", (200, 1), (100,), 4096, 1.5, None, "bf16x3"),
    # above 100 units: the kernels of grad_wide.hip, the forward image through L2 as well                                   [ref 0.4 s]
    ("gru", (40, 1), (128,), 4096, 3.0, None, "f32mfma"),
    # config 2 with two layers (cfg2_l2): MLGrad with NL > 1 at scale                                                       [ref 2.1 s]
    ("gru", (80, 1), (50, 50), 10000, 3.0, "persistent", "bf16x3"),
    # unequal widths: the narrower layer is padded inside the library, unpack drops the padding                              [ref 0.7 s]
    ("gru", (40, 1), (64, 20), 10000, 3.0, "persistent", "f32mfma"),
    # parity-symmetric: two backward passes, each sample weighted by the direction's share                                   [ref 0.8 s]
    ("parity", (40, 1), (50,), 9008, 3.0, "persistent", "bf16x3"),
    # BASELINE config 3: complex cost, amplitude and phase heads; and two layers                                            [ref 0.6 s, 1.1 s]
    ("crnn", (40, 1), (50,), 10000, 3.0, "persistent", "bf16x3"),
    ("crnn", (40, 1), (50, 50), 10000, 3.0, "persistent", "bf16x3"),
    # float64 GRU on the 12 x 12 raster at its largest one-layer width (100 units: grad_wide.hip), and a stack                [ref 1.0 s, 1.4 s]
    ("gru64", (12, 12), (100,), 2048, 3.0, None, "f64mfma"),
    ("gru64", (12, 12), (50, 50), 2048, 3.0, None, "f64mfma"),
    # BASELINE config 4: the 2D RNN on the zig-zag path (mdrnn_grad_kernels.h), all 10 000 samples                              [ref 1.7 s]
    ("mdrnn", (12, 12), (50,), 10000, 1.25, None, "f64mfma"),
]


def _id(c):
    return "%s-%dx%d-%s-%d-x%g" % (c[0], c[1][0], c[1][1], "x".join(map(str, c[2])), c[3], c[4])


@pytest.mark.parametrize("family,shape,units,ns,sharp,side,engine", CASES, ids=[_id(c) for c in CASES])
def test_every_gradient_element_against_float64_autograd(family, shape, units, ns, sharp, side, engine):
    from rnnwavefunctions_amd import _lib
    mid, prm, couplings = build(family, shape, units, seed=111, sharp=sharp)
    wf = _lib.NativeWavefunction(mid, shape[0], shape[1], units)
    wf.set_params(prm, scope=SCOPE)
    out = wf.vmc_step(ns, seed=111, step=0, couplings=couplings, want_samples=True, want_eloc=True)
    s = out["samples"]
    e = out["eloc"].astype(np.complex128) if family == "crnn" else out["eloc"]
    grads, n_bwd, n_gemm = hip_gradient(wf, prm, e, ns)
    cus, nsb = wf.device_info()["cu_count"], (ns + 15) // 16
    label = "[%s]" % _id((family, shape, units, ns, sharp))
    print("%s engine %s, %d CUs, %d blocks of 16 chains (pair threshold %d), %d backward passes, %d weight-gradient products" %
          (label, wf.engine_name(), cus, nsb, 2 * cus, n_bwd, n_gemm))
    g64, g32, seconds = reference(family, prm, s, e)
    print("%s reference (float64 + float32 autograd): %.1f s" % (label, seconds))
    worst, failures = judge(label, family, prm, grads, g64, g32)
    # which path ran, from what the handle exposes
    passes = len(units) * (2 if family == "parity" else 1)
    assert (n_bwd, n_gemm) == (passes, passes)
    assert wf.engine_name() == engine
    if side == "pair":
        assert nsb <= 2 * cus
    elif side == "persistent":
        assert nsb > 2 * cus
    assert not failures, "tensors beyond %g x the yardstick: %s" % (A.FACTOR, failures)


def test_run_script_batch_on_the_pair_kernel_and_on_the_four_wave_kernel():
    """1DTFIM/run_1dTFIM.py's size (N = 20, 50 units, 500 samples = 32 blocks): GradPair by default; the SAME batch loaded into a
    fresh handle created under RNNWF_NO_COOP=1 takes the four-wave persistent kernel (GruGrad::run).  Each against the reference. [ref < 0.1 s]"""
    from rnnwavefunctions_amd import _lib
    family, shape, units, ns = "gru", (20, 1), (50,), 500
    mid, prm, couplings = build(family, shape, units, seed=111)
    wf = _lib.NativeWavefunction(mid, shape[0], 1, units)
    wf.set_params(prm, scope=SCOPE)
    out = wf.vmc_step(ns, seed=111, step=0, couplings=couplings, want_samples=True, want_eloc=True)
    s, e = out["samples"], out["eloc"]
    cus = wf.device_info()["cu_count"]
    assert (ns + 15) // 16 <= 2 * cus                      # pair-eligible
    assert wf.engine_name() == "f32mfma"                   # a batch this small: cooperative base pass, 16-chain f32 flip kernel
    g_pair, n_bwd, n_gemm = hip_gradient(wf, prm, e, ns)
    assert (n_bwd, n_gemm) == (1, 1)
    assert "RNNWF_NO_COOP" not in os.environ
    os.environ["RNNWF_NO_COOP"] = "1"                      # read once per handle, at creation
    try:
        wf4 = _lib.NativeWavefunction(mid, shape[0], 1, units)
    finally:
        del os.environ["RNNWF_NO_COOP"]
    wf4.set_params(prm, scope=SCOPE)
    wf4.load_batch(s, e)
    g_four, n_bwd, n_gemm = hip_gradient(wf4, prm, e, ns)
    assert (n_bwd, n_gemm) == (1, 1)
    g64, g32, seconds = reference(family, prm, s, e)
    print("[run-script size] engine %s, %d CUs, reference %.1f s" % (wf.engine_name(), cus, seconds))
    results = [judge("[gru-20x1-50-500 pair]", family, prm, g_pair, g64, g32),
               judge("[gru-20x1-50-500 RNNWF_NO_COOP=1]", family, prm, g_four, g64, g32)]
    same = all(np.array_equal(g_pair[k], g_four[k]) for k in g_pair)
    print("[run-script size] pair and four-wave gradients bit-identical: %s" % same)
    for worst, failures in results:
        assert not failures, "tensors beyond %g x the yardstick: %s" % (A.FACTOR, failures)
