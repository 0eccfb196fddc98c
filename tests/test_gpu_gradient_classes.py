"""EVERY element of the VMC-cost gradient against exact float64 autograd, for EVERY gradient kernel class.

tests/test_gpu_gradient_full.py does this at the benchmarked sizes and reaches seven classes; with_gru_grad / gru_widths (grad.hip) pick
one class per (family, layers, NFULL) - 23 for the positive GRU, 23 for the complex one, 17 for the float64 GRU - the 2D RNN has five
of its own (mdrnn.hip) and the parity-symmetric model runs the positive GRU's twice per gradient.  The table of
tests/gradient_classes_reference.py (its docstring names the lines of the dispatch code it restates) has at least one case per class,
both ends of every one-layer width class, first and last widths alternating over the stacks, stacks of unequal widths, five chain
lengths, all at the smallest shapes at which these kernels can still go wrong: 33 / 34 sites or a 11 x 3, 17 x 2, 7 x 5 lattice, 40
samples (two full 16-chain blocks and a ragged one of 8).  Each case draws its batch with vmc_step on sharpened weights, takes
cost_gradient(...) and compares every element of every tensor with one float64 reverse-mode pass of tests/autograd_reference.py.

The bound.  autograd_reference.verdict as test_gpu_gradient_full.py uses it: per tensor and in both norms (max and l2, normalised by
that tensor of the reference alone) at most 16 x the deviation of the FLOAT32 autograd gradient from the float64 one on the same
batch; x 2^-29 for the float64 families; absolute for a tensor whose reference is zero to rounding.
The floor.  At 40 samples that deviation can collapse far below one ulp of what is summed (docs/sr.md: 1.0e-9 against 4.1e-8 on
wf_dense/bias), so a tensor's yardstick is the LARGER of it and  N x unit round-off of the model's type x max_k sum_s |w_s d log
psi_s / d theta_k| / max |g_ref|  (the expression of tests/test_gpu_sr.py's tie bound), from the reference's float64 per-sample
derivatives.  Every printed tensor line says which of the two applied.  No other constant.

What the bound rejects is shown on the reference alone by tests/test_gradient_classes_reference.py, at one case per family and layer
count (its REJECT_CASES): the last chain of the ragged block dropped; the last site's term dropped; the one-hot fed into site 32
taken from site 31 (void, and so not claimed, where the batch's spins agree there: the two- and three-layer complex and the
two-layer parity case); the last unit dropped from the reset gate's recurrent product (2D RNN: from the horizontal product); any
one tensor x 1.001 and one unit's row of it x 1.001 (except the one-layer complex case's phase bias, bound
1.0e-4, and most tensors of the three-layer complex case, where float32 autograd itself is 0.6e-4 .. 3e-4 off); for stacks the top layer fed the wrong layer below; for the complex model the phase's weight in the cost negated; for the
parity model the two directions' shares swapped.  The same module shows that the bound accepts, on every case of the table, the
float64 gradient rounded to the model's type and a second float32 evaluation in another summation order.

Which kernel ran.  Asserted from what the handle exposes: engine_name() and the launch counts of timers 3 and 4 (layers x 2 for the
parity model).  A batch of 3 blocks is pair-eligible on any device (3 <= 2 x CUs), so in the classes that have the two-waves-per-block
kernel (GradPair::FITS: NFULL 1, 2, 3 of the f32 families, gradient_classes_reference.pair_fits) the table's run IS the pair kernel;
test_pair_kernel_and_four_wave_kernel runs one case of each such class on the default handle and again, same batch through
load_batch, on a handle created under RNNWF_NO_COOP=1 (the four-wave persistent kernel), scores both, and prints whether they agree
bit for bit - not asserted: the pair kernel's forward wave and the four-wave kernel re-compute the gates in different code.

Largest deviation / bound observed on MI355X per family (profiles/gradient_width_classes.txt; limit 16; the whole module takes about
45 s there, 0.0 - 0.7 s per case, nearly all of it the references):
    GRU f32         3.85 (four layers of 17 units under RNNWF_NO_COOP=1; the table's cases at most 2.1)
    complex U(1)    1.76
    GRU f64         1.78
    parity          1.53
    2D RNN          1.94
No case exceeded the bound; no kernel defect was found.
"""
import os
import time

import numpy as np
import pytest

import autograd_reference as A
import gradient_classes_reference as G

pytestmark = pytest.mark.gpu
SCOPE = G.SCOPE


def hip_gradient(wf, prm, e, ns):
    """cost_gradient with the timers on: (gradient, backward passes, weight-gradient products)."""
    from rnnwavefunctions_amd.training import cost_gradient
    wf.timing_enable(True)
    wf.timing_reset()
    g = cost_gradient(wf, prm, SCOPE, e.mean(), ns)
    return g, wf.timing_get(3)["launches"], wf.timing_get(4)["launches"]


def handle(c, prm):
    from rnnwavefunctions_amd import _lib
    wf = _lib.NativeWavefunction(G.model_id(c), c.shape[0], c.shape[1], c.units)
    wf.set_params(prm, scope=SCOPE)
    return wf


def drawn(c, wf):
    out = wf.vmc_step(c.ns, seed=111, step=0, couplings=G.couplings(c), want_samples=True, want_eloc=True)
    return out["samples"], (out["eloc"].astype(np.complex128) if c.family == "crnn" else out["eloc"])


def checked(label, c, prm, grads, ref):
    assert set(grads) == set(prm)
    for k in prm:
        assert grads[k].shape == prm[k].shape, k
        assert np.all(np.isfinite(grads[k])), k
    return G.judge(label, c, grads, ref)


@pytest.mark.parametrize("c", G.CASES, ids=G.IDS)
def test_every_gradient_element_of_every_class(c):
    t0 = time.time()
    prm = G.parameters(c)
    wf = handle(c, prm)
    s, e = drawn(c, wf)
    grads, n_bwd, n_gemm = hip_gradient(wf, prm, e, c.ns)
    cus, nsb, name = wf.device_info()["cu_count"], (c.ns + 15) // 16, wf.engine_name()
    wf.close()
    ref = G.reference(c, prm, s, e)
    label = "[%s]" % G.case_id(c)
    worst, failures = checked(label, c, prm, grads, ref)
    nf = G.nfull(c.family, c.units)
    print("CLASS %s NFULL %d layers %d%s: engine %s, %d blocks, launches %d + %d, worst deviation / bound %.3f (limit %g), reference %.2f s, "
          "case %.2f s" % (label, nf, len(c.units), " pair" if G.pair_fits(c.family, nf) else "", name, nsb, n_bwd, n_gemm, worst, A.FACTOR,
                           ref.seconds, time.time() - t0))
    assert (n_bwd, n_gemm) == (G.passes(c), G.passes(c))
    assert name == G.engine(c)
    assert nsb <= 2 * cus                                   # pair-eligible wherever the class has the pair kernel
    assert not failures, "tensors beyond %g x the bound: %s" % (A.FACTOR, failures)


@pytest.mark.parametrize("c", G.PAIR_CASES, ids=[G.case_id(c) for c in G.PAIR_CASES])
def test_pair_kernel_and_four_wave_kernel(c):
    """One case of every class with GradPair::FITS: the default handle (3 blocks <= 2 x CUs: GradPair) and a fresh handle created under
    RNNWF_NO_COOP=1 with the same batch loaded (the four-wave persistent kernel, GLaunch::run), each against the reference."""
    prm = G.parameters(c)
    wf = handle(c, prm)
    s, e = drawn(c, wf)
    assert (c.ns + 15) // 16 <= 2 * wf.device_info()["cu_count"]
    g_pair, n_bwd, n_gemm = hip_gradient(wf, prm, e, c.ns)
    wf.close()
    assert (n_bwd, n_gemm) == (G.passes(c), G.passes(c))
    assert "RNNWF_NO_COOP" not in os.environ
    os.environ["RNNWF_NO_COOP"] = "1"                       # read once per handle, at creation
    try:
        wf4 = handle(c, prm)
    finally:
        del os.environ["RNNWF_NO_COOP"]
    wf4.load_batch(s, e)
    g_four, n_bwd, n_gemm = hip_gradient(wf4, prm, e, c.ns)
    wf4.close()
    assert (n_bwd, n_gemm) == (G.passes(c), G.passes(c))
    ref = G.reference(c, prm, s, e)
    label = "[%s" % G.case_id(c)
    results = [checked(label + " pair]", c, prm, g_pair, ref), checked(label + " RNNWF_NO_COOP=1]", c, prm, g_four, ref)]
    same = all(np.array_equal(g_pair[k], g_four[k]) for k in g_pair)
    print("PAIR %s] NFULL %d layers %d: worst deviation / bound pair %.3f, four-wave %.3f (limit %g); bit-identical: %s; reference %.2f s" %
          (label, G.nfull(c.family, c.units), len(c.units), results[0][0], results[1][0], A.FACTOR, same, ref.seconds))
    for worst, failures in results:
        assert not failures, "tensors beyond %g x the bound: %s" % (A.FACTOR, failures)


@pytest.mark.parametrize("family,units,message", G.REFUSED, ids=["%s-%s" % (f, "x".join(map(str, u))) for f, u, _ in G.REFUSED])
def test_refused_classes_say_so(family, units, message):
    """Widths and stacks without a gradient class are refused when the handle is created, with the message the table states."""
    from rnnwavefunctions_amd import _lib
    c = G.Case(family, (6, 1) if family in ("gru", "crnn") else (3, 2), units, G.NS, 1.0)
    with pytest.raises(ValueError) as err:
        _lib.NativeWavefunction(G.model_id(c), c.shape[0], c.shape[1], units)
    assert str(err.value).startswith(message), str(err.value)
