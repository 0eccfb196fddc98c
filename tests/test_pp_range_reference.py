"""The range word of the g-state image (csrc/pack_split.h: gstate_range), which lets the one-layer ping-pong flip kernel take one
reciprocal for update gate and candidate (csrc/split_pp.h: MERGED).  No GPU: the packer and the range function through the host-only
entry points rnnwf_host_split_images / rnnwf_host_split_range, against tests/pp_range_reference.py.

  * the library's bound equals the NumPy restatement's (float64 sums in another order: 1e-12 relative), at 37, 38, 44, 49, 50 units,
    glorot and x 3 kernels with random biases; the verdict is the word of the g image and says bound <= 120;
  * the bound holds: over 4 000 random states g in [0, 1]^units per image and both input spins, applied to the g image as the kernel
    does (a_u = start + W g; a_c = xc + r q with r = 1 / (1 + exp2(a_r))), |a_u| <= A_u and |a_c| <= A_c for every unit, so the largest
    |a_u| + |a_c| never exceeds the bound; the corner states that attain sup |a_u| (in h: h_j = +-1) reach A_u to 1e-12 - the bound is
    the supremum, not merely above it;
  * the verdict flips exactly at 120: one update-gate bias alone, chosen so that the start value is 120 (in range) and the next
    float32 above it (out of range);
  * the merged sequence in float32 (NumPy, v_rcp_f32's flush of a sub-normal result modelled) on a grid of exponent arguments with
    a_u + a_c <= 120 and five more (the slack the limit leaves for the accumulators' rounding): the denominator is finite with a
    normal reciprocal, g' is finite and in [0, 1 + 2^-22], and its deviation from float64 is within FACTOR = 16 x the two-reciprocal
    float32 form's on the same inputs (floor: one float32 rounding of a value in [0, 1]) - the bound tests/test_gpu_pp_merged_rcp.py
    holds the kernel to, taken from the reference.  Beyond the range the same restatement returns NaN where the two-reciprocal form is finite, which
    is why the word exists.
"""
import numpy as np
import pytest

import pp_range_reference as PR
import sampler_reference as R

WIDTHS = [37, 38, 44, 49, 50]
SEED = 111


def _states(rng, n):
    g = rng.uniform(0.0, 1.0, (n, 2, PR.NU))
    g[: n // 8] = rng.randint(0, 2, (n // 8, 2, PR.NU))          # corners of the cube among them
    return g


@pytest.mark.parametrize("sharp", [1.0, 3.0], ids=["glorot", "x3"])
@pytest.mark.parametrize("units", WIDTHS)
def test_bound_against_numpy_and_against_random_states(units, sharp):
    prm = R.build_params("gru", (units,), seed=SEED, sharp=sharp)
    ih, ig, L = PR.images(units, prm)
    bound, word = PR.library_range(units, prm)
    A_u, A_c = PR.bounds(ih, L)
    ref = float((A_u + A_c).max())
    assert abs(bound - ref) <= 1e-12 * ref, (bound, ref)
    assert word == PR.range_word(ig, L) == int(bound <= PR.LIMIT)
    assert PR.range_word(ih, L) == 0                                # the h image carries no verdict
    assert int(((A_u + A_c) > 0).sum()) == units                    # padded units: zero rows, zero bound
    # the exponent arguments the kernel meets, from the image it reads
    Wg, Cg = PR.gate_rows(*PR.decode(ig, L)[:2])
    XC = PR.decode(ig, L)[2]
    rng = np.random.RandomState(units)
    g = _states(rng, 4000)
    worst_u = worst_c = worst_sum = 0.0
    for sgm in range(2):
        pre = Cg[:, sgm][None] + np.einsum("ghekj,nkj->nghe", Wg, g)      # [state, gate, hh, e]
        a_u = np.abs(pre[:, 1])
        r = 1.0 / (1.0 + np.exp2(pre[:, 0]))
        a_c = np.abs(XC[sgm][None] + r * pre[:, 2])
        assert np.all(a_u <= A_u[None]) and np.all(a_c <= A_c[None])
        worst_u, worst_c = max(worst_u, float((a_u / np.maximum(A_u, 1e-300)).max())), max(worst_c, float((a_c / np.maximum(A_c, 1e-300)).max()))
        worst_sum = max(worst_sum, float((a_u + a_c).max()))
    assert worst_sum <= bound
    # the corners that attain sup |a_u|, in h on the image in h: exact to a float64 sum
    Wh, Ch = PR.gate_rows(*PR.decode(ih, L)[:2])
    sup = np.abs(Ch[1]).max(axis=0) + np.abs(Wh[1]).sum(axis=(2, 3))
    assert np.all(np.abs(sup - A_u) <= 1e-12 * np.maximum(A_u, 1.0))
    print("[range, %d units, kernels x %g] bound %.3f (A_u <= %.3f, A_c <= %.3f), verdict %d; largest |a| / A over 8 000 states: u %.3f, c %.3f; "
          "largest |a_u| + |a_c| %.3f" % (units, sharp, bound, A_u.max(), A_c.max(), word, worst_u, worst_c, worst_sum))


def _one_bias(units, value):
    """every parameter zero but the update-gate bias of unit 0"""
    prm = R.build_params("gru", (units,), seed=SEED, sharp=None)
    prm = {k: np.zeros_like(v) for k, v in prm.items()}
    key = [k for k in prm if k.endswith("gates/bias")][0]
    b = prm[key].astype(np.float64)
    b[units] = value                                                 # columns r | u
    prm[key] = b
    return prm


@pytest.mark.parametrize("units", [37, 50])
def test_verdict_flips_exactly_at_120(units):
    scale = 1.44269504088896340736                                   # csrc/pack.h: PackScale<float>::gate = -log2(e)
    at = np.float32(120.0)
    above = np.nextafter(at, np.float32(np.inf))
    below = np.nextafter(at, np.float32(0.0))
    seen = {}
    for name, target in (("below", below), ("at", at), ("above", above)):
        b = -float(target) / scale                                  # start value -scale * b rounds to the float32 `target`
        assert np.float32(-scale * b) == target
        bound, word = PR.library_range(units, _one_bias(units, b))
        assert bound == float(target), (name, bound, float(target))
        seen[name] = word
    assert seen == {"below": 1, "at": 1, "above": 0}, seen
    # and the sign does not matter: the bound is on |a_u|
    bound, word = PR.library_range(units, _one_bias(units, float(above) / scale))
    assert bound == float(above) and word == 0


def test_merged_sequence_in_float32_within_the_range():
    rng = np.random.RandomState(SEED)
    # exponent arguments on a grid over the whole admitted region, both signs, plus random ones; five beyond the limit
    ax = np.concatenate([np.linspace(-125.0, 125.0, 251), [-150.0, -127.0, -0.5, 0.0, 0.5]])
    a_u, a_c = (x.ravel() for x in np.meshgrid(ax, ax))
    keep = np.maximum(a_u, 0.0) + np.maximum(a_c, 0.0) <= PR.LIMIT + 5.0
    a_u, a_c = a_u[keep], a_c[keep]
    a_u = np.concatenate([a_u, rng.uniform(-20, 20, 20000)]).astype(np.float32)
    a_c = np.concatenate([a_c, rng.uniform(-20, 20, 20000)]).astype(np.float32)
    worst = 0.0
    for g in (0.0, 1.0, 0.5, None):
        gv = rng.uniform(0, 1, a_u.size).astype(np.float32) if g is None else np.full(a_u.size, g, dtype=np.float32)
        got, D = PR.merged32(a_u, a_c, gv)
        assert np.all(np.isfinite(D)) and np.all(D < np.float32(2.0 ** 126) * np.float32(1.0 + 2.0 ** -20)), "denominator out of range"
        assert np.all(PR._rcp32(D) > 0), "a reciprocal was flushed"
        assert np.all(np.isfinite(got)) and got.min() >= 0.0 and got.max() <= 1.0 + 2.0 ** -22
        ref = PR.exact64(a_u, a_c, gv)
        yard = max(float(np.abs(PR.two_rcp32(a_u, a_c, gv) - ref).max()), 2.0 ** -24)
        err = float(np.abs(got - ref).max())
        worst = max(worst, err / (16.0 * yard))
        assert err <= 16.0 * yard, (g, err, yard)
    print("[merged gate tail, float32] %d inputs x 4 states: worst deviation from float64 / (16 x the two-reciprocal form's) = %.3f" % (a_u.size, worst))
    # what the word guards against: an exp2 beyond float32 turns the merged form into inf x 0
    beyond, _ = PR.merged32(np.float32([130.0, 0.0]), np.float32([0.0, 130.0]), np.float32([0.5, 0.5]))
    assert not np.isfinite(beyond).any()
    assert np.all(np.isfinite(PR.two_rcp32(np.float32([130.0, 0.0]), np.float32([0.0, 130.0]), np.float32([0.5, 0.5]))))
