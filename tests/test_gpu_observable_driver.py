"""GPU test of what the four observable passes share (csrc/observable.h: pass loop, scratch carving, common kernel arguments):
rnnwf_renyi2_swap, rnnwf_correlations, rnnwf_renyi2_regions and rnnwf_pauli_step keep their scratch, tables and checkpoints in
buffers of the handle, two of them in the same one.  Nothing of one call may survive into another entry point's call: on one handle,
all four interleaved in two different orders must return, bit for bit, what each returns on a handle of its own.

Shapes, the smallest that take every path: N = 33 (two spin / mask words), 10 units, 17 pairs = 34 chains (a partial 16-chain block),
the f32 and the f64 model, the caller's samples and a device draw, and once more under RNNWF_STATE_BUDGET_MB=1, where the
correlations (whose trunk states make a 16-chain block about 1 MB) run in several passes.

The Pauli and region-Renyi entry points of the 2D RNN and the complex RNN run the same drivers (csrc/pauli_driver.h,
csrc/region_driver.h) over their own policies, and get the same test on their own handles; the last test pins the rule that a
Pauli step's new resident batch invalidates the Jacobian of stochastic reconfiguration.
"""
import numpy as np
import pytest

import crnn_pauli_reference as CR
import pauli_2d_reference as Q
from rnnwavefunctions_amd import params as P

pytestmark = pytest.mark.gpu

SCOPE = "RNNwavefunction"
N, H, NPAIRS = 33, 10, 17
NS = 2 * NPAIRS
SEED, STEP, OFFSET = 7, 3, 5


def mask_of(sites):
    m = np.zeros(N, dtype=np.int32)
    m[list(sites)] = 1
    return m


REGIONS = np.stack([mask_of(range(5, 21)), mask_of([0, 32]), mask_of([]), mask_of(range(N))])
# X_0 (first flipped site 0), X_31 X_32 (across the word boundary), Z_3 Z_4 (diagonal), Z_5 X_0 (the first term's flip mask again)
FLIP = np.stack([mask_of([0]), mask_of([31, 32]), mask_of([]), mask_of([0])])
SIGN = np.stack([mask_of([]), mask_of([]), mask_of([3, 4]), mask_of([5])])
COEFF = np.array([-1.0, 0.5, 0.25, 2.0])


def make_wf(f64, prm):
    from rnnwavefunctions_amd import _lib
    wf = _lib.NativeWavefunction(_lib.MODEL_GRU1D_F64 if f64 else _lib.MODEL_GRU1D, N, 1, (H,))
    wf.set_params(prm, scope=SCOPE)
    wf.timing_enable(True)
    return wf


def entry_points(samples):
    """name -> call(wf) of the four entry points, on the caller's samples or (None) drawn on the device, everything returned"""
    pair = dict(samples=samples) if samples is not None else dict(seed=SEED, step=STEP, pair_offset=OFFSET)
    chain = dict(samples=samples) if samples is not None else dict(seed=SEED, step=STEP, sample_offset=OFFSET)
    return {
        "renyi2_swap": lambda wf: wf.renyi2_swap(NPAIRS, want_log_ratio=True, want_samples=True, **pair),
        "correlations": lambda wf: wf.correlations(NS, want_log_ratio=True, want_samples=True, **chain),
        "renyi2_regions": lambda wf: wf.renyi2_regions(REGIONS, NPAIRS, log_ratio=True, **pair),
        "pauli_step": lambda wf: wf.pauli_step(FLIP, SIGN, COEFF, NS, want_eloc=True, want_log_ratio=True, want_samples=True, **chain),
    }


ORDERS = (["renyi2_swap", "correlations", "renyi2_regions", "pauli_step"], ["pauli_step", "renyi2_regions", "renyi2_swap", "correlations"])


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("source", ["samples", "drawn", "drawn-1MB"])
def test_interleaved_calls_equal_fresh_handles(f64, source, monkeypatch):
    prm = P.randomize_biases(P.scale_kernels(P.init_gru_params([H], seed=20, dtype=np.float64 if f64 else np.float32), 3.0), 21)
    samples = make_wf(f64, prm).sample(NS, 11) if source == "samples" else None
    if source == "drawn-1MB":
        monkeypatch.setenv("RNNWF_STATE_BUDGET_MB", "1")         # read when a handle is created
    calls = entry_points(samples)
    fresh = {}
    for name, call in calls.items():
        wf = make_wf(f64, prm)
        fresh[name] = call(wf)
        passes = wf.timing_get(2)["launches"]                    # assembly brackets: one per pass (pauli_step: two)
        print("%s %s %s: %d assembly launches" % ("f64" if f64 else "f32", source, name, passes))
        if source == "drawn-1MB" and name == "correlations":
            assert passes >= 2
    assert fresh["pauli_step"]["log_ratio"].shape == (2, NS)    # the duplicate flip mask is evaluated once
    shared = make_wf(f64, prm)
    for order in ORDERS:
        for name in order:
            got = calls[name](shared)
            assert sorted(got) == sorted(fresh[name])
            for key, want in fresh[name].items():
                assert np.array_equal(got[key], want), (order, name, key)


def check_interleaved(make, calls, orders, min_assembly=None):
    """every call of `calls` on a handle of its own, then on one shared handle in each of `orders`: equal bit for bit (NaN and -inf
    included: the bytes are compared).  min_assembly: name -> least number of assembly launches of the call on its own handle.
    Returns the results on the fresh handles."""
    fresh = {}
    for name, call in calls.items():
        wf = make()
        fresh[name] = call(wf)
        launches = wf.timing_get(2)["launches"]
        print("%s: %d assembly launches" % (name, launches))
        if min_assembly:
            assert launches >= min_assembly[name], (name, launches)
    shared = make()
    for order in orders:
        for name in order:
            got = calls[name](shared)
            assert sorted(got) == sorted(fresh[name])
            for key, want in fresh[name].items():
                assert got[key].shape == want.shape and got[key].dtype == want.dtype, (order, name, key)
                assert np.ascontiguousarray(got[key]).tobytes() == np.ascontiguousarray(want).tobytes(), (order, name, key)
    return fresh


# ---- the 2D RNN: 5 x 7 sites (N = 35: two spin words, both snake directions, Nx != Ny so that a transposed map cannot pass), 20 units
NX, NY, H2 = 5, 7, 20
N2 = NX * NY


def lattice_mask(positions):
    """(N2,) lattice-indexed mask of the given PATH positions"""
    return Q.from_positions(NX, NY, positions).reshape(N2).astype(np.int32)


def lattice_rect(x0, x1, y0, y1):
    m = np.zeros((NX, NY), dtype=np.int32)
    m[x0:x1, y0:y1] = 1
    return m.reshape(N2)


def passes_2d_at_1mb():
    """(chains, pairs) per pass of pauli_step_2d and renyi2_regions_2d under RNNWF_STATE_BUDGET_MB=1, as csrc/mdrnn_observable.h
    (md_chains_per_pass) and the two policies compute them: 20 units are NFULL = 1, KT = 5 k-steps, (KT + 1) / 2 * 64 * 16 = 3072 bytes
    of states per 16-chain block and position"""
    hs = 3 * 64 * 16
    budget = ((1 << 20) // (N2 * hs)) * N2 * hs                       # the family's pass: whole blocks of N states
    M, R = 2, 4
    pauli = budget // (N2 * hs + (N2 + 2 + 2 * M) * 16 * 8) * 16
    regions = budget // (N2 * hs + N2 * 16 * 8 + R * 16 * 8 + R * 8 * 8) * 16 // 2
    return pauli, regions


@pytest.mark.parametrize("source", ["samples", "drawn", "drawn-1MB"])
def test_interleaved_calls_equal_fresh_handles_2d(source, monkeypatch):
    """pauli_step_2d and renyi2_regions_2d on one handle, in both orders, against handles of their own.  17 pairs = 34 chains leave a
    ragged 16-chain block.  1 MB, the smallest budget a handle takes, holds 8 blocks of this lattice per pass (passes_2d_at_1mb: 128
    chains, 64 pairs), so 34 chains cannot split: the 1 MB case runs one full pass and 18 chains more (73 pairs: a full block and a
    ragged one in the second pass)."""
    from rnnwavefunctions_amd import _lib
    prm = Q.weights(H2, 4, 1.0)
    # masks by lattice index: first flipped path position 0; path positions 31, 32 (across the word boundary); diagonal; the first again
    flip = np.stack([lattice_mask([0, 9]), lattice_mask([31, 32]), lattice_mask([]), lattice_mask([0, 9])])
    sign = np.stack([lattice_mask([]), lattice_mask([]), lattice_mask([3, 4]), lattice_mask([5])])
    coeff = np.array([-1.0, 0.5, 0.25, 2.0])
    regions = np.stack([lattice_rect(1, 4, 2, 5), lattice_mask([0, N2 - 1]), lattice_mask([]), lattice_mask(range(N2))])
    assert lattice_mask([0])[Q.site(NX, NY, 0, 0)] == 1 and Q.visit_positions(NX, NY).shape[0] == N2

    def make():
        wf = _lib.NativeWavefunction(_lib.MODEL_MDRNN2D, NX, NY, (H2,))
        wf.set_params(prm, scope=SCOPE)
        wf.timing_enable(True)
        return wf

    npairs, min_assembly = NPAIRS, None
    if source == "drawn-1MB":
        chains, pairs = passes_2d_at_1mb()
        assert (chains, pairs) == (128, 64)
        npairs = pairs + 9
        monkeypatch.setenv("RNNWF_STATE_BUDGET_MB", "1")         # read when a handle is created
        min_assembly = {"pauli_step_2d": 4, "renyi2_regions_2d": 2}      # assembly brackets: one per pass, pauli_step_2d two
    ns = 2 * npairs
    samples = make().sample(ns, 11) if source == "samples" else None
    pair = dict(samples=samples) if samples is not None else dict(seed=SEED, step=STEP, pair_offset=OFFSET)
    chain = dict(samples=samples) if samples is not None else dict(seed=SEED, step=STEP, sample_offset=OFFSET)
    calls = {
        "pauli_step_2d": lambda wf: wf.pauli_step_2d(flip, sign, coeff, ns, want_eloc=True, want_log_ratio=True, want_samples=True, **chain),
        "renyi2_regions_2d": lambda wf: wf.renyi2_regions_2d(regions, npairs, log_ratio=True, **pair),
    }
    fresh = check_interleaved(make, calls, (["pauli_step_2d", "renyi2_regions_2d"], ["renyi2_regions_2d", "pauli_step_2d"]), min_assembly)
    assert fresh["pauli_step_2d"]["log_ratio"].shape == (2, ns)     # the duplicate flip mask is evaluated once
    assert np.all(np.isfinite(fresh["pauli_step_2d"]["log_ratio"])) and np.all(np.isfinite(fresh["renyi2_regions_2d"]["log_ratio"]))


# ---- the complex RNN: N = 34 (even, two words), 10 units
NC = 34


def cmask(sites):
    m = np.zeros(NC, dtype=np.int32)
    m[list(sites)] = 1
    return m


@pytest.mark.parametrize("source", ["samples", "drawn"])
def test_interleaved_calls_equal_fresh_handles_complex(source):
    """pauli_step_complex and renyi2_regions_complex on one handle, in both orders, against handles of their own, in_sector included.
    The flips (0, 1) and (31, 32, across the word boundary) keep the magnetisation where the two spins differ; X_5 alone leaves the
    sector on every chain: its log-ratios are -inf, and they are compared too."""
    from rnnwavefunctions_amd import _lib
    prm = CR.weights(H, seed=20)
    flip = np.stack([cmask([0, 1]), cmask([31, 32]), cmask([]), cmask([0, 1]), cmask([5])])
    sign = np.stack([cmask([]), cmask([]), cmask([3, 4]), cmask([5]), cmask([])])
    coeff = np.array([-1.0, 0.5 + 0.25j, 0.25, 2.0j, 1.0])
    regions = np.stack([cmask(range(5, 21)), cmask([0, NC - 1]), cmask([]), cmask(range(NC))])

    def make():
        wf = _lib.NativeWavefunction(_lib.MODEL_CRNN_U1, NC, 1, (H,))
        wf.set_params(prm, scope=SCOPE)
        wf.timing_enable(True)
        return wf

    samples = make().sample(NS, 11) if source == "samples" else None       # drawn by the model: in the sector
    pair = dict(samples=samples) if samples is not None else dict(seed=SEED, step=STEP, pair_offset=OFFSET)
    chain = dict(samples=samples) if samples is not None else dict(seed=SEED, step=STEP, sample_offset=OFFSET)
    calls = {
        "pauli_step_complex": lambda wf: wf.pauli_step_complex(flip, sign, coeff, NS, want_eloc=True, want_log_ratio=True, want_samples=True,
                                                              **chain),
        "renyi2_regions_complex": lambda wf: wf.renyi2_regions_complex(regions, NPAIRS, log_ratio=True, **pair),
    }
    fresh = check_interleaved(make, calls, (["pauli_step_complex", "renyi2_regions_complex"], ["renyi2_regions_complex", "pauli_step_complex"]))
    lr = fresh["pauli_step_complex"]["log_ratio"]
    assert lr.shape == (3, NS)                                       # the duplicate flip mask is evaluated once
    assert np.all(np.isneginf(lr[2].real))                           # X_5 leaves the sector
    assert np.isfinite(lr[:2].real).any() and np.isneginf(lr[:2].real).any()      # the pair flips: both branches
    assert "in_sector" in fresh["renyi2_regions_complex"]


def test_pauli_step_invalidates_the_jacobian():
    """vmc_step, stochastic reconfiguration (which builds the per-sample Jacobian of that batch), then a one-pass pauli_step of as many
    samples under another seed: the same SR calls must now answer for the new batch, bit for bit as on a handle that ran the
    pauli_step alone (csrc/rnnwf_api.hip keep_resident: the resident batch and the Jacobian's validity change together)."""
    from rnnwavefunctions_amd import _lib
    n, h, ns, lam = 6, 5, 8, 1e-3
    prm = P.randomize_biases(P.scale_kernels(P.init_gru_params([h], seed=20, dtype=np.float64), 3.0), 21)

    def m(sites):
        out = np.zeros(n, dtype=np.int32)
        out[list(sites)] = 1
        return out

    flip = np.stack([m([0]), m([2, 3]), m([])])
    sign = np.stack([m([]), m([1]), m([3, 4])])
    coeff = np.array([-1.0, 0.5, 0.25])

    def make():
        wf = _lib.NativeWavefunction(_lib.MODEL_GRU1D_F64, n, 1, (h,))
        wf.set_params(prm, scope=SCOPE)
        return wf

    def sr_calls(wf):
        return wf.sr_direction(lam), wf.sr_gram()[0], wf.log_derivatives()

    def pauli(wf):
        out = wf.pauli_step(flip, sign, coeff, ns, seed=9, step=1, want_eloc=True, want_samples=True)
        assert wf.resident_samples() == ns                           # one pass: the batch stays
        return out

    fresh = make()
    want_pauli, want = pauli(fresh), sr_calls(fresh)
    wf = make()
    wf.vmc_step(ns, 3, 0, np.append(np.ones(n), 1.0))
    before = sr_calls(wf)                                            # builds J for the vmc_step's batch
    got_pauli, got = pauli(wf), sr_calls(wf)
    assert np.array_equal(got_pauli["samples"], want_pauli["samples"]) and np.array_equal(got_pauli["eloc"], want_pauli["eloc"])
    assert not np.array_equal(before[2], want[2])                    # another batch: a stale J would show
    for a, b in zip(got, want):
        assert np.array_equal(a, b)
