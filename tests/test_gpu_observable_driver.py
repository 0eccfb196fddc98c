"""GPU test of what the four observable passes share (csrc/observable.h: pass loop, scratch carving, common kernel arguments):
rnnwf_renyi2_swap, rnnwf_correlations, rnnwf_renyi2_regions and rnnwf_pauli_step keep their scratch, tables and checkpoints in
buffers of the handle, two of them in the same one.  Nothing of one call may survive into another entry point's call: on one handle,
all four interleaved in two different orders must return, bit for bit, what each returns on a handle of its own.

Shapes, the smallest that take every path: N = 33 (two spin / mask words), 10 units, 17 pairs = 34 chains (a partial 16-chain block),
the f32 and the f64 model, the caller's samples and a device draw, and once more under RNNWF_STATE_BUDGET_MB=1, where the
correlations (whose trunk states make a 16-chain block about 1 MB) run in several passes.
"""
import numpy as np
import pytest

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
