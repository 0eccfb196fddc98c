"""Paired masked-tail pass of rnnwf_renyi2_regions_lstm vs the flip-mask pass of rnnwf_pauli_step_lstm at equal cell work, alternating in
one process on one handle (not part of bench.py).  Regions = the N - 1 suffix sets {l..N-1}; Pauli masks = the single sites 1..N-1: both
restart at f = 1..N-1, N (N - 1) / 2 cell evaluations per chain.  Prints the HIP-event medians of kernel ids 0 / 1 / 2 of both, the id-1
time per cell evaluation and their ratio (docs/renyi_lstm.md: the project expects <= 1.15 of a PAIRED form against its !PAIRED form -
the only added work is one DPP move and two bit operations per 32 sites).

    python tools/lstm_renyi_time.py [--nx 10] [--ny 10] [--H 50] [--pairs 5000] [--reps 7] [--out profiles/lstm_renyi_time.txt]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rnnwavefunctions_amd import _lib, params as P  # noqa: E402

SCOPE = "RNNwavefunction"


def timed(wf, call, k):
    wf.timing_reset()
    call(k)
    return [wf.timing_get(i) for i in (0, 1, 2)]


def summary(name, rs):
    t = {i: np.median([x[i]["total_ms"] for x in rs]) for i in (0, 1, 2)}
    cells = rs[0][1]["cell_evals"]
    line = ("%-7s: id0 %.3f ms, id1 %.3f ms (min %.3f, max %.3f), id2 %.3f ms; id1 cells %.6g -> %.4f ns per cell evaluation"
            % (name, t[0], t[1], min(x[1]["total_ms"] for x in rs), max(x[1]["total_ms"] for x in rs), t[2], cells, t[1] * 1e6 / cells))
    return line, t[1] / cells


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=10)
    ap.add_argument("--ny", type=int, default=10)
    ap.add_argument("--H", type=int, default=50)
    ap.add_argument("--pairs", type=int, default=5000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    nx, ny, H, npairs = args.nx, args.ny, args.H, args.pairs
    N = nx * ny
    wf = _lib.NativeWavefunction(_lib.MODEL_LSTM1D_F64, nx, ny, (H,))
    wf.set_params(P.randomize_biases(P.scale_kernels(P.init_lstm_params([H], seed=111, scope=SCOPE), 2.0), 112), scope=SCOPE)
    wf.timing_enable(True)
    suffixes = (np.arange(N)[None, :] >= np.arange(1, N)[:, None]).astype(np.int32)
    flip = np.eye(N, dtype=np.int32)[1:]
    sign, coeff = np.zeros_like(flip), np.ones(len(flip))

    def pauli(k):
        wf.pauli_step_lstm(flip, sign, coeff, 2 * npairs, seed=111, step=k)

    def regions(k):
        wf.renyi2_regions_lstm(suffixes, npairs, seed=111, step=k)

    for k in range(2):                                   # warm-up: code objects, buffers
        pauli(k)
        regions(k)
    rows = {"pauli": [], "regions": []}
    for r in range(args.reps):                           # alternating: drifts of clock and temperature hit both
        rows["pauli"].append(timed(wf, pauli, 10 + r))
        rows["regions"].append(timed(wf, regions, 10 + r))
    wf.close()
    lines = ["LSTM1D_F64 %d x %d, %d units, %d pairs = %d chains, %d suffix regions / %d single-site masks; %d reps alternating on one handle, "
             "medians of HIP-event times" % (nx, ny, H, npairs, 2 * npairs, N - 1, N - 1, args.reps)]
    per = {}
    for name, rs in rows.items():
        assert all(x[1]["launches"] == 1 for x in rs)
        line, per[name] = summary(name, rs)
        lines.append(line)
    assert rows["pauli"][0][1]["cell_evals"] == rows["regions"][0][1]["cell_evals"] == npairs * N * (N - 1)
    ratio = per["regions"] / per["pauli"]
    lines.append("regions / pauli (id 1, per cell evaluation) = %.3f   (expectation: <= 1.15)" % ratio)
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0 if ratio <= 1.15 else 1


if __name__ == "__main__":
    sys.exit(main())
