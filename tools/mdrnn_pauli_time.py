"""Masked-tail pass of rnnwf_pauli_step_2d vs the flip pass of the fused 2D-TFIM step at equal cell work, alternating in one process
on one handle (not part of bench.py).  BASELINE config 4's size: the 2D RNN on 12 x 12 sites, 50 units, 10 000 chains.  The masks are
the N single-X masks, which are exactly the flip pass's tiles (the flip at the last position costs the flip pass nothing and the
masked-tail pass one head): work[0] = ns N (N - 1) / 2 for both.  Prints the HIP-event medians of kernel ids 0 / 1 / 2 of both, the
id-1 time per cell evaluation and their ratio.  The flip pass is the yardstick.

    python tools/mdrnn_pauli_time.py [--Nx 12] [--Ny 12] [--H 50] [--ns 10000] [--reps 7] [--out profiles/mdrnn_pauli_time.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rnnwavefunctions_amd import _lib, params as P  # noqa: E402


def timed(wf, call, k):
    wf.timing_reset()
    t0 = time.perf_counter()
    call(k)
    wall = (time.perf_counter() - t0) * 1e3
    return [wf.timing_get(i) for i in (0, 1, 2)] + [wall]


def summary(name, rs):
    t = {i: np.median([x[i]["total_ms"] for x in rs]) for i in (0, 1, 2)}
    cells = rs[0][1]["cell_evals"]
    line = ("%-11s: id0 %.3f ms, id1 %.3f ms (min %.3f, max %.3f), id2 %.3f ms, wall %.3f ms; id1 cells %.6g -> %.4f ns per cell evaluation"
            % (name, t[0], t[1], min(x[1]["total_ms"] for x in rs), max(x[1]["total_ms"] for x in rs), t[2],
               np.median([x[3] for x in rs]), cells, t[1] * 1e6 / max(cells, 1)))
    return line, t[1] / max(cells, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--Nx", type=int, default=12)
    ap.add_argument("--Ny", type=int, default=12)
    ap.add_argument("--H", type=int, default=50)
    ap.add_argument("--ns", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    Nx, Ny, H, ns = args.Nx, args.Ny, args.H, args.ns
    N = Nx * Ny
    wf = _lib.NativeWavefunction(_lib.MODEL_MDRNN2D, Nx, Ny, (H,))
    wf.set_params(P.init_mdrnn_params(H, seed=111), scope="RNNwavefunction")
    wf.timing_enable(True)
    couplings = np.append(np.ones(N), 3.0)
    masks = np.eye(N, dtype=np.int32)
    zeros, coeff = np.zeros_like(masks), -3.0 * np.ones(N)

    def flip(k):
        wf.vmc_step(ns, seed=111, step=k, couplings=couplings)

    def tail(k):
        wf.pauli_step_2d(masks, zeros, coeff, ns, seed=111, step=k)

    for k in range(2):                                   # warm-up: code objects, buffers
        flip(k)
        tail(k)
    rows = {"flip pass": [], "masked tail": []}
    for r in range(args.reps):                           # alternating: drifts of clock and temperature hit both
        rows["flip pass"].append(timed(wf, flip, 10 + r))
        rows["masked tail"].append(timed(wf, tail, 10 + r))
    lines = ["2D RNN %dx%d, %d units, %d chains, the %d single-X masks; %d reps alternating on one handle, medians of HIP-event times"
             % (Nx, Ny, H, ns, N, args.reps)]
    per = {}
    for name, rs in rows.items():
        line, per[name] = summary(name, rs)
        lines.append(line)
    assert rows["flip pass"][0][1]["cell_evals"] == rows["masked tail"][0][1]["cell_evals"] == ns * N * (N - 1) / 2
    lines.append("masked tail / flip pass (id 1, per cell evaluation) = %.3f   (expected: same-box alternation noise; explain above 1.05)"
                 % (per["masked tail"] / per["flip pass"]))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
