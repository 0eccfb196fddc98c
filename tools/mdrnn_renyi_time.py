"""Paired masked-tail pass of rnnwf_renyi2_regions_2d vs the masked-tail pass of rnnwf_pauli_step_2d at equal cell work, alternating in
one process on one handle (not part of bench.py).  BASELINE config 4's size: the 2D RNN on 12 x 12 sites, 50 units, 10 000 chains
(5 000 pairs).  The Pauli masks are the single-X masks of the positions 1..N-1 of the path and the regions the single positions
1..N-1, so both passes run one tile per (position f, 16-chain block) with N - 1 - f cell evaluations each: work[0] = ns (N-1)(N-2)/2
for both.  Prints the HIP-event medians of kernel ids 0 / 1 / 2 of both, the id-1 time per cell evaluation and their ratio.  The Pauli
pass is the yardstick: per tile the paired kernel adds one word read per spin word.

    python tools/mdrnn_renyi_time.py [--Nx 12] [--Ny 12] [--H 50] [--ns 10000] [--reps 7] [--out profiles/mdrnn_renyi_time.txt]
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
    assert ns % 2 == 0
    wf = _lib.NativeWavefunction(_lib.MODEL_MDRNN2D, Nx, Ny, (H,))
    wf.set_params(P.init_mdrnn_params(H, seed=111), scope="RNNwavefunction")
    wf.timing_enable(True)
    # lattice index of every position of the path but the first: site (nx, ny) is visited at ny Nx + (nx or Nx-1-nx)
    site_of_pos = [(p % Nx if (p // Nx) % 2 == 0 else Nx - 1 - p % Nx) * Ny + p // Nx for p in range(N)]
    masks = np.zeros((N - 1, N), dtype=np.int32)
    masks[np.arange(N - 1), site_of_pos[1:]] = 1
    zeros, coeff = np.zeros_like(masks), np.ones(N - 1)

    def pauli(k):
        wf.pauli_step_2d(masks, zeros, coeff, ns, seed=111, step=k)

    def regions(k):
        wf.renyi2_regions_2d(masks, ns // 2, seed=111, step=k)

    for k in range(2):                                   # warm-up: code objects, buffers
        pauli(k)
        regions(k)
    rows = {"pauli tail": [], "paired tail": []}
    for r in range(args.reps):                           # alternating: drifts of clock and temperature hit both
        rows["pauli tail"].append(timed(wf, pauli, 10 + r))
        rows["paired tail"].append(timed(wf, regions, 10 + r))
    lines = ["2D RNN %dx%d, %d units, %d chains, the %d single positions 1..N-1 as X masks and as regions; %d reps alternating on one handle, "
             "medians of HIP-event times" % (Nx, Ny, H, ns, N - 1, args.reps)]
    per = {}
    for name, rs in rows.items():
        line, per[name] = summary(name, rs)
        lines.append(line)
    assert rows["pauli tail"][0][1]["cell_evals"] == rows["paired tail"][0][1]["cell_evals"] == ns * (N - 1) * (N - 2) / 2
    lines.append("paired tail / pauli tail (id 1, per cell evaluation) = %.3f   (expected: same-box alternation noise; explain above 1.05)"
                 % (per["paired tail"] / per["pauli tail"]))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
