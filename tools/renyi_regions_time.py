"""Region pass of rnnwf_renyi2_regions vs the swap pass of rnnwf_renyi2_swap at equal cell work, alternating in one process on one
handle (not part of bench.py).  Regions = the N - 1 suffix sets {l..N-1}: N (N - 1) cell evaluations per pair, as the swap pass.
Prints the HIP-event medians of kernel ids 0 / 1 / 2 of both, the id-1 time per cell evaluation and their ratio (docs/renyi.md
expects <= 1.15 of a kernel of this step form).  Then one 2D case on its own: the f64 raster model with all column cuts and all
corner squares.

    python tools/renyi_regions_time.py [--N 80] [--H 50] [--pairs 5000] [--reps 7] [--out profiles/renyi_regions_time.txt]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rnnwavefunctions_amd import _lib, params as P  # noqa: E402
from rnnwavefunctions_amd.observables import column_cut_regions, rectangle_region  # noqa: E402


def make(model, Nx, Ny, H, dtype):
    wf = _lib.NativeWavefunction(model, Nx, Ny, (H,))
    wf.set_params(P.randomize_biases(P.scale_kernels(P.init_gru_params([H], seed=111, dtype=dtype), 2.0), 112), scope="RNNwavefunction")
    wf.timing_enable(True)
    return wf


def timed(wf, call, k):
    wf.timing_reset()
    call(k)
    return [wf.timing_get(i) for i in (0, 1, 2)]


def summary(name, rs):
    t = {i: np.median([x[i]["total_ms"] for x in rs]) for i in (0, 1, 2)}
    cells = rs[0][1]["cell_evals"]
    line = ("%-7s: id0 %.3f ms, id1 %.3f ms (min %.3f, max %.3f), id2 %.3f ms; id1 cells %.6g -> %.4f ns per cell evaluation"
            % (name, t[0], t[1], min(x[1]["total_ms"] for x in rs), max(x[1]["total_ms"] for x in rs), t[2], cells,
               t[1] * 1e6 / cells))
    return line, t[1] / cells


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=80)
    ap.add_argument("--H", type=int, default=50)
    ap.add_argument("--pairs", type=int, default=5000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    N, H, npairs = args.N, args.H, args.pairs
    wf = make(_lib.MODEL_GRU1D, N, 1, H, np.float32)
    suffixes = (np.arange(N)[None, :] >= np.arange(1, N)[:, None]).astype(np.int32)

    def swap(k):
        wf.renyi2_swap(npairs, seed=111, step=k)

    def regions(k):
        wf.renyi2_regions(suffixes, npairs, seed=111, step=k)

    for k in range(2):                                   # warm-up: code objects, buffers
        swap(k)
        regions(k)
    rows = {"swap": [], "regions": []}
    for r in range(args.reps):                           # alternating: drifts of clock and temperature hit both
        rows["swap"].append(timed(wf, swap, 10 + r))
        rows["regions"].append(timed(wf, regions, 10 + r))
    lines = ["N=%d H=%d f32, %d pairs, regions = the %d suffix sets; %d reps alternating on one handle, medians of HIP-event times"
             % (N, H, npairs, N - 1, args.reps)]
    per = {}
    for name, rs in rows.items():
        line, per[name] = summary(name, rs)
        lines.append(line)
    assert rows["swap"][0][1]["cell_evals"] == rows["regions"][0][1]["cell_evals"] == npairs * N * (N - 1)
    lines.append("regions / swap (id 1, per cell evaluation) = %.3f   (expected <= 1.15)" % (per["regions"] / per["swap"]))

    Nx = Ny = 8
    wf2 = make(_lib.MODEL_GRU1D_F64, Nx, Ny, H, np.float64)
    corners = [rectangle_region(Nx, Ny, x0, x0 + L, y0, y0 + L) for L in range(1, Nx) for x0 in (0, Nx - L) for y0 in (0, Ny - L)]
    masks = np.concatenate([column_cut_regions(Nx, Ny), np.stack(corners)])

    def raster(k):
        wf2.renyi2_regions(masks, npairs, seed=111, step=k)

    def raster_swap(k):
        wf2.renyi2_swap(npairs, seed=111, step=k)

    for k in range(2):
        raster(k)
        raster_swap(k)
    rows2 = {"swap": [], "regions": []}
    for r in range(args.reps):
        rows2["swap"].append(timed(wf2, raster_swap, 10 + r))
        rows2["regions"].append(timed(wf2, raster, 10 + r))
    lines.append("%dx%d H=%d f64, %d pairs, %d regions (%d column cuts + %d corner squares) beside the swap pass's %d cuts; %d reps"
                 % (Nx, Ny, H, npairs, len(masks), Nx - 1, len(corners), Nx * Ny - 1, args.reps))
    per2 = {}
    for name, rs in rows2.items():
        line, per2[name] = summary(name, rs)
        lines.append(line)
    lines.append("regions / swap (id 1, per cell evaluation) = %.3f" % (per2["regions"] / per2["swap"]))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
