"""Paired masked-tail pass of rnnwf_renyi2_regions_stack vs the flip-mask pass of rnnwf_pauli_step_stack at equal cell work, alternating
in one process on one handle (not part of bench.py).  Regions = the N - 1 suffix sets {l..N-1}; Pauli masks = the single sites 1..N-1:
both restart at f = 1..N-1, N (N - 1) / 2 steps of the whole stack per chain.  Prints the HIP-event medians of kernel ids 0 / 1 / 2 of
both, the id-1 time per cell evaluation and their ratio (docs/renyi_stack.md: <= 1.15, the margin docs/renyi_regions.md set for the
one-layer region kernel against its sibling - the only added work is one partner word per 32 sites).  Two cases: a float32 chain and
a float64 raster lattice.

    python tools/renyi_stack_time.py [--N 80] [--L 8] [--H 50] [--layers 2] [--pairs 5000] [--reps 7] [--out profiles/renyi_stack_time.txt]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rnnwavefunctions_amd import _lib, params as P  # noqa: E402


def make(model, Nx, Ny, units, dtype):
    wf = _lib.NativeWavefunction(model, Nx, Ny, tuple(units))
    wf.set_params(P.randomize_biases(P.scale_kernels(P.init_gru_params(list(units), seed=111, dtype=dtype), 2.0), 112), scope="RNNwavefunction")
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
            % (name, t[0], t[1], min(x[1]["total_ms"] for x in rs), max(x[1]["total_ms"] for x in rs), t[2], cells, t[1] * 1e6 / cells))
    return line, t[1] / cells


def case(label, wf, npairs, reps):
    N = wf.N
    suffixes = (np.arange(N)[None, :] >= np.arange(1, N)[:, None]).astype(np.int32)
    flip = np.eye(N, dtype=np.int32)[1:]
    sign, coeff = np.zeros_like(flip), np.ones(len(flip))

    def pauli(k):
        wf.pauli_step_stack(flip, sign, coeff, 2 * npairs, seed=111, step=k)

    def regions(k):
        wf.renyi2_regions_stack(suffixes, npairs, seed=111, step=k)

    for k in range(2):                                   # warm-up: code objects, buffers
        pauli(k)
        regions(k)
    rows = {"pauli": [], "regions": []}
    for r in range(reps):                                # alternating: drifts of clock and temperature hit both
        rows["pauli"].append(timed(wf, pauli, 10 + r))
        rows["regions"].append(timed(wf, regions, 10 + r))
    lines = ["%s, %d pairs = %d chains, %d suffix regions / %d single-site masks; %d reps alternating on one handle, medians of HIP-event times"
             % (label, npairs, 2 * npairs, N - 1, N - 1, reps)]
    per = {}
    for name, rs in rows.items():
        line, per[name] = summary(name, rs)
        lines.append(line)
    assert rows["pauli"][0][1]["cell_evals"] == rows["regions"][0][1]["cell_evals"] == npairs * N * (N - 1)
    ratio = per["regions"] / per["pauli"]
    lines.append("regions / pauli (id 1, per cell evaluation) = %.3f   (condition: <= 1.15)" % ratio)
    return lines, ratio


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=80)
    ap.add_argument("--L", type=int, default=8)
    ap.add_argument("--H", type=int, default=50)
    ap.add_argument("--layers", type=int, default=2)
    ap.add_argument("--pairs", type=int, default=5000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    units = (args.H,) * args.layers
    name = " x ".join(str(u) for u in units)
    lines, ratios = [], []
    for label, wf in [("N=%d, %s units f32" % (args.N, name), make(_lib.MODEL_GRU1D, args.N, 1, units, np.float32)),
                      ("%dx%d, %s units f64" % (args.L, args.L, name), make(_lib.MODEL_GRU1D_F64, args.L, args.L, units, np.float64))]:
        ls, ratio = case(label, wf, args.pairs, args.reps)
        lines += ls
        ratios.append(ratio)
        wf.close()
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0 if max(ratios) <= 1.15 else 1


if __name__ == "__main__":
    sys.exit(main())
