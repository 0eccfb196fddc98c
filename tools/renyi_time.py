"""Swap pass of rnnwf_renyi2_swap vs the f32-input-MFMA flip pass at equal cell work, alternating in one process (not part of
bench.py).  Both do N (N - 1) / 2 cell evaluations per chain: the swap pass on `pairs` pairs (2 pairs chains), the flip pass of a
vmc_step on 2 pairs chains with RNNWF_ENGINE=f32.  Prints the HIP-event time of kernel id 1 of both, their ratio and each one's
fraction of the 157.3 TF f32 MFMA peak on the MFMA flops it issues (rnnwf_timing_get work[1]).

    python tools/renyi_time.py [--N 80] [--H 50] [--pairs 5000] [--reps 7] [--out profiles/renyi_time.txt]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rnnwavefunctions_amd import _lib, params as P  # noqa: E402

PEAK_F32 = 157.3e12


def make(N, H):
    os.environ["RNNWF_ENGINE"] = "f32"                 # read at create: the flip pass on the f32-input MFMA
    try:
        wf = _lib.NativeWavefunction(_lib.MODEL_GRU1D, N, 1, (H,))
    finally:
        os.environ.pop("RNNWF_ENGINE", None)
    wf.set_params(P.randomize_biases(P.scale_kernels(P.init_gru_params([H], seed=111), 2.0), 112), scope="RNNwavefunction")
    wf.timing_enable(True)
    return wf


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=80)
    ap.add_argument("--H", type=int, default=50)
    ap.add_argument("--pairs", type=int, default=5000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    N, H, npairs = args.N, args.H, args.pairs
    wf = make(N, H)
    couplings = np.append(np.ones(N), 1.0)

    def swap(k):
        wf.timing_reset()
        wf.renyi2_swap(npairs, seed=111, step=k)
        return [wf.timing_get(i) for i in (0, 1, 2)]

    def flip(k):
        wf.timing_reset()
        wf.vmc_step(2 * npairs, seed=111, step=k, couplings=couplings)
        return [wf.timing_get(i) for i in (0, 1, 2)]

    for k in range(2):                                   # warm-up: code objects, buffers
        swap(k)
        flip(k)
    rows = {"swap": [], "flip": []}
    for r in range(args.reps):                           # alternating: drifts of clock and temperature hit both
        rows["swap"].append(swap(10 + r))
        rows["flip"].append(flip(10 + r))
    lines = ["N=%d H=%d pairs=%d (swap) / chains=%d (flip, engine %s), %d reps alternating, medians of HIP-event times"
             % (N, H, npairs, 2 * npairs, wf.engine_name(), args.reps)]
    med = {}
    for name, rs in rows.items():
        t = {i: np.median([x[i]["total_ms"] for x in rs]) for i in (0, 1, 2)}
        cells, flops = rs[0][1]["cell_evals"], rs[0][1]["mfma_flops"]
        med[name] = t[1]
        lines.append("%-4s: id0 %.3f ms, id1 %.3f ms (min %.3f, max %.3f), id2 %.3f ms; id1 cells %.4g, MFMA flops %.4g -> %.1f %% of "
                     "the f32 MFMA peak" % (name, t[0], t[1], min(x[1]["total_ms"] for x in rs), max(x[1]["total_ms"] for x in rs),
                                            t[2], cells, flops, 100.0 * flops / (t[1] * 1e-3) / PEAK_F32))
    lines.append("swap / flip (id 1) = %.3f" % (med["swap"] / med["flip"]))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
