"""LSTM gradient vs the float64 GRU's at equal (Nx, Ny, H, ns): HIP-event time of the backward pass (timer 3) and of the
weight-gradient product (timer 4), alternating the two models in one process (not part of bench.py).  Sizes: the run script's
4x4 / 50 units / 500 samples and 10x10 / 50 / 10 000.  The LSTM runs lstm_vmc_gradient_step (fused step + gradient), the GRU
vmc_step + vmc_gradient; the timers bracket the same two kernel groups in both.  The yardstick for the ratio is the flip pass's,
1.38-1.43 (docs/lstm.md).

    python tools/lstm_grad_time.py [--reps 7] [--sizes 4x4x50x500,10x10x50x10000] [--out profiles/lstm_grad_time.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rnnwavefunctions_amd import _lib, params as P  # noqa: E402

SCOPE = "RNNwavefunction"


def make(model, Nx, Ny, H):
    wf = _lib.NativeWavefunction(model, Nx, Ny, (H,))
    if model == _lib.MODEL_LSTM1D_F64:
        prm = P.init_lstm_params([H], seed=111)
    else:
        prm = P.init_gru_params([H], seed=111, dtype=np.float64)
    prm = P.scale_kernels(prm, 1.5)
    wf.set_params(prm, scope=SCOPE)
    return wf, {k[len(SCOPE) + 1:]: v.shape for k, v in prm.items()}


def one(name, wf, shapes, ns, couplings, step):
    wf.timing_reset()
    t0 = time.perf_counter()
    if name == "lstm":
        wf.lstm_vmc_gradient_step(ns, seed=111, step=step, couplings=couplings, shapes=shapes)
    else:
        s1, _, n, _ = wf.vmc_step(ns, seed=111, step=step, couplings=couplings)["moments"]
        wf.vmc_gradient(s1 / n, n, shapes)
    wall = (time.perf_counter() - t0) * 1e3
    return wall, wf.timing_get(3)["total_ms"], wf.timing_get(4)["total_ms"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sizes", default="4x4x50x500,10x10x50x10000", help="Nx x Ny x H x ns, comma separated")
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    args = ap.parse_args()
    lines = []

    def say(line):
        print(line)
        lines.append(line)

    for Nx, Ny, H, ns in (tuple(int(v) for v in sz.split("x")) for sz in args.sizes.split(",")):
        couplings = np.append(np.ones(Nx * Ny), 3.0)
        wfs = {"lstm": make(_lib.MODEL_LSTM1D_F64, Nx, Ny, H), "gru64": make(_lib.MODEL_GRU1D_F64, Nx, Ny, H)}
        for k, (wf, shapes) in wfs.items():
            wf.timing_enable(True)
            for j in range(2):                                   # warm-up: kernel loads, buffers
                one(k, wf, shapes, ns, couplings, j)
        res = {k: [] for k in wfs}
        for r in range(args.reps):                               # alternating, so drifts of clock and temperature hit both
            for k, (wf, shapes) in wfs.items():
                res[k].append(one(k, wf, shapes, ns, couplings, 10 + r))
        med, spread = {}, {}
        for k, rows in res.items():
            a = np.array(rows)
            med[k] = np.median(a, axis=0)
            spread[k] = (a[:, 1].max() - a[:, 1].min()) / med[k][1]
            say("%dx%d H=%d ns=%d %-5s: whole iteration %.3f ms (host wall), backward pass %.3f ms (min %.3f max %.3f over %d), "
                "weight-gradient product %.3f ms" % (Nx, Ny, H, ns, k, med[k][0], med[k][1], a[:, 1].min(), a[:, 1].max(), len(a), med[k][2]))
        say("%dx%d H=%d ns=%d: backward LSTM / GRU f64 = %.2f (run-to-run spread %.1f %% / %.1f %%), product LSTM / GRU f64 = %.2f"
            % (Nx, Ny, H, ns, med["lstm"][1] / med["gru64"][1], 100 * spread["lstm"], 100 * spread["gru64"],
               med["lstm"][2] / med["gru64"][2]))
        for wf, _ in wfs.values():
            wf.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
