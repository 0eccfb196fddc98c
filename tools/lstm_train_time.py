"""LSTM training: the host loop (training_lstm.lstm_training_loop: one fused call, the dW image's download and unpack, training.Adam
in NumPy, set_params' re-pack and upload per iteration) against the device loop (lstm_train_steps: K iterations per call, Adam and the
re-pack of both images on the device), alternating the two in one process (not part of bench.py).  Sizes: the run script's 4x4 / 50
units / 500 samples and 10x10 / 50 / 10 000.  A repetition is K = 50 iterations of either loop from the same parameters; its figure is
wall time / K.  The yardstick is the host loop in the same process: the device loop removes work and adds none, so it must not be
slower than the host loop by more than the run-to-run spread printed here.  A last, separately timed block of either loop gives the
HIP-event time of the kernel groups per iteration (events cost host time: these blocks are not in the wall figures).

    python tools/lstm_train_time.py [--reps 7] [--k 50] [--sizes 4x4x50x500,10x10x50x10000] [--out profiles/lstm_train_time.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rnnwavefunctions_amd import _lib, params as P, training, training_lstm  # noqa: E402

SCOPE = "RNNwavefunction"
GROUPS = ("base", "flip", "assembly", "backward", "product")


def lr_of_it(lr0, it):
    return 1.0 / ((1.0 / lr0) + it / 10)


def block(wf, prm, couplings, ns, K, device):
    """K iterations from `prm` with a fresh optimizer: wall ms per iteration"""
    wf.set_params(prm, scope=SCOPE)
    wf.synchronize()
    t0 = time.perf_counter()
    training_lstm.lstm_training_loop(wf, {k: v.copy() for k, v in prm.items()}, SCOPE, couplings, K - 1, ns, 333, np.float64(1e-3), lr_of_it,
                                     training.Adam(), device_steps=K if device else None)
    return (time.perf_counter() - t0) * 1e3 / K


def kernel_times(wf, prm, couplings, ns, K, device):
    wf.timing_enable(True)
    wf.timing_reset()
    block(wf, prm, couplings, ns, K, device)
    out = [wf.timing_get(i)["total_ms"] / K for i in range(5)]
    wf.timing_enable(False)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--k", type=int, default=50, help="iterations per repetition (and per device call)")
    ap.add_argument("--sizes", default="4x4x50x500,10x10x50x10000", help="Nx x Ny x H x ns, comma separated")
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    args = ap.parse_args()
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    for Nx, Ny, H, ns in (tuple(int(v) for v in sz.split("x")) for sz in args.sizes.split(",")):
        couplings = np.append(np.ones(Nx * Ny), 2.0)
        prm = P.init_lstm_params([H], seed=111, scope=SCOPE, dtype=np.float64)
        wfs = {"host": _lib.NativeWavefunction(_lib.MODEL_LSTM1D_F64, Nx, Ny, (H,)), "device": _lib.NativeWavefunction(_lib.MODEL_LSTM1D_F64, Nx, Ny, (H,))}
        for k, wf in wfs.items():                                # warm-up: kernel loads, buffers, the device loop's tables
            block(wf, prm, couplings, ns, 3, k == "device")
        res = {k: [] for k in wfs}
        for _ in range(args.reps):                               # alternating, so drifts of clock and temperature hit both
            for k, wf in wfs.items():
                res[k].append(block(wf, prm, couplings, ns, args.k, k == "device"))
        med, spread = {}, {}
        for k, rows in res.items():
            a = np.array(rows)
            med[k] = np.median(a)
            spread[k] = (a.max() - a.min()) / med[k]
            say("%dx%d H=%d ns=%d %-6s loop: %.3f ms per iteration (median of %d blocks of %d; min %.3f max %.3f, spread %.1f %%)"
                % (Nx, Ny, H, ns, k, med[k], len(a), args.k, a.min(), a.max(), 100 * spread[k]))
        say("%dx%d H=%d ns=%d: device / host = %.3f (%.3f ms per iteration saved; run-to-run spread host %.1f %%, device %.1f %%)"
            % (Nx, Ny, H, ns, med["device"] / med["host"], med["host"] - med["device"], 100 * spread["host"], 100 * spread["device"]))
        for k, wf in wfs.items():
            t = kernel_times(wf, prm, couplings, ns, args.k, k == "device")
            say("%dx%d H=%d ns=%d %-6s loop, kernel groups per iteration (HIP events): %s; sum %.3f ms"
                % (Nx, Ny, H, ns, k, ", ".join("%s %.3f" % (g, v) for g, v in zip(GROUPS, t)), sum(t)))
            wf.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
