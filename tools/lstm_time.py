"""LSTM vs float64 GRU over the raster path at equal (Nx, Ny, H, ns): ms per vmc_step and the flip pass's HIP-event time,
alternating the two models in one process (not part of bench.py).  Sizes: the run script's 4x4 / 50 units / 500 samples and
10x10 / 50 / 10 000.  The flip pass's fraction of the 78.6 TF float64 MFMA peak is taken on useful work,
F_cell = 8 h^2 + 2 h (LSTM: [x, h] K over the four gates, the one-hot rows folded into the bias table; head: one logit
difference) and 6 h^2 + 2 h (GRU), per cell evaluation of the flip pass (docs/lstm.md); the "issued" figure counts the padded
MFMAs the kernels actually run (rnnwf_timing_get work[1]).

    python tools/lstm_time.py [--reps 5] [--sizes 4x4x50x500,10x10x50x10000]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rnnwavefunctions_amd import _lib, params as P  # noqa: E402

PEAK_F64 = 78.6e12


def make(model, Nx, Ny, H):
    wf = _lib.NativeWavefunction(model, Nx, Ny, (H,))
    if model == _lib.MODEL_LSTM1D_F64:
        prm = P.init_lstm_params([H], seed=111)
    else:
        prm = P.init_gru_params([H], seed=111, dtype=np.float64)
    wf.set_params(P.scale_kernels(prm, 1.5), scope="RNNwavefunction")
    return wf


def one(wf, ns, couplings, step):
    wf.timing_reset()
    t0 = time.perf_counter()
    wf.vmc_step(ns, seed=111, step=step, couplings=couplings)
    wall = (time.perf_counter() - t0) * 1e3
    f = wf.timing_get(1)
    return wall, f["total_ms"], f["cell_evals"], f["mfma_flops"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="4x4x50x500,10x10x50x10000", help="Nx x Ny x H x ns, comma separated")
    args = ap.parse_args()
    for Nx, Ny, H, ns in (tuple(int(v) for v in sz.split("x")) for sz in args.sizes.split(",")):
        couplings = np.append(np.ones(Nx * Ny), 3.0)
        wfs = {"lstm": make(_lib.MODEL_LSTM1D_F64, Nx, Ny, H), "gru64": make(_lib.MODEL_GRU1D_F64, Nx, Ny, H)}
        fcell = {"lstm": 8.0 * H * H + 2.0 * H, "gru64": 6.0 * H * H + 2.0 * H}
        for wf in wfs.values():
            wf.timing_enable(True)
            for k in range(2):                                   # warm-up: kernel loads, buffers
                one(wf, ns, couplings, k)
        res = {k: [] for k in wfs}
        for r in range(args.reps):                               # alternating, so drifts of clock and temperature hit both
            for k, wf in wfs.items():
                res[k].append(one(wf, ns, couplings, 10 + r))
        med = {}
        for k, rows in res.items():
            a = np.array(rows)
            wall, flip, cells, issued = np.median(a[:, 0]), np.median(a[:, 1]), a[0, 2], a[0, 3]
            med[k] = flip
            print("%dx%d H=%d ns=%d %-5s: %.3f ms per vmc_step, flip pass %.3f ms, %.1f %% of the f64 MFMA peak "
                  "(useful F_cell = %.0f), %.1f %% issued"
                  % (Nx, Ny, H, ns, k, wall, flip, 100.0 * cells * fcell[k] / (flip * 1e-3) / PEAK_F64, fcell[k],
                     100.0 * issued / (flip * 1e-3) / PEAK_F64))
        print("%dx%d H=%d ns=%d: flip LSTM / GRU f64 = %.2f" % (Nx, Ny, H, ns, med["lstm"] / med["gru64"]))
        for wf in wfs.values():
            wf.close()


if __name__ == "__main__":
    main()
