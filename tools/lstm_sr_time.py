"""Times of one minSR iteration of the LSTM wave function beside its plain gradient iteration (docs/sr_lstm.md):

    python tools/lstm_sr_time.py [--reps 7] [--sizes 4x4:50:500,10x10:50:2000]

In one process and on one handle per size, alternating: rnnwf_sr_step_lstm (fused step, Jacobian, Gram matrix, solve, direction) and
rnnwf_lstm_vmc_gradient_step (fused step, backward pass, weight-gradient product), each one call with one host synchronisation, timed
with the host clock; after three warm-up rounds the median, minimum and maximum of --reps rounds, and the ratio of the medians.
Then the split of one minSR iteration by the library's timers (HIP events, rnnwf_timing_get): base and flip pass of the fused step,
and - by calls on the batch that step left, the timers reset between them - the backward pass in unit-weight mode, the outer-product
pass, the column means with the Gram matrix, the Cholesky solve, and dO^T y; beside them the weighted backward pass and the
weight-gradient product of the plain gradient.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from rnnwavefunctions_amd import _lib, params as P  # noqa: E402

SCOPE = "RNNwavefunction"
SHIFT = 1e-3
BASE, FLIP, ASSEMBLY, BACKPROP, GEMM = range(5)


def timers(wf):
    return [wf.timing_get(k)["total_ms"] for k in range(5)]


def one_size(nx, ny, units, ns, reps):
    wf = _lib.NativeWavefunction(_lib.MODEL_LSTM1D_F64, nx, ny, (units,))
    prm = P.init_lstm_params([units], seed=111)
    wf.set_params(prm, scope=SCOPE)
    shapes = {k[len(SCOPE) + 1:]: v.shape for k, v in prm.items()}
    couplings = np.append(np.ones(nx * ny), 2.0)
    t = {"sr": [], "grad": []}
    for rep in range(reps + 3):
        t0 = time.perf_counter()
        wf.sr_step_lstm(ns, 111, rep, couplings, SHIFT)
        t1 = time.perf_counter()
        wf.lstm_vmc_gradient_step(ns, 111, rep, couplings, shapes)
        t2 = time.perf_counter()
        t["sr"].append((t1 - t0) * 1e3)
        t["grad"].append((t2 - t1) * 1e3)
    sr_ms, g_ms = np.array(t["sr"][3:]), np.array(t["grad"][3:])
    print("%dx%d, %d units (%d parameters), %d samples, %d rounds after 3 warm-up [ms]:" % (nx, ny, units, wf.num_params(), ns, reps))
    print("  sr_step_lstm            median %.3f  min %.3f  max %.3f" % (np.median(sr_ms), sr_ms.min(), sr_ms.max()))
    print("  lstm_vmc_gradient_step  median %.3f  min %.3f  max %.3f" % (np.median(g_ms), g_ms.min(), g_ms.max()))
    print("  minSR step / plain gradient step  %.2f" % (np.median(sr_ms) / np.median(g_ms)))
    # the split, by timer: medians over the same number of rounds
    wf.timing_enable(True)
    split = {k: [] for k in ("base", "flip", "assembly", "backward_sr", "outer", "gram", "solve", "apply", "backward", "tn_gemm")}
    for rep in range(reps + 1):
        wf.timing_reset()
        out = wf.vmc_step(ns, 111, rep, couplings, want_samples=True, want_eloc=True)
        wf.synchronize()
        tm = timers(wf)
        split["base"].append(tm[BASE]); split["flip"].append(tm[FLIP]); split["assembly"].append(tm[ASSEMBLY])
        wf.lstm_load_batch(out["samples"], out["eloc"])
        wf.timing_reset()
        wf._check(wf.lib.rnnwf_log_derivatives_lstm(wf.h, None, 0, 0))
        wf.synchronize()
        tm = timers(wf)
        split["backward_sr"].append(tm[BACKPROP]); split["outer"].append(tm[GEMM])
        wf.timing_reset()
        wf.sr_gram_lstm()
        gram = timers(wf)[GEMM]
        split["gram"].append(gram)
        wf.timing_reset()
        y = wf.sr_solve_lstm(SHIFT)
        split["solve"].append(timers(wf)[GEMM] - gram)              # the solving entry forms the Gram matrix again
        wf.timing_reset()
        wf.sr_apply_lstm(y)
        split["apply"].append(timers(wf)[GEMM])
        wf.timing_reset()
        wf.lstm_gradient(out["samples"], (out["eloc"] - out["eloc"].mean()) / ns, shapes)
        tm = timers(wf)
        split["backward"].append(tm[BACKPROP]); split["tn_gemm"].append(tm[GEMM])
    wf.timing_enable(False)
    med = {k: float(np.median(v[1:])) for k, v in split.items()}
    print("  by timer [ms]: base %.3f  flip %.3f  assembly %.3f | backward (unit weights) %.3f  outer product %.3f  Gram %.3f  solve %.3f  dO^T y %.3f"
          " | backward (weighted) + head reduction %.3f  P^T Q %.3f"
          % tuple(med[k] for k in ("base", "flip", "assembly", "backward_sr", "outer", "gram", "solve", "apply", "backward", "tn_gemm")))
    on_batch = med["backward_sr"] + med["outer"] + med["gram"] + med["solve"] + med["apply"]
    print("  on the resident batch: Jacobian + Gram + solve + dO^T y %.3f against backward + P^T Q %.3f: ratio %.2f"
          % (on_batch, med["backward"] + med["tn_gemm"], on_batch / (med["backward"] + med["tn_gemm"])))
    wf.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sizes", default="4x4:50:500,10x10:50:2000")
    a = ap.parse_args()
    for size in a.sizes.split(","):
        lat, units, ns = size.split(":")
        nx, ny = (int(v) for v in lat.split("x"))
        one_size(nx, ny, int(units), int(ns), a.reps)


if __name__ == "__main__":
    main()
