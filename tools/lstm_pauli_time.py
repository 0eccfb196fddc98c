"""HIP-event time per cell evaluation of the LSTM's masked-tail pass (lstm_masked_tail_kernel, rnnwf_pauli_step_lstm) against the TFIM
flip pass (lstm_flip_kernel, rnnwf_vmc_step) on the same wave function, alternating in one process (docs/pauli_lstm.md; not part of
bench.py).

    10 x 10, 50 units, 10 000 samples, one single-X mask per site: N (N + 1) / 2 cell evaluations per chain in the masked-tail pass
    (the mask of site f restarts at f and runs N - f cells), N (N - 1) / 2 in the flip pass (it restarts one site later)

Both are timer id 1 of rnnwf_timing_get: events around the one kernel launch, cell evaluations from its work counter.  Medians over
--reps launches of each leg.

    python tools/lstm_pauli_time.py [--reps 7] [--out profiles/lstm_pauli_time.txt]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rnnwavefunctions_amd import _lib, params as P  # noqa: E402

SCOPE = "RNNwavefunction"


def timed(wf, call):
    """(ms, cell evaluations) of timer id 1 over one call"""
    wf.timing_reset()
    call()
    wf.synchronize()
    t = wf.timing_get(1)
    assert t["launches"] == 1
    return t["total_ms"], t["cell_evals"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=10)
    ap.add_argument("--ny", type=int, default=10)
    ap.add_argument("--H", type=int, default=50)
    ap.add_argument("--ns", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    nx, ny, H, ns = args.nx, args.ny, args.H, args.ns
    N = nx * ny
    wf = _lib.NativeWavefunction(_lib.MODEL_LSTM1D_F64, nx, ny, (H,))
    wf.set_params(P.init_lstm_params([H], seed=111, scope=SCOPE), scope=SCOPE)
    flip = np.eye(N, dtype=np.int32)
    sign, coeff = np.zeros_like(flip), np.ones(N)
    couplings = np.append(np.ones(N), 3.0)
    wf.timing_enable(True)

    def tails():
        wf.pauli_step_lstm(flip, sign, coeff, ns, seed=111, step=0)

    def flips():
        wf.vmc_step(ns, seed=111, step=0, couplings=couplings)

    timed(wf, tails)                                     # warm-up: code objects, buffers
    timed(wf, flips)
    tt, tf = [], []
    for _ in range(args.reps):                           # alternating: drifts of clock and temperature hit both
        tt.append(timed(wf, tails))
        tf.append(timed(wf, flips))
    wf.close()
    cells_t, cells_f = tt[0][1], tf[0][1]
    assert cells_t == ns * N * (N + 1) / 2 and cells_f == ns * N * (N - 1) / 2
    mt, mf = np.median([t for t, _ in tt]), np.median([t for t, _ in tf])
    pt, pf = mt * 1e6 / cells_t, mf * 1e6 / cells_f
    lines = ["LSTM1D_F64 %d x %d, %d units, %d samples, one single-X mask per site; HIP events around the one launch of timer id 1, %d launches "
             "per leg alternating in one process, medians" % (nx, ny, H, ns, args.reps),
             "    lstm_masked_tail_kernel  %9.3f ms (%.3f .. %.3f)  %.4e cell evaluations  %.4f ns per cell evaluation"
             % (mt, min(t for t, _ in tt), max(t for t, _ in tt), cells_t, pt),
             "    lstm_flip_kernel         %9.3f ms (%.3f .. %.3f)  %.4e cell evaluations  %.4f ns per cell evaluation"
             % (mf, min(t for t, _ in tf), max(t for t, _ in tf), cells_f, pf),
             "    masked tail / flip, per cell evaluation: %.3f" % (pt / pf)]
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
