"""Times of the LSTM's all-pair correlation pass (rnnwf_correlations_lstm: lstm_trunk_kernel + lstm_branch_kernel) against the same
matrix through the masked-tail pass (rnnwf_pauli_step_lstm with one mask per site and per pair: lstm_masked_tail_kernel) on the same
wave function, alternating in one process (docs/correlations_lstm.md; not part of bench.py).

    8 x 8, 50 units, 1 000 chains and 4 x 4, 50 units, 500 chains; every site and every pair
    trunk + branch: N(N-1)/2 + N(N-1)(N-2)/6 cell evaluations per chain; masks: N(N+1)/2 + (N-1)N(N+1)/3

Per size: timer id 1 of rnnwf_timing_get (HIP events around the recurrent launches, cell evaluations from the work counter) and the
whole call (host clock around the call and a synchronisation, samples drawn on the device).  Medians over --reps rounds after a
warm-up round.

    python tools/lstm_corr_time.py [--reps 7] [--out profiles/lstm_corr_time.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rnnwavefunctions_amd import _lib, params as P  # noqa: E402

SCOPE = "RNNwavefunction"
SIZES = ((8, 8, 50, 1000), (4, 4, 50, 500))


def timed(wf, call, launches):
    """(ms of timer id 1, cell evaluations, whole-call ms) of one call"""
    wf.timing_reset()
    wf.synchronize()
    t0 = time.perf_counter()
    call()
    wf.synchronize()
    wall = (time.perf_counter() - t0) * 1e3
    t = wf.timing_get(1)
    assert t["launches"] == launches, t
    return t["total_ms"], t["cell_evals"], wall


def one_size(nx, ny, H, ns, reps):
    N = nx * ny
    wf = _lib.NativeWavefunction(_lib.MODEL_LSTM1D_F64, nx, ny, (H,))
    wf.set_params(P.init_lstm_params([H], seed=111, scope=SCOPE), scope=SCOPE)
    pi, pj = np.triu_indices(N, 1)
    flip = np.zeros((N + len(pi), N), dtype=np.int32)
    flip[np.arange(N), np.arange(N)] = 1
    flip[N + np.arange(len(pi)), pi] = 1
    flip[N + np.arange(len(pi)), pj] = 1
    sign, coeff = np.zeros_like(flip), np.ones(len(flip))
    wf.timing_enable(True)

    def corr():
        wf.correlations_lstm(ns, seed=111, step=0)

    def masks():
        wf.pauli_step_lstm(flip, sign, coeff, ns, seed=111, step=0)

    timed(wf, corr, 2)                                   # warm-up: code objects, buffers
    timed(wf, masks, 1)
    tc, tm = [], []
    for _ in range(reps):                                # alternating: drifts of clock and temperature hit both
        tc.append(timed(wf, corr, 2))
        tm.append(timed(wf, masks, 1))
    wf.close()
    cells_c, cells_m = tc[0][1], tm[0][1]
    assert cells_c == ns * (N * (N - 1) // 2 + N * (N - 1) * (N - 2) // 6)
    assert cells_m == ns * (N * (N + 1) // 2 + (N - 1) * N * (N + 1) // 3)
    kc, km = np.median([t[0] for t in tc]), np.median([t[0] for t in tm])
    wc, wm = np.median([t[2] for t in tc]), np.median([t[2] for t in tm])
    pc, pm = kc * 1e6 / cells_c, km * 1e6 / cells_m
    return ["LSTM1D_F64 %d x %d, %d units, %d chains, every site and pair (%d rows); %d rounds alternating in one process, medians"
            % (nx, ny, H, ns, len(flip), reps),
            "    trunk + branch (id 1)    %9.3f ms (%.3f .. %.3f)  %.4e cell evaluations  %.4f ns per cell evaluation"
            % (kc, min(t[0] for t in tc), max(t[0] for t in tc), cells_c, pc),
            "    masked tails   (id 1)    %9.3f ms (%.3f .. %.3f)  %.4e cell evaluations  %.4f ns per cell evaluation"
            % (km, min(t[0] for t in tm), max(t[0] for t in tm), cells_m, pm),
            "    trunk + branch / masked tails, per cell evaluation: %.3f   (evaluations: masks / trunk + branch = %.3f)"
            % (pc / pm, cells_m / cells_c),
            "    whole call: correlations_lstm %9.3f ms (%.3f .. %.3f), pauli_step_lstm %9.3f ms (%.3f .. %.3f): %.3f x"
            % (wc, min(t[2] for t in tc), max(t[2] for t in tc), wm, min(t[2] for t in tm), max(t[2] for t in tm), wm / wc)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []
    for nx, ny, H, ns in SIZES:
        lines += one_size(nx, ny, H, ns, args.reps)
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
