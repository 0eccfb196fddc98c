"""Trunk + branch passes of rnnwf_correlations vs the f32-input-MFMA (f64: f64-MFMA) flip pass of the same handle, alternating in
one process (not part of bench.py).  The correlation pass does N(N-1)/2 + N(N-1)(N-2)/6 cell evaluations per chain, the flip pass of
a vmc_step N(N-1)/2; the comparison is per cell evaluation.  Prints the HIP-event time of kernel id 1 of both, the time per cell
evaluation and their ratio, each one's fraction of the MFMA peak (157.3 TF f32, 78.6 TF f64) on the MFMA flops it issues
(rnnwf_timing_get work[1]), and the bytes of trunk states written with the HBM rate they imply.

    python tools/corr_time.py [--reps 7] [--out profiles/corr_time.txt]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rnnwavefunctions_amd import _lib, params as P  # noqa: E402

PEAK = {False: 157.3e12, True: 78.6e12}
# f64, Nx, Ny, units, chains
CONFIGS = [(False, 80, 1, 50, 1000), (False, 80, 1, 50, 10000), (True, 8, 8, 50, 1000)]


def make(f64, Nx, Ny, H):
    os.environ["RNNWF_ENGINE"] = "f32"                 # read at create: the flip pass on the f32-input MFMA
    try:
        wf = _lib.NativeWavefunction(_lib.MODEL_GRU1D_F64 if f64 else _lib.MODEL_GRU1D, Nx, Ny, (H,))
    finally:
        os.environ.pop("RNNWF_ENGINE", None)
    prm = P.init_gru_params([H], seed=111, dtype=np.float64 if f64 else np.float32)
    wf.set_params(P.randomize_biases(P.scale_kernels(prm, 2.0), 112), scope="RNNwavefunction")
    wf.timing_enable(True)
    return wf


def state_bytes(f64, H):
    nfull = next(nf for nf in (1, 2, 3, 4, 6, 8, 12, 16) if 16 * nf + 4 >= H)
    return (16 * nfull + 4) // 4 * 64 * (8 if f64 else 4)      # KT x 64 lanes x element: one 16-chain block's state


def measure(f64, Nx, Ny, H, ns, reps):
    N = Nx * Ny
    wf = make(f64, Nx, Ny, H)
    couplings = np.append(np.ones(N), 1.0)

    def corr(k):
        wf.timing_reset()
        wf.correlations(ns, seed=111, step=k)
        return [wf.timing_get(i) for i in (0, 1, 2)]

    def flip(k):
        wf.timing_reset()
        wf.vmc_step(ns, seed=111, step=k, couplings=couplings)
        return [wf.timing_get(i) for i in (0, 1, 2)]

    for k in range(2):                                   # warm-up: code objects, buffers
        corr(k)
        flip(k)
    rows = {"corr": [], "flip": []}
    for r in range(reps):                                # alternating: drifts of clock and temperature hit both
        rows["corr"].append(corr(10 + r))
        rows["flip"].append(flip(10 + r))
    lines = ["%s %dx%d H=%d chains=%d (flip engine %s), %d reps alternating, medians of HIP-event times"
             % ("f64" if f64 else "f32", Nx, Ny, H, ns, wf.engine_name(), reps)]
    per_cell = {}
    for name, rs in rows.items():
        t = {i: float(np.median([x[i]["total_ms"] for x in rs])) for i in (0, 1, 2)}
        cells, flops = rs[0][1]["cell_evals"], rs[0][1]["mfma_flops"]
        per_cell[name] = t[1] * 1e6 / cells
        lines.append("%-4s: id0 %.3f ms, id1 %.3f ms (min %.3f, max %.3f), id2 %.3f ms; id1 cells %.4g -> %.4f ns per cell evaluation; "
                     "MFMA flops %.4g -> %.1f %% of the MFMA peak"
                     % (name, t[0], t[1], min(x[1]["total_ms"] for x in rs), max(x[1]["total_ms"] for x in rs), t[2], cells,
                        per_cell[name], flops, 100.0 * flops / (t[1] * 1e-3) / PEAK[f64]))
        if name == "corr":
            t1 = t[1]
    nsb = (ns + 15) // 16
    written = (N - 1) * (N - 2) // 2 * nsb * state_bytes(f64, H)          # trunk states stored (sites i+1..N-2 of every trunk) = read back once
    lines.append("time per cell evaluation, corr / flip = %.3f" % (per_cell["corr"] / per_cell["flip"]))
    lines.append("trunk states written %.3f GB (and read once by the branch pass): %.1f GB/s over the id 1 time"
                 % (written / 1e9, 2.0 * written / 1e9 / (t1 * 1e-3)))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []
    for cfg in CONFIGS:
        lines += measure(*cfg, reps=args.reps) + [""]
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
