"""Masked-tail pass of rnnwf_pauli_step_complex vs the J1-J2 swap pass of the fused step, alternating in one process on one handle
created under RNNWF_ENGINE=f32 (both passes on the f32-input MFMA; not part of bench.py).  BASELINE config 3's size: the complex RNN
on N = 40 sites, 50 units.  The Hamiltonian is observables_complex.j1j2_hamiltonian at the step's couplings: one flip mask per bond,
N - f cell evaluations per chain and mask, whether or not the bond is anti-aligned - the swap pass evaluates N - 1 - lo cells and only
for anti-aligned bonds, so the two passes do different amounts of work; the figure compared is the id-1 time PER cell evaluation
(work[0] of each).  Prints the HIP-event medians of kernel ids 0 / 1 / 2 of both, the time per cell evaluation and the ratio.  No
ratio is fixed in advance.

    python tools/crnn_pauli_time.py [--N 40] [--H 50] [--ns 10000] [--reps 7] [--out profiles/crnn_pauli_time.txt]
"""
import argparse
import os
import sys
import time

os.environ["RNNWF_ENGINE"] = "f32"                        # read at rnnwf_create

import numpy as np  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rnnwavefunctions_amd import _lib, observables_complex as OC, params as P  # noqa: E402


def timed(wf, call, k):
    wf.timing_reset()
    t0 = time.perf_counter()
    call(k)
    wall = (time.perf_counter() - t0) * 1e3
    return [wf.timing_get(i) for i in (0, 1, 2)] + [wall]


def summary(name, rs):
    t = {i: np.median([x[i]["total_ms"] for x in rs]) for i in (0, 1, 2)}
    cells = np.median([x[1]["cell_evals"] for x in rs])
    per = np.median([x[1]["total_ms"] / max(x[1]["cell_evals"], 1) for x in rs])       # ms per cell evaluation, the ratio's unit too
    line = ("%-11s: id0 %.3f ms, id1 %.3f ms (min %.3f, max %.3f), id2 %.3f ms, wall %.3f ms; id1 cells %.6g -> %.4e ms per cell evaluation"
            % (name, t[0], t[1], min(x[1]["total_ms"] for x in rs), max(x[1]["total_ms"] for x in rs), t[2],
               np.median([x[3] for x in rs]), cells, per))
    return line, per


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=40)
    ap.add_argument("--H", type=int, default=50)
    ap.add_argument("--ns", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    N, H, ns = args.N, args.H, args.ns
    wf = _lib.NativeWavefunction(_lib.MODEL_CRNN_U1, N, 1, (H,))
    wf.set_params(P.init_gru_params([H], seed=111, heads=("wf_dense_ampl", "wf_dense_phase")), scope="RNNwavefunction")
    wf.timing_enable(True)
    J1, J2, Bz = np.ones(N), 0.2 * np.ones(N), np.zeros(N)
    couplings = np.concatenate([J1, J2, Bz, [0.0, 0.0]])
    ham = OC.j1j2_hamiltonian(J1, J2, Bz)

    def swap(k):
        wf.vmc_step(ns, seed=111, step=k, couplings=couplings)

    def tail(k):
        wf.pauli_step_complex(ham.flip, ham.sign, ham.coeff, ns, seed=111, step=k)

    for k in range(2):                                   # warm-up: code objects, buffers
        swap(k)
        tail(k)
    rows = {"swap pass": [], "masked tail": []}
    for r in range(args.reps):                           # alternating: drifts of clock and temperature hit both
        rows["swap pass"].append(timed(wf, swap, 10 + r))
        rows["masked tail"].append(timed(wf, tail, 10 + r))
    lines = ["complex RNN N = %d, %d units, %d chains, engine %s, open J1-J2 chain (J2 = 0.2): %d terms; %d reps alternating on one handle, "
             "medians of HIP-event times" % (N, H, ns, wf.engine_name(), len(ham), args.reps)]
    per = {}
    for name, rs in rows.items():
        line, per[name] = summary(name, rs)
        lines.append(line)
    lines.append("masked tail / swap pass (id 1, ms per cell evaluation) = %.3f" % (per["masked tail"] / per["swap pass"]))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
