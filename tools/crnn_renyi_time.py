"""Paired tail pass of rnnwf_renyi2_regions_complex (survivors only, compacted) vs the masked-tail pass of rnnwf_pauli_step_complex,
alternating in one process on one handle and on the same chains (not part of bench.py).  BASELINE config 3's size: the complex RNN
on N = 40 sites, 50 units, 5 000 pairs = 10 000 chains.  The Renyi pass runs the N - 1 cuts of the chain; the Pauli pass N - 1
two-site flip masks {l - 1, l}, l = 1..N-1, whose first sites and hence chain lengths are close to the cuts'.  Id 1 of the Renyi
pass holds the survivor lists, the tile scan and the paired tails; of the Pauli pass its one masked-tail launch.  Printed from the
medians of the HIP-event times:

  * ms per EVALUATED cell step of both passes (id 1 over work[0]) and their ratio - the once-per-tile gather, the list kernels and
    the ragged last tile of every region are what it holds beyond 1;
  * the measured survivor fraction over the cuts (surviving chains x steps over all chains x steps);
  * id 1 of the Renyi pass over (the cells an uncompacted pass would run) x (the Pauli pass's time per cell): what compaction
    leaves of the uncompacted cost; close to the survivor fraction if the per-cell times agree.

    python tools/crnn_renyi_time.py [--N 40] [--H 50] [--npairs 5000] [--reps 7] [--out profiles/crnn_renyi_time.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rnnwavefunctions_amd import _lib, params as P  # noqa: E402


def timed(wf, call):
    wf.timing_reset()
    t0 = time.perf_counter()
    call()
    wall = (time.perf_counter() - t0) * 1e3
    return [wf.timing_get(i) for i in (0, 1, 2)] + [wall]


def summary(name, rs):
    t = {i: np.median([x[i]["total_ms"] for x in rs]) for i in (0, 1, 2)}
    cells = np.median([x[1]["cell_evals"] for x in rs])
    per = np.median([x[1]["total_ms"] / max(x[1]["cell_evals"], 1) for x in rs])
    line = ("%-11s: id0 %.3f ms, id1 %.3f ms (min %.3f, max %.3f), id2 %.3f ms, wall %.3f ms; id1 cells %.6g -> %.4e ms per evaluated cell step"
            % (name, t[0], t[1], min(x[1]["total_ms"] for x in rs), max(x[1]["total_ms"] for x in rs), t[2],
               np.median([x[3] for x in rs]), cells, per))
    return line, per, t[1], cells


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=40)
    ap.add_argument("--H", type=int, default=50)
    ap.add_argument("--npairs", type=int, default=5000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    N, H, npairs = args.N, args.H, args.npairs
    wf = _lib.NativeWavefunction(_lib.MODEL_CRNN_U1, N, 1, (H,))
    wf.set_params(P.init_gru_params([H], seed=111, heads=("wf_dense_ampl", "wf_dense_phase")), scope="RNNwavefunction")
    wf.timing_enable(True)
    samples = wf.sample(2 * npairs, seed=111)
    cuts = (np.arange(N)[None, :] < np.arange(1, N)[:, None]).astype(np.int32)
    bonds = np.zeros((N - 1, N), dtype=np.int32)
    for l in range(1, N):
        bonds[l - 1, l - 1:l + 1] = 1
    zero, ones = np.zeros_like(bonds), np.ones(N - 1)

    def renyi():
        return wf.renyi2_regions_complex(cuts, npairs, samples=samples)

    def pauli():
        return wf.pauli_step_complex(bonds, zero, ones, 2 * npairs, samples=samples)

    for _ in range(2):                                   # warm-up: code objects, buffers
        renyi()
        pauli()
    rows = {"paired tail": [], "masked tail": []}
    for _ in range(args.reps):                           # alternating: drifts of clock and temperature hit both
        rows["paired tail"].append(timed(wf, renyi))
        rows["masked tail"].append(timed(wf, pauli))
    lines = ["complex RNN N = %d, %d units, %d pairs = %d chains, engine %s: %d cuts vs %d two-site masks on the same chains; %d reps "
             "alternating on one handle, medians of HIP-event times" % (N, H, npairs, 2 * npairs, wf.engine_name(), N - 1, N - 1, args.reps)]
    res = {}
    for name, rs in rows.items():
        line, per, id1, cells = summary(name, rs)
        res[name] = (per, id1, cells)
        lines.append(line)
    uncompacted = 2.0 * npairs * sum(N - l for l in range(1, N))      # every chain of every cut from its first swapped site
    frac = res["paired tail"][2] / uncompacted
    lines.append("paired tail / masked tail (id 1, ms per evaluated cell step) = %.3f   (expected <= 1.15)" % (res["paired tail"][0] / res["masked tail"][0]))
    lines.append("survivor fraction over the cuts (evaluated / uncompacted cell steps) = %.4f" % frac)
    lines.append("paired tail id 1 / (uncompacted cell steps x masked tail per-cell time) = %.4f"
                 % (res["paired tail"][1] / (uncompacted * res["masked tail"][0])))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
