"""Flip-mask pass of rnnwf_pauli_step vs the region pass of rnnwf_renyi2_regions at equal cell work, alternating in one process on
one handle (not part of bench.py).  Regions = the N - 1 suffix sets {l..N-1} on `pairs` pairs; masks = the same sets on 2 x pairs
chains: the same first sites, so work[0] is equal.  Prints the HIP-event medians of kernel ids 0 / 1 / 2 of both, the id-1 time per
cell evaluation and their ratio (the region pass is the yardstick; docs/renyi_regions.md allowed it 1.15 over the swap pass, and the
flip-mask pass runs the same step with one spin word read instead of two).  Once for the f32 chain (N = 80, 50 units) and once for
the f64 raster model (8 x 8, 50 units).  Then, for information: pauli_step with tfim_hamiltonian against rnnwf_vmc_step under
RNNWF_ENGINE=f32 at the same size; the defaults (N = 80, 50 units, 2 x 5000 = 10 000 chains) are BASELINE.md's config 2.

    python tools/pauli_time.py [--N 80] [--H 50] [--pairs 5000] [--reps 7] [--out profiles/pauli_time.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rnnwavefunctions_amd import _lib, params as P  # noqa: E402
from rnnwavefunctions_amd.observables import tfim_hamiltonian  # noqa: E402


def make(model, Nx, Ny, H, dtype):
    wf = _lib.NativeWavefunction(model, Nx, Ny, (H,))
    wf.set_params(P.randomize_biases(P.scale_kernels(P.init_gru_params([H], seed=111, dtype=dtype), 2.0), 112), scope="RNNwavefunction")
    wf.timing_enable(True)
    return wf


def timed(wf, call, k):
    wf.timing_reset()
    t0 = time.perf_counter()
    call(k)
    wall = (time.perf_counter() - t0) * 1e3
    return [wf.timing_get(i) for i in (0, 1, 2)] + [wall]


def summary(name, rs):
    t = {i: np.median([x[i]["total_ms"] for x in rs]) for i in (0, 1, 2)}
    cells = rs[0][1]["cell_evals"]
    line = ("%-9s: id0 %.3f ms, id1 %.3f ms (min %.3f, max %.3f), id2 %.3f ms, wall %.3f ms; id1 cells %.6g -> %.4f ns per cell evaluation"
            % (name, t[0], t[1], min(x[1]["total_ms"] for x in rs), max(x[1]["total_ms"] for x in rs), t[2],
               np.median([x[3] for x in rs]), cells, t[1] * 1e6 / max(cells, 1)))
    return line, t[1] / max(cells, 1)


def region_vs_flip_mask(wf, N, npairs, reps, label):
    suffixes = (np.arange(N)[None, :] >= np.arange(1, N)[:, None]).astype(np.int32)
    zeros, ones = np.zeros_like(suffixes), np.ones(N - 1)

    def regions(k):
        wf.renyi2_regions(suffixes, npairs, seed=111, step=k)

    def pauli(k):
        wf.pauli_step(suffixes, zeros, ones, 2 * npairs, seed=111, step=k)

    for k in range(2):                                   # warm-up: code objects, buffers
        regions(k)
        pauli(k)
    rows = {"regions": [], "flip-mask": []}
    for r in range(reps):                                # alternating: drifts of clock and temperature hit both
        rows["regions"].append(timed(wf, regions, 10 + r))
        rows["flip-mask"].append(timed(wf, pauli, 10 + r))
    lines = ["%s, %d pairs = %d chains, the %d suffix sets; %d reps alternating on one handle, medians of HIP-event times"
             % (label, npairs, 2 * npairs, N - 1, reps)]
    per = {}
    for name, rs in rows.items():
        line, per[name] = summary(name, rs)
        lines.append(line)
    assert rows["regions"][0][1]["cell_evals"] == rows["flip-mask"][0][1]["cell_evals"] == npairs * N * (N - 1)
    lines.append("flip-mask / regions (id 1, per cell evaluation) = %.3f   (expected <= 1.15)" % (per["flip-mask"] / per["regions"]))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=80)
    ap.add_argument("--H", type=int, default=50)
    ap.add_argument("--pairs", type=int, default=5000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    N, H, npairs = args.N, args.H, args.pairs
    lines = region_vs_flip_mask(make(_lib.MODEL_GRU1D, N, 1, H, np.float32), N, npairs, args.reps, "N=%d H=%d f32" % (N, H))
    lines += region_vs_flip_mask(make(_lib.MODEL_GRU1D_F64, 8, 8, H, np.float64), 64, npairs, args.reps, "8x8 H=%d f64" % H)

    # for information, no bound: the generic path on the hard-wired Hamiltonian's own ground
    before = os.environ.get("RNNWF_ENGINE")
    os.environ["RNNWF_ENGINE"] = "f32"
    try:
        wf = make(_lib.MODEL_GRU1D, N, 1, H, np.float32)
    finally:
        if before is None:
            del os.environ["RNNWF_ENGINE"]
        else:
            os.environ["RNNWF_ENGINE"] = before
    ns = 2 * npairs
    ham = tfim_hamiltonian(np.ones(N), 1.0)
    couplings = np.append(np.ones(N), 1.0)

    def step(k):
        wf.vmc_step(ns, seed=111, step=k, couplings=couplings)

    def pauli(k):
        wf.pauli_step(ham.flip, ham.sign, ham.coeff, ns, seed=111, step=k)

    for k in range(2):
        step(k)
        pauli(k)
    rows = {"vmc_step": [], "pauli_step": []}
    for r in range(args.reps):
        rows["vmc_step"].append(timed(wf, step, 10 + r))
        rows["pauli_step"].append(timed(wf, pauli, 10 + r))
    lines.append("TFIM, N=%d H=%d f32 (RNNWF_ENGINE=f32), %d chains: rnnwf_vmc_step vs rnnwf_pauli_step with tfim_hamiltonian (%d terms); "
                 "for information" % (N, H, ns, len(ham)))
    for name, rs in rows.items():
        lines.append(summary(name, rs)[0])
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
