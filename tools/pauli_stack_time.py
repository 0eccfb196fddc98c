"""ms per training iteration of a STACK of GRU layers on a generic Pauli-string Hamiltonian: the host loop (pauli_step_stack ->
cost_gradient -> training.Adam -> set_params, what observables_stack.minimize_hamiltonian(device_steps=None) runs) against the
device-resident iterations (pauli_train_steps_stack, what device_steps=K runs), alternating in one process (docs/pauli_stack.md; not
part of bench.py).

    N = 20, two layers of 50 units, 500 samples (GRU1D, float32), open XXZ chain (xxz_hamiltonian, Jxy = -1, Jz = 0.5)

A chunk is K iterations.  The host clock is read only around calls that end in a stream synchronisation: a host-loop chunk ends in
set_params behind vmc_gradient's synchronisation and is closed by wf.synchronize(); a device chunk is one call.  Medians over --reps
chunks of each leg.  Exit status 1 if the device path is slower than the host loop.

    python tools/pauli_stack_time.py [--K 64] [--reps 7] [--out profiles/pauli_stack_time.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rnnwavefunctions_amd import _lib, observables as O, params as P, training as T  # noqa: E402

SCOPE = "RNNwavefunction"


def legs(wf, ham, prm, ns, K):
    state = {"params": {k: np.array(v) for k, v in prm.items()}, "opt": T.Adam()}

    def host(it0):
        params, opt = state["params"], state["opt"]
        for it in range(it0, it0 + K):
            s1, s2, n, _ = wf.pauli_step_stack(ham.flip, ham.sign, ham.coeff, ns, seed=111, step=it)["moments"]
            grads = T.cost_gradient(wf, params, SCOPE, s1 / n, n)
            params = opt.step(params, grads, 5e-3)
            wf.set_params(params, scope=SCOPE)
        wf.synchronize()
        state["params"] = params

    def device(it0):
        wf.pauli_train_steps_stack(ham.flip, ham.sign, ham.coeff, ns, 111, it0, [5e-3] * K)

    return host, device


def clocked(call, it0):
    t0 = time.perf_counter()
    call(it0)
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=20)
    ap.add_argument("--H", type=int, default=50)
    ap.add_argument("--layers", type=int, default=2)
    ap.add_argument("--ns", type=int, default=500)
    ap.add_argument("--K", type=int, default=64)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    N, H, NL, ns, K = args.N, args.H, args.layers, args.ns, args.K
    lines = ["N = %d, %d layers of %d units, %d samples, chunks of K = %d iterations, %d chunks per leg alternating in one process, medians of "
             "host-clock times around calls that end in a synchronisation" % (N, NL, H, ns, K, args.reps)]
    prm = P.init_gru_params([H] * NL, seed=111)
    ham = O.xxz_hamiltonian(N, -1.0, 0.5)
    wf = _lib.NativeWavefunction(_lib.MODEL_GRU1D, N, 1, (H,) * NL)
    wf.set_params(prm, scope=SCOPE)
    host, device = legs(wf, ham, prm, ns, K)
    host(0)                                              # warm-up: code objects, buffers, the tables of the device path
    device(K)
    th, td = [], []
    for r in range(args.reps):                           # alternating: drifts of clock and temperature hit both
        th.append(clocked(host, (2 + 2 * r) * K))
        td.append(clocked(device, (3 + 2 * r) * K))
    mh, md = np.median(th) / K, np.median(td) / K
    nmasks = len({r.tobytes() for r in ham.flip if r.any()})
    lines.append("GRU1D float32 stack, open XXZ chain (Jxy = -1, Jz = 0.5): %d terms on %d flip masks" % (len(ham), nmasks))
    lines.append("    host loop       %8.3f ms per iteration (chunks %.1f .. %.1f ms)" % (mh, min(th), max(th)))
    lines.append("    device_steps=%-3d %8.3f ms per iteration (chunks %.1f .. %.1f ms)   host / device = %.1f" % (K, md, min(td), max(td), mh / md))
    wf.close()
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 1 if md > mh else 0


if __name__ == "__main__":
    sys.exit(main())
