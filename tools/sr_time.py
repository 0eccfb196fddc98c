"""Times of the stochastic-reconfiguration entry points beside the plain gradient on the same resident batch (docs/sr.md):

    python tools/sr_time.py [--N 20] [--units 50] [--ns 500] [--f64] [--reps 20]

Per repetition the batch is loaded again (untimed), which drops the resident Jacobian; then, each ending in a device synchronise and
timed with the host clock: the Jacobian build (rnnwf_log_derivatives with out = NULL), rnnwf_sr_gram, rnnwf_sr_apply, the host
Cholesky solve, and rnnwf_vmc_gradient (untouched by the SR code: the gradient's time as before it); then, on a Jacobian that is
already built, one rnnwf_sr_direction call (Gram matrix, Cholesky factorisation, both triangular solves and dO^T y on the device): the
"device direction" column, to be set against gram + host solve + apply.  Prints the median of each.

    python tools/sr_time.py --train [--N 20] [--units 50] [--ns 500] [--f64] [--reps 20] [--K 32]

times one whole minSR training iteration both ways, from the same start: K iterations of the host loop, sr.train_tfim(solver="device")
(per iteration a synchronisation, the direction's download, the NumPy update, set_params_flat and the host packers), and the same K
iterations as ONE rnnwf_sr_train_steps call, sr.train_tfim(device_steps=K); each wall time / K, median over the repetitions, and
their ratio.  The two runs must return the same energies, bit for bit.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from rnnwavefunctions_amd import _lib, params as P, sr  # noqa: E402


def train_mode(a):
    wf = _lib.NativeWavefunction(_lib.MODEL_GRU1D_F64 if a.f64 else _lib.MODEL_GRU1D, a.N, 1, (a.units,))
    prm = P.init_gru_params([a.units], seed=111, dtype=np.float64 if a.f64 else np.float32)
    times, energies = {None: [], a.K: []}, {}
    for rep in range(a.reps + 3):
        for device_steps in times:
            t0 = time.perf_counter()
            energies[device_steps] = sr.train_tfim(wf, np.ones(a.N), 1.0, prm, numsteps=a.K - 1, numsamples=a.ns, learningrate=1e-2, diag_shift=1e-3,
                                                   seed=111, solver="device", device_steps=device_steps)
            wf.synchronize()
            times[device_steps].append((time.perf_counter() - t0) * 1e3 / a.K)
        assert energies[None] == energies[a.K], "the device iterations left the host loop's trajectory"
    host, dev = (float(np.median(v[3:])) for v in (times[None], times[a.K]))          # the first three repetitions warm up
    print("N %d units %d ns %d %s, %d params, one minSR training iteration, median of %d repetitions of %d iterations [ms]: host loop %.3f  "
          "device iterations (%d per call) %.3f  ratio %.2f  (E %.5f -> %.5f both ways)"
          % (a.N, a.units, a.ns, "f64" if a.f64 else "f32", wf.num_params(), a.reps, a.K, host, a.K, dev, host / dev, energies[a.K][0][0], energies[a.K][0][-1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=20)
    ap.add_argument("--units", type=int, default=50)
    ap.add_argument("--ns", type=int, default=500)
    ap.add_argument("--f64", action="store_true")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--train", action="store_true", help="time a whole training iteration: host loop against rnnwf_sr_train_steps")
    ap.add_argument("--K", type=int, default=32, help="--train: iterations per run and per device call")
    a = ap.parse_args()
    if a.train:
        return train_mode(a)
    wf = _lib.NativeWavefunction(_lib.MODEL_GRU1D_F64 if a.f64 else _lib.MODEL_GRU1D, a.N, 1, (a.units,))
    wf.init_params(111)
    couplings = np.append(np.ones(a.N), 1.0)
    out = wf.vmc_step(a.ns, 111, 0, couplings, want_samples=True, want_eloc=True)
    s, e = out["samples"], out["eloc"]
    times = {k: [] for k in ("jacobian", "gram", "solve", "apply", "gradient", "direction")}

    def timed(key, fn):
        t0 = time.perf_counter()
        r = fn()
        wf.synchronize()
        times[key].append((time.perf_counter() - t0) * 1e3)
        return r

    def build_jacobian():
        wf._check(wf.lib.rnnwf_log_derivatives(wf.h, None, 0, 0))

    for rep in range(a.reps + 3):
        wf.load_batch(s, e)
        timed("jacobian", build_jacobian)
        gram, eps = timed("gram", wf.sr_gram)
        y = timed("solve", lambda: sr.solve_shifted(gram, eps, 1e-3))
        timed("apply", lambda: wf.sr_apply(y))
        timed("gradient", lambda: wf._check(wf.lib.rnnwf_vmc_gradient(wf.h, float(e.mean()), 0.0, float(a.ns))))
        build_jacobian()                                                  # untimed: the gradient reused the Jacobian's inputs
        timed("direction", lambda: wf.sr_direction(1e-3))
    med = {k: float(np.median(v[3:])) for k, v in times.items()}          # the first three repetitions warm up
    print("N %d units %d ns %d %s, %d params, median of %d repetitions [ms]: jacobian %.3f  gram %.3f  apply %.3f  host solve %.3f  device direction %.3f  |  vmc_gradient %.3f"
          % (a.N, a.units, a.ns, "f64" if a.f64 else "f32", wf.num_params(), a.reps, med["jacobian"], med["gram"], med["apply"], med["solve"],
             med["direction"], med["gradient"]))


if __name__ == "__main__":
    main()
