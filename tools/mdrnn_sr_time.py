"""Times of the 2D RNN's stochastic-reconfiguration entry points beside the plain gradient on the same resident batch
(docs/sr_2d.md):

    python tools/mdrnn_sr_time.py [--nx 5] [--ny 5] [--units 50] [--ns 500] [--reps 20]

Per repetition the batch is loaded again (untimed), which drops the resident Jacobian; then, each ending in a device synchronise and
timed with the host clock: the Jacobian build (rnnwf_log_derivatives_2d with out = NULL: the unit-weight backward pass and the
outer-product pass), rnnwf_sr_gram_2d, rnnwf_sr_apply_2d and rnnwf_vmc_gradient (untouched by the SR code); then, on a Jacobian that
is already built, one rnnwf_sr_direction_2d call (Gram matrix, Cholesky factorisation, both triangular solves and dO^T y on the
device).  Prints the median of each.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from rnnwavefunctions_amd import _lib  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=5)
    ap.add_argument("--ny", type=int, default=5)
    ap.add_argument("--units", type=int, default=50)
    ap.add_argument("--ns", type=int, default=500)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    wf = _lib.NativeWavefunction(_lib.MODEL_MDRNN2D, a.nx, a.ny, (a.units,))
    wf.init_params(111)
    couplings = np.append(np.ones(a.nx * a.ny), 2.0)
    out = wf.vmc_step(a.ns, 111, 0, couplings, want_samples=True, want_eloc=True)
    s, e = out["samples"], out["eloc"]
    y = np.random.RandomState(1).standard_normal(a.ns)
    times = {k: [] for k in ("jacobian", "gram", "apply", "gradient", "direction")}

    def timed(key, fn):
        t0 = time.perf_counter()
        r = fn()
        wf.synchronize()
        times[key].append((time.perf_counter() - t0) * 1e3)
        return r

    def build_jacobian():
        wf._check(wf.lib.rnnwf_log_derivatives_2d(wf.h, None, 0, 0))

    mean = float(e.mean())
    for rep in range(a.reps + 3):
        wf.load_batch(s, e)
        timed("jacobian", build_jacobian)
        timed("gram", wf.sr_gram_2d)
        timed("apply", lambda: wf.sr_apply_2d(y))
        timed("gradient", lambda: wf._check(wf.lib.rnnwf_vmc_gradient(wf.h, mean, 0.0, float(a.ns))))
        build_jacobian()                                                  # untimed: the gradient reused the Jacobian's inputs
        timed("direction", lambda: wf.sr_direction_2d(1e-3))
    med = {k: float(np.median(v[3:])) for k, v in times.items()}          # the first three repetitions warm up
    print("2D RNN, %d x %d units %d ns %d, %d params, median of %d repetitions [ms]: jacobian %.3f  gram %.3f  apply %.3f  "
          "device direction %.3f  |  vmc_gradient %.3f"
          % (a.nx, a.ny, a.units, a.ns, wf.num_params(), a.reps, med["jacobian"], med["gram"], med["apply"], med["direction"], med["gradient"]))


if __name__ == "__main__":
    main()
