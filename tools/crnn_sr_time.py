"""Times of the complex RNN's stochastic-reconfiguration entry points beside the plain gradient on the same resident batch
(docs/sr_complex.md):

    python tools/crnn_sr_time.py [--N 20] [--units 50] [--ns 500] [--reps 20]

Per repetition the batch is loaded again (untimed), which drops the resident Jacobian; then, each ending in a device synchronise and
timed with the host clock: the Jacobian build (rnnwf_log_derivatives_complex with out = NULL: two backward passes and two
outer-product passes), rnnwf_sr_gram_complex (order 2 ns), rnnwf_sr_apply_complex and rnnwf_vmc_gradient (untouched by the SR code);
then, on a Jacobian that is already built, one rnnwf_sr_direction_complex call (Gram matrix, Cholesky factorisation, both triangular
solves and Obar^T y on the device).  Prints the median of each.
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
    ap.add_argument("--N", type=int, default=20)
    ap.add_argument("--units", type=int, default=50)
    ap.add_argument("--ns", type=int, default=500)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    wf = _lib.NativeWavefunction(_lib.MODEL_CRNN_U1, a.N, 1, (a.units,))
    wf.init_params(111)
    couplings = np.concatenate([np.ones(a.N), 0.2 * np.ones(a.N), np.zeros(a.N), [0.0, 0.0]])
    out = wf.vmc_step(a.ns, 111, 0, couplings, want_samples=True, want_eloc=True)
    s, e = out["samples"], out["eloc"]
    y = np.random.RandomState(1).standard_normal(2 * a.ns)
    times = {k: [] for k in ("jacobian", "gram", "apply", "gradient", "direction")}

    def timed(key, fn):
        t0 = time.perf_counter()
        r = fn()
        wf.synchronize()
        times[key].append((time.perf_counter() - t0) * 1e3)
        return r

    def build_jacobian():
        wf._check(wf.lib.rnnwf_log_derivatives_complex(wf.h, None, 0, 0))

    mean = complex(e.mean())
    for rep in range(a.reps + 3):
        wf.load_batch(s, e)
        timed("jacobian", build_jacobian)
        timed("gram", wf.sr_gram_complex)
        timed("apply", lambda: wf.sr_apply_complex(y))
        timed("gradient", lambda: wf._check(wf.lib.rnnwf_vmc_gradient(wf.h, mean.real, mean.imag, float(a.ns))))
        build_jacobian()                                                  # untimed: the gradient reused the Jacobian's inputs
        timed("direction", lambda: wf.sr_direction_complex(1e-3))
    med = {k: float(np.median(v[3:])) for k, v in times.items()}          # the first three repetitions warm up
    print("complex RNN, N %d units %d ns %d (order %d), %d params, median of %d repetitions [ms]: jacobian %.3f  gram %.3f  apply %.3f  "
          "device direction %.3f  |  vmc_gradient %.3f"
          % (a.N, a.units, a.ns, 2 * a.ns, wf.num_params(), a.reps, med["jacobian"], med["gram"], med["apply"], med["direction"], med["gradient"]))


if __name__ == "__main__":
    main()
