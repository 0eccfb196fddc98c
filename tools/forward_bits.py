#!/usr/bin/env python3
"""One sha256 per output of the one-wave forward kernels of the f32/f64-input MFMA engine, for a fixed list of configurations.

    tools/forward_bits.py [--coop] [--lib PATH/librnnwf_hip.so]

Run it on two builds on the same machine and compare the listings line for line: a refactor of prnn_base_kernel / prnn_flip_kernel /
prnn_ml_* / crnn_base_kernel / crnn_swap_kernel / crnn_ml_* that keeps arithmetic and order keeps every line
(profiles/forward_stack_bits.txt).  RNNWF_ENGINE=f32 and RNNWF_NO_COOP=1 are set here, so these kernels are the ones that run.
Outputs: samples, their log-probabilities, teacher-forced log-probabilities (cRNN: log-amplitudes too), the log_probs queue, E_loc.

--coop: a second list of the same kind for the COOPERATIVE base passes (gru_kernels.h: coop_base_pass, coop_base_pass_bf; ml_coop.h),
with RNNWF_ENGINE and RNNWF_NO_COOP left unset so that they are the kernels that run (profiles/coop_core_bits.txt).  Widths 16, 20, 36,
37, 50, 52 and 68 units: every NFULL class with and without a remainder wave's worth of units.  Up to 52 units once on the default
pass - the bf16x3 pass where it exists (37 .. 52 units), else the f32 pass - and once with RNNWF_BASE=f32; 68 units have the f32 pass
alone.  Stacks of 2 and 3 layers at 20 and 50 units.  ns = 17 and 70 are 2 and 5 blocks of 16 chains: one workgroup each, in slot 0 of
the passes that keep NB blocks per workgroup (grid = min(blocks, resident workgroups); sb = round NB grid + b grid + k).  Those passes
fill a second slot only beyond that grid - one or two workgroups on each of 256 CUs - so they also run at ns = 8262, 517 blocks: slot 1
(two resident workgroups per CU) or slots 1 and 2 (one) hold blocks, and the last slot of some workgroups idles.
"""
import argparse
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, NS = 33, 17


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:32]


def prnn(_lib, P, model, dt, H, L, ns=NS, budget=None, parity=False, base=None):
    tag = "prnn %s%s H=%d L=%d ns=%d%s%s" % (dt, " parity" if parity else "", H, L, ns, " budget=%dMB" % budget if budget else "",
                                           " base=" + base if base else "")
    prm = P.randomize_biases(P.scale_kernels(P.init_gru_params([H] * L, seed=H + L, dtype=np.float64 if dt == "f64" else np.float32), 1.6), H)
    if budget:
        os.environ["RNNWF_STATE_BUDGET_MB"] = str(budget)
    if base:
        os.environ["RNNWF_BASE"] = base
    try:
        wf = _lib.NativeWavefunction(model, 11, 3, (H,) * L) if dt == "f64" else _lib.NativeWavefunction(model, N, 1, (H,) * L)
    finally:
        os.environ.pop("RNNWF_STATE_BUDGET_MB", None)
        os.environ.pop("RNNWF_BASE", None)
    wf.set_params(prm, scope="RNNwavefunction")
    s, lg = wf.sample(ns, seed=21, step=3, return_log=True)
    rng = np.random.RandomState(H + L)
    t = rng.randint(0, 2, (ns, N)).astype(np.int32)
    Jz = 1.0 + 0.1 * rng.standard_normal((11, 3) if dt == "f64" else N)
    q = np.zeros((N + 1) * ns)
    e = wf.tfim_eloc(t, Jz, 0.9, log_probs=q)
    outs = [("samples", s), ("sample_logp", lg), ("log_prob", wf.log_prob(t)), ("queue", q), ("eloc", e)]
    if not budget:      # a fused step is one pass: it refuses a batch beyond the budget
        out = wf.vmc_step(ns, seed=5, step=1, couplings=np.append(Jz.ravel(), 0.9), want_samples=True, want_eloc=True)
        outs += [("step_samples", out["samples"]), ("step_eloc", out["eloc"])]
    for name, a in outs:
        print("%-44s %-12s %s" % (tag, name, sha(a)))


def crnn(_lib, P, H, L, ns=NS, budget=None, base=None):
    n = N + 1          # the U(1) mask needs an even chain: 34 sites, two spin words
    tag = "crnn H=%d L=%d ns=%d%s%s" % (H, L, ns, " budget=%dMB" % budget if budget else "", " base=" + base if base else "")
    prm = P.randomize_biases(P.scale_kernels(P.init_gru_params([H] * L, seed=H + L, heads=("wf_dense_ampl", "wf_dense_phase")), 1.6), H)
    if budget:
        os.environ["RNNWF_STATE_BUDGET_MB"] = str(budget)
    if base:
        os.environ["RNNWF_BASE"] = base
    try:
        wf = _lib.NativeWavefunction(_lib.MODEL_CRNN_U1, n, 1, (H,) * L)
    finally:
        os.environ.pop("RNNWF_STATE_BUDGET_MB", None)
        os.environ.pop("RNNWF_BASE", None)
    wf.set_params(prm, scope="RNNwavefunction")
    s, lg = wf.sample(ns, seed=21, step=3, return_log=True)
    rng = np.random.RandomState(H + L)
    t = np.stack([rng.permutation(np.repeat([0, 1], n // 2)) for _ in range(ns)]).astype(np.int32)
    J1, J2, Bz = 1.0 + 0.1 * rng.standard_normal(n), 0.5 + 0.1 * rng.standard_normal(n), 0.1 * rng.standard_normal(n)
    e, ncon = wf.j1j2_eloc(t, J1, J2, Bz, periodic=True, marshall=False)
    outs = [("samples", s), ("sample_logp", lg), ("log_prob", wf.log_prob(t)), ("log_amp", wf.log_amp(t)), ("j1j2_eloc", e),
            ("j1j2_ncon", np.int64(ncon))]
    if not budget:
        out = wf.vmc_step(ns, seed=5, step=1, couplings=np.concatenate([J1, J2, Bz, [1.0, 0.0]]), want_samples=True, want_eloc=True)
        outs += [("step_samples", out["samples"]), ("step_eloc", out["eloc"])]
    for name, a in outs:
        print("%-44s %-12s %s" % (tag, name, sha(a)))


def coop(_lib, P):
    for model in (lambda *a, **k: prnn(_lib, P, _lib.MODEL_GRU1D, "f32", *a, **k), lambda *a, **k: crnn(_lib, P, *a, **k)):
        for H in (16, 20, 36, 37, 50, 52, 68):
            for base in (None, "f32") if H <= 52 else (None,):
                for ns in (17, 70) + ((8262,) if 37 <= H <= 52 and not base else ()):
                    model(H, 1, ns=ns, base=base)
        for L in (2, 3):
            for H in (20, 50):
                for ns in (17, 70, 8262):
                    model(H, L, ns=ns)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", help="shared library to load instead of the package's own")
    ap.add_argument("--coop", action="store_true", help="the list for the cooperative base passes")
    args = ap.parse_args()
    if not args.coop:
        os.environ["RNNWF_ENGINE"] = "f32"
        os.environ["RNNWF_NO_COOP"] = "1"
    from rnnwavefunctions_amd import _lib, params as P
    if args.lib:
        _lib.LIB_PATH = os.path.abspath(args.lib)
    if args.coop:
        return coop(_lib, P)
    for dt, model in (("f32", _lib.MODEL_GRU1D), ("f64", _lib.MODEL_GRU1D_F64)):
        for L in (1, 2, 3):
            for H in (20, 50, 68, 128):
                if H > 68 and (L > 1 or dt == "f64"):
                    continue            # 128 units (image through L2): one float32 layer
                prnn(_lib, P, model, dt, H, L)
    prnn(_lib, P, _lib.MODEL_GRU1D_PARITY, "f32", 20, 2, parity=True)
    for L in (1, 2, 3):
        for H in (20, 50, 128):
            if L > 1 and H > 100:
                continue                # stacks up to 100 units
            crnn(_lib, P, H, L)
    prnn(_lib, P, _lib.MODEL_GRU1D, "f32", 68, 3, ns=81, budget=1)      # 2 blocks of 16 chains per pass: 32 + 32 + 17
    crnn(_lib, P, 50, 2, ns=150, budget=1)                              # 4 blocks per pass: 64 + 64 + 22
    prnn(_lib, P, _lib.MODEL_GRU1D, "f32", 20, 2, ns=5)                 # one block: the shrinking launch starts fewer waves than WAVES
    crnn(_lib, P, 20, 2, ns=5)


if __name__ == "__main__":
    main()
