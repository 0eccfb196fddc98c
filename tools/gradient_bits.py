#!/usr/bin/env python3
"""One sha256 per output of the gradient's kernels and host paths, for a fixed list of small configurations.

    tools/gradient_bits.py [--lib PATH/librnnwf_hip.so]

Run it on two builds on the same machine and compare the listings line for line: a refactor of gru_bwd_kernel /
gru_upper_bwd_kernel / mdrnn_bwd_kernel, of their launch path or of the packers and unpackers of grad.hip / mdrnn.hip / sr.hip that
keeps arithmetic and order keeps every line (profiles/gradient_core_bits.txt).
Outputs: every named gradient array of rnnwf_get_grad and the flat vector of rnnwf_get_grads_flat on the batch a vmc_step drew;
the flat parameters after three rnnwf_train_steps iterations; per-sample log-derivatives and the minSR direction.
33 sites (34 for the complex RNN's even chain, 11 x 3 for the float64 GRU, 4 x 3 for the 2D RNN): two spin words; 17 samples: a
ragged second block of 16 chains.
"""
import argparse
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, NS = 33, 17
SCOPE = "RNNwavefunction"


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:32]


def make(_lib, P, family, H, L):
    """(handle, parameters, couplings) of one model at L layers of H units"""
    rng = np.random.RandomState(H + L)
    if family == "mdrnn":
        prm = P.scale_kernels(P.init_mdrnn_params(H, seed=H), 1.6)
        wf = _lib.NativeWavefunction(_lib.MODEL_MDRNN2D, 4, 3, (H,))
        coup = np.append(1.0 + 0.1 * rng.standard_normal(12), 0.9)
    elif family == "crnn":
        prm = P.randomize_biases(P.scale_kernels(P.init_gru_params([H] * L, seed=H + L, heads=("wf_dense_ampl", "wf_dense_phase")), 1.6), H)
        wf = _lib.NativeWavefunction(_lib.MODEL_CRNN_U1, N + 1, 1, (H,) * L)
        coup = np.concatenate([1.0 + 0.1 * rng.standard_normal(N + 1), 0.5 + 0.1 * rng.standard_normal(N + 1),
                               0.1 * rng.standard_normal(N + 1), [1.0, 0.0]])
    else:
        f64 = family == "f64"
        prm = P.randomize_biases(P.scale_kernels(P.init_gru_params([H] * L, seed=H + L, dtype=np.float64 if f64 else np.float32), 1.6), H)
        model = {"f32": _lib.MODEL_GRU1D, "parity": _lib.MODEL_GRU1D_PARITY, "f64": _lib.MODEL_GRU1D_F64}[family]
        wf = _lib.NativeWavefunction(model, 11, 3, (H,) * L) if f64 else _lib.NativeWavefunction(model, N, 1, (H,) * L)
        coup = np.append(1.0 + 0.1 * rng.standard_normal(N), 0.9)
    wf.set_params(prm, scope=SCOPE)
    return wf, prm, coup


def gradient(_lib, P, family, H, L, ns=NS, no_coop=False):
    tag = "%s H=%d L=%d ns=%d%s" % (family, H, L, ns, " RNNWF_NO_COOP=1" if no_coop else "")
    if no_coop:
        os.environ["RNNWF_NO_COOP"] = "1"                # read once per handle, at creation
    try:
        wf, prm, coup = make(_lib, P, family, H, L)
    finally:
        os.environ.pop("RNNWF_NO_COOP", None)
    m = wf.vmc_step(ns, seed=5, step=1, couplings=coup)["moments"]
    mean = complex(m[0] / m[2], m[3] / m[2]) if family == "crnn" else m[0] / m[2]
    shapes = {k[len(SCOPE) + 1:]: v.shape for k, v in prm.items()}
    flat = wf.vmc_gradient(mean, m[2], shapes)                                   # all tensors: rnnwf_get_grads_flat
    named = wf.vmc_gradient(mean, m[2], {k: shapes[k] for k in list(shapes)[:-1]})    # a subset: rnnwf_get_grad per tensor
    wf.close()
    for k in named:
        print("%-40s %-72s %s" % (tag, k, sha(named[k])))
    print("%-40s %-72s %s" % (tag, "flat", sha(np.concatenate([flat[k].ravel() for k in shapes]))))


def trained(_lib, P, family, H, L):
    wf, prm, coup = make(_lib, P, family, H, L)
    if not wf.device_training_supported():
        raise SystemExit("device-resident training refused %s H=%d L=%d" % (family, H, L))
    wf.train_steps(NS, 7, 0, coup, [1e-2, 5e-3, 2e-3])
    out = wf.get_params_dict(prm, SCOPE)
    wf.close()
    print("%-40s %-72s %s" % ("%s H=%d L=%d train_steps x3" % (family, H, L), "flat parameters",
                                  sha(np.concatenate([np.asarray(v, dtype=np.float64).ravel() for v in out.values()]))))


def minsr(_lib, P, family, H):
    from rnnwavefunctions_amd import sr
    wf, prm, coup = make(_lib, P, family, H, 1)
    wf.vmc_step(NS, seed=5, step=1, couplings=coup)
    tag = "%s H=%d L=1 ns=%d minSR" % (family, H, NS)
    print("%-40s %-72s %s" % (tag, "log_derivatives", sha(wf.log_derivatives())))
    print("%-40s %-72s %s" % (tag, "direction (device solve)", sha(sr.minsr_direction(wf, 1e-3, solver="device"))))
    wf.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", help="shared library to load instead of the package's own")
    args = ap.parse_args()
    from rnnwavefunctions_amd import _lib, params as P
    if args.lib:
        _lib.LIB_PATH = os.path.abspath(args.lib)
    for family in ("f32", "parity", "crnn", "f64"):       # LDS-resident images; top, middle and bottom pass of a stack
        for L in (1, 2, 3):
            for H in (20, 50):
                gradient(_lib, P, family, H, L)
    for H in (10, 50):
        gradient(_lib, P, "mdrnn", H, 1)
    gradient(_lib, P, "f32", 100, 1)                      # backward operand through L2 (GradStream)
    gradient(_lib, P, "f64", 68, 1)
    gradient(_lib, P, "f32", 128, 1)                      # the wide kernels' translation unit
    gradient(_lib, P, "crnn", 128, 1)
    gradient(_lib, P, "f64", 100, 1)
    gradient(_lib, P, "f32", 68, 2)                       # upper layers with their images through L2
    gradient(_lib, P, "crnn", 68, 2)
    gradient(_lib, P, "crnn", 32, 2)                      # complex stack at 21..36 units
    gradient(_lib, P, "f32", 50, 1, no_coop=True)         # four-wave kernel where the small batch selects the pair kernel
    gradient(_lib, P, "crnn", 50, 1, no_coop=True)
    gradient(_lib, P, "f32", 20, 2, ns=5)                 # fewer blocks than waves
    gradient(_lib, P, "crnn", 20, 2, ns=5)
    # more 16-chain blocks than any grid of four-wave workgroups holds (at most 32 waves per CU): every wave walks a second block
    wf = _lib.NativeWavefunction(_lib.MODEL_GRU1D, N, 1, (20,))
    cus = wf.device_info()["cu_count"]
    wf.close()
    gradient(_lib, P, "f32", 20, 1, ns=16 * 32 * cus + 17)
    trained(_lib, P, "f32", 20, 1)                        # device moments (mom != nullptr) and the Lin packers
    trained(_lib, P, "f32", 20, 2)
    minsr(_lib, P, "f32", 20)                             # the kernel's per-sample head rows
    minsr(_lib, P, "f64", 20)


if __name__ == "__main__":
    main()
