"""float64 yardstick of stochastic reconfiguration for the complex RNN (docs/sr_complex.md) - TEST INFRASTRUCTURE ONLY.

psi = sqrt(P) e^{i phi} with REAL parameters theta (flat order of rnnwf_set_params_flat: tensors by name, each in the caller's shape):

    O[s, k] = d log psi(sigma_s) / d theta_k = 1/2 d log P / d theta_k + i d phi / d theta_k,     eps_s = E_loc,s - mean E  (complex)
    S = Re(dO^H dO) / ns,   F = Re(dO^H eps) / ns,   delta = (S + lambda I)^-1 F

and, stacked into real arrays of 2 ns rows, each half centred with its own mean,

    Obar = [Re dO ; Im dO],  ebar = [Re eps ; Im eps]:   S = Obar^T Obar / ns,  F = Obar^T ebar / ns,
    delta = Obar^T (Obar Obar^T + ns lambda I)^-1 ebar.

The Jacobians of Re log psi and Im log psi come from torch.autograd over autograd_reference.crnn_log_amplitude (two batched reverse
passes: row s of the identity as grad_outputs); everything after them is float64 NumPy.  `dtype` is the cell arithmetic.
"""
import numpy as np
import torch

import autograd_reference as A
import sr_reference as R

HEADS = ("wf_dense_ampl", "wf_dense_phase")
names, flatten, unflatten = R.names, R.flatten, R.unflatten


def jacobian_dicts(params, samples, dtype=torch.float64, **kw):
    """({name: (ns,) + shape}, the same): d Re log psi(sigma_s) / d tensor and d Im log psi(sigma_s) / d tensor, float64.
    kw: passed on to crnn_log_amplitude (site_weight)."""
    leaves = A.to_torch(params, dtype, requires_grad=True)
    la = A.crnn_log_amplitude(leaves, samples, **kw)
    order = names(params)
    eye = torch.eye(la.shape[0], dtype=torch.float64)
    out = []
    for part in (la.real, la.imag):
        g = torch.autograd.grad(part, [leaves[k] for k in order], grad_outputs=eye, is_grads_batched=True, retain_graph=True,
                                allow_unused=True)
        out.append({k: (np.zeros((la.shape[0],) + tuple(leaves[k].shape)) if v is None else v.detach().to(torch.float64).numpy())
                    for k, v in zip(order, g)})
    return out[0], out[1]


def jacobian(params, samples, dtype=torch.float64, **kw):
    """(ns, nparams) complex128 in the flat order"""
    re, im = jacobian_dicts(params, samples, dtype, **kw)
    return flatten(re) + 1j * flatten(im)


def stacked(o):
    """Obar (2 ns, nparams) float64: [Re dO ; Im dO], each half centred with its own column mean"""
    return np.concatenate([R.centred(o.real), R.centred(o.imag)], axis=0)


def epsilon(eloc):
    """ebar (2 ns,) float64: [Re eps ; Im eps], each half centred"""
    e = np.asarray(eloc, dtype=np.complex128)
    return np.concatenate([e.real - e.real.mean(), e.imag - e.imag.mean()])


def gram(o):
    b = stacked(o)
    return b @ b.T


def qgt(o):
    b = stacked(o)
    return b.T @ b / o.shape[0]


def force(o, eloc):
    return stacked(o).T @ epsilon(eloc) / o.shape[0]


def minsr_direction(o, eloc, diag_shift):
    """Obar^T (Obar Obar^T + ns lambda I)^-1 ebar"""
    ns = o.shape[0]
    return stacked(o).T @ np.linalg.solve(gram(o) + ns * diag_shift * np.eye(2 * ns), epsilon(eloc))


def sr_direction(o, eloc, diag_shift):
    """(S + lambda I)^-1 F, the parameter-space form"""
    return np.linalg.solve(qgt(o) + diag_shift * np.eye(o.shape[1]), force(o, eloc))
