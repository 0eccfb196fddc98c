"""float64 yardstick of stochastic reconfiguration (docs/sr.md) - TEST INFRASTRUCTURE ONLY.

The per-sample log-derivatives O[s, k] = d log psi(sigma_s) / d theta_k = 1/2 d log P(sigma_s) / d theta_k of the positive GRU by
torch.autograd over autograd_reference.prnn_log_probability (one batched reverse pass: row s of the identity as grad_outputs), and
from them the centred Gram matrix, the force, the quantum geometric tensor and the minSR direction.  theta is in the flat order of
rnnwf_set_params_flat: tensors by name (byte-wise), each in the caller's shape.  `dtype` is the cell arithmetic, as in
autograd_reference; everything after the Jacobian is float64 NumPy.
"""
import numpy as np
import torch

import autograd_reference as A


def names(params):
    """the tensors in the flat order of rnnwf_set_params_flat"""
    return sorted(params)


def jacobian_dict(params, samples, dtype=torch.float64):
    """{name: (ns,) + shape float64}: d log psi(sigma_s) / d tensor"""
    leaves = A.to_torch(params, dtype, requires_grad=True)
    lp = A.prnn_log_probability(leaves, samples)
    order = names(params)
    eye = torch.eye(lp.shape[0], dtype=lp.dtype)
    g = torch.autograd.grad(lp, [leaves[k] for k in order], grad_outputs=eye, is_grads_batched=True)
    return {k: 0.5 * v.detach().to(torch.float64).numpy() for k, v in zip(order, g)}


def flatten(jd):
    """{name: (ns,) + shape} -> (ns, nparams) in the flat order"""
    return np.concatenate([jd[k].reshape(jd[k].shape[0], -1) for k in names(jd)], axis=1)


def unflatten(o, like):
    """(ns, nparams) or (nparams,) in the flat order -> {name: leading axes + shape of like[name]}"""
    out, off = {}, 0
    o = np.asarray(o)
    for k in names(like):
        n = int(np.size(like[k]))
        out[k] = o[..., off:off + n].reshape(o.shape[:-1] + np.shape(like[k]))
        off += n
    assert off == o.shape[-1], (off, o.shape)
    return out


def jacobian(params, samples, dtype=torch.float64):
    return flatten(jacobian_dict(params, samples, dtype))


def centred(o):
    return o - o.mean(axis=0)


def epsilon(eloc):
    e = np.asarray(eloc, dtype=np.float64)
    return e - e.mean()


def gram(o):
    d = centred(o)
    return d @ d.T


def qgt(o):
    d = centred(o)
    return d.T @ d / o.shape[0]


def force(o, eloc):
    return centred(o).T @ epsilon(eloc) / o.shape[0]


def minsr_direction(o, eloc, diag_shift):
    """dO^T (dO dO^T + ns lambda I)^-1 eps"""
    ns = o.shape[0]
    return centred(o).T @ np.linalg.solve(gram(o) + ns * diag_shift * np.eye(ns), epsilon(eloc))


def sr_direction(o, eloc, diag_shift):
    """(S + lambda I)^-1 F, the parameter-space form"""
    return np.linalg.solve(qgt(o) + diag_shift * np.eye(o.shape[1]), force(o, eloc))
