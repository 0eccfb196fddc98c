"""float64 yardstick of stochastic reconfiguration for the 2D RNN (docs/sr_2d.md) - TEST INFRASTRUCTURE ONLY.

The per-sample log-derivatives O[s, k] = 1/2 d log P(sigma_s) / d theta_k of the 2D RNN on the zig-zag path by torch.autograd over
autograd_reference.mdrnn_log_probability, as one batched reverse pass (row s of the identity as grad_outputs) like
tests/sr_reference.py.  psi = sqrt(P) is real and positive, so everything after the Jacobian is sr_reference's: flatten, gram, qgt,
force, minsr_direction (re-exported here).  theta is in the flat order of rnnwf_set_params_flat; `dtype` is the cell arithmetic.
"""
import torch

import autograd_reference as A
from sr_reference import (centred, epsilon, flatten, force, gram, minsr_direction, names, qgt, sr_direction,  # noqa: F401
                          unflatten)


def jacobian_dict(params, samples, dtype=torch.float64, **kw):
    """{name: (ns,) + shape float64}: d log psi(sigma_s) / d tensor; samples (ns, Nx, Ny)"""
    leaves = A.to_torch(params, dtype, requires_grad=True)
    lp = A.mdrnn_log_probability(leaves, samples, **kw)
    order = names(params)
    eye = torch.eye(lp.shape[0], dtype=lp.dtype)
    g = torch.autograd.grad(lp, [leaves[k] for k in order], grad_outputs=eye, is_grads_batched=True)
    return {k: 0.5 * v.detach().to(torch.float64).numpy() for k, v in zip(order, g)}


def jacobian(params, samples, dtype=torch.float64, **kw):
    return flatten(jacobian_dict(params, samples, dtype, **kw))
