"""float64 yardstick of stochastic reconfiguration for the LSTM wave function (docs/sr_lstm.md) - TEST INFRASTRUCTURE ONLY.

The per-sample log-derivatives O[s, k] = 1/2 d log P(sigma_s) / d theta_k of the LSTM wave function on the raster path by
torch.autograd over lstm_grad_reference.lstm_log_probability, as one batched reverse pass (row s of the identity as grad_outputs) like
tests/sr_reference.py.  psi = sqrt(P) is real and positive, so everything after the Jacobian is sr_reference's: flatten, centred, gram,
epsilon, qgt, force, minsr_direction (re-exported here).  theta is in the flat order of rnnwf_set_params_flat (wf._layout()); `dtype`
is the cell arithmetic.  Keyword arguments reach lstm_log_probability: its switches that make it deliberately wrong, and site_weight,
which tests/test_lstm_sr_reference.py uses to take the sites one at a time.
"""
import torch

import autograd_reference as A
import lstm_grad_reference as G
from sr_reference import (centred, epsilon, flatten, force, gram, minsr_direction, names, qgt, sr_direction,  # noqa: F401
                          unflatten)


def jacobian_dict(params, samples, dtype=torch.float64, **kw):
    """{name: (ns,) + shape float64}: d log psi(sigma_s) / d tensor; samples (ns, Nx, Ny) or (ns, N)"""
    leaves = A.to_torch(params, dtype, requires_grad=True)
    lp = G.lstm_log_probability(leaves, samples, **kw)
    order = names(params)
    eye = torch.eye(lp.shape[0], dtype=lp.dtype)
    g = torch.autograd.grad(lp, [leaves[k] for k in order], grad_outputs=eye, is_grads_batched=True)
    return {k: 0.5 * v.detach().to(torch.float64).numpy() for k, v in zip(order, g)}


def jacobian(params, samples, dtype=torch.float64, **kw):
    return flatten(jacobian_dict(params, samples, dtype, **kw))
