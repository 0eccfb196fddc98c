"""torch-CPU restatement of the FORWARD of every wave function that has a gradient, so that one reverse-mode pass gives every
element of the gradient of the VMC cost exactly - the yardstick of tests/test_gpu_gradient_full.py.  TEST INFRASTRUCTURE ONLY.

Written from oracle/models.py (which cites the reference lines), not from the HIP code:

    prnn_log_probability            <- models.prnn_log_probability            positive GRU, one layer or a stack, any widths
    prnn_paritysym_log_probability  <- models.prnn_paritysym_log_probability  log(0.5 (P(s) + P(reversed s)))
    crnn_log_amplitude              <- models.crnn_log_amplitude              complex U(1) GRU: masked amplitude, phase head
    mdrnn_log_probability           <- models.mdrnn_log_probability           2D MDRNN on the zig-zag path
    (the float64 GRU on the 2D raster is prnn_log_probability on the (ns, Nx * Ny) samples with float64 parameters)

`dtype` is the cell arithmetic (torch.float64 or torch.float32); the selected probabilities are cast to float64 before the log and
the sum over sites, as the oracle does (1DTFIM/RNNwavefunction.py:113-116).  Parameters are {scoped tf name: tensor} of that dtype.

The costs are the reference's: cost_real (TrainingRNN_1DTFIM.py:156) and cost_complex (TrainingRNN_J1J2.py:197), the local energies
being constants.  gradient() returns {scoped tf name: float64 ndarray} in the caller's shapes from one backward().

The comparator (compare / verdict) scores a gradient against a reference PER TENSOR and over EVERY element:
max |g - g_ref| / max |g_ref|  and  ||g - g_ref||_2 / ||g_ref||_2, both normalised by that tensor alone.

torch's thread count is left to the environment (OMP_NUM_THREADS); nothing here sizes a pool.
"""
import numpy as np
import torch

from oracle import models as M

SCOPE = "RNNwavefunction"
GRU = M.GRU
FACTOR = 16.0                      # a gradient must stay within FACTOR x the yardstick (see verdict)
F64_OVER_F32 = 2.0 ** -29          # ratio of the unit round-offs 2^-53 / 2^-24


# ---- parameters ---------------------------------------------------------------------------------------------------------

def to_torch(params, dtype=torch.float64, requires_grad=False):
    """{name: ndarray} -> {name: leaf tensor of the cell dtype}."""
    return {k: torch.tensor(np.asarray(v), dtype=dtype, requires_grad=requires_grad) for k, v in params.items()}


def _p(params, scope, name):
    return params[scope + "/" + name]


def _num_layers(params, scope):
    n = 0
    while (scope + "/" + GRU % n + "gates/kernel") in params:
        n += 1
    return n


def _one_hot(col, dtype):
    return torch.eye(2, dtype=dtype)[col]


# ---- the cuDNN-compatible GRU stack (models.gru_cell / multi_gru) ---------------------------------------------------------

def gru_cell(x, h, params, scope, layer):
    pre = GRU % layer
    Wg, bg = _p(params, scope, pre + "gates/kernel"), _p(params, scope, pre + "gates/bias")
    Wci, bci = _p(params, scope, pre + "candidate/input_projection/kernel"), _p(params, scope, pre + "candidate/input_projection/bias")
    Wch, bch = _p(params, scope, pre + "candidate/hidden_projection/kernel"), _p(params, scope, pre + "candidate/hidden_projection/bias")
    nh = h.shape[1]
    g = torch.sigmoid(torch.cat([x, h], dim=1) @ Wg + bg)
    r, u = g[:, :nh], g[:, nh:]
    c = torch.tanh((x @ Wci + bci) + r * (h @ Wch + bch))
    return (1 - u) * c + u * h


def multi_gru(x, states, params, scope):
    new_states = []
    for layer, h in enumerate(states):
        x = gru_cell(x, h, params, scope, layer)
        new_states.append(x)
    return x, new_states


def _zero_states(params, scope, batch, dtype):
    return [torch.zeros((batch, _p(params, scope, GRU % layer + "candidate/hidden_projection/kernel").shape[0]), dtype=dtype)
            for layer in range(_num_layers(params, scope))]


def _as_index(samples):
    return torch.as_tensor(np.ascontiguousarray(samples), dtype=torch.int64)


def _cell_dtype(params):
    return next(iter(params.values())).dtype


# ---- positive RNN (models.prnn_site_probs / prnn_log_probability) ----------------------------------------------------------

def prnn_log_probability(params, samples, scope=SCOPE, inputs=None, site_weight=None, stack=None):
    """float64 (B,).  `inputs` (default: the samples) are the spins whose one-hots are fed to the next site, `site_weight` (default:
    all ones) multiplies each site's term and `stack` (default: multi_gru) is the cell: tests of the comparator pass deliberately
    wrong ones; nothing else uses them."""
    dtype = _cell_dtype(params)
    s = _as_index(samples).reshape(len(samples), -1)
    fed = s if inputs is None else _as_index(inputs).reshape(len(samples), -1)
    B, N = s.shape
    Wd, bd = _p(params, scope, "wf_dense/kernel"), _p(params, scope, "wf_dense/bias")
    x = torch.zeros((B, 2), dtype=dtype)
    states = _zero_states(params, scope, B, dtype)
    lp = torch.zeros(B, dtype=torch.float64)
    for n in range(N):
        out, states = (stack or multi_gru)(x, states, params, scope)
        probs = torch.softmax(out @ Wd + bd, dim=1).to(torch.float64)
        term = torch.log(probs.gather(1, s[:, n:n + 1])[:, 0])
        lp = lp + (term if site_weight is None else site_weight[n] * term)
        x = _one_hot(fed[:, n], dtype)
    return lp


def prnn_paritysym_log_probability(params, samples, scope=SCOPE, inputs=None, **kw):
    s = np.asarray(samples)
    lp1 = prnn_log_probability(params, s, scope, inputs=inputs, **kw)
    lp2 = prnn_log_probability(params, s[:, ::-1], scope, inputs=None if inputs is None else np.asarray(inputs)[:, ::-1], **kw)
    return torch.log(0.5 * (torch.exp(lp1) + torch.exp(lp2)))


# ---- complex RNN with the U(1) mask (models.crnn_log_amplitude) -------------------------------------------------------------

def _heavyside(x):
    return 0.5 * (torch.sign(torch.sign(x) + 0.1) + 1.0)


def crnn_log_amplitude(params, samples, scope=SCOPE, inputs=None, site_weight=None, stack=None):
    """complex128 (B,): sum over the sites of log(ampl) + i phase of the selected spin.  (The oracle takes the complex log of
    ampl exp(i phase); phase = pi softsign(z) lies inside (-pi, pi), so the principal value is log(ampl) + i phase.)
    inputs, site_weight, stack: as in prnn_log_probability (the U(1) mask always counts the samples themselves)."""
    dtype = _cell_dtype(params)
    s = _as_index(samples)
    fed = s if inputs is None else _as_index(inputs)
    B, N = s.shape
    Wa, ba = _p(params, scope, "wf_dense_ampl/kernel"), _p(params, scope, "wf_dense_ampl/bias")
    Wp, bp = _p(params, scope, "wf_dense_phase/kernel"), _p(params, scope, "wf_dense_phase/bias")
    x = torch.zeros((B, 2), dtype=dtype)
    states = _zero_states(params, scope, B, dtype)
    log_abs = torch.zeros(B, dtype=torch.float64)
    arg = torch.zeros(B, dtype=torch.float64)
    for n in range(N):
        out, states = (stack or multi_gru)(x, states, params, scope)
        ampl = torch.sqrt(torch.softmax(out @ Wa + ba, dim=1))
        if n >= N / 2:
            num_up = s[:, :n].sum(dim=1).to(dtype)
            baseline = float(N // 2 - 1)
            act_up = _heavyside(baseline - num_up)
            act_down = _heavyside(baseline - (float(n) - num_up))
            ampl = ampl * torch.stack([act_down, act_up], dim=1)
            ss = torch.clamp((ampl * ampl).sum(dim=1, keepdim=True), min=1e-30)
            ampl = ampl / torch.sqrt(ss)
        z = out @ Wp + bp
        phase = np.pi * (z / (1 + torch.abs(z)))
        col = s[:, n:n + 1]
        w = 1.0 if site_weight is None else site_weight[n]
        log_abs = log_abs + w * torch.log(ampl.to(torch.float64).gather(1, col)[:, 0])
        arg = arg + w * phase.to(torch.float64).gather(1, col)[:, 0]
        x = _one_hot(fed[:, n], dtype)
    return torch.complex(log_abs, arg)


# ---- 2D MDRNN on the zig-zag path (models.mdrnn_cell / _mdrnn_run) -----------------------------------------------------------

def _mdrnn_pre(xh, hh, xv, hv, Uh, Wh, Uv, Wv, b):
    return xh @ Uh + hh @ Wh + xv @ Uv + hv @ Wv + b


def mdrnn_log_probability(params, samples, scope=SCOPE, name="rnn_0", inputs=None, site_weight=None, pre_activation=None):
    """inputs, site_weight: as in prnn_log_probability (site_weight indexed by the position on the zig-zag path); pre_activation
    (default: _mdrnn_pre) is the cell's affine part, for a test that passes a deliberately wrong one."""
    dtype = _cell_dtype(params)
    s = _as_index(samples)
    fed = s if inputs is None else _as_index(inputs)
    B, Nx, Ny = s.shape
    Uh, Wh = _p(params, scope, "Uh_" + name), _p(params, scope, "Wh_" + name)
    Uv, Wv = _p(params, scope, "Uv_" + name), _p(params, scope, "Wv_" + name)
    b = _p(params, scope, "b_" + name)
    Wd, bd = _p(params, scope, "wf_dense/kernel"), _p(params, scope, "wf_dense/bias")
    zeros_h = torch.zeros((B, Wh.shape[0]), dtype=dtype)
    zeros_x = torch.zeros((B, 2), dtype=dtype)
    h, x = {}, {}
    lp = torch.zeros(B, dtype=torch.float64)
    for pos, (nx, ny, nxh) in enumerate(M.zigzag_order(Nx, Ny)):
        hh, xh = h.get((nxh, ny), zeros_h), x.get((nxh, ny), zeros_x)
        hv, xv = h.get((nx, ny - 1), zeros_h), x.get((nx, ny - 1), zeros_x)
        pre = (pre_activation or _mdrnn_pre)(xh, hh, xv, hv, Uh, Wh, Uv, Wv, b)
        hn = torch.where(pre > 0, pre, torch.expm1(torch.clamp(pre, max=0.0)))
        probs = torch.softmax(hn @ Wd + bd, dim=1).to(torch.float64)
        term = torch.log(probs.gather(1, s[:, nx, ny].reshape(B, 1))[:, 0])
        lp = lp + (term if site_weight is None else site_weight[pos] * term)
        h[(nx, ny)] = hn
        x[(nx, ny)] = _one_hot(fed[:, nx, ny], dtype)
    return lp


FORWARD = {"gru": prnn_log_probability, "parity": prnn_paritysym_log_probability, "crnn": crnn_log_amplitude,
           "mdrnn": mdrnn_log_probability}


# ---- the two costs ----------------------------------------------------------------------------------------------------------

def cost_real(log_probs, eloc):
    """TrainingRNN_1DTFIM.py:156 (tests/test_gpu_training.py: oracle_cost)."""
    e = torch.as_tensor(np.asarray(eloc, dtype=np.float64))
    return torch.mean(log_probs * e) - torch.mean(e) * torch.mean(log_probs)


def cost_complex(log_amps, eloc):
    """TrainingRNN_J1J2.py:197 (tests/test_gpu_training.py: oracle_cost_complex)."""
    e = torch.as_tensor(np.asarray(eloc, dtype=np.complex128))
    return 2 * torch.real(torch.mean(torch.conj(log_amps) * e) - torch.conj(torch.mean(log_amps)) * torch.mean(e))


def cost(family, params, samples, eloc, scope=SCOPE, **kw):
    log_psi = FORWARD[family](params, samples, scope, **kw)
    return cost_complex(log_psi, eloc) if family == "crnn" else cost_real(log_psi, eloc)


def gradient(family, params, samples, eloc, dtype=torch.float64, scope=SCOPE, **kw):
    """{scoped tf name: float64 ndarray, the caller's shape}: d cost / d parameter, every element, from one backward()."""
    leaves = to_torch(params, dtype, requires_grad=True)
    cost(family, leaves, samples, eloc, scope, **kw).backward()
    return {k: v.grad.detach().to(torch.float64).numpy().reshape(np.shape(params[k])) for k, v in leaves.items()}


# ---- the comparator ---------------------------------------------------------------------------------------------------------

def compare(g, g_ref):
    """{name: dict(max_rel, l2_rel, max_abs, ref_max)} - per tensor, over every element, normalised by that tensor of the
    reference alone.  The relative figures are inf where the reference tensor is exactly zero and g is not."""
    assert set(g) == set(g_ref), sorted(set(g) ^ set(g_ref))
    out = {}
    for k, ref in g_ref.items():
        a = np.asarray(g[k], dtype=np.float64)
        ref = np.asarray(ref, dtype=np.float64)
        assert a.shape == ref.shape, (k, a.shape, ref.shape)
        d = a - ref
        max_abs, ref_max = float(np.abs(d).max()), float(np.abs(ref).max())
        l2, ref_l2 = float(np.sqrt((d * d).sum())), float(np.sqrt((ref * ref).sum()))
        with np.errstate(divide="ignore", invalid="ignore"):
            out[k] = dict(max_rel=float(np.float64(max_abs) / ref_max) if max_abs else 0.0,
                          l2_rel=float(np.float64(l2) / ref_l2) if l2 else 0.0, max_abs=max_abs, ref_max=ref_max)
    return out


def verdict(g, g64, g32, unit_roundoff_ratio=1.0, factor=FACTOR, label="", echo=print, floor=None):
    """Score g against the float64 reference g64 with the deviation of the float32 restatement g32 as the yardstick:
    every tensor must stay within  factor x unit_roundoff_ratio x (g32's deviation from g64)  in BOTH norms.  A tensor whose
    reference is zero to rounding (max |g64| <= max |g32 - g64|) is compared absolutely: max |g - g64| <= that bound x
    max |g32 - g64|.  unit_roundoff_ratio = F64_OVER_F32 for a float64 kernel (first-order rounding error of one algorithm is
    linear in the unit round-off).  `floor` (default none: the yardstick alone) is {tensor: a deviation relative to that tensor's
    reference maximum that no evaluation in the kernel's type can be expected to beat}: the tensor's yardstick is then the LARGER of
    the float32-autograd one and the floor, in both norms (absolute, floor x max |g64|, on the zero-reference branch), and the printed
    line says which of the two applied.  Prints deviation, yardstick and ratio of every tensor; returns (worst ratio, [failures])."""
    dev, yard = compare(g, g64), compare(g32, g64)
    worst, failures = 0.0, []
    for k in sorted(dev):
        d, y = dev[k], yard[k]
        fl = None if floor is None else float(floor[k])
        if y["ref_max"] <= y["max_abs"]:
            bound, note = unit_roundoff_ratio * y["max_abs"], ""
            if fl is not None:
                note = "  [floor]" if fl * y["ref_max"] > bound else "  [autograd]"
                bound = max(bound, fl * y["ref_max"])
            ratios = [d["max_abs"] / bound if bound > 0 else (0.0 if d["max_abs"] == 0 else np.inf)]
            echo("%s %-90s ZERO REFERENCE  |d| %.3e  yardstick %.3e  ratio %.3f%s" % (label, k, d["max_abs"], bound, ratios[0], note))
        else:
            ratios, bounds, note = [], [], ""
            for norm in ("max_rel", "l2_rel"):
                bound = unit_roundoff_ratio * y[norm]
                if fl is not None:
                    note += " [%s]" % ("floor" if fl > bound else "autograd")
                    bound = max(bound, fl)
                bounds.append(bound)
                ratios.append(d[norm] / bound if bound > 0 else (0.0 if d[norm] == 0 else np.inf))
            echo("%s %-90s max %.3e / %.3e = %6.3f   l2 %.3e / %.3e = %6.3f%s" %
                 (label, k, d["max_rel"], bounds[0], ratios[0], d["l2_rel"], bounds[1], ratios[1], note and " " + note))
        r = max(ratios)
        worst = max(worst, r)
        if not r <= factor:
            failures.append((k, r))
    return worst, failures


# ---- central differences of the NumPy oracle's cost (the tiny-shape check of tests/test_gpu_training.py) ---------------------

def fd_check(grads, prm64, cost_fn, n_per_tensor=10, eps=1e-6, per_tensor=False):
    """max over n_per_tensor random elements of every tensor of |central difference - grads| / max |grads|, the maximum taken
    over all tensors (the figure of test_gpu_training.py's finite-difference tests) or, per_tensor=True, over that tensor."""
    rng = np.random.RandomState(0)
    worst = 0.0
    scale = max(np.abs(g).max() for g in grads.values())
    for name, g in grads.items():
        assert g.shape == prm64[name].shape
        flat = prm64[name].ravel()
        if per_tensor:
            scale = np.abs(g).max() or 1.0            # an all-zero tensor (N = 1: nothing reaches the hidden kernels): absolute
        for idx in rng.choice(flat.size, size=min(flat.size, n_per_tensor), replace=False):
            old = flat[idx]
            flat[idx] = old + eps
            cp = cost_fn()
            flat[idx] = old - eps
            cm = cost_fn()
            flat[idx] = old
            worst = max(worst, abs((cp - cm) / (2 * eps) - g.ravel()[idx]) / scale)
    return worst
