"""What licenses the bound of tests/test_gpu_gradient_classes.py, shown on the reference alone - no GPU.

The table (tests/gradient_classes_reference.py) covers every class the dispatch code admits, and for EVERY case of it, on a batch the
NumPy oracle draws, the bound (16 x the larger of the float32-autograd yardstick and the rounding floor, x 2^-29 on the yardstick
for the float64 families) ACCEPTS
  * a second float32 evaluation with the batch permuted and summed in four parts (float32 families; for the float64 families that
    evaluation is the yardstick's own kind of error, 2^29 x the bound, and is not a candidate), and
  * the float64 gradient rounded once to the model's type.
At one case per family and layer count (REJECT_CASES) it REJECTS each of these gradients, built from the reference:
  chain dropped        the last chain of the ragged block missing, every other weight (E_s - <E>) / ns unchanged
  last site dropped    the last site's term of log psi missing (parity: of either direction)
  input shifted        the one-hot fed into site 32 is the one fed into site 31 (path positions on the 2D RNN); VOID_SHIFT names
                       the three cases whose batches it does not change
  unit dropped         the last unit (the mixed tile's remainder) missing from the reset gate's recurrent product in layer 0
                       (2D RNN: from the horizontal recurrent product)
  tensor x 1.001       every tensor in turn; that tensor and no other is reported (LOOSE_TENSORS names those that are not)
  unit row x 1.001     in every tensor in turn, the slice of the unit that holds the tensor's largest entry (the same)
  wrong layer below    stacks: the top layer is fed the state of the layer two below (two layers: layer 0's state of the
                       previous site)
  phase negated        complex model: the weight of Im log psi in the cost negated
  shares swapped       parity: each direction's backward pass weighted with the other direction's share of P_sym
"""
import functools

import numpy as np
import pytest
import torch

import autograd_reference as A
import gradient_classes_reference as G
from test_autograd_reference import batch

MUTE = dict(echo=lambda *a: None)


@functools.lru_cache(maxsize=2)
def prepared(i):
    c = G.CASES[i]
    prm = G.parameters(c)
    s, e = batch(c.family, prm, c.shape, c.ns)
    return c, prm, s, e, G.reference(c, prm, s, e)


# ---- the table against the code's own class list -----------------------------------------------------------------------------------

def test_table_covers_every_class_the_dispatch_admits():
    covered = {G.gradient_class(c) for c in G.CASES}
    assert covered == G.admitted_classes()
    assert len([k for k in covered if k[0] == "gru"]) == 23 and len([k for k in covered if k[0] == "crnn"]) == 23
    assert len([k for k in covered if k[0] == "gru64"]) == 17 and len([k for k in covered if k[0] == "mdrnn"]) == 5
    # both ends of every one-layer class, and of every NFULL / every layer count among the stacks
    for family in ("gru", "crnn", "gru64", "mdrnn"):
        for nf in sorted({k[2] for k in covered if k[0] == family and k[1] == 1}):
            widths = {c.units[0] for c in G.CASES if c.family == family and len(c.units) == 1}
            assert (20 if nf == 1 else G.CLASS_WIDTHS[nf][0]) in widths and G.CLASS_WIDTHS[nf][1] in widths and 6 in widths
    for family in ("gru", "crnn", "gru64"):
        stacks = [c for c in G.CASES if c.family == family and len(c.units) > 1 and len(set(c.units)) == 1]
        for key in ("layers", "nfull"):
            groups = {}
            for c in stacks:
                nf = G.nfull(family, c.units)
                groups.setdefault(len(c.units) if key == "layers" else nf, set()).add(G.CLASS_WIDTHS[nf].index(c.units[0]))
            assert all(v == {0, 1} for v in groups.values()), (family, key, groups)
    unequal = [c for c in G.CASES if len(set(c.units)) > 1]
    assert len(unequal) >= 3 and any(c.units[-1] == max(c.units) and c.units[-1] > c.units[0] for c in unequal)
    parity = [c for c in G.CASES if c.family == "parity"]
    assert {G.nfull("parity", c.units) for c in parity if len(c.units) == 1} == {1, 2, 3, 4, 6, 8, 12, 16}
    assert len([c for c in parity if len(c.units) > 1]) == 2
    lengths = [c for c in G.CASES if c.ns == G.NS_LENGTHS]
    assert [c.shape[0] for c in lengths] == [1, 2, 4, 33, 65] and len({c.ns for c in lengths}) == 1
    assert [(c.shape[0] * c.ns) % 4 == 0 for c in lengths] == [False, False, True, False, False]
    assert len(set(G.IDS)) == len(G.IDS)


def test_pair_kernel_classes():
    """GradPair::FITS from the layouts' byte counts: NFULL 1, 2, 3 of the f32 families (at NFULL 4 the two hand-over slots no longer
    fit next to the images), never float64, never the wide kernels."""
    for family in ("gru", "parity", "crnn"):
        assert [nf for nf in (1, 2, 3, 4, 6, 8, 12, 16) if G.pair_fits(family, nf)] == [1, 2, 3]
    assert not any(G.pair_fits(f, nf) for f in G.F64_FAMILIES for nf in (1, 2, 3, 4, 5, 6))
    assert len(G.PAIR_CASES) == 3 * 4 * 2 + 3 * 1 + 2        # gru, crnn: 3 widths x 4 layer counts; parity: one layer, and its two stacks
    assert all(refusal for _, _, refusal in G.REFUSED)


# ---- accepted: every case -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("i", range(len(G.CASES)), ids=G.IDS)
def test_bound_accepts_what_it_must(i):
    c, prm, s, e, ref = prepared(i)
    label = "[%s]" % G.case_id(c)
    for k in prm:
        assert np.all(np.isfinite(ref.g64[k])) and np.all(np.isfinite(ref.g32[k])), k
    # the float64 gradient rounded once to the model's type
    rounded = {k: v.astype(prm[k].dtype).astype(np.float64) for k, v in ref.g64.items()}
    worst_r, failures = G.judge(label + " rounded:", c, rounded, ref, **MUTE)
    assert not failures, failures
    worst_o = 0.0
    if c.family not in G.F64_FAMILIES:
        # a second float32 evaluation: the batch permuted and summed in four parts (.grad accumulates in float32)
        perm = np.random.RandomState(7).permutation(c.ns)
        leaves = A.to_torch(prm, torch.float32, requires_grad=True)
        w = (e - e.mean()) / len(e)                  # the weights of the WHOLE batch
        for part in np.array_split(perm, 4):
            lp = A.FORWARD[G.autograd_family(c.family)](leaves, s[part], G.SCOPE)
            d = torch.as_tensor(w[part])
            (2.0 * (lp.real * d.real + lp.imag * d.imag) if c.family == "crnn" else lp * d).sum().backward()
        again = {k: (leaves[k].grad if leaves[k].grad is not None else torch.zeros_like(leaves[k])).to(torch.float64).numpy()
                 .reshape(ref.g64[k].shape) for k in ref.g64}
        worst_o, failures = G.judge(label + " float32, other order:", c, again, ref)
        assert not failures, failures
    print("%s reference %.2f s; rounded float64 %.3f, second float32 evaluation %.3f x the yardstick (bound %g)" %
          (label, ref.seconds, worst_r, worst_o, A.FACTOR))


# ---- rejected: one case per family and layer count ------------------------------------------------------------------------------------

def _shifted_input(c, s):
    """the samples with the one-hot fed into site 32 replaced by the one fed into site 31 (positions on the path for the 2D RNN)"""
    fed, N = np.array(s), c.shape[0] * c.shape[1]
    if c.family == "mdrnn":
        path = [(nx, ny) for nx, ny, _ in A.M.zigzag_order(*c.shape)]
        fed[:, path[31][0], path[31][1]] = s[:, path[30][0], path[30][1]]
        return fed
    flat = fed.reshape(len(s), N)
    flat[:, 31] = np.asarray(s).reshape(len(s), N)[:, 30]
    return flat.reshape(np.shape(s))


def _first(family, layers):
    """the first case of the table with this family and layer count, equal widths, a remainder unit, and a batch in which the shifted
    input differs from the true one in some chain (sharpened weights freeze the tail of many batches: there the defect is void)"""
    fitting = [i for i, c in enumerate(G.CASES) if c.family == family and len(c.units) == layers and len(set(c.units)) == 1
               and c.ns == G.NS and max(c.units) > 16]
    for i in fitting:
        c = G.CASES[i]
        s, _ = batch(c.family, G.parameters(c), c.shape, c.ns)
        if not np.array_equal(_shifted_input(c, s), s):
            return i
    return fitting[0]              # no such batch (test_bound_rejects_every_defect names these)


REJECT_CASES = [_first(f, n) for f in ("gru", "crnn", "gru64") for n in (1, 2, 3, 4)] + [_first("parity", 1), _first("parity", 2),
                                                                                           _first("mdrnn", 1)]


def _unit_dropped_cell(x, h, params, scope, layer):
    """gru_cell whose reset gate's recurrent product in layer 0 misses the last unit"""
    if layer != 0:
        return A.gru_cell(x, h, params, scope, layer)
    pre = A.GRU % layer
    Wg, bg = A._p(params, scope, pre + "gates/kernel"), A._p(params, scope, pre + "gates/bias")
    Wci, bci = A._p(params, scope, pre + "candidate/input_projection/kernel"), A._p(params, scope, pre + "candidate/input_projection/bias")
    Wch, bch = A._p(params, scope, pre + "candidate/hidden_projection/kernel"), A._p(params, scope, pre + "candidate/hidden_projection/bias")
    nh = h.shape[1]
    a = torch.cat([x, h], dim=1) @ Wg + bg
    a = torch.cat([a[:, :nh] - h[:, -1:] @ Wg[-1:, :nh], a[:, nh:]], dim=1)
    g = torch.sigmoid(a)
    r, u = g[:, :nh], g[:, nh:]
    c = torch.tanh((x @ Wci + bci) + r * (h @ Wch + bch))
    return (1 - u) * c + u * h


def _unit_dropped_stack(x, states, params, scope):
    new_states = []
    for layer, h in enumerate(states):
        x = _unit_dropped_cell(x, h, params, scope, layer)
        new_states.append(x)
    return x, new_states


def _wrong_layer_stack(x, states, params, scope):
    """the top layer reads the new state of the layer two below; with two layers, layer 0's state of the previous site"""
    new_states, top = [], len(states) - 1
    for layer, h in enumerate(states):
        if layer == top:
            x = states[0] if top == 1 else new_states[top - 2]
        x = A.gru_cell(x, h, params, scope, layer)
        new_states.append(x)
    return x, new_states


def _md_unit_dropped(xh, hh, xv, hv, Uh, Wh, Uv, Wv, b):
    return xh @ Uh + hh[:, :-1] @ Wh[:-1] + xv @ Uv + hv @ Wv + b


def _with(fam, prm, s, e, **kw):
    """A.gradient with a tensor the defect leaves unused counted as zero"""
    return _gradient_of(prm, lambda leaves: A.cost(fam, leaves, s, e, **kw))


def _gradient_of(prm, cost_of_leaves):
    leaves = A.to_torch(prm, torch.float64, requires_grad=True)
    cost_of_leaves(leaves).backward()
    return {k: (v.grad if v.grad is not None else torch.zeros_like(v)).numpy().reshape(np.shape(prm[k])) for k, v in leaves.items()}


def defects(c, prm, s, e, ref):
    """{name: gradient with that defect}, all from the float64 reference"""
    fam, N = G.autograd_family(c.family), c.shape[0] * c.shape[1]
    out = {"chain dropped": {k: ref.g64[k] - ref.terms[k][-1] for k in ref.g64}}
    weight = np.ones(N)
    weight[-1] = 0.0
    out["last site dropped"] = _with(fam, prm, s, e, site_weight=weight)
    if c.family == "mdrnn":
        out["unit dropped"] = _with(fam, prm, s, e, pre_activation=_md_unit_dropped)
    else:
        out["unit dropped"] = _with(fam, prm, s, e, stack=_unit_dropped_stack)
    out["input shifted"] = _with(fam, prm, s, e, inputs=_shifted_input(c, s))
    if len(c.units) > 1:
        out["wrong layer below"] = _with(fam, prm, s, e, stack=_wrong_layer_stack)
    d = (np.asarray(e) - np.mean(e)) / len(e)
    if c.family == "crnn":
        def negated(leaves):
            lp = A.crnn_log_amplitude(leaves, s)
            return (2.0 * (lp.real * torch.as_tensor(d.real) - lp.imag * torch.as_tensor(d.imag))).sum()
        out["phase negated"] = _gradient_of(prm, negated)
    if c.family == "parity":
        def swapped(leaves):
            lpF = A.prnn_log_probability(leaves, s)
            lpR = A.prnn_log_probability(leaves, np.asarray(s)[:, ::-1])
            shF = torch.sigmoid(lpF - lpR).detach()                      # P_F / (P_F + P_R)
            return (torch.as_tensor(d) * ((1 - shF) * lpF + shF * lpR)).sum()
        out["shares swapped"] = _gradient_of(prm, swapped)
    return out


# Cases on which a defect is NOT rejected, with the reason (test_bound_rejects_every_defect asserts that each entry still holds).
# input shifted: in every 40-chain oracle batch of the equal-width two- and three-layer complex stacks and of the parity model's
# equal-width stack, the spins of sites 30 and 31 agree in all chains (the sharpened weights, and for the complex model the U(1) mask,
# leave the tail of every chain filled with one value), so the shifted input IS the true one.  The one- and four-layer complex cases,
# the one-layer parity case and all cases of the other families reject it.
VOID_SHIFT = ("crnn-34x1-17x17-40", "crnn-34x1-20x20x20-40", "parity-33x1-21x21-40")
# x 1.001 (whole tensor, and so a unit's row) on a tensor whose own bound exceeds 1e-3 cannot be told from rounding: {case: tensors}.
# The one-layer complex case's two-element phase bias has a bound of 1.0e-4.  On the three-layer complex case ("*": any tensor) float32
# autograd itself is 0.6e-4 .. 3e-4 from float64 on most tensors, so only some of them are tight enough (the amplitude head, at
# ratios near 400, and the top layer's are); there the test requires that at least one tensor rejects the scaling, and that
# whatever is reported is the scaled tensor alone.
LOOSE_TENSORS = {"crnn-34x1-37-40": ("wf_dense_phase/bias",), "crnn-34x1-20x20x20-40": "*"}


@pytest.mark.parametrize("i", REJECT_CASES, ids=[G.IDS[i] for i in REJECT_CASES])
def test_bound_rejects_every_defect(i):
    """Every defect of the module docstring is rejected on every case of REJECT_CASES (one per family and layer count), with these
    statements of what 'rejected' means: the worst ratio exceeds 16 and at least one tensor is reported.  A scaled tensor reports
    that tensor and no other; a scaled unit row reports its tensor and no other."""
    c, prm, s, e, ref = prepared(i)
    label = "[%s]" % G.case_id(c)
    missed = []
    for name, g in defects(c, prm, s, e, ref).items():
        worst, failures = G.judge(label, c, g, ref, **MUTE)
        print("%s %-20s worst ratio %10.1f, %d of %d tensors reported" % (label, name, worst, len(failures), len(g)))
        if name == "input shifted" and np.array_equal(_shifted_input(c, s), s):
            assert worst == 0.0 and G.case_id(c) in VOID_SHIFT       # the defect does not change this batch
        elif not (failures and worst > A.FACTOR):
            missed.append((name, worst))
    tight = 0
    for k, v in ref.g64.items():
        if not np.abs(v).max() > 0:
            continue
        scaled = dict(ref.g64)
        scaled[k] = v * 1.001
        worst, failures = G.judge(label, c, scaled, ref, **MUTE)
        listed = LOOSE_TENSORS.get(G.case_id(c), ())
        if listed == "*" and not failures:
            continue
        if k[len(G.SCOPE) + 1:] in listed:
            assert not failures, k                   # the entry still holds
            continue
        tight += 1
        if [n for n, _ in failures] != [k]:
            missed.append(("tensor x 1.001: " + k, worst))
        unit = np.unravel_index(np.abs(v).argmax(), v.shape)[-1]
        row = v.copy()
        row[..., unit] *= 1.001                      # the last axis indexes the unit (gate columns: unit or H + unit)
        if v.shape == (max(c.units), 2) or v.shape == (c.units[-1], 2):
            row = v.copy()                           # a head kernel [H, 2]: the unit is the row
            row[np.unravel_index(np.abs(v).argmax(), v.shape)[0], :] *= 1.001
        scaled[k] = row
        worst_row, failures = G.judge(label, c, scaled, ref, **MUTE)
        print("%s %-100s x 1.001: ratio %8.1f, one unit's row: %8.1f" % (label, k[len(G.SCOPE) + 1:], worst, worst_row))
        if [n for n, _ in failures] != [k]:
            missed.append(("unit row x 1.001: " + k, worst_row))
    assert not missed, missed
    assert tight > 0
