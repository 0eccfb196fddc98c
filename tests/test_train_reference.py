"""CPU checks of tests/train_reference.py: the float64 restatement of TF-1 Adam against torch.optim.Adam and closed forms,
training.Adam (the drivers' host optimizer) against the restatement bit for bit, and the consistency of the case table of
tests/test_gpu_train_images.py."""
import math

import numpy as np
import pytest
import torch

import gradient_classes_reference as G
import train_reference as T

B1, B2, EPS = 0.9, 0.999, 1e-8
LRS = (1e-2, 3e-3, 7e-3, 5e-4, 2e-2)                 # five steps, distinct learning rates
NAMES = ("a/kernel", "a/bias", "b/kernel")
SHAPES = ((40, 30), (77,), (13, 5, 7))


def _inputs(dtype, seed=0):
    """theta ~ N(0, 1) in the model's type; per step gradients of magnitude 10^U(-9, 1) with random signs; every seventh element has
    g = 0 in every step"""
    rng = np.random.RandomState(seed)
    theta = {k: rng.standard_normal(s).astype(dtype) for k, s in zip(NAMES, SHAPES)}
    grads = []
    for _ in LRS:
        g = {}
        for k, s in zip(NAMES, SHAPES):
            a = 10.0 ** rng.uniform(-9.0, 1.0, s) * rng.choice([-1.0, 1.0], s)
            a.reshape(-1)[::7] = 0.0
            g[k] = a
        grads.append(g)
    return theta, grads


def _run_reference(dtype, theta, grads):
    ref = T.AdamReference(dtype, B1, B2, EPS)
    cur = {k: v.astype(np.float64) for k, v in theta.items()}
    history = []
    for g, lr in zip(grads, LRS):
        cur = ref.step(cur, g, lr)
        history.append(cur)
    return ref, history


def test_float64_restatement_agrees_with_torch_adam():
    """torch.optim.Adam divides by sqrt(v) / sqrt(1 - beta2^t) + eps; with eps = epsilon / sqrt(1 - beta2^t) before step t that is
    (sqrt(v) + epsilon) / sqrt(1 - beta2^t), and its step lr / (1 - beta1^t) times m over it is TF-1's lr_t m / (sqrt(v) + epsilon).
    Bound: 4 ulp of max(1, |theta|) per element (each side rounds the subtraction once per step)."""
    theta, grads = _inputs(np.float64)
    _, history = _run_reference(np.float64, theta, grads)
    tp = {k: torch.nn.Parameter(torch.tensor(v, dtype=torch.float64)) for k, v in theta.items()}
    opt = torch.optim.Adam(list(tp.values()), lr=LRS[0], betas=(B1, B2), eps=EPS, foreach=False)
    worst = 0.0
    for t, (g, lr) in enumerate(zip(grads, LRS), start=1):
        for grp in opt.param_groups:
            grp["lr"] = lr
            grp["eps"] = EPS / math.sqrt(1.0 - B2 ** t)
        for k in NAMES:
            tp[k].grad = torch.tensor(g[k], dtype=torch.float64)
        opt.step()
        for k in NAMES:
            got, want = history[t - 1][k], tp[k].detach().numpy()
            ulp = np.spacing(np.maximum(1.0, np.abs(want)))
            worst = max(worst, float((np.abs(got - want) / ulp).max()))
    print("restatement vs torch.optim.Adam over %d steps: worst deviation %.2f ulp of max(1, |theta|)" % (len(LRS), worst))
    assert worst <= 4.0


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_closed_forms(dtype):
    """After ONE step m = (1 - beta1) g, v = (1 - beta2) g^2, lr_1 = lr sqrt(1 - beta2) / (1 - beta1), so every element moves by
    lr sign(g) / (1 + epsilon / (sqrt(1 - beta2) |g|)): asserted for EVERY element with g != 0 (to the rounding of the model's type),
    and in the form lr (1 +- 1e-4) sign(g) wherever epsilon / (sqrt(1 - beta2) |g|) <= 1e-4, i.e. |g| >= 3.17e-3.  (At |g| = 1e-3 the
    exact move is lr (1 - 3.16e-4): no correct Adam is within 1e-4 of lr there.)  An element with g = 0 in every step never moves."""
    theta, grads = _inputs(dtype)
    _, history = _run_reference(dtype, theta, grads)
    lr = LRS[0]
    u = 2.0 ** -24 if dtype == np.float32 else 2.0 ** -53
    threshold = EPS / (1e-4 * math.sqrt(1.0 - B2))
    assert 3.1e-3 < threshold < 3.2e-3
    checked = 0
    for k in NAMES:
        t0, g = theta[k].astype(np.float64), grads[0][k]
        move = history[0][k] - t0
        nz = g != 0
        exact = -lr * np.sign(g[nz]) / (1.0 + EPS / (math.sqrt(1.0 - B2) * np.abs(g[nz])))
        assert np.all(np.abs(move[nz] - exact) <= 2 * u * np.maximum(1.0, np.abs(t0[nz])) + 1e-12 * lr), k
        big = np.abs(g) >= threshold
        checked += int(big.sum())
        assert np.all(np.abs(move[big] + lr * np.sign(g[big])) <= 1e-4 * lr + 2 * u * np.maximum(1.0, np.abs(t0[big]))), k
        never = np.all([gs[k] == 0 for gs in grads], axis=0)
        assert never.sum() >= g.size // 7
        assert np.array_equal(history[-1][k][never], t0[never]), k
    assert checked > 500


def test_float32_models_keep_theta_representable_in_float32():
    theta, grads = _inputs(np.float32)
    ref, history = _run_reference(np.float32, theta, grads)
    for cur in history:
        for k in NAMES:
            assert cur[k].dtype == np.float64
            assert np.array_equal(cur[k].astype(np.float32).astype(np.float64), cur[k]), k
    # ... and the moments are NOT rounded: some element of m needs more than float32
    assert any(not np.array_equal(ref.m[k].astype(np.float32).astype(np.float64), ref.m[k]) for k in NAMES)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_training_adam_equals_the_restatement_bit_for_bit(dtype):
    """What makes test_device_resident_training_equals_the_host_optimizer_bit_for_bit rest on something: the host optimizer of the
    drivers IS TF-1 Adam as restated, to the last bit, in both model types."""
    from rnnwavefunctions_amd.training import Adam
    theta, grads = _inputs(dtype)
    ref, history = _run_reference(dtype, theta, grads)
    opt = Adam(B1, B2, EPS)
    cur = {k: v.copy() for k, v in theta.items()}
    for t, (g, lr) in enumerate(zip(grads, LRS)):
        cur = opt.step(cur, g, lr)
        for k in NAMES:
            assert cur[k].dtype == dtype
            assert np.array_equal(cur[k].astype(np.float64), history[t][k]), (t, k)
    assert opt.t == ref.t == len(LRS)
    for k in NAMES:
        assert np.array_equal(opt.m[k], ref.m[k]) and np.array_equal(opt.v[k], ref.v[k]), k


def test_case_table_is_consistent():
    assert len(set(T.CASE_IDS)) == len(T.CASES)
    have = [(c[1], c[3], c[5]) for c in T.CASES]
    for row in T.REQUIRED:
        assert row in have, "no case for %r" % (row,)
    reached = set()
    for cid, family, shape, units, ns, env, engine, why in T.CASES:
        assert why and ns == T.NS, cid
        assert G.refusal(family, units) is None, cid                          # rnnwf_create admits the row
        nf = T.nfull(family, units)
        assert nf == G.nfull(family, units) and nf is not None, cid
        assert nf == min(n for n in (1, 2, 3, 4, 5, 6, 8, 12, 16) if (n != 5 or family == "mdrnn") and 16 * n + 4 >= max(units)), cid
        assert engine == T.expected_engine(family, units, env), cid
        assert shape == ((3, 2) if family in T.F64_FAMILIES else (6, 1)), cid
        assert set(env) <= {"RNNWF_ENGINE", "RNNWF_BASE"}, cid
        if env.get("RNNWF_ENGINE") == "bf16x3":                               # a pinned row must reach the bf16x3 images
            assert T.engine_split(family, units, env) and engine == "bf16x3", cid
        reached |= T.table_rows(family, units, env)
    missing = T.REQUIRED_TABLE_ROWS - reached
    assert not missing, "packer table rows no case replays: %s" % sorted(map(str, missing))
    # the rows the engine names stand for: the positive GRU reads the bf16x3 images only in the pinned rows
    assert T.case("gru-52")[6] == "f32mfma" and T.case("gru-52-bf16x3")[6] == "bf16x3" and T.case("gru-101")[6] == "f32mfma"
    assert T.case("crnn-100")[6] == "bf16x3" and T.case("crnn-132")[6] == "f32mfma" and T.case("crnn-stack-68-20")[6] == "f32mfma"
    assert T.case("gru64-100")[6] == "f64mfma" and T.case("mdrnn-84")[6] == "f64mfma"
