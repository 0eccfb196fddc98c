"""GPU tests of rnnwf_sr_train_steps (docs/sr.md, "Iterations on the device"): K whole minSR iterations per host synchronisation.

Every comparison is an equality of bits.  The device loop runs the kernels of the host loop (sr.train_tfim with solver="device":
vmc_step, sr_direction, theta - lr delta in NumPy, set_params_flat) on the same inputs in the same order; its update is the same two
IEEE operations and the same rounding to the model's type; its weight images are re-packed by the tables that test_gpu_train_images.py
checks against the host packers.  So there is no tolerance to choose.  The one bound in this file is the Jacobian's against float64
autograd at the new parameters, 1e-10 N x the row's largest element, the bound of tests/test_gpu_sr.py for the float64 model.

Sizes: N = 6 or 8, 37 samples (a ragged last 32 x 32 Cholesky panel and a partial block of 16 chains), 65 (three block rows), K <= 8;
units 10, 36 and 68 = width classes NFULL 1, 2 and 4 (68 units, float64: the backward operand streamed through L2).
"""
import functools

import numpy as np
import pytest

import sr_reference as R
from rnnwavefunctions_amd import params as P
from rnnwavefunctions_amd import sr

pytestmark = pytest.mark.gpu
SCOPE = "RNNwavefunction"
LR, SHIFT, SEED = 0.05, 1e-2, 111


def make_wf(N, units, f64, layers=1, model=None):
    from rnnwavefunctions_amd import _lib
    mid = model if model is not None else (_lib.MODEL_GRU1D_F64 if f64 else _lib.MODEL_GRU1D)
    return _lib.NativeWavefunction(mid, N, 1, (units,) * layers)


def make_params(units, f64, seed=7):
    prm = P.init_gru_params([units], seed=seed + units, dtype=np.float64 if f64 else np.float32)
    return P.randomize_biases(P.scale_kernels(prm, 2.0), seed + units + 1)


def coup(N):
    return np.append(np.ones(N), 1.0)


def flat(wf, prm):
    return sr.flatten_params(wf, wf.get_params_dict(prm, SCOPE), SCOPE)


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@functools.lru_cache(maxsize=None)
def host_loop(N, units, f64, ns, K):
    """sr.train_tfim(solver="device") with the default device_steps: (moments (K, 4), final flat parameters, means, variances)"""
    prm = make_params(units, f64)
    wf = make_wf(N, units, f64)
    rows, step = [], wf.vmc_step

    def recording_step(*a, **kw):
        out = step(*a, **kw)
        rows.append(np.array(out["moments"]))
        return out

    wf.vmc_step = recording_step
    mean, var = sr.train_tfim(wf, np.ones(N), 1.0, prm, numsteps=K - 1, numsamples=ns, learningrate=LR, diag_shift=SHIFT, seed=SEED,
                              scope=SCOPE, solver="device")
    last = sr.flatten_params(wf, sr.train_tfim.last_params, SCOPE)
    wf.close()
    return np.array(rows), last, np.array(mean), np.array(var)


def device_wf(N, units, f64):
    prm = make_params(units, f64)
    wf = make_wf(N, units, f64)
    wf.set_params(prm, scope=SCOPE)
    return wf, prm


@pytest.mark.parametrize("N,units,f64,ns", [(6, u, f64, 37) for u in (10, 36, 68) for f64 in (False, True)] + [(6, 10, False, 65), (6, 10, True, 65)],
                         ids=lambda v: str(v))
def test_trajectory_equals_the_host_loop(N, units, f64, ns):
    K = 5
    mom_host, theta_host, _, _ = host_loop(N, units, f64, ns, K)
    wf, prm = device_wf(N, units, f64)
    theta0 = flat(wf, prm)
    mom = wf.sr_train_steps(K, ns, SEED, 0, coup(N), LR, SHIFT)
    theta = flat(wf, prm)
    wf.close()
    assert mom.shape == (K, 4) and np.all(mom[:, 2] == ns)
    diff = np.flatnonzero(theta.view(np.uint64) != theta_host.view(np.uint64))
    print("moments rows differing: %s; parameters differing: %d of %d; moved from the start: %d"
          % (np.flatnonzero((mom.view(np.uint64) != mom_host.view(np.uint64)).any(axis=1)).tolist(), diff.size, theta.size,
             np.count_nonzero(theta != theta0)))
    assert same_bits(mom, mom_host)
    assert same_bits(theta, theta_host)
    assert np.count_nonzero(theta != theta0) > theta.size // 2                  # it did move
    if not f64:
        assert np.array_equal(theta, theta.astype(np.float32).astype(np.float64))


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
def test_chunking_is_invisible(f64):
    N, units, ns, K = 6, 10, 37, 6
    runs = []
    for chunks in ([6], [3, 3], [1] * 6):
        wf, prm = device_wf(N, units, f64)
        rows, step0 = [], 0
        for k in chunks:
            rows.append(wf.sr_train_steps(k, ns, SEED, step0, coup(N), LR, SHIFT))
            step0 += k
        runs.append((np.concatenate(rows), flat(wf, prm)))
        wf.close()
    assert runs[0][0].shape == (K, 4)
    for mom, theta in runs[1:]:
        assert same_bits(mom, runs[0][0]) and same_bits(theta, runs[0][1])


def test_schedules():
    N, units, ns = 6, 10, 37
    lrs, shifts = [0.05, 0.02, 0.08, 0.01], [1e-2, 3e-3, 5e-2, 1e-3]
    wf, prm = device_wf(N, units, False)
    mom = wf.sr_train_steps(4, ns, SEED, 0, coup(N), lrs, shifts)
    theta = flat(wf, prm)
    wf.close()
    wf, prm = device_wf(N, units, False)
    single = np.concatenate([wf.sr_train_steps(1, ns, SEED, k, coup(N), lrs[k], shifts[k]) for k in range(4)])
    theta_single = flat(wf, prm)
    constant = device_wf(N, units, False)[0].sr_train_steps(4, ns, SEED, 0, coup(N), lrs[0], shifts[0])
    wf.close()
    assert same_bits(mom, single) and same_bits(theta, theta_single)
    assert same_bits(mom[0], constant[0]) and not same_bits(mom[2], constant[2])     # the schedule is used, slot by slot


def test_state_after_the_call():
    from rnnwavefunctions_amd import _lib
    N, units, ns, K = 6, 10, 37, 5
    _, theta_host, _, _ = host_loop(N, units, True, ns, K)
    wf, prm = device_wf(N, units, True)
    wf.vmc_step(ns, SEED, 0, coup(N))
    assert wf.resident_samples() == ns
    wf.sr_train_steps(K, ns, SEED, 0, coup(N), LR, SHIFT)
    assert wf.resident_samples() == 0
    with pytest.raises(_lib.RnnwfError, match="vmc_step first"):
        wf.sr_gram()
    new = wf.get_params_dict(prm, SCOPE)
    assert same_bits(sr.flatten_params(wf, new, SCOPE), theta_host)
    # the Jacobian of a batch loaded afterwards is the one at the NEW parameters (weight images and backward image re-packed)
    rng = np.random.RandomState(5)
    s = rng.randint(0, 2, size=(ns, N)).astype(np.int32)
    e = rng.standard_normal(ns) * 2.0 - 3.0
    wf.load_batch(s, e)
    O = wf.log_derivatives()
    wf.close()
    ref, old = R.jacobian(new, s), R.jacobian(prm, s)
    rel = np.abs(O - ref).max(axis=1) / np.abs(ref).max(axis=1)
    print("jacobian at the new parameters: worst row error / row max %.3e (bound %.1e); new against old parameters %.3e"
          % (rel.max(), 1e-10 * N, np.abs(ref - old).max() / np.abs(old).max()))
    assert np.abs(ref - old).max() > 1e-3 * np.abs(old).max()
    assert rel.max() <= 1e-10 * N


def test_adam_is_untouched():
    from rnnwavefunctions_amd import _lib
    from rnnwavefunctions_amd import training as T
    N, units, ns = 6, 10, 37
    wf, prm = device_wf(N, units, False)
    rng = np.random.RandomState(9)
    n = wf.num_params()
    wf.adam_set_state(rng.standard_normal(n), rng.random_sample(n), 3)
    m0, v0, t0 = wf.adam_get_state()
    wf.sr_train_steps(3, ns, SEED, 0, coup(N), LR, SHIFT)
    m1, v1, t1 = wf.adam_get_state()
    assert t0 == t1 == 3 and same_bits(m0, m1) and same_bits(v0, v1) and np.abs(m0).max() > 0
    # Adam iterations on the device after it against the host optimizer started from the parameters minSR left
    start = wf.get_params_dict(prm, SCOPE)
    wf.adam_set_state(None, None, 0)
    mom_dev = wf.train_steps(ns, SEED, 3, coup(N), [5e-3] * 3)
    dev = wf.get_params_dict(prm, SCOPE)
    wf.close()
    shapes = {k[len(SCOPE) + 1:]: v.shape for k, v in prm.items()}
    ref = _lib.NativeWavefunction(_lib.MODEL_GRU1D, N, 1, (units,))
    opt, host = T.Adam(), dict(start)
    for it in range(3):
        ref.set_params(host, scope=SCOPE)
        m = ref.vmc_step(ns, SEED, 3 + it, coup(N))["moments"]
        assert same_bits(m, mom_dev[it]), it
        g = ref.vmc_gradient(m[0] / m[2], m[2], shapes)
        host = opt.step(host, {SCOPE + "/" + k: v for k, v in g.items()}, 5e-3)
    ref.close()
    for k in prm:
        assert np.array_equal(dev[k], host[k]), k


def test_refusals_touch_nothing():
    from rnnwavefunctions_amd import _lib
    N, ns = 6, 37
    refused = [(make_wf(N, 10, False, model=_lib.MODEL_GRU1D_PARITY), "parity"),
               (make_wf(N, 10, False, model=_lib.MODEL_CRNN_U1), "complex RNN"),
               (_lib.NativeWavefunction(_lib.MODEL_MDRNN2D, 3, 2, (10,)), "2D RNN"),
               (make_wf(N, 10, True, model=_lib.MODEL_LSTM1D_F64), "LSTM"),
               (make_wf(N, 10, False, layers=2), "stacked layers"),
               (make_wf(N, 70, False), "wider than 68")]
    for wf, why in refused:
        wf.init_params(5)
        with pytest.raises(ValueError, match="rnnwf_sr_train_steps: .*" + why):
            wf.sr_train_steps(2, ns, SEED, 0, coup(N), LR, SHIFT)
        wf.close()
    wf, prm = device_wf(N, 10, False)
    wf.vmc_step(48, 3, 0, coup(N))
    gram0, theta0 = wf.sr_gram()[0], flat(wf, prm)
    nan, inf = float("nan"), float("inf")
    bad = [("1 <= K <= 1024", dict(K=0)), ("1 <= K <= 1024", dict(K=1025)), ("wrong number of couplings", dict(couplings=np.ones(N)))]
    bad += [("diag_shift must be positive and finite", dict(K=3, diag_shifts=[SHIFT, SHIFT, v])) for v in (0.0, -1.0, nan, inf)]
    bad += [("diag_shift must be positive and finite", dict(K=3, diag_shifts=[nan, SHIFT, SHIFT])),
            ("learning_rate must be finite", dict(K=3, learning_rates=[LR, nan, LR])), ("learning_rate must be finite", dict(learning_rates=inf))]
    for why, kw in bad:
        a = dict(K=2, numsamples=ns, seed=SEED, step0=0, couplings=coup(N), learning_rates=LR, diag_shifts=SHIFT)
        a.update(kw)
        with pytest.raises(ValueError, match="rnnwf_sr_train_steps: .*" + why):
            wf.sr_train_steps(**a)
        assert wf.resident_samples() == 48 and same_bits(wf.sr_gram()[0], gram0), why
    with pytest.raises(_lib.RnnwfError, match="rnnwf_sr_train_steps: ns too large for the SR workspace"):
        wf.sr_train_steps(2, 4112, SEED, 0, coup(N), LR, SHIFT)
    assert wf.resident_samples() == 48 and same_bits(wf.sr_gram()[0], gram0)
    assert same_bits(flat(wf, prm), theta0)
    wf.close()
    # uncommitted parameters
    fresh = make_wf(N, 10, False)
    with pytest.raises(_lib.RnnwfError, match="rnnwf_sr_train_steps: parameters not committed"):
        fresh.sr_train_steps(2, ns, SEED, 0, coup(N), LR, SHIFT)
    fresh.close()


def test_train_tfim_on_the_device_equals_the_host_loop():
    """the configuration of test_gpu_sr.py's training test: the same 61 energies and variances, so that test's criteria hold"""
    N, units, ns, steps, seed = 8, 10, 200, 60, 111
    prm = P.init_gru_params([units], seed=seed)
    out = []
    for device_steps in (None, 16):
        wf = make_wf(N, units, False)
        mean, var = sr.train_tfim(wf, np.ones(N), 1.0, prm, numsteps=steps, numsamples=ns, learningrate=LR, diag_shift=SHIFT, seed=seed,
                                  solver="device", device_steps=device_steps)
        out.append((np.array(mean), np.array(var), sr.flatten_params(wf, sr.train_tfim.last_params, SCOPE), sr.train_tfim.last_params))
        wf.close()
    assert len(out[1][0]) == len(out[1][1]) == steps + 1
    assert same_bits(out[0][0], out[1][0]) and same_bits(out[0][1], out[1][1]) and same_bits(out[0][2], out[1][2])
    assert all(out[1][3][k].dtype == prm[k].dtype and out[1][3][k].shape == prm[k].shape for k in prm)
    assert out[1][0][-1] < out[1][0][0]
