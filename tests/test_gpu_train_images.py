"""Device-resident training (rnnwf_train_steps / rnnwf_adam_step, csrc/train.hip) at every width class: after the device's own Adam
updates, is every weight image the kernels read the one the host packers would have built from the same parameters?

One case per packer-table row (tests/train_reference.py: CASES), through _lib.NativeWavefunction directly.  Handle A trains on the
device for three iterations; then

  a. a second handle replays the iterations on the host - vmc_step, vmc_gradient from its moments, the float64 restatement of TF-1
     Adam (train_reference.AdamReference, checked on the CPU against torch.optim.Adam), set_params: moments, parameters and the
     optimizer state of A are EXACTLY the replay's - the contract train.hip states (the dW-to-flat gather table, adam_kernel);
  b. a fresh handle given A's downloaded parameters agrees with A bit for bit on every entry point, one assertion per image read:
     the sampler, log_prob / log_amp, the local energies with their log-probability queue, a VMC step and every gradient tensor;
  c. A's log_prob / log_amp is the float64 oracle's of A's downloaded parameters within the suite's bounds for these entry points
     (a stale image is off by about learning rate x N, orders of magnitude more);
  d. every tensor moved, no element by more than sum(lr) x 3.2 - (1 - beta1) / sqrt(1 - beta2) = 3.16 bounds |m| / sqrt(v);
  e. one more rnnwf_adam_step on the gradient just taken, and (b)'s forward comparisons again against another fresh handle: the
     re-pack after the backward image joined the combined table.

(b) is asserted before (a): a stale image also spoils the second iteration of A's own trajectory, and the failure should name the
image.  With the wsplit16 table taken out of train.hip (tried once, not committed) gru-69-bf16x3 and gru-100-bf16x3 fail at
"(b) local energies (tfim_eloc, engine bf16x3): the log-probability queue" and every other row passes.
"""
import time

import numpy as np
import pytest

import train_reference as T

pytestmark = pytest.mark.gpu
SCOPE = T.SCOPE
STEP_MOVE = 3.2


def _model_id(family):
    from rnnwavefunctions_amd import _lib
    return {"gru": _lib.MODEL_GRU1D, "parity": _lib.MODEL_GRU1D_PARITY, "crnn": _lib.MODEL_CRNN_U1, "gru64": _lib.MODEL_GRU1D_F64,
            "mdrnn": _lib.MODEL_MDRNN2D}[family]


def _handle(family, shape, units, prm):
    """the environment is read once, at rnnwf_create: the caller has set it"""
    from rnnwavefunctions_amd import _lib
    wf = _lib.NativeWavefunction(_model_id(family), shape[0], shape[1], units)
    wf.set_params(prm, scope=SCOPE)
    return wf


def _mean_energy(family, m):
    return complex(m[0] / m[2], m[3] / m[2]) if family == "crnn" else m[0] / m[2]


def _as_model(family, theta, like):
    return {k: theta[k].astype(like[k].dtype) for k in like}


def _same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and np.array_equal(a, b), \
        "%s: %d of %d entries differ, max |d| = %.3e" % (what, int((a != b).sum()), a.size, float(np.abs(a - b).max()))


def _forward_images(cid, tag, family, ham, cfg, ns, a, c):
    """sampler, log_prob / log_amp, local energies with the log-probability queue: trained handle `a` against the host-packed `c`"""
    N = a.N
    sa, la = a.sample(ns, T.SEED, step=7, return_log=True)
    sc, lc = c.sample(ns, T.SEED, step=7, return_log=True)
    _same(sa, sc, "%s %s sample(step=7): spins" % (cid, tag))
    _same(la, lc, "%s %s sample(step=7): log-probabilities" % (cid, tag))
    _same(a.log_prob(cfg), c.log_prob(cfg), "%s %s log_prob" % (cid, tag))
    if family == "crnn":
        _same(a.log_amp(cfg), c.log_amp(cfg), "%s %s log_amp" % (cid, tag))
        ea, na = a.j1j2_eloc(cfg, ham["J1"], ham["J2"], ham["Bz"])
        ec, nc = c.j1j2_eloc(cfg, ham["J1"], ham["J2"], ham["Bz"])
        assert na == nc, "%s %s j1j2_eloc: %d vs %d connected configurations" % (cid, tag, na, nc)
        _same(ea, ec, "%s %s local energies (j1j2_eloc, engine %s): E_loc" % (cid, tag, a.engine_name()))
    else:
        qa, qc = np.zeros((N + 1) * len(cfg)), np.zeros((N + 1) * len(cfg))
        ea = a.tfim_eloc(cfg, ham["Jz"], ham["Bx"], log_probs=qa)
        ec = c.tfim_eloc(cfg, ham["Jz"], ham["Bx"], log_probs=qc)
        _same(qa, qc, "%s %s local energies (tfim_eloc, engine %s): the log-probability queue" % (cid, tag, a.engine_name()))
        _same(ea, ec, "%s %s local energies (tfim_eloc, engine %s): E_loc" % (cid, tag, a.engine_name()))


@pytest.mark.parametrize("cid", T.CASE_IDS)
def test_device_trained_images_equal_the_host_packed_ones(cid, monkeypatch):
    _, family, shape, units, ns, env, engine, why = T.case(cid)
    for k in ("RNNWF_ENGINE", "RNNWF_BASE"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    t_start = time.time()
    N = shape[0] * shape[1]
    prm = T.parameters(family, units)
    shapes = {k[len(SCOPE) + 1:]: v.shape for k, v in prm.items()}
    ham = T.hamiltonian(family, N)
    coup = T.couplings(family, ham)
    cfg = T.configurations(family, shape)
    lrs = list(T.LEARNING_RATES)

    # ---- handle A: three iterations on the device
    a = _handle(family, shape, units, prm)
    assert a.device_training_supported(), "%s: the library refuses device training" % cid
    mom_a = a.train_steps(ns, T.SEED, 0, coup, lrs)
    trained = a.get_params_dict(prm, SCOPE)
    m_a, v_a, t_a = a.adam_get_state()

    # ---- (b) every image against a fresh handle's host-packed one - first, so that a stale image is named as such and not as the
    #      trajectory it spoils
    c = _handle(family, shape, units, trained)
    _forward_images(cid, "(b)", family, ham, cfg, ns, a, c)
    assert a.engine_name() == engine, "%s: engine %s, the row is meant for %s" % (cid, a.engine_name(), engine)
    assert c.engine_name() == engine
    oa = a.vmc_step(ns, seed=T.SEED, step=9, couplings=coup, want_samples=True, want_eloc=True)
    oc = c.vmc_step(ns, seed=T.SEED, step=9, couplings=coup, want_samples=True, want_eloc=True)
    _same(oa["samples"], oc["samples"], "%s (b) vmc_step samples" % cid)
    _same(oa["eloc"], oc["eloc"], "%s (b) vmc_step local energies" % cid)
    _same(oa["moments"], oc["moments"], "%s (b) vmc_step moments" % cid)
    ga = a.vmc_gradient(_mean_energy(family, oa["moments"]), oa["moments"][2], shapes)
    gc = c.vmc_gradient(_mean_energy(family, oc["moments"]), oc["moments"][2], shapes)
    for k in shapes:
        assert np.all(np.isfinite(gc[k])) and np.abs(gc[k]).max() > 0, k
        _same(ga[k], gc[k], "%s (b) vmc_gradient (backward image) %s" % (cid, k))

    # ---- (a) the host replay with the independent optimizer (handle b shares nothing with a)
    b = _handle(family, shape, units, prm)
    ref = T.AdamReference(T.model_dtype(family))
    theta = {k: v.astype(np.float64) for k, v in prm.items()}
    for it, lr in enumerate(lrs):
        m = b.vmc_step(ns, seed=T.SEED, step=it, couplings=coup)["moments"]
        _same(mom_a[it], m, "%s (a) moments of iteration %d" % (cid, it))
        g = b.vmc_gradient(_mean_energy(family, m), m[2], shapes)
        theta = ref.step(theta, {SCOPE + "/" + k: v for k, v in g.items()}, lr)
        b.set_params(_as_model(family, theta, prm), scope=SCOPE)
    for k in prm:
        assert trained[k].dtype == prm[k].dtype
        _same(trained[k].astype(np.float64), theta[k], "%s (a) parameters after %d device iterations: %s" % (cid, len(lrs), k))
    order = [SCOPE + "/" + nm for nm, _ in a._layout()]
    m_ref, v_ref = ref.flat(order)
    assert t_a == ref.t == len(lrs)
    _same(m_a, m_ref, "%s (a) Adam first moments" % cid)
    _same(v_a, v_ref, "%s (a) Adam second moments" % cid)

    # ---- (d) it trained, within Adam's step bound
    for k in prm:
        moved = np.abs(trained[k].astype(np.float64) - prm[k].astype(np.float64))
        assert moved.max() > 0, "%s (d) %s did not move" % (cid, k)
        assert moved.max() <= sum(lrs) * STEP_MOVE, "%s (d) %s moved by %.3e" % (cid, k, moved.max())

    # ---- (c) the trained weights are what the kernels compute with
    trained64 = {k: v.astype(np.float64) for k, v in trained.items()}
    want = T.oracle_value(family, trained64, cfg)
    bound = T.oracle_bound(family, N, len(units))
    assert np.all(np.isfinite(want))
    if family == "crnn":
        got = a.log_amp(cfg)
        err_re, err_im = np.abs(got.real - want.real).max(), np.abs(got.imag - want.imag).max()
        assert err_re <= bound and err_im <= 4 * bound, "%s (c) log_amp vs f64 oracle: re %.2e im %.2e, bound %.2e / %.2e" % (
            cid, err_re, err_im, bound, 4 * bound)               # the phase's bound is test_gpu_crnn.py's
        err = max(err_re, err_im)
    else:
        err = np.abs(a.log_prob(cfg) - want).max()
        assert err <= bound, "%s (c) log_prob vs f64 oracle: %.2e, bound %.2e" % (cid, err, bound)
    stale = np.abs(T.oracle_value(family, {k: v.astype(np.float64) for k, v in prm.items()}, cfg) - want).max()
    assert stale > 100 * bound, "%s (c) the initial weights' values are within %.1e of the trained ones: a stale image would pass" % (cid, stale)

    # ---- (e) one more update from the gradient just taken: the second re-pack with the backward image in the table
    a.adam_step(lrs[-1])
    again = a.get_params_dict(prm, SCOPE)
    assert any(not np.array_equal(again[k], trained[k]) for k in prm)
    d = _handle(family, shape, units, again)
    _forward_images(cid, "(e)", family, ham, cfg, ns, a, d)
    theta = ref.step(theta, {SCOPE + "/" + k: v for k, v in ga.items()}, lrs[-1])
    for k in prm:
        _same(again[k].astype(np.float64), theta[k], "%s (e) parameters after rnnwf_adam_step: %s" % (cid, k))
    print("%s: engine %s, |A - f64 oracle| %.2e (bound %.2e, stale weights %.2e), %.2f s  [%s]" %
          (cid, a.engine_name(), err, bound, stale, time.time() - t_start, why))


def test_host_parameters_set_between_two_device_runs_are_the_ones_trained():
    """params_to_device's flags (train.hip: host_newer / dev_newer): set_params with new weights after a train_steps call, then
    train_steps again - equal, exactly, to a fresh handle given those weights and the saved Adam state through adam_set_state."""
    family, shape, units, ns = "gru", (6, 1), (50,), T.NS
    prm = T.parameters(family, units)
    other = T.parameters(family, units, seed=T.SEED + 7)
    ham = T.hamiltonian(family, 6)
    coup = T.couplings(family, ham)
    a = _handle(family, shape, units, prm)
    a.train_steps(ns, T.SEED, 0, coup, [1e-2, 5e-3])
    m, v, t = a.adam_get_state()
    assert t == 2 and np.abs(m).max() > 0
    a.set_params(other, scope=SCOPE)
    for k in other:                                                   # the host's values are what the handle now reports ...
        _same(a.get_param(k[len(SCOPE) + 1:], other[k].shape, other[k].dtype), other[k], "get_param after set_params: " + k)
    mom_a = a.train_steps(ns, T.SEED, 2, coup, [2e-3, 1e-3])
    f = _handle(family, shape, units, other)
    f.adam_set_state(m, v, t)
    mom_f = f.train_steps(ns, T.SEED, 2, coup, [2e-3, 1e-3])
    _same(mom_a, mom_f, "moments")
    pa, pf = a.get_params_dict(prm, SCOPE), f.get_params_dict(prm, SCOPE)
    for k in prm:
        _same(pa[k], pf[k], "parameters: " + k)
        assert not np.array_equal(pa[k], other[k]), k
    sa, sf = a.adam_get_state(), f.adam_get_state()
    assert sa[2] == sf[2] == 4
    _same(sa[0], sf[0], "Adam first moments")
    _same(sa[1], sf[1], "Adam second moments")
    cfg = T.configurations(family, shape)
    _same(a.log_prob(cfg), f.log_prob(cfg), "log_prob after the second run")
