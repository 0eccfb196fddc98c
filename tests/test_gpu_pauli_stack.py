"""GPU tests of Pauli strings, generic Hamiltonian energies and device-resident training for STACKED GRU layers
(rnnwf_pauli_step_stack, rnnwf_pauli_train_steps_stack: csrc/pauli_stack.hip, csrc/stack_chain_kernels.h; docs/pauli_stack.md).

Log-ratios, E_loc and per-term sums are compared with the float64 brute force of tests/pauli_stack_reference.py (every flipped
configuration scored from site 0 by the oracle's stacked GRU) on caller-supplied samples; the bounds are that module's: float64
1e-11 N per log-ratio, float32 twice the measured error of the existing stack flip pass at the same shape, E_loc and the sums from the
reference's own ratios.  Everything else is an identity under np.array_equal: draws, passes, repeats, the gradient of the resident
batch, and the trajectory of the device-resident iterations against the host loop pauli_step_stack -> cost_gradient -> training.Adam
-> set_params.

Measured on an MI355X (docs/pauli_stack.md has the table): float32 log-ratios at most 0.59 of their tolerance (N = 34, 1.69e-05 of
2.88e-05), float64 at most 2.2e-14 (5x7) of 3.5e-10, E_loc at most 0.17 of its bound, per-term sums 0.33; the end-to-end run goes from
E = -9.879 +- 0.107 to -11.418 +- 0.016 (ground state -11.4499).  The module takes 10 s, its slowest accuracy case 1.3 s.
"""
import re

import numpy as np
import pytest

import pauli_stack_reference as SR
from conftest import all_configs
from rnnwavefunctions_amd import observables as O
from rnnwavefunctions_amd import observables_stack as OS
from rnnwavefunctions_amd import params as P
from rnnwavefunctions_amd import training as T

pytestmark = pytest.mark.gpu

SCOPE = SR.SCOPE
STEP_ENTRY, TRAIN_ENTRY = "rnnwf_pauli_step_stack", "rnnwf_pauli_train_steps_stack"
NS = 37                         # two full 16-chain blocks and a ragged third
STRIDE_NS_F32 = 4000            # 250 blocks x 33 masks = 8250 tiles > 32 waves on each of 256 CUs
STRIDE_NS_F64 = 1664            # 104 blocks x 10 masks = 1040 tiles > 4 waves on each of 256 CUs (one wave per SIMD at 2 x 50 float64 units)


def make_wf(f64, shape, units, prm):
    from rnnwavefunctions_amd import _lib
    wf = _lib.NativeWavefunction(_lib.MODEL_GRU1D_F64 if f64 else _lib.MODEL_GRU1D, shape[0], shape[1], tuple(units))
    wf.set_params(prm, scope=SCOPE)
    return wf


def weights(f64, units, seed=111, sharp=3.0):
    return SR.weights("gru64" if f64 else "gru", units, seed=seed, sharp=sharp)


# (float64, lattice, units, samples, Hamiltonian).  "mixed" has a mask starting at site 0, one at site N - 1, the dense mask and, from
# 33 sites on, one run across the word boundary (test_pauli_stack_reference.py asserts it)
F32 = [(False, (6, 1), u, NS, "mixed") for u in [(10, 10), (10, 10, 10), (10, 10, 10, 10), (20, 20), (37, 37), (50, 50), (68, 68), (100, 100),
                                                 (10, 20), (37, 20)]] + \
      [(False, (6, 1), (10, 10), NS, "tfim"), (False, (6, 1), (10, 10), NS, "diagonal"), (False, (34, 1), (10, 10), NS, "mixed"),
       (False, (34, 1), (10, 10), STRIDE_NS_F32, "xxz")]
F64 = [(True, (3, 2), u, NS, "mixed") for u in [(10, 10), (10, 10, 10), (10, 10, 10, 10), (20, 20), (37, 37), (50, 50), (68, 68), (37, 20)]] + \
      [(True, (5, 7), (10, 10), NS, "mixed"), (True, (3, 2), (50, 50), STRIDE_NS_F64, "mixed")]


def case_id(c):
    return "%s-%dx%d-%s-ns%d-%s" % ("f64" if c[0] else "f32", c[1][0], c[1][1], "x".join(str(u) for u in c[2]), c[3], c[4])


@pytest.mark.parametrize("case", F32 + F64, ids=case_id)
def test_log_ratios_eloc_and_term_sums_against_float64(case):
    f64, shape, units, ns, name = case
    N = shape[0] * shape[1]
    prm = weights(f64, units)
    wf = make_wf(f64, shape, units, prm)
    ham = SR.hamiltonian(name, N)
    nmasks = len({r.tobytes() for r in ham.flip if r.any()})
    if ns > NS:                                       # the grid-stride loop: more tiles than the chip holds waves
        cus, tiles = wf.device_info()["cu_count"], nmasks * ((ns + 15) // 16)
        print("[%s] %d CUs, %d tiles" % (case_id(case), cus, tiles))
        assert tiles > (4 if f64 else 32) * cus
    s = wf.sample(ns, seed=111, step=0).reshape(ns, N)
    out = wf.pauli_step_stack(ham.flip, ham.sign, ham.coeff, ns, samples=s, want_eloc=True, want_log_ratio=True)
    ref = SR.reference(prm, s, ham)
    tol = SR.f64_tol(N) if f64 else SR.f32_tol(units, N, ns)
    SR.judge("[%s]" % case_id(case), out, ref, tol)
    assert out["moments"][2] == ns and np.isclose(out["moments"][0], out["eloc"].sum(), rtol=1e-13, atol=0)
    assert wf.resident_samples() == ns
    if nmasks:                                        # the weights are sharp: the ratios spread
        r = np.exp(ref["log_ratio"])
        assert r.std() > 0.2 * r.mean()


def test_exact_energy_from_all_configurations():
    """N = 6, two float64 layers: all 64 configurations as samples, weighted with P - the dense <psi|H|psi> to 1e-10"""
    units, shape, N = (10, 10), (3, 2), 6
    prm = weights(True, units)
    wf = make_wf(True, shape, units, prm)
    c = all_configs(N).astype(np.int32)
    lp = wf.log_prob(c)
    psi = np.exp(0.5 * lp)
    assert abs(np.exp(lp).sum() - 1.0) < 1e-10
    for name in ("xxz", "tfim", "diagonal", "mixed"):
        ham = SR.hamiltonian(name, N)
        e = wf.pauli_step_stack(ham.flip, ham.sign, ham.coeff, 64, samples=c, want_eloc=True)["eloc"]
        exact = psi @ SR.dense(ham) @ psi
        print("[exact %s] sum P E_loc = %.12f, <H> = %.12f" % (name, (np.exp(lp) * e).sum(), exact))
        assert abs((np.exp(lp) * e).sum() - exact) <= 1e-10
    got = OS.energy(wf, SR.hamiltonian("xxz", N), 64, samples=c, want_eloc=True)
    assert np.isclose(got["mean"], got["eloc"].mean(), rtol=1e-13) and got["err"] > 0.0


@pytest.mark.parametrize("f64,shape,units", [(True, (3, 2), (10, 10)), (False, (34, 1), (10, 10)), (False, (10, 1), (68, 68))],
                         ids=["f64-3x2-10x10", "f32-34-10x10", "f32-10-68x68"])
def test_bit_exact_identities(f64, shape, units, monkeypatch):
    from rnnwavefunctions_amd import _lib
    N = shape[0] * shape[1]
    ns = 600
    prm = weights(f64, units)
    ham = SR.hamiltonian("mixed", N)
    args = (ham.flip, ham.sign, ham.coeff)
    wf = make_wf(f64, shape, units, prm)
    # drawn samples are rnnwf_sample's at the same (seed, step, offset)
    drawn = wf.pauli_step_stack(*args, ns, seed=5, step=3, sample_offset=7, want_eloc=True, want_log_ratio=True, want_samples=True)
    s = wf.sample(ns, seed=5, step=3, sample_offset=7).reshape(ns, N)
    assert np.array_equal(drawn["samples"].reshape(ns, N), s)
    # ... and the call on them as caller-supplied samples gives the same; a repeated call is bit-identical
    one = wf.pauli_step_stack(*args, ns, samples=s, want_eloc=True, want_log_ratio=True)
    again = wf.pauli_step_stack(*args, ns, samples=s, want_eloc=True, want_log_ratio=True)
    for k in ("eloc", "log_ratio", "term_sums", "moments"):
        assert np.array_equal(one[k], drawn[k]) and np.array_equal(one[k], again[k]), k
    assert wf.resident_samples() == ns
    # the gradient of the resident batch is the gradient after load_batch(samples, eloc) on a fresh handle, every tensor.  The
    # float32 stacks of up to 52 units take the cooperative base kernel in load_batch, whose accumulation order is its own
    # (docs/pauli_stack.md): the fresh handle keeps the one-wave kernel there, as the stack entries always do
    m = one["moments"]
    g = T.cost_gradient(wf, prm, SCOPE, m[0] / m[2], m[2])
    if not f64 and max(units) <= 52:
        monkeypatch.setenv("RNNWF_NO_COOP", "1")
    fresh = make_wf(f64, shape, units, prm)
    monkeypatch.delenv("RNNWF_NO_COOP", raising=False)
    fresh.load_batch(s, one["eloc"])
    g_ref = T.cost_gradient(fresh, prm, SCOPE, m[0] / m[2], m[2])
    assert set(g) == set(g_ref) == set(prm)
    for k in g:
        assert np.array_equal(g[k], g_ref[k]) and np.abs(g[k]).max() > 0.0, k
    # several passes under a small state budget: E_loc and log-ratios bit for bit, sums and moments added in pass order
    monkeypatch.setenv("RNNWF_STATE_BUDGET_MB", "1")
    many = make_wf(f64, shape, units, prm)
    monkeypatch.delenv("RNNWF_STATE_BUDGET_MB")
    kt = 4 * next(nf for nf in (1, 2, 3, 4, 6) if 16 * nf + 4 >= max(units)) + 1          # k-steps of a hidden vector: 4 NFULL + 1
    nmasks = len({r.tobytes() for r in ham.flip if r.any()})
    per_block = N * len(units) * kt * 64 * (8 if f64 else 4) + (N + 2 + 2 * nmasks) * 16 * 8
    chains = max(1, (1 << 20) // per_block) * 16
    print("[passes %s] %d bytes per block: %d chains per pass, %d passes" % (units, per_block, chains, -(-ns // chains)))
    assert chains < ns
    multi = many.pauli_step_stack(*args, ns, samples=s, want_eloc=True, want_log_ratio=True)
    assert many.resident_samples() == 0                       # several passes leave no batch
    assert np.array_equal(multi["eloc"], one["eloc"]) and np.array_equal(multi["log_ratio"], one["log_ratio"])
    sums, mom = np.zeros_like(one["term_sums"]), np.zeros(4)
    for k in range(0, ns, chains):
        part = wf.pauli_step_stack(*args, len(s[k:k + chains]), samples=s[k:k + chains])
        sums += part["term_sums"]
        mom[:3] += part["moments"][:3]
    assert np.array_equal(multi["term_sums"], sums) and np.array_equal(multi["moments"], mom)
    assert np.allclose(multi["term_sums"], one["term_sums"], rtol=1e-13, atol=0)
    # a mask with f = 0 runs all N sites from the zero states in the base pass's arithmetic: where rnnwf_log_prob takes the same
    # one-wave kernel (float64, and float32 above 52 units) log r is 1/2 (log P(sigma ^ m) - log P(sigma)) of rnnwf_log_prob bit for bit
    if f64 or max(units) > 52:
        masks, _ = O.group_by_mask(ham.flip)
        own = wf.log_prob(s)
        hits = 0
        for m_, row in zip(masks, one["log_ratio"]):
            if m_[0]:
                assert np.array_equal(row, 0.5 * (wf.log_prob(s ^ m_[None, :].astype(s.dtype)) - own))
                hits += 1
        assert hits >= 3


# ---- training ------------------------------------------------------------------------------------------------------------------------
K = 4
LRS = [5e-3, 2e-2, 1e-3, 7e-3]
TRAIN_CASES = [(False, (10, 1), (10, 10)), (False, (10, 1), (37, 37)), (True, (3, 2), (10, 10, 10))]


def train_weights(f64, units):
    return weights(f64, units, seed=5, sharp=2.0)


def host_loop(wf, ham, prm, ns, seed, lrs, step0=0):
    """the host loop: (moments (K, 4), term sums (K, nterms, 2), parameters, the optimizer)"""
    opt = T.Adam()
    params = {k: np.array(v) for k, v in prm.items()}
    wf.set_params(params, scope=SCOPE)
    moms, sums = [], []
    for k, lr in enumerate(lrs):
        out = wf.pauli_step_stack(ham.flip, ham.sign, ham.coeff, ns, seed=seed, step=step0 + k)
        s1, s2, n, _ = out["moments"]
        moms.append(out["moments"].copy())
        sums.append(out["term_sums"].copy())
        grads = T.cost_gradient(wf, params, SCOPE, s1 / n, n)
        params = opt.step(params, grads, lr)
        wf.set_params(params, scope=SCOPE)
    return np.array(moms), np.array(sums), params, opt


def assert_state_equals(wf, prm_like, params, opt):
    got = wf.get_params_dict(prm_like, SCOPE)
    for k in params:
        assert got[k].dtype == params[k].dtype and np.array_equal(got[k], params[k]), k
    m, v, t = wf.adam_get_state()
    m0, v0 = opt.to_flat(wf, params, SCOPE)
    assert t == opt.t and np.array_equal(m, m0) and np.array_equal(v, v0)


def reset(wf, prm):
    wf.set_params(prm, scope=SCOPE)
    wf.adam_set_state(None, None, 0)


@pytest.fixture(scope="module")
def trajectories():
    """the host loop's trajectory of every case, computed once: {case: (prm, moments, sums, params, opt)}"""
    cache = {}

    def get(case):
        if case not in cache:
            f64, shape, units = case
            prm = train_weights(f64, units)
            wf = make_wf(f64, shape, units, prm)
            cache[case] = (prm,) + host_loop(wf, SR.hamiltonian("mixed", shape[0] * shape[1]), prm, NS, 11, LRS)
            wf.close()
        return cache[case]
    return get


@pytest.mark.parametrize("case", TRAIN_CASES, ids=lambda c: "%s-%dx%d-%s" % ("f64" if c[0] else "f32", c[1][0], c[1][1], "x".join(map(str, c[2]))))
def test_trajectory_equals_the_host_loop_bit_for_bit(case, trajectories):
    f64, shape, units = case
    prm, moms, sums, params, opt = trajectories(case)
    ham = SR.hamiltonian("mixed", shape[0] * shape[1])
    args = (ham.flip, ham.sign, ham.coeff)
    wf = make_wf(f64, shape, units, prm)
    out = wf.pauli_train_steps_stack(*args, NS, 11, 0, LRS, want_term_sums=True)
    assert np.all(np.isfinite(moms)) and moms[:, 1].min() > 0.0 and not np.array_equal(moms[0], moms[-1])
    assert np.array_equal(out["moments"], moms)
    assert out["term_sums"].shape == (K, len(ham.coeff), 2) and np.array_equal(out["term_sums"], sums)
    assert wf.resident_samples() == 0 and wf.adam_get_state()[2] == K
    assert_state_equals(wf, prm, params, opt)
    # one call of four iterations equals four calls of one
    reset(wf, prm)
    rows = [wf.pauli_train_steps_stack(*args, NS, 11, k, [LRS[k]], want_term_sums=True) for k in range(K)]
    assert np.array_equal(np.array([r["moments"][0] for r in rows]), moms)
    assert np.array_equal(np.array([r["term_sums"][0] for r in rows]), sums)
    assert_state_equals(wf, prm, params, opt)
    # the device parameters are current: the next step runs on them
    nxt = wf.pauli_step_stack(*args, NS, seed=11, step=K)
    ref = make_wf(f64, shape, units, params).pauli_step_stack(*args, NS, seed=11, step=K)
    assert np.array_equal(nxt["moments"], ref["moments"]) and wf.resident_samples() == NS


def test_minimize_hamiltonian_device_steps_equals_the_host_loop():
    f64, shape, units = TRAIN_CASES[0]
    prm = train_weights(f64, units)
    ham = SR.hamiltonian("mixed", shape[0])
    wf = make_wf(f64, shape, units, prm)
    mean, var = OS.minimize_hamiltonian(wf, ham, prm, numsteps=K - 1, numsamples=NS, learningrate=1e-2, seed=111)
    p_h = OS.minimize_hamiltonian.last_params
    mean_d, var_d = OS.minimize_hamiltonian(wf, ham, prm, numsteps=K - 1, numsamples=NS, learningrate=1e-2, seed=111, device_steps=2)
    p_d = OS.minimize_hamiltonian.last_params
    assert len(mean) == K and mean_d == mean and var_d == var
    assert all(np.array_equal(p_d[k], p_h[k]) and p_d[k].dtype == p_h[k].dtype for k in p_h)
    assert any(not np.array_equal(p_h[k], prm[k]) for k in prm)


def test_minimize_hamiltonian_lowers_the_energy_towards_the_ground_state():
    """N = 6 XXZ chain (ferromagnetic XY coupling) in a transverse field, two layers of 10 units: stoquastic, so the ground state is
    positive.  The criteria are those of tests/test_gpu_pauli.py's one-layer test: the energy falls by more than five standard errors
    and does not end below the exact ground energy by more than five."""
    N, units, ns, steps = 6, (10, 10), 1000, 150
    ham = O.Hamiltonian(N, O.xxz_hamiltonian(N, -1.0, 0.5).terms + [(-0.8, [("X", i)]) for i in range(N)])
    e0 = np.linalg.eigvalsh(SR.dense(ham))[0]
    prm = P.init_gru_params(list(units), seed=111)
    wf = make_wf(False, (N, 1), units, prm)
    mean, var = OS.minimize_hamiltonian(wf, ham, prm, numsteps=steps, numsamples=ns, learningrate=5e-3, seed=111, device_steps=64)
    assert len(mean) == len(var) == steps + 1
    err_i, err_f = np.sqrt(var[0] / ns), np.sqrt(var[-1] / ns)
    print("minimize_hamiltonian stack: E %.4f +- %.4f -> %.4f +- %.4f, ground state %.4f" % (mean[0], err_i, mean[-1], err_f, e0))
    assert mean[-1] < mean[0] - 5.0 * np.hypot(err_i, err_f)
    assert mean[-1] >= e0 - 5.0 * err_f
    assert mean[-1] <= e0 + 0.05 * abs(e0)                    # and it has come most of the way: within 5 % of the ground energy


# ---- refusals ------------------------------------------------------------------------------------------------------------------------

def test_refusals_happen_before_any_work_and_leave_the_batch_usable():
    from rnnwavefunctions_amd import _lib
    N, units = 6, (10, 10)
    prm = weights(False, units)
    ham = SR.hamiltonian("xxz", N)
    args = (ham.flip, ham.sign, ham.coeff)
    wf = make_wf(False, (N, 1), units, prm)
    ok = wf.pauli_step_stack(*args, NS, seed=1, step=2)
    m = ok["moments"]
    g0 = T.cost_gradient(wf, prm, SCOPE, m[0] / m[2], m[2])

    def untouched():
        g1 = T.cost_gradient(wf, prm, SCOPE, m[0] / m[2], m[2])
        return wf.resident_samples() == NS and all(np.array_equal(g0[k], g1[k]) for k in g0) and wf.adam_get_state()[2] == 0
    step, train = wf.pauli_step_stack, wf.pauli_train_steps_stack
    bad = ham.flip.copy()
    bad[1, 3] = 2
    for call, entry, word in [
            (lambda: step(*args, 0), STEP_ENTRY, "ns must be"), (lambda: step(*args, NS, sample_offset=-1), STEP_ENTRY, "sample_offset"),
            (lambda: step(bad, ham.sign, ham.coeff, NS), STEP_ENTRY, r"flip\[1\]\[3\] = 2"),
            (lambda: train(bad, ham.sign, ham.coeff, NS, 1, 0, [1e-2]), TRAIN_ENTRY, r"flip\[1\]\[3\] = 2"),
            (lambda: train(*args, NS, 1, 0, []), TRAIN_ENTRY, "K must be"), (lambda: train(*args, NS, 1, 0, [1e-2] * 1025), TRAIN_ENTRY, "K must be"),
            (lambda: train(*args, 0, 1, 0, [1e-2]), TRAIN_ENTRY, "numsamples"), (lambda: train(*args, NS, 1, 0, [np.nan]), TRAIN_ENTRY, "finite")]:
        with pytest.raises(ValueError, match=entry + ": .*" + word):
            call()
        assert untouched()
    # null pointers and nterms = 0 through the C entries
    I32P, F64P = _lib._I32P, _lib._F64P
    fl, sg = np.ascontiguousarray(ham.flip, dtype=np.int32), np.ascontiguousarray(ham.sign, dtype=np.int32)
    co = np.ascontiguousarray(ham.coeff, dtype=np.float64)
    sums, mom, lr = np.zeros((len(fl), 2)), np.zeros((1, 4)), np.array([1e-2])
    full_step = [fl.ctypes.data_as(I32P), sg.ctypes.data_as(I32P), co.ctypes.data_as(F64P), len(fl), None, NS, 1, 0, 0,
                 sums.ctypes.data_as(F64P), None, None, None, None]
    full_train = [fl.ctypes.data_as(I32P), sg.ctypes.data_as(I32P), co.ctypes.data_as(F64P), len(fl), 1, NS, 1, 0, 0, lr.ctypes.data_as(F64P),
                  0.9, 0.999, 1e-8, mom.ctypes.data_as(F64P), None, None]
    for fn, entry, full, nulls in [(wf.lib.rnnwf_pauli_step_stack, STEP_ENTRY, full_step, (0, 1, 2, 9)),
                                   (wf.lib.rnnwf_pauli_train_steps_stack, TRAIN_ENTRY, full_train, (0, 1, 2, 9, 13))]:
        for idx, value, word in [(i, None, "non-null") for i in nulls] + [(3, 0, "nterms")]:
            a = list(full)
            a[idx] = value
            assert fn(wf.h, *a) == -1
            msg = wf.lib.rnnwf_last_error(wf.h).decode()
            assert msg.startswith(entry + ": ") and re.search(word, msg), msg
        assert untouched()
    # one-layer handles, with the pointer to the entry that serves them; that entry keeps refusing the stack
    for model, nx, ny in [(_lib.MODEL_GRU1D, N, 1), (_lib.MODEL_GRU1D_F64, 3, 2)]:
        w = _lib.NativeWavefunction(model, nx, ny, (10,))
        w.init_params(1)
        with pytest.raises(ValueError, match=STEP_ENTRY + ": .*one layer; rnnwf_pauli_step serves it"):
            w.pauli_step_stack(*args, NS)
        with pytest.raises(ValueError, match=TRAIN_ENTRY + ": .*one layer; rnnwf_pauli_train_steps serves it"):
            w.pauli_train_steps_stack(*args, NS, 1, 0, [1e-2])
        assert w.resident_samples() == 0
    with pytest.raises(ValueError, match="rnnwf_pauli_step: not implemented for stacked layers"):
        wf.pauli_step(*args, NS)
    with pytest.raises(ValueError, match="rnnwf_pauli_train_steps: not implemented for stacked layers"):
        wf.pauli_train_steps(*args, NS, 1, 0, [1e-2])
    assert untouched()
    # the other models, in the existing entries' words
    for model, nx, ny, un, word in [(_lib.MODEL_GRU1D_PARITY, N, 1, (10,), "parity"), (_lib.MODEL_CRNN_U1, N, 1, (10, 10), "complex RNN"),
                                    (_lib.MODEL_MDRNN2D, 3, 2, (10,), "MDRNN"), (_lib.MODEL_LSTM1D_F64, 3, 2, (10,), "LSTM")]:
        w = _lib.NativeWavefunction(model, nx, ny, un)
        w.init_params(1)
        with pytest.raises(ValueError, match=STEP_ENTRY + ": .*" + word):
            w.pauli_step_stack(*args, NS)
        with pytest.raises(ValueError, match=TRAIN_ENTRY + ": .*" + word):
            w.pauli_train_steps_stack(*args, NS, 1, 0, [1e-2])
    # uncommitted parameters
    fresh = _lib.NativeWavefunction(_lib.MODEL_GRU1D, N, 1, units)
    for call in (lambda: fresh.pauli_step_stack(*args, NS), lambda: fresh.pauli_train_steps_stack(*args, NS, 1, 0, [1e-2])):
        with pytest.raises(_lib.RnnwfError, match="not committed") as e:
            call()
        assert not isinstance(e.value, ValueError)
    # a communicator on the train entry
    wc = make_wf(False, (N, 1), units, prm)
    wc.comm_init(wc.comm_unique_id(), 0, 1)
    with pytest.raises(ValueError, match=TRAIN_ENTRY + ": .*communicator"):
        wc.pauli_train_steps_stack(*args, NS, 1, 0, [1e-2])
    # the Python layer: a one-layer wave function never reaches the library
    one = _lib.NativeWavefunction(_lib.MODEL_GRU1D, N, 1, (10,))
    with pytest.raises(ValueError, match="one layer; observables.py"):
        OS.energy(one, ham, NS)
    assert untouched()
