"""Device-resident Adam training of the LSTM wave function (rnnwf_lstm_train_steps, rnnwf_lstm_pauli_train_steps; docs/lstm.md,
"Device-resident training") on the GPU, against the host loop it replaces: lstm_vmc_gradient_step / lstm_pauli_gradient_step ->
training.Adam -> set_params.  The two perform the same IEEE operations in the same order, so every comparison is np.array_equal, as
tests/test_gpu_training.py has them for the other families.

Weights: tests/lstm_grad_reference.parameters (init_lstm_params, kernels x 3, every bias randomised, so that no bias row of the image is
a plain zero); 40 samples (two full 16-chain blocks and a ragged one of 8); Bx = 2.  Widths 10, 20, 21, 36, 37, 52, 53, 68: NFULL 1..4,
each at its narrowest and its widest mixed tile, the backward operand in LDS and streamed.
"""
import os

import numpy as np
import pytest

import lstm_grad_reference as LG

pytestmark = pytest.mark.gpu
SCOPE = LG.SCOPE
NS = LG.NS
WIDTHS = (10, 20, 21, 36, 37, 52, 53, 68)
SEED = 333
LR0 = np.float64(1e-2)


def lr_of_it(lr0, it):
    return 1.0 / ((1.0 / lr0) + it / 10)


def rates(first, K):
    return [float(lr_of_it(LR0, it)) for it in range(first, first + K)]


def handle(shape, units, prm=None):
    from rnnwavefunctions_amd import _lib
    wf = _lib.NativeWavefunction(_lib.MODEL_LSTM1D_F64, shape[0], shape[1], (units,))
    if prm is not None:
        wf.set_params(prm, scope=SCOPE)
    return wf


def couplings(shape, Bx=2.0):
    return np.append(np.ones(shape[0] * shape[1]), Bx)


def copy(prm):
    return {k: np.array(v) for k, v in prm.items()}


def host_iterations(wf, prm, shape, first, count, opt):
    """`count` iterations of training_lstm's host loop from iteration `first` on the handle that holds `prm`: (moments rows, params)"""
    prm = copy(prm)
    rows = []
    for it in range(first, first + count):
        out = wf.lstm_vmc_gradient_step(NS, seed=SEED, step=it, couplings=couplings(shape), shapes=LG.shapes(prm))
        rows.append(out["moments"].copy())
        prm = opt.step(prm, LG.scoped(out["grads"]), lr_of_it(LR0, it))
        wf.set_params(prm, scope=SCOPE)
    return np.array(rows), prm


_host = {}


def host_trajectory(shape, units, count):
    """the host loop's first `count` iterations at (shape, units), computed once: (moments, params, m, v, t)"""
    from rnnwavefunctions_amd import training
    key = (shape, units, count)
    if key not in _host:
        prm = LG.parameters(units)
        wf = handle(shape, units, prm)
        opt = training.Adam()
        rows, out = host_iterations(wf, prm, shape, 0, count, opt)
        m, v = opt.to_flat(wf, out, SCOPE)
        wf.close()
        for a in (rows, m, v) + tuple(out.values()):
            a.setflags(write=False)
        _host[key] = (rows, out, m, v, opt.t)
    return _host[key]


def same_params(a, b):
    assert set(a) == set(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def fixed_configurations(N, n=NS, seed=5):
    return np.random.RandomState(seed).randint(0, 2, size=(n, N)).astype(np.int32)


def images_agree(wf, shape, units, prm):
    """the device-re-packed images of `wf` against a fresh handle that set_params the read-back parameters: log_prob reads the forward
    image (every BINIT variant, the forget bias, the head difference), lstm_gradient the backward operand as well"""
    N = shape[0] * shape[1]
    s = fixed_configurations(N)
    w = LG.weights(NS)
    back = wf.get_params_dict(prm, SCOPE)
    fresh = handle(shape, units, back)
    lp_dev, lp_host = wf.log_prob(s), fresh.log_prob(s)
    g_dev, g_host = wf.lstm_gradient(s, w, LG.shapes(prm)), fresh.lstm_gradient(s, w, LG.shapes(prm))
    fresh.close()
    assert np.all(np.isfinite(lp_dev)) and np.array_equal(lp_dev, lp_host)
    for k in g_host:
        assert np.any(g_host[k] != 0.0), k
        assert np.array_equal(g_dev[k], g_host[k]), k
    return back


@pytest.mark.parametrize("units", WIDTHS)
def test_trajectory_and_repacked_images(units):
    """five iterations as K = 2 then K = 3 (adam_t carries over) against five of the host loop; then both re-packed images"""
    shape = (3, 3)
    rows, ref, m_ref, v_ref, t_ref = host_trajectory(shape, units, 5)
    prm = LG.parameters(units)
    wf = handle(shape, units, prm)
    mom = np.concatenate([wf.lstm_train_steps(NS, SEED, 0, couplings(shape), rates(0, 2)),
                          wf.lstm_train_steps(NS, SEED, 2, couplings(shape), rates(2, 3))])
    assert mom.shape == (5, 4) and np.array_equal(mom, rows)
    assert np.all(mom[:, 2] == NS) and len({r.tobytes() for r in mom}) == 5            # five different batches
    got = wf.get_params_dict(prm, SCOPE)
    same_params(got, ref)
    assert any(not np.array_equal(got[k], prm[k]) for k in prm)
    m, v, t = wf.adam_get_state()
    assert t == t_ref == 5 and np.array_equal(m, m_ref) and np.array_equal(v, v_ref)
    same_params(images_agree(wf, shape, units, prm), ref)
    wf.close()


def test_repacked_images_beyond_two_spin_words():
    """13 x 5 (65 sites: the second spin word, the refetch at site 64), 37 units, K = 2"""
    shape, units = (13, 5), 37
    rows, ref, _, _, _ = host_trajectory(shape, units, 2)
    prm = LG.parameters(units)
    wf = handle(shape, units, prm)
    mom = wf.lstm_train_steps(NS, SEED, 0, couplings(shape), rates(0, 2))
    assert np.array_equal(mom, rows)
    same_params(images_agree(wf, shape, units, prm), ref)
    wf.close()


@pytest.mark.parametrize("units", [10, 37])
def test_hand_over_between_host_and_device(units):
    from rnnwavefunctions_amd import training
    shape = (3, 3)
    rows, ref, m_ref, v_ref, _ = host_trajectory(shape, units, 4)
    prm = LG.parameters(units)
    # device, then host with Adam seeded from the device's state
    wf = handle(shape, units, prm)
    mom = wf.lstm_train_steps(NS, SEED, 0, couplings(shape), rates(0, 2))
    mid = wf.get_params_dict(prm, SCOPE)
    opt = training.Adam()
    opt.from_flat(wf, mid, SCOPE, *wf.adam_get_state())
    assert opt.t == 2
    rows_h, out = host_iterations(wf, mid, shape, 2, 2, opt)
    assert np.array_equal(np.concatenate([mom, rows_h]), rows)
    same_params(out, ref)
    wf.close()
    # host, then the device with the host's state
    wf = handle(shape, units, prm)
    opt = training.Adam()
    rows_h, mid = host_iterations(wf, prm, shape, 0, 2, opt)
    wf.adam_set_state(*opt.to_flat(wf, mid, SCOPE), opt.t)
    mom = wf.lstm_train_steps(NS, SEED, 2, couplings(shape), rates(2, 2))
    assert np.array_equal(np.concatenate([rows_h, mom]), rows)
    same_params(wf.get_params_dict(prm, SCOPE), ref)
    m, v, t = wf.adam_get_state()
    assert t == 4 and np.array_equal(m, m_ref) and np.array_equal(v, v_ref)
    # set_params after device steps: the next device call starts from the new host values (and from the state it is given)
    wf.set_params(prm, scope=SCOPE)
    same_params(wf.get_params_dict(prm, SCOPE), prm)
    wf.adam_set_state(None, None, 0)
    mom = wf.lstm_train_steps(NS, SEED, 0, couplings(shape), rates(0, 4))
    assert np.array_equal(mom, rows)
    same_params(wf.get_params_dict(prm, SCOPE), ref)
    wf.close()


@pytest.mark.parametrize("units", [10, 37])
def test_pauli_trajectory(units):
    """an XXZ chain along the raster path of 3 x 2, K = 3, against three iterations of observables_lstm.minimize_hamiltonian's loop"""
    from rnnwavefunctions_amd import observables_lstm as OL
    from rnnwavefunctions_amd import training, training_lstm
    shape, numsteps, lr = (3, 2), 2, 2e-2
    ham = OL.xxz_hamiltonian(6, -1.0, 0.5)
    prm = LG.parameters(units)
    # the host loop with its term sums: minimize_loop's iterations (the fused call, Adam, set_params)
    wf = handle(shape, units, prm)
    opt, p, rows, sums = training.Adam(), copy(prm), [], []
    for it in range(numsteps + 1):
        out = wf.lstm_pauli_gradient_step(ham.flip, ham.sign, ham.coeff, NS, seed=SEED, step=it, shapes=LG.shapes(p))
        rows.append(out["moments"].copy())
        sums.append(out["term_sums"].copy())
        p = opt.step(p, LG.scoped(out["grads"]), OL.lr_schedule(lr, it))
        wf.set_params(p, scope=SCOPE)
    wf.close()
    rows, sums = np.array(rows), np.array(sums)
    # ... which is what the public function runs
    wf = handle(shape, units)
    mean_h, var_h = OL.minimize_hamiltonian(wf, ham, prm, numsteps=numsteps, numsamples=NS, learningrate=lr, seed=SEED)
    same_params(OL.minimize_hamiltonian.last_params, p)
    assert np.array_equal(mean_h, rows[:, 0] / rows[:, 2])
    wf.close()
    # the entry
    wf = handle(shape, units, prm)
    out = wf.lstm_pauli_train_steps(ham.flip, ham.sign, ham.coeff, NS, SEED, 0, [float(OL.lr_schedule(lr, it)) for it in range(3)],
                                    want_term_sums=True, want_eloc=True)
    assert np.array_equal(out["moments"], rows)
    assert out["term_sums"].shape == sums.shape and np.array_equal(out["term_sums"], sums)
    assert out["eloc"].shape == (NS,) and np.all(np.isfinite(out["eloc"]))
    assert out["eloc"].sum() == pytest.approx(rows[2, 0], rel=1e-12)                       # the last iteration's batch
    same_params(wf.get_params_dict(prm, SCOPE), p)
    assert wf.adam_get_state()[2] == 3
    wf.close()
    # the driver on that entry, cut into blocks of 2
    wf = handle(shape, units)
    mean_d, var_d = training_lstm.minimize_hamiltonian_device(wf, ham, prm, numsteps=numsteps, numsamples=NS, learningrate=lr, seed=SEED,
                                                              device_steps=2)
    assert mean_d == mean_h and var_d == var_h
    same_params(training_lstm.minimize_hamiltonian_device.last_params, p)
    wf.close()


def test_driver_with_device_steps(tmp_path):
    from rnnwavefunctions_amd import training_lstm
    kw = dict(numsteps=12, systemsize_x=3, systemsize_y=3, num_units=10, numsamples=40, verbose=False)
    (tmp_path / "host").mkdir()
    (tmp_path / "device").mkdir()
    mean_h, var_h = training_lstm.run_2DTFIM_1DRNN_LSTM(save_dir=str(tmp_path / "host"), **kw)
    last_h = training_lstm.run_2DTFIM_1DRNN_LSTM.last_params
    mean_d, var_d = training_lstm.run_2DTFIM_1DRNN_LSTM(save_dir=str(tmp_path / "device"), device_steps=5, **kw)
    last_d = training_lstm.run_2DTFIM_1DRNN_LSTM.last_params
    assert len(mean_h) == 13 and mean_d == mean_h and var_d == var_h
    same_params(last_d, last_h)
    names = sorted(os.listdir(tmp_path / "host"))
    assert names == sorted(os.listdir(tmp_path / "device")) and len(names) >= 3
    for name in names:
        a, b = (tmp_path / "host" / name).read_bytes(), (tmp_path / "device" / name).read_bytes()
        assert a == b, name


def test_refusals():
    from rnnwavefunctions_amd import _lib
    from rnnwavefunctions_amd import observables_lstm as OL
    from rnnwavefunctions_amd import params as P
    shape, units = (3, 3), 10
    N = 9
    prm = LG.parameters(units)
    ham = OL.tfim_hamiltonian(np.ones(shape), 2.0)
    terms = (ham.flip, ham.sign, ham.coeff)
    # a non-LSTM handle
    gru = _lib.NativeWavefunction(_lib.MODEL_GRU1D_F64, shape[0], shape[1], (units,))
    gru.set_params(P.init_gru_params([units], seed=111, dtype=np.float64), scope=SCOPE)
    with pytest.raises(ValueError, match="rnnwf_lstm_train_steps: needs an LSTM1D_F64 handle"):
        gru.lstm_train_steps(NS, 1, 0, couplings(shape), [1e-3])
    with pytest.raises(ValueError, match="rnnwf_lstm_pauli_train_steps: needs an LSTM1D_F64 handle"):
        gru.lstm_pauli_train_steps(*terms, NS, 1, 0, [1e-3])
    gru.close()
    # parameters not committed
    wf = handle(shape, units)
    with pytest.raises(_lib.RnnwfError, match="parameters not committed"):
        wf.lstm_train_steps(NS, 1, 0, couplings(shape), [1e-3])
    with pytest.raises(_lib.RnnwfError, match="parameters not committed"):
        wf.lstm_pauli_train_steps(*terms, NS, 1, 0, [1e-3])
    # K outside 1..1024, a wrong number of couplings, a learning rate that is not finite: nothing is touched
    wf.set_params(prm, scope=SCOPE)
    for K in (0, 1025):
        with pytest.raises(ValueError, match=r"rnnwf_lstm_train_steps: K must be 1\.\.1024"):
            wf.lstm_train_steps(NS, 1, 0, couplings(shape), np.full(K, 1e-3))
        with pytest.raises(ValueError, match=r"rnnwf_lstm_pauli_train_steps: K must be 1\.\.1024"):
            wf.lstm_pauli_train_steps(*terms, NS, 1, 0, np.full(K, 1e-3))
    with pytest.raises(ValueError, match="wrong number of couplings"):
        wf.lstm_train_steps(NS, 1, 0, np.ones(N), [1e-3])
    with pytest.raises(ValueError, match="must be finite"):
        wf.lstm_train_steps(NS, 1, 0, couplings(shape), [1e-3, np.nan])
    same_params(wf.get_params_dict(prm, SCOPE), prm)
    assert wf.adam_get_state()[2] == 0
    # a served call, then the refusals tests/test_gpu_lstm.py pins, on the same handle
    mom = wf.lstm_train_steps(NS, SEED, 0, couplings(shape), rates(0, 2))
    assert np.array_equal(mom, host_trajectory(shape, units, 5)[0][:2])
    with pytest.raises(ValueError, match="no gradient for the LSTM cell"):
        wf.adam_step(1e-3)
    with pytest.raises(ValueError, match="no gradient for the LSTM cell"):
        wf.train_steps(20, 1, 0, couplings(shape), [1e-3])
    with pytest.raises(ValueError, match="no gradient for the LSTM cell"):
        wf.vmc_gradient(0.0, 1.0, LG.shapes(prm))
    with pytest.raises(ValueError, match="no gradient for the LSTM cell"):
        wf.load_batch(np.zeros((4, N), dtype=np.int32), np.zeros(4))
    assert wf.device_training_supported() is False
    assert wf.resident_samples() == 0
    # a handle with a communicator
    wf.comm_init(wf.comm_unique_id(), 0, 1)
    with pytest.raises(ValueError, match="rnnwf_lstm_train_steps: single process only"):
        wf.lstm_train_steps(NS, 1, 0, couplings(shape), [1e-3])
    with pytest.raises(ValueError, match="rnnwf_lstm_pauli_train_steps: single process only"):
        wf.lstm_pauli_train_steps(*terms, NS, 1, 0, [1e-3])
    wf.close()
    # past the state budget: 1 MB holds 25 blocks of 8 checkpoints x 5 120 B = 400 chains at 9 sites and 10 units
    assert "RNNWF_STATE_BUDGET_MB" not in os.environ
    os.environ["RNNWF_STATE_BUDGET_MB"] = "1"                 # read once per handle, at creation
    try:
        small = handle(shape, units, prm)
    finally:
        del os.environ["RNNWF_STATE_BUDGET_MB"]
    with pytest.raises(_lib.RnnwfError, match="rnnwf_lstm_train_steps: 500 samples exceed the state budget of one pass; split the batch"):
        small.lstm_train_steps(500, 1, 0, couplings(shape), [1e-3])
    with pytest.raises(_lib.RnnwfError, match="rnnwf_lstm_pauli_train_steps: 500 samples exceed the state budget of one pass; split the batch"):
        small.lstm_pauli_train_steps(*terms, 500, 1, 0, [1e-3])
    same_params(small.get_params_dict(prm, SCOPE), prm)
    assert np.array_equal(small.lstm_train_steps(NS, SEED, 0, couplings(shape), rates(0, 2)), mom)         # what fits still runs
    small.close()
