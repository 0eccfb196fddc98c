"""GPU tests of the LSTM wave function over the raster path (model LSTM1D_F64, csrc/lstm_kernels.h) through the C ABI and the
reference-named facade, against the NumPy float64 restatement in tests/lstm_reference.py.

Tolerances (float64 throughout; only summation order, the folded forget bias and exp/tanh to ~1e-16 differ):
  log P(sigma) : |hip - reference| <= 1e-11 * N
  E_loc        : relative 1e-10;  every row of the log-probability queue: absolute 1e-10
  samples      : identical rows except near-ties |u - p0| < 1e-12 (counted, at most 2)
"""
import numpy as np
import pytest

from conftest import all_configs
from lstm_reference import LSTM, lstm_log_probability, lstm_sample
from oracle import estimators as E
from oracle import philox
from rnnwavefunctions_amd import params as P

pytestmark = pytest.mark.gpu

SCOPE = "RNNwavefunction"


def trained_like(H, seed, scale=1.8):
    return P.randomize_biases(P.scale_kernels(P.init_lstm_params([H], seed=seed), scale), seed + 1)


def make_wf(Nx, Ny, H, prm):
    from rnnwavefunctions_amd import _lib
    wf = _lib.NativeWavefunction(_lib.MODEL_LSTM1D_F64, Nx, Ny, (H,))
    wf.set_params(prm, scope=SCOPE)
    return wf


def random_samples(B, N, seed):
    return np.random.RandomState(seed).randint(0, 2, size=(B, N)).astype(np.int32)


# every NFULL (1..4) and every width of the mixed tile's remainder (0..4 units), on square and non-square lattices
@pytest.mark.parametrize("H,Nx,Ny", [(1, 2, 2), (4, 3, 2), (5, 2, 5), (10, 4, 4), (16, 3, 7), (17, 5, 5), (20, 6, 4), (21, 2, 9),
                                     (36, 7, 7), (37, 4, 6), (50, 10, 10), (52, 5, 8), (53, 9, 3), (64, 8, 8), (68, 10, 7)])
def test_log_prob_matches_the_reference(H, Nx, Ny):
    N = Nx * Ny
    prm = trained_like(H, seed=H, scale=1.5 if H > 40 else 2.0)
    wf = make_wf(Nx, Ny, H, prm)
    s = random_samples(37, N, seed=H)
    got = wf.log_prob(s)
    ref = lstm_log_probability(prm, s, Nx, Ny)
    err = np.abs(got - ref).max()
    print("LSTM %dx%d H=%d: max |lp - ref| = %.2e (|lp| ~ %.1f)" % (Nx, Ny, H, err, np.abs(ref).mean()))
    assert err <= 1e-11 * N


def test_normalised_over_all_configurations_of_4x4():
    prm = trained_like(10, seed=3)
    wf = make_wf(4, 4, 10, prm)
    lp = wf.log_prob(all_configs(16))
    assert abs(np.exp(lp).sum() - 1.0) < 1e-12


@pytest.mark.parametrize("H,Nx,Ny", [(5, 3, 4), (50, 4, 4), (68, 3, 3)])
def test_sampling_matches_the_reference_and_its_own_log_prob(H, Nx, Ny):
    N, ns, seed = Nx * Ny, 1000, 111
    prm = trained_like(H, seed=H + 7)
    wf = make_wf(Nx, Ny, H, prm)
    s, lg = wf.sample(ns, seed=seed, step=2, return_log=True)
    u = philox.uniforms(seed, 2, 0, ns, N)
    ref, ref_lp, p0 = lstm_sample(prm, Nx, Ny, u)
    differ = np.flatnonzero((s != ref).any(axis=1))
    for r in differ:                         # a row may only differ after a near-tie draw
        n = int(np.flatnonzero(s[r] != ref[r])[0])
        assert abs(u[r, n] - p0[r, n]) < 1e-12, "row %d differs at site %d away from a tie" % (r, n)
    assert len(differ) <= 2
    same = np.setdiff1d(np.arange(ns), differ)
    assert np.abs(lg[same] - ref_lp[same]).max() <= 1e-11 * N
    assert np.array_equal(lg, wf.log_prob(s))                              # bit for bit: the same base kernel, same arithmetic
    a, la = wf.sample(300, seed=seed, step=2, sample_offset=0, return_log=True)
    b, lb = wf.sample(700, seed=seed, step=2, sample_offset=300, return_log=True)
    assert np.array_equal(np.concatenate([a, b]), s)
    assert np.array_equal(np.concatenate([la, lb]), lg)


@pytest.mark.parametrize("Nx,Ny,H,ns,Bx", [(3, 3, 10, 64, 2.0), (4, 4, 50, 500, 3.0), (2, 5, 68, 50, 2.0), (5, 3, 20, 33, 3.0)])
def test_tfim2d_eloc_matches_the_reference_estimator(Nx, Ny, H, ns, Bx):
    N = Nx * Ny
    prm = trained_like(H, seed=N + H)
    wf = make_wf(Nx, Ny, H, prm)
    Jz = np.random.RandomState(N).uniform(0.5, 1.5, size=(Nx, Ny))
    s = wf.sample(ns, seed=5, step=0)
    lp = np.zeros((N + 1) * ns)
    e = wf.tfim_eloc(s, Jz, Bx, log_probs=lp)
    e_ref, lp_ref = E.ising2d_local_energies(Jz, Bx, Nx, Ny, s, lambda x: lstm_log_probability(prm, x, Nx, Ny),
                                             return_log_probs=True)
    print("LSTM eloc %dx%d H=%d: max rel |E - ref| = %.2e, max |lp - ref| = %.2e"
          % (Nx, Ny, H, np.abs(e - e_ref).max() / np.abs(e_ref).max(), np.abs(lp.reshape(N + 1, ns) - lp_ref).max()))
    assert np.allclose(e, e_ref, rtol=1e-10, atol=0)
    assert np.allclose(lp.reshape(N + 1, ns), lp_ref, rtol=0, atol=1e-10)


def test_multi_pass_under_the_state_budget_is_bit_identical(monkeypatch):
    Nx, Ny, H, ns, Bx = 4, 4, 50, 500, 3.0
    prm = trained_like(H, seed=21)
    Jz = np.random.RandomState(1).uniform(0.5, 1.5, size=(Nx, Ny))
    one = make_wf(Nx, Ny, H, prm)
    s = one.sample(ns, seed=9, step=0)
    lp1 = np.zeros((Nx * Ny + 1) * ns)
    e1 = one.tfim_eloc(s, Jz, Bx, log_probs=lp1)
    monkeypatch.setenv("RNNWF_STATE_BUDGET_MB", "1")             # 15 checkpoints x 13 KB per 16 chains: 80 chains per pass
    many = make_wf(Nx, Ny, H, prm)
    lp2 = np.zeros_like(lp1)
    e2 = many.tfim_eloc(s, Jz, Bx, log_probs=lp2)
    assert np.array_equal(e1, e2) and np.array_equal(lp1, lp2)
    with pytest.raises(Exception, match="split the batch"):
        many.vmc_step(ns, seed=9, step=0, couplings=np.append(Jz.ravel(), Bx))
    out = many.vmc_step(80, seed=9, step=0, couplings=np.append(Jz.ravel(), Bx))       # within the budget: runs
    assert out["moments"][2] == 80


def test_vmc_step_equals_sample_eloc_and_moments():
    Nx, Ny, H, ns, Bx = 4, 3, 20, 300, 2.0
    prm = trained_like(H, seed=2)
    wf = make_wf(Nx, Ny, H, prm)
    Jz = np.random.RandomState(4).uniform(0.5, 1.5, size=(Nx, Ny))
    wf.timing_enable(True)
    out = wf.vmc_step(ns, seed=77, step=3, couplings=np.append(Jz.ravel(), Bx), want_samples=True, want_eloc=True)
    s = wf.sample(ns, seed=77, step=3)
    assert np.array_equal(out["samples"], s)
    e = wf.tfim_eloc(s, Jz, Bx)
    assert np.array_equal(out["eloc"], e)
    m = out["moments"]
    assert m[2] == ns and np.isclose(m[0], e.sum(), rtol=1e-13) and np.isclose(m[1], (e * e).sum(), rtol=1e-13)
    for kid in (0, 1, 2):                                           # HIP-event timing of base, flip and assembly
        t = wf.timing_get(kid)
        assert t["launches"] >= 1 and t["total_ms"] > 0
    same = np.repeat(s[:1], 40, axis=0)                             # copies of one configuration: identical values
    e_same = wf.tfim_eloc(same, Jz, Bx)
    assert np.all(e_same == e_same[0]) and np.all(wf.log_prob(same) == wf.log_prob(same)[0])


@pytest.mark.parametrize("H,count", [(10, 542), (50, 10702)])
def test_init_params_in_the_library_equals_init_lstm_params(H, count):
    from rnnwavefunctions_amd import _lib
    wf = _lib.NativeWavefunction(_lib.MODEL_LSTM1D_F64, 4, 4, (H,))
    for seed in (111, 7):
        wf.init_params(seed)
        ref = P.init_lstm_params([H], seed=seed)
        assert wf.num_params() == count == P.count_params(ref)
        for name, v in ref.items():
            assert np.array_equal(wf.get_param(name[len(SCOPE) + 1:], v.shape), v), name
    s = wf.sample(8, seed=1, step=0)
    assert np.allclose(wf.log_prob(s), lstm_log_probability(ref, s, 4, 4), rtol=0, atol=1e-11 * 16)


def test_facade_runs_the_reference_call_sequence(tmp_path):
    from rnnwavefunctions_amd import compat as tf
    from rnnwavefunctions_amd.TFIM2D_1DRNN.Training1DRNN_2DTFIM import Ising2D_local_energies, RNNwavefunction
    from rnnwavefunctions_amd import _lib
    Nx, Ny, numsamples, Bx = 4, 4, 200, 3.0
    N = Nx * Ny
    wf = RNNwavefunction(Nx, Ny, cell=tf.contrib.rnn.LSTMCell, activation=tf.nn.relu, units=[10], scope=SCOPE, seed=111)
    assert wf._native.model == _lib.MODEL_LSTM1D_F64
    assert wf.num_params() == 542
    assert [v.name for v in wf.rnn.variables] == [SCOPE + "/" + LSTM + "kernel:0", SCOPE + "/" + LSTM + "bias:0"]
    assert wf.dense.count_params() == 22
    wf.set_params(trained_like(10, seed=8))
    prm = wf.get_params()
    with tf.Session(graph=wf.graph) as sess:
        samples_ = wf.sample(numsamples=numsamples, inputdim=2)
        samples = sess.run(samples_)
        assert samples.shape == (numsamples, N) and samples.dtype == np.int64
        ph = tf.placeholder(dtype=tf.int32, shape=[None, N])
        log_probs_ = wf.log_probability(ph, inputdim=2)
        lp = sess.run(log_probs_, feed_dict={ph: samples})
        assert np.abs(lp - lstm_log_probability(prm, samples, Nx, Ny)).max() <= 1e-11 * N
        Jz = np.ones((Nx, Ny))
        log_probs = np.zeros((N + 1) * numsamples, dtype=np.float64)
        queue_samples = np.zeros((N + 1, numsamples, N), dtype=np.int32)
        e = Ising2D_local_energies(Jz, Bx, Nx, Ny, samples, queue_samples, log_probs_, ph, log_probs, sess)
    e_ref = E.ising2d_local_energies(Jz, Bx, Nx, Ny, samples, lambda x: lstm_log_probability(prm, x, Nx, Ny))
    assert np.allclose(e, e_ref, rtol=1e-10, atol=0)
    # save / restore: .npz and a TF V2 bundle under the LSTMCell's variable names
    for path in (str(tmp_path / "lstm.npz"), str(tmp_path / "ckpt" / "lstm")):
        if not path.endswith(".npz"):
            (tmp_path / "ckpt").mkdir()
        wf.save(path)
        other = RNNwavefunction(Nx, Ny, cell=tf.nn.rnn_cell.LSTMCell, units=[10], scope=SCOPE, seed=5)
        other.restore(path)
        assert all(np.array_equal(other.params[k], prm[k]) for k in prm)
        assert np.array_equal(other._native.log_prob(samples), wf._native.log_prob(samples))
    from rnnwavefunctions_amd import tf_checkpoint as T
    names = set(T.read_checkpoint(str(tmp_path / "ckpt" / "lstm")))
    assert {SCOPE + "/" + LSTM + "kernel", SCOPE + "/" + LSTM + "bias"} <= names
    # no gradient: the optimizer of the reference's loop refuses the LSTM wave function
    Eloc = tf.placeholder(dtype=tf.float64, shape=[numsamples])
    cost = tf.reduce_mean(tf.multiply(log_probs_, tf.stop_gradient(Eloc))) - \
        tf.reduce_mean(tf.stop_gradient(Eloc)) * tf.reduce_mean(log_probs_)
    with pytest.raises(NotImplementedError, match="no gradient for the LSTM cell"):
        tf.train.AdamOptimizer(1e-3).compute_gradients(cost)
    # the repository's default cell stays the GRU
    assert RNNwavefunction(Nx, Ny, units=[10])._native.model == _lib.MODEL_GRU1D_F64


def test_refusals():
    from rnnwavefunctions_amd import _lib
    from rnnwavefunctions_amd import compat as tf
    from rnnwavefunctions_amd.TFIM2D_1DRNN.RNNwavefunction import RNNwavefunction
    with pytest.raises(ValueError, match="one layer"):
        _lib.NativeWavefunction(_lib.MODEL_LSTM1D_F64, 4, 4, (10, 10))
    with pytest.raises(ValueError, match="<= 68"):
        _lib.NativeWavefunction(_lib.MODEL_LSTM1D_F64, 4, 4, (69,))
    with pytest.raises(ValueError, match="one layer"):
        RNNwavefunction(4, 4, cell=tf.contrib.rnn.LSTMCell, units=[10, 10])
    wf = make_wf(3, 3, 10, trained_like(10, seed=1))
    N = 9
    s = wf.sample(20, seed=1, step=0)
    wf.vmc_step(20, seed=1, step=0, couplings=np.append(np.ones(N), 2.0))
    with pytest.raises(ValueError, match="no gradient for the LSTM cell"):
        wf.vmc_gradient(0.0, 20, {"wf_dense/bias": (2,)})
    with pytest.raises(ValueError, match="no gradient for the LSTM cell"):
        wf.load_batch(s, np.zeros(20))
    with pytest.raises(ValueError, match="no gradient for the LSTM cell"):
        wf.adam_step(1e-3)
    with pytest.raises(ValueError, match="no gradient for the LSTM cell"):
        wf.train_steps(20, 1, 0, np.append(np.ones(N), 2.0), [1e-3])
    assert wf.device_training_supported() is False
    s32, jz, e = np.ascontiguousarray(s, dtype=np.int32), np.ones(N), np.zeros(20)
    rc = wf.lib.rnnwf_tfim_eloc(wf.h, s32.ctypes.data_as(_lib._I32P), 20, jz.ctypes.data_as(_lib._F64P), 1.0,
                                e.ctypes.data_as(_lib._F64P), None)
    with pytest.raises(ValueError, match="1D positive RNN"):
        wf._check(rc)
    with pytest.raises(ValueError, match="only the complex RNN"):
        wf.log_amp(s)
    with pytest.raises(ValueError, match="complex RNN"):
        wf.j1j2_eloc(s, np.ones(N), np.ones(N), np.zeros(N))
