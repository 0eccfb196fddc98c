"""The LSTM wave function's gradient (rnnwf_lstm_gradient, rnnwf_lstm_vmc_gradient_step, training_lstm) on the GPU.

EVERY element of every tensor of lstm_gradient against one float64 reverse-mode pass of tests/lstm_grad_reference.py: widths 10, 16,
17, 20, 21, 33, 36, 37, 50, 52, 53, 67, 68 (every NFULL, full tiles, a full and a partial mixed tile) on 11 x 3, 17 x 2 and 7 x 5
(33 to 35 sites: the spin-word boundary is crossed) and 2 x 1 (a single checkpoint), 40 samples (two full 16-chain blocks and a ragged
one of 8) drawn with vmc_step on sharpened weights, weights with both signs and exact zeros.  The bound is the float64 families' of
tests/test_gpu_gradient_classes.py: autograd_reference.verdict with unit_roundoff_ratio 2^-29, FACTOR 16 and that module's rounding
floor; tests/test_lstm_grad_reference.py shows on the reference alone what it rejects.  The same on lattices of one to five spin words (LG.BIG_LATTICES: 32, 64, 65, 96, 100
and 144 sites, every width in rotation and every NFULL at 65, 100 and 144 sites), where the backward pass's word walk swaps and
refetches; a wide batch at 10 x 10 (1 000 rows, NFULL 2 to 4) that fills many workgroups and gives the weight-gradient product blocks
longer than its floor.  Then: a long batch whose blocks outnumber the persistent grid's waves, at every NFULL; exact zero for zero weights, bit-identical repeats, additivity in the weights; the fused step against
vmc_step + lstm_gradient bit for bit; every gradient along five iterations of the driver's loop; training against the float64 GRU;
the refusals.
"""
import os
import time

import numpy as np
import pytest

import autograd_reference as A
import ed
import lstm_grad_reference as LG

pytestmark = pytest.mark.gpu
SCOPE = LG.SCOPE


def handle(shape, units, prm=None):
    from rnnwavefunctions_amd import _lib
    wf = _lib.NativeWavefunction(_lib.MODEL_LSTM1D_F64, shape[0], shape[1], (units,))
    if prm is not None:
        wf.set_params(prm, scope=SCOPE)
    return wf


def couplings(shape, Bx=3.0):
    return np.append(np.ones(shape[0] * shape[1]), Bx)


def drawn(wf, shape, ns, step=0):
    out = wf.vmc_step(ns, seed=111, step=step, couplings=couplings(shape), want_samples=True, want_eloc=True)
    return out["samples"], out["eloc"], out["moments"]


def native_gradient(wf, prm, s, w):
    return LG.scoped(wf.lstm_gradient(s, w, LG.shapes(prm)))


def checked(label, prm, grads, ref):
    assert set(grads) == set(prm)
    for k in prm:
        assert grads[k].shape == prm[k].shape, k
        assert np.all(np.isfinite(grads[k])), k
    return LG.judge(label, grads, ref)


# every width on one of the three lattices of 33 to 35 sites, in turn; the single checkpoint at the last width of every NFULL
CASES = [(LG.LATTICES[k % 3], u) for k, u in enumerate(LG.WIDTHS)] + [(LG.LATTICES[3], u) for u in (20, 36, 52, 68)]


@pytest.mark.parametrize("shape,units", CASES, ids=["%dx%d-%d" % (s[0], s[1], u) for s, u in CASES])
def test_every_gradient_element(shape, units):
    t0 = time.time()
    prm = LG.parameters(units)
    wf = handle(shape, units, prm)
    s, _, _ = drawn(wf, shape, LG.NS)
    w = LG.weights(LG.NS)
    wf.timing_enable(True)
    wf.timing_reset()
    grads = native_gradient(wf, prm, s, w)
    launches = wf.timing_get(3)["launches"], wf.timing_get(4)["launches"]
    wf.close()
    ref = LG.reference(prm, s, w)
    label = "[lstm-%dx%d-%d]" % (shape[0], shape[1], units)
    worst, failures = checked(label, prm, grads, ref)
    print("LSTMGRAD %s NFULL %d: launches %d + %d, worst deviation / bound %.3f (limit %g), reference %.2f s, case %.2f s"
          % (label, LG.nfull(units), launches[0], launches[1], worst, A.FACTOR, ref.seconds, time.time() - t0))
    assert launches == (1, 1)
    assert not failures, "tensors beyond %g x the bound: %s" % (A.FACTOR, failures)


BIG_CASES = LG.big_cases()


@pytest.mark.parametrize("shape,units", BIG_CASES, ids=["%dx%d-%d" % (s[0], s[1], u) for s, u in BIG_CASES])
def test_every_gradient_element_on_one_to_five_spin_words(shape, units):
    """test_every_gradient_element on LG.BIG_LATTICES (32, 64, 65, 96, 100 and 144 sites): the backward pass's spin-word walk swaps at
    every multiple of 32 and refetches from site 64 down.  The drawn rows with non-zero weight hold both spin values at sites 31 and
    63, so a spin handed over from the wrong word changes the gradient (tests/test_lstm_grad_reference.py: by 1e12 bounds)."""
    t0 = time.time()
    prm = LG.parameters(units, sharp=LG.big_sharp(shape, units))
    wf = handle(shape, units, prm)
    s, _, _ = drawn(wf, shape, LG.NS)
    w = LG.weights(LG.NS)
    wf.timing_enable(True)
    wf.timing_reset()
    grads = native_gradient(wf, prm, s, w)
    launches = wf.timing_get(3)["launches"], wf.timing_get(4)["launches"]
    wf.close()
    ones = s.reshape(LG.NS, -1)[w != 0.0].mean(axis=0)
    print("LSTMGRAD [lstm-%dx%d-%d] sharp %g: ones among the weighted rows %.2f at site 31%s, %.2f overall"
          % (shape[0], shape[1], units, LG.big_sharp(shape, units), ones[31], ", %.2f at site 63" % ones[63] if len(ones) > 63 else "",
             ones.mean()))
    assert LG.word_boundaries_mixed(s, w)
    ref = LG.reference(prm, s, w)
    label = "[lstm-%dx%d-%d]" % (shape[0], shape[1], units)
    worst, failures = checked(label, prm, grads, ref)
    print("LSTMGRAD %s NFULL %d: launches %d + %d, worst deviation / bound %.3f (limit %g), reference %.2f s, case %.2f s"
          % (label, LG.nfull(units), launches[0], launches[1], worst, A.FACTOR, ref.seconds, time.time() - t0))
    assert launches == (1, 1)
    assert not failures, "tensors beyond %g x the bound: %s" % (A.FACTOR, failures)


@pytest.mark.parametrize("units", LG.WIDE["widths"])
def test_wide_batch_fills_many_workgroups_and_long_gemm_blocks(units):
    """10 x 10, 1 000 rows = 62 full 16-chain blocks and a ragged one of 8: more than one workgroup of four waves, so head_reduce_kernel
    sums head rows over several workgroups, and N ns = 100 000 rows > 256 cu_count, so tn_gemm_launch_cols gives every block of the
    weight-gradient product more than its floor of 64 rows.  The rows repeat 40 device-drawn configurations, the 16 of a block all
    different, each row with a weight of its own (LG.wide_batch); the floor comes from the 40 configurations' terms."""
    t0 = time.time()
    shape, ns = LG.WIDE["shape"], LG.WIDE["ns"]
    N = shape[0] * shape[1]
    prm = LG.parameters(units)
    wf = handle(shape, units, prm)
    configs, _, _ = drawn(wf, shape, LG.WIDE["configs"])
    s, _ = LG.wide_batch(configs, ns)
    w = LG.weights(ns)
    wf.timing_enable(True)
    wf.timing_reset()
    grads = native_gradient(wf, prm, s, w)
    launches = wf.timing_get(3)["launches"], wf.timing_get(4)["launches"]
    cus = wf.device_info()["cu_count"]
    wf.close()
    assert N * ns > 256 * cus                                       # rows per block of the product: ceil(N ns / (4 cu_count)) > 64
    assert (ns + 15) // 16 > 4 and ns % 16 == 8                     # more than one workgroup of four waves; a ragged last block
    assert LG.word_boundaries_mixed(s, w)
    ref = LG.reference(prm, s, w, keep_terms=False)
    label = "[lstm-10x10-%d-%d]" % (units, ns)
    worst, failures = checked(label, prm, grads, ref)
    print("LSTMGRAD %s NFULL %d: launches %d + %d, worst deviation / bound %.3f (limit %g), reference %.2f s, case %.2f s"
          % (label, LG.nfull(units), launches[0], launches[1], worst, A.FACTOR, ref.seconds, time.time() - t0))
    assert launches == (1, 1)
    assert not failures, "tensors beyond %g x the bound: %s" % (A.FACTOR, failures)


@pytest.mark.parametrize("units", [10, 36, 52, 68])
def test_long_batch_wraps_the_persistent_grid(units):
    """2 x 2, 40 000 samples = 2 500 blocks of 16 chains: more than the grid's waves (four per workgroup, at most two workgroups per
    CU by registers: profiles/lstm_grad_kernel_resources.txt), so waves walk several blocks and sum their head rows over them - at 52
    and 68 units (NFULL 3 and 4, one workgroup per CU) with the backward operand streamed through L2."""
    t0 = time.time()
    shape, ns = (2, 2), 40000
    prm = LG.parameters(units)
    wf = handle(shape, units, prm)
    s, _, _ = drawn(wf, shape, ns)
    w = LG.weights(ns)
    grads = native_gradient(wf, prm, s, w)
    cus = wf.device_info()["cu_count"]
    wf.close()
    assert (ns + 15) // 16 > 2 * 4 * cus
    ref = LG.reference(prm, s, w, keep_terms=False)
    label = "[lstm-2x2-%d-%d]" % (units, ns)
    worst, failures = checked(label, prm, grads, ref)
    print("LSTMGRAD long batch %s NFULL %d: worst deviation / bound %.3f (limit %g), reference %.2f s, case %.2f s"
          % (label, LG.nfull(units), worst, A.FACTOR, ref.seconds, time.time() - t0))
    assert not failures, "tensors beyond %g x the bound: %s" % (A.FACTOR, failures)


def test_identities():
    shape, units = (11, 3), 21
    prm = LG.parameters(units)
    wf = handle(shape, units, prm)
    s, _, _ = drawn(wf, shape, LG.NS)
    w1, w2 = LG.weights(LG.NS, seed=7), LG.weights(LG.NS, seed=8)
    zero = native_gradient(wf, prm, s, np.zeros(LG.NS))
    assert all(not v.any() for v in zero.values())                                    # exactly zero
    g1 = native_gradient(wf, prm, s, w1)
    g2 = native_gradient(wf, prm, s, w2)
    g1_again = native_gradient(wf, prm, s, w1)
    assert all(np.array_equal(g1[k], g1_again[k]) for k in g1)                        # bit-identical
    g12 = native_gradient(wf, prm, s, w1 + w2)
    wf.close()
    ref = LG.reference(prm, s, w1 + w2)
    for label, g in (("[w1 + w2]", g12), ("[g(w1) + g(w2)]", {k: g1[k] + g2[k] for k in g1})):
        worst, failures = checked(label, prm, g, ref)
        assert not failures, (label, failures)


@pytest.mark.parametrize("shape,units", [((7, 5), 37), ((10, 10), 50)], ids=["7x5-37", "10x10-50"])
def test_fused_step_is_vmc_step_plus_lstm_gradient_bit_for_bit(shape, units):
    ns = 200
    prm = LG.parameters(units, sharp=1.5)
    wf = handle(shape, units, prm)
    fused = wf.lstm_vmc_gradient_step(ns, seed=111, step=3, couplings=couplings(shape), shapes=LG.shapes(prm), want_samples=True,
                                      want_eloc=True)
    two = wf.vmc_step(ns, seed=111, step=3, couplings=couplings(shape), want_samples=True, want_eloc=True)
    assert np.array_equal(fused["moments"], two["moments"])
    assert np.array_equal(fused["samples"], two["samples"])
    assert np.array_equal(fused["eloc"], two["eloc"])
    s1, _, n, _ = two["moments"]
    g = wf.lstm_gradient(two["samples"], (two["eloc"] - s1 / n) * (1.0 / n), LG.shapes(prm))
    wf.close()
    assert set(g) == set(fused["grads"])
    for k in g:
        assert np.any(g[k] != 0.0), k
        assert np.array_equal(g[k], fused["grads"][k]), k


def test_gradients_along_the_drivers_trajectory():
    """five iterations of training_lstm's loop on 3 x 3, 10 units, 200 samples: the gradient each iteration used, at that iteration's
    parameters, under the every-element bound"""
    from rnnwavefunctions_amd import params as P
    from rnnwavefunctions_amd import training, training_lstm
    shape, units, ns = (3, 3), 10, 200
    prm = P.init_lstm_params([units], seed=111, scope=SCOPE)
    wf = handle(shape, units, prm)
    seen = []

    def on_gradient(it, params, out):
        seen.append((it, {k: v.copy() for k, v in params.items()}, out["samples"].copy(), out["eloc"].copy(), out["moments"].copy(),
                     {k: v.copy() for k, v in out["grads"].items()}))

    lr = np.float64(1e-2)
    meanE, varE, _ = training_lstm.lstm_training_loop(wf, prm, SCOPE, couplings(shape, 2.0), 4, ns, 333, lr,
                                                      lambda lr0, it: 1.0 / ((1.0 / lr0) + it / 10), training.Adam(),
                                                      on_gradient=on_gradient)
    wf.close()
    assert len(seen) == 5 == len(meanE)
    for it, params, s, e, mom, grads in seen:
        if it:
            assert any(not np.array_equal(params[k], seen[it - 1][1][k]) for k in params)          # the update was applied
        w = (e - mom[0] / mom[2]) * (1.0 / mom[2])
        ref = LG.reference(params, s, w)
        worst, failures = checked("[trajectory it %d]" % it, params, LG.scoped(grads), ref)
        assert not failures, (it, failures)


# ---- training works -----------------------------------------------------------------------------------------------------------------

TRAIN = dict(shape=(3, 3), Bx=2.0, units=10, ns=200, numsteps=300, lr=1e-2, gru_seeds=(333, 334, 335, 336, 337))


def all_configs(N):
    idx = np.arange(2 ** N)
    return ((idx[:, None] >> (N - 1 - np.arange(N))[None, :]) & 1).astype(np.int64)


def exact_energy(log_prob):
    """<H> of psi = sqrt(P) over all 512 configurations of 3 x 3 (tests/ed.py's Hamiltonian): no Monte-Carlo noise"""
    Nx, Ny = TRAIN["shape"]
    H = ed.tfim2d_hamiltonian(np.ones((Nx, Ny)), TRAIN["Bx"], Nx, Ny)
    psi = np.exp(0.5 * log_prob)
    assert abs(psi @ psi - 1.0) < 1e-10
    return float(psi @ (H @ psi)), float(np.linalg.eigvalsh(H)[0])


def test_training_lowers_the_exact_energy_as_the_gru_does():
    """3 x 3, Bx = 2, 10 units, 200 samples, 300 iterations at learning rate 1 / (100 + it / 10) of run_2DTFIM_1DRNN_LSTM (seed 333)
    and of run_2DTFIM_1DRNN (the float64 GRU, seeds 333..337).  The exact variational energy over all 512 configurations must be lower
    after training than at initialisation, and its gap to the ED ground energy at most the GRU's worst-seed gap times the GRU's own
    seed-to-seed spread (max / min gap).  Measured on MI355X (docs/lstm.md, "Gradient"), 300 iterations, ED -19.794136: LSTM
    -18.262941 -> -19.649955, gap 0.14418; GRU -17.484984 -> gaps 0.14444, 0.14582, 0.14140, 0.14042, 0.13602, worst 0.14582, spread
    1.072, allowed LSTM gap 0.15632.  The whole test takes 0.4 s."""
    import torch
    import lstm_reference as LR
    from rnnwavefunctions_amd import params as P
    from rnnwavefunctions_amd import training, training_lstm
    Nx, Ny = TRAIN["shape"]
    t0 = time.time()
    cfgs = all_configs(Nx * Ny)
    kw = dict(numsteps=TRAIN["numsteps"], systemsize_x=Nx, systemsize_y=Ny, Bx=TRAIN["Bx"], num_units=TRAIN["units"], num_layers=1,
              numsamples=TRAIN["ns"], learningrate=TRAIN["lr"], verbose=False)
    e_init, e0 = exact_energy(LR.lstm_log_probability(P.init_lstm_params([TRAIN["units"]], seed=111), cfgs, Nx, Ny))
    training_lstm.run_2DTFIM_1DRNN_LSTM(seed=333, **kw)
    e_lstm, _ = exact_energy(LR.lstm_log_probability(training_lstm.run_2DTFIM_1DRNN_LSTM.last_params, cfgs, Nx, Ny))
    t_lstm = time.time() - t0
    gru_gaps = []
    for seed in TRAIN["gru_seeds"]:
        training.run_2DTFIM_1DRNN(seed=seed, **kw)
        lp = A.prnn_log_probability(A.to_torch(training.run_2DTFIM_1DRNN.last_params, torch.float64), cfgs).numpy()
        gru_gaps.append(exact_energy(lp)[0] - e0)
    gru_init = exact_energy(A.prnn_log_probability(A.to_torch(P.init_gru_params([TRAIN["units"]], seed=111, dtype=np.float64),
                                                              torch.float64), cfgs).numpy())[0]
    spread = max(gru_gaps) / min(gru_gaps)
    print("LSTMTRAIN ED %.6f; LSTM exact energy %.6f -> %.6f (gap %.4e) in %d iterations, %.1f s; GRU %.6f -> gaps %s, worst %.4e, "
          "spread %.3f; allowed LSTM gap %.4e; all %.1f s"
          % (e0, e_init, e_lstm, e_lstm - e0, TRAIN["numsteps"], t_lstm, gru_init, " ".join("%.4e" % g for g in gru_gaps), max(gru_gaps),
             spread, max(gru_gaps) * spread, time.time() - t0))
    assert all(g < gru_init - e0 for g in gru_gaps)               # every GRU seed trained at these settings
    assert e_lstm < e_init
    assert e_lstm - e0 <= max(gru_gaps) * spread


# ---- refusals ---------------------------------------------------------------------------------------------------------------------

def test_refusals():
    from rnnwavefunctions_amd import _lib
    from rnnwavefunctions_amd import params as P
    shape, units = (11, 3), 10
    prm = LG.parameters(units)
    s, w = np.zeros((LG.NS, 33), dtype=np.int32), LG.weights(LG.NS)
    # a non-LSTM handle
    gru = _lib.NativeWavefunction(_lib.MODEL_GRU1D_F64, shape[0], shape[1], (units,))
    gprm = P.init_gru_params([units], seed=111, dtype=np.float64)
    gru.set_params(gprm, scope=SCOPE)
    with pytest.raises(ValueError, match="rnnwf_lstm_gradient: needs an LSTM1D_F64 handle"):
        gru.lstm_gradient(s, w, LG.shapes(gprm))
    with pytest.raises(ValueError, match="rnnwf_lstm_vmc_gradient_step: needs an LSTM1D_F64 handle"):
        gru.lstm_vmc_gradient_step(LG.NS, 111, 0, couplings(shape), LG.shapes(gprm))
    gru.close()
    # parameters not committed
    wf = handle(shape, units)
    with pytest.raises(_lib.RnnwfError, match="parameters not committed"):
        wf.lstm_gradient(s, w, LG.shapes(prm))
    with pytest.raises(_lib.RnnwfError, match="parameters not committed"):
        wf.lstm_vmc_gradient_step(LG.NS, 111, 0, couplings(shape), LG.shapes(prm))
    wf.close()
    # past the state budget: 1 MB holds 6 blocks of 32 checkpoints x 5 120 B = 96 chains at 33 sites and 10 units
    assert "RNNWF_STATE_BUDGET_MB" not in os.environ
    os.environ["RNNWF_STATE_BUDGET_MB"] = "1"                 # read once per handle, at creation
    try:
        small = handle(shape, units, prm)
    finally:
        del os.environ["RNNWF_STATE_BUDGET_MB"]
    big = np.zeros((200, 33), dtype=np.int32)
    with pytest.raises(_lib.RnnwfError, match="rnnwf_lstm_gradient: 200 samples exceed the state budget of one pass; split the batch"):
        small.lstm_gradient(big, LG.weights(200), LG.shapes(prm))
    with pytest.raises(_lib.RnnwfError, match="200 samples exceed the state budget of one pass; split the batch"):
        small.lstm_vmc_gradient_step(200, 111, 0, couplings(shape), LG.shapes(prm))
    g = small.lstm_gradient(big[:96], LG.weights(96), LG.shapes(prm))                 # what fits still runs
    assert all(np.all(np.isfinite(v)) for v in g.values())
    small.close()
