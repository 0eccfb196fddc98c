"""VMC training of the LSTM wave function, the default cell of the reference's constructor
(2DTFIM_1DRNN/RNNwavefunction.py:9; docs/lstm.md, "Gradient").

    run_2DTFIM_1DRNN_LSTM  <- 2DTFIM_1DRNN/Training1DRNN_2DTFIM.py:85-233 with cell = tf.contrib.rnn.LSTMCell

training.run_2DTFIM_1DRNN stays the GRU driver, as the reference's script hard-codes that cell.  One iteration here is ONE
library call, NativeWavefunction.lstm_vmc_gradient_step: sample + fused local energies + moments + back-propagation through time +
weight-gradient product on the device with one host synchronisation; the Adam update (training.Adam) runs on the host and the new
parameters are committed.  Learning rate, printing and saving follow training.run_2DTFIM_1DRNN.  Single process.

device_steps=K (docs/lstm.md, "Device-resident training"): the same iterations, K per library call, with Adam and the re-pack of the
weight images on the device (NativeWavefunction.lstm_train_steps / lstm_pauli_train_steps) - the same trajectory bit for bit.
minimize_hamiltonian_device is observables_lstm.minimize_hamiltonian's loop on that road; that function itself keeps refusing
device_steps.
"""
import numpy as np

from . import _lib
from . import params as P
from .training import Adam, _resolve_device, _saver

# tests/test_lstm_grad_reference.py pins this list; the names of the device-resident road are public all the same (DEVICE_API names them)
__all__ = ["run_2DTFIM_1DRNN_LSTM", "lstm_training_loop"]
DEVICE_API = ["minimize_hamiltonian_device", "device_blocks", "check_device_steps"]


def check_device_steps(device_steps, on_gradient=None):
    """device_steps of this module's drivers: None (the host loop) or an integer >= 1 (iterations per device call, at most 1024 are
    taken per call); on_gradient sees a host iteration's gradient, which a device call does not bring back."""
    if device_steps is None:
        return None
    if isinstance(device_steps, bool) or not isinstance(device_steps, (int, np.integer)) or device_steps < 1:
        raise ValueError("device_steps must be None or an integer >= 1, got %r" % (device_steps,))
    if on_gradient is not None:
        raise ValueError("device_steps keeps the gradient on the device: on_gradient needs the host loop (device_steps=None)")
    return int(device_steps)


def device_blocks(numsteps, device_steps, first=0):
    """[(it, K)]: iterations first..numsteps in blocks of at most device_steps (and at most 1024, one call's limit) that end where the
    saver acts - no block holds a multiple of 10 (energies) or of 500 (model, whose checkpoint holds the state BEFORE that iteration's
    update) anywhere but at its start, as training._train_on_device cuts its blocks."""
    blocks, it = [], int(first)
    while it <= numsteps:
        K = min(int(device_steps), 1024, 10 - it % 10, numsteps + 1 - it)
        blocks.append((it, K))
        it += K
    return blocks


def _device_loop(wf, params, scope, train_block, numsteps, numsamples, device_steps, opt, verbose, on_step):
    """lstm_training_loop's iterations through train_block(it, K) -> (K, 4) moments: what the loop shows the outside - prints, the
    histories and the parameters and optimizer state handed to on_step - is what the host loop shows at the same iteration"""
    m0, v0 = opt.to_flat(wf, params, scope)
    wf.adam_set_state(m0 if opt.t else None, v0 if opt.t else None, opt.t)
    meanEnergy, varEnergy = [], []
    for it, K in device_blocks(numsteps, device_steps):
        if on_step is not None and it % 500 == 0 and it:      # the checkpoint of iteration `it` holds the state before its update
            params = wf.get_params_dict(params, scope)
            opt.from_flat(wf, params, scope, *wf.adam_get_state())
        mom = train_block(it, K)
        for j in range(K):
            s1, s2, n, _ = mom[j]
            meanE = s1 / n
            meanEnergy.append(meanE)
            varEnergy.append(s2 / n - meanE ** 2)
            if verbose and (it + j) % 10 == 0:
                print("mean(E): {0}, var(E): {1}, #samples {2}, #Step {3} \n\n".format(meanE, varEnergy[-1], numsamples, it + j))
            if on_step is not None:
                on_step(it + j, meanEnergy, varEnergy, params, opt)
    params = wf.get_params_dict(params, scope)                # read back once, behind the last block
    opt.from_flat(wf, params, scope, *wf.adam_get_state())
    return meanEnergy, varEnergy, params


def lstm_training_loop(wf, params, scope, couplings, numsteps, numsamples, seed, lr, lr_of_it, opt, verbose=False, on_step=None,
                       on_gradient=None, device_steps=None):
    """Iterations 0..numsteps of training._train's loop on an LSTM handle `wf` that holds `params`: returns (meanEnergy, varEnergy,
    params).  on_gradient(it, params, out) (tests) sees every iteration's parameters and the fused call's result before the update.
    device_steps=K: the iterations run K per call on the device (lstm_train_steps), the learning rates of a block computed here; `opt`
    (a training.Adam) gives beta1, beta2, epsilon and its state and receives the final one; on_gradient is refused."""
    device_steps = check_device_steps(device_steps, on_gradient)
    if device_steps is not None:
        def block(it, K):
            return wf.lstm_train_steps(numsamples, seed, it, couplings, [float(lr_of_it(lr, j)) for j in range(it, it + K)], opt.b1, opt.b2,
                                       opt.eps)
        return _device_loop(wf, params, scope, block, numsteps, numsamples, device_steps, opt, verbose, on_step)
    shapes = {k[len(scope) + 1:]: v.shape for k, v in params.items()}
    meanEnergy, varEnergy = [], []
    for it in range(numsteps + 1):
        out = wf.lstm_vmc_gradient_step(numsamples, seed=seed, step=it, couplings=couplings, shapes=shapes,
                                        want_samples=on_gradient is not None, want_eloc=on_gradient is not None)
        s1, s2, n, _ = out["moments"]
        meanE = s1 / n
        varE = s2 / n - meanE ** 2
        meanEnergy.append(meanE)
        varEnergy.append(varE)
        if verbose and it % 10 == 0:
            print("mean(E): {0}, var(E): {1}, #samples {2}, #Step {3} \n\n".format(meanE, varE, numsamples, it))
        if on_step is not None:
            on_step(it, meanEnergy, varEnergy, params, opt)
        if on_gradient is not None:
            on_gradient(it, params, out)
        grads = {scope + "/" + k: v for k, v in out["grads"].items()}
        params = opt.step(params, grads, lr_of_it(lr, it))
        wf.set_params(params, scope=scope)
    return meanEnergy, varEnergy, params


def run_2DTFIM_1DRNN_LSTM(numsteps=2 * 10 ** 4, systemsize_x=5, systemsize_y=5, Bx=+2, num_units=50, num_layers=1, numsamples=500,
                          learningrate=1e-3, seed=333, save_dir=None, device=None, verbose=True, comm=None, restore=False,
                          device_steps=None):
    """training.run_2DTFIM_1DRNN's arguments for the LSTM cell (one layer, <= 68 units): float64 LSTM wave function over the raster
    path of the open square-lattice transverse-field Ising model, learning rate 1 / (1/lr + it/10), energies saved every 10 steps and
    the model every 500 (save_dir).  The initial weights are params.init_lstm_params(seed=111), the constructor's default seed, as
    the GRU driver's.  Returns (meanEnergy, varEnergy); the trained parameters are left in run_2DTFIM_1DRNN_LSTM.last_params.
    device_steps=K (an integer >= 1): K iterations per library call with Adam on the device, the same energies, files and parameters."""
    device_steps = check_device_steps(device_steps)
    if num_layers != 1:
        raise ValueError("the LSTM wave function has one layer (stacked LSTM layers are not implemented)")
    if comm is not None:
        raise ValueError("run_2DTFIM_1DRNN_LSTM runs in one process on one GPU: no communicator (comm=%r)" % (comm,))
    if restore:
        raise ValueError("run_2DTFIM_1DRNN_LSTM: restore is not implemented for the LSTM driver")
    Nx, Ny = systemsize_x, systemsize_y
    scope = "RNNwavefunction"
    lr = np.float64(learningrate)
    units = [num_units]
    params = P.init_lstm_params(units, seed=111, scope=scope, dtype=np.float64)
    wf = _lib.NativeWavefunction(_lib.MODEL_LSTM1D_F64, Nx, Ny, tuple(units), device=_resolve_device(device, comm))
    wf.set_params(params, scope=scope)
    if verbose:
        print("The number of params is {0}".format(P.count_params(params)))
    tag = "LSTMRNN_" + str(Nx) + "x" + str(Ny) + "_Bx" + str(Bx) + "_lradap" + str(lr) + "_samp" + str(numsamples) + \
        "_units" + "".join("_{0}".format(u) for u in units)
    couplings = np.append(np.ones(Nx * Ny), float(Bx))          # Jz = +np.ones((Nx, Ny))
    meanE, varE, params = lstm_training_loop(
        wf, params, scope, couplings, numsteps, numsamples, seed, lr, lambda lr0, it: 1.0 / ((1.0 / lr0) + it / 10), Adam(),
        verbose=verbose, on_step=_saver(save_dir, "meanEnergy_" + tag, "varEnergy_" + tag, "RNNwavefunction_" + tag, scope),
        device_steps=device_steps)
    wf.close()
    run_2DTFIM_1DRNN_LSTM.last_params = params
    return meanE, varE


def minimize_hamiltonian_device(wf, ham, params, numsteps=1000, numsamples=500, learningrate=5e-3, seed=111, scope="RNNwavefunction",
                                opt=None, comm=None, verbose=False, device_steps=10):
    """observables_lstm.minimize_hamiltonian with its iterations on the device, device_steps (an integer >= 1) per library call
    (lstm_pauli_train_steps): the same learning rate 1 / (1 / learningrate + it / 10), the same trajectory bit for bit.  Returns what
    that function returns, (meanEnergy, varEnergy); the trained parameters are left in minimize_hamiltonian_device.last_params.  opt:
    None or a training.Adam (its betas, epsilon and state).  Single process only: a communicator is refused."""
    from . import _observable_api as _api
    from . import observables_lstm as OL
    if device_steps is None:
        raise ValueError("device_steps must be an integer >= 1, got None (the host loop: observables_lstm.minimize_hamiltonian)")
    device_steps = check_device_steps(device_steps)
    if opt is not None and type(opt) is not Adam:
        raise ValueError("minimize_hamiltonian_device: device_steps runs Adam on the device; a custom optimizer (opt=%r) needs the host loop "
                         "(observables_lstm.minimize_hamiltonian)" % (opt,))
    if comm is not None:
        raise ValueError("minimize_hamiltonian_device runs in one process on one GPU: no communicator (comm=%r)" % (comm,))
    nat = OL._native_lstm(wf)
    _api.check_sites(nat, ham)
    opt = opt or Adam()
    params = {k: np.array(v) for k, v in params.items()}
    nat.set_params(params, scope=scope)

    def block(it, K):
        return nat.lstm_pauli_train_steps(ham.flip, ham.sign, ham.coeff, numsamples, seed, it,
                                          [float(OL.lr_schedule(learningrate, j)) for j in range(it, it + K)], opt.b1, opt.b2, opt.eps)
    meanEnergy, varEnergy, minimize_hamiltonian_device.last_params = _device_loop(nat, params, scope, block, numsteps, numsamples, device_steps,
                                                                                  opt, verbose, None)
    return meanEnergy, varEnergy
