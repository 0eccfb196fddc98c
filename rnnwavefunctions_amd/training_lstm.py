"""VMC training of the LSTM wave function, the default cell of the reference's constructor
(2DTFIM_1DRNN/RNNwavefunction.py:9; docs/lstm.md, "Gradient").

    run_2DTFIM_1DRNN_LSTM  <- 2DTFIM_1DRNN/Training1DRNN_2DTFIM.py:85-233 with cell = tf.contrib.rnn.LSTMCell

training.run_2DTFIM_1DRNN stays the GRU driver, as the reference's script hard-codes that cell.  One iteration here is ONE
library call, NativeWavefunction.lstm_vmc_gradient_step: sample + fused local energies + moments + back-propagation through time +
weight-gradient product on the device with one host synchronisation; the Adam update (training.Adam) runs on the host and the new
parameters are committed.  Learning rate, printing and saving follow training.run_2DTFIM_1DRNN.  Single process.
"""
import numpy as np

from . import _lib
from . import params as P
from .training import Adam, _resolve_device, _saver

__all__ = ["run_2DTFIM_1DRNN_LSTM", "lstm_training_loop"]


def lstm_training_loop(wf, params, scope, couplings, numsteps, numsamples, seed, lr, lr_of_it, opt, verbose=False, on_step=None,
                       on_gradient=None):
    """Iterations 0..numsteps of training._train's loop on an LSTM handle `wf` that holds `params`: returns (meanEnergy, varEnergy,
    params).  on_gradient(it, params, out) (tests) sees every iteration's parameters and the fused call's result before the update."""
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
                          learningrate=1e-3, seed=333, save_dir=None, device=None, verbose=True, comm=None, restore=False):
    """training.run_2DTFIM_1DRNN's arguments for the LSTM cell (one layer, <= 68 units): float64 LSTM wave function over the raster
    path of the open square-lattice transverse-field Ising model, learning rate 1 / (1/lr + it/10), energies saved every 10 steps and
    the model every 500 (save_dir).  The initial weights are params.init_lstm_params(seed=111), the constructor's default seed, as
    the GRU driver's.  Returns (meanEnergy, varEnergy); the trained parameters are left in run_2DTFIM_1DRNN_LSTM.last_params."""
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
        verbose=verbose, on_step=_saver(save_dir, "meanEnergy_" + tag, "varEnergy_" + tag, "RNNwavefunction_" + tag, scope))
    wf.close()
    run_2DTFIM_1DRNN_LSTM.last_params = params
    return meanE, varE
