"""Stochastic reconfiguration (natural gradient) in its minSR form for the positive one-layer GRU (docs/sr.md).

psi = sqrt(P) is real and positive.  With O[s, k] = d log psi(sigma_s) / d theta_k, dO = O - mean_s O and eps_s = E_loc,s - mean E
the direction with diagonal shift lambda is

    delta = dO^T (dO dO^T + ns lambda I)^-1 eps  =  (S + lambda I)^-1 F,     S = dO^T dO / ns,  F = dO^T eps / ns

and the update is theta <- theta - lr delta (2 F is the gradient of the reference's cost).  The device builds the per-sample
Jacobian, the ns x ns Gram matrix and dO^T y (NativeWavefunction.log_derivatives / sr_gram / sr_apply).  The ns x ns solve is a
Cholesky factorisation in float64, O(ns^3) with ns <= 4096: solver="host" (the default) does it here with LAPACK on the matrix
sr_gram copies back, solver="device" leaves it to NativeWavefunction.sr_direction, which factorises and solves on the device and
returns the direction alone.
"""
import numpy as np


def _check_shift(diag_shift):
    lam = float(diag_shift)
    if not (lam > 0.0 and np.isfinite(lam)):
        raise ValueError("diag_shift must be positive and finite, got %r" % (diag_shift,))
    return lam


def solve_shifted(gram, eps, diag_shift):
    """y of (gram + ns diag_shift I) y = eps by Cholesky in float64; gram (ns, ns) symmetric positive semi-definite, eps (ns,)."""
    lam = _check_shift(diag_shift)
    g = np.array(gram, dtype=np.float64)
    e = np.asarray(eps, dtype=np.float64)
    if g.ndim != 2 or g.shape[0] != g.shape[1] or e.shape != (g.shape[0],):
        raise ValueError("gram must be (ns, ns) and eps (ns,), got %r and %r" % (g.shape, e.shape))
    ns = g.shape[0]
    g[np.diag_indices(ns)] += ns * lam
    c = np.linalg.cholesky(g)
    return np.linalg.solve(c.T, np.linalg.solve(c, e))


def _check_solver(solver):
    if solver not in ("host", "device"):
        raise ValueError("solver must be 'host' or 'device', got %r" % (solver,))
    return solver


def _real_direction(wf, suffix, diag_shift, solver):
    """the direction of a real positive wave function through the facade methods sr_gram / sr_apply / sr_direction + suffix
    ("" the positive GRU's, "_2d" the 2D RNN's)"""
    lam = _check_shift(diag_shift)
    if _check_solver(solver) == "device":
        return getattr(wf, "sr_direction" + suffix)(lam)
    gram, eps = getattr(wf, "sr_gram" + suffix)()
    return getattr(wf, "sr_apply" + suffix)(solve_shifted(gram, eps, diag_shift))


def _real_qgt(o):
    d = o - o.mean(axis=0)
    return d.T @ d / o.shape[0]


def minsr_direction(wf, diag_shift, solver="host"):
    """delta (num_params,) float64 on the resident batch of `wf` (the last vmc_step / load_batch), flat order of wf._layout().
    solver "host": Gram matrix to the host, LAPACK Cholesky, sr_apply; "device": wf.sr_direction, the whole direction on the device."""
    return _real_direction(wf, "", diag_shift, solver)


def qgt(wf):
    """S = dO^T dO / ns (num_params, num_params) float64 from the per-sample log-derivatives of the resident batch: the quantum
    geometric tensor of a real positive wave function.  For diagnostics and small models (it holds num_params^2 doubles)."""
    return _real_qgt(wf.log_derivatives())


def flatten_params(wf, params, scope="RNNwavefunction"):
    """{scoped tf name: array} -> float64 vector in the order of wf._layout()"""
    return np.concatenate([np.asarray(params[scope + "/" + nm], dtype=np.float64).ravel() for nm, _ in wf._layout()])


def unflatten_params(wf, flat, like, scope="RNNwavefunction"):
    """the inverse: {scoped tf name: array} with the shapes and dtypes of `like`"""
    out, off = {}, 0
    for nm, cnt in wf._layout():
        k = scope + "/" + nm
        out[k] = np.asarray(flat[off:off + cnt]).reshape(like[k].shape).astype(like[k].dtype)
        off += cnt
    return out


def _check_device_steps(device_steps):
    if device_steps is None:
        return None
    if isinstance(device_steps, bool) or not isinstance(device_steps, (int, np.integer)) or device_steps < 1:
        raise ValueError("device_steps must be None or an integer >= 1, got %r" % (device_steps,))
    return int(device_steps)


def _real_host_loop(wf, suffix, theta, dtype, couplings, numsteps, numsamples, learningrate, diag_shift, seed, solver, meanEnergy, varEnergy):
    """iterations 0..numsteps of vmc_step (step = iteration) -> _real_direction -> theta -= lr delta, rounded to `dtype` ->
    set_params_flat; appends every iteration's energy and variance, returns the last theta"""
    for it in range(int(numsteps) + 1):
        s1, s2, n, _ = wf.vmc_step(int(numsamples), seed, it, couplings)["moments"]
        meanE = s1 / n
        meanEnergy.append(meanE)
        varEnergy.append(s2 / n - meanE ** 2)
        theta = (theta - learningrate * _real_direction(wf, suffix, diag_shift, solver)).astype(dtype).astype(np.float64)
        wf.set_params_flat(theta)
    return theta


def train_tfim(wf, Jz, Bx, params, numsteps=100, numsamples=500, learningrate=1e-2, diag_shift=1e-3, seed=111, scope="RNNwavefunction",
               solver="host", device_steps=None):
    """Minimise the 1D / raster TFIM energy of `wf` (a NativeWavefunction of GRU1D or GRU1D_F64 with one layer, holding `params`)
    by minSR: vmc_step (samples, local energies, moments; the batch stays resident) -> minsr_direction -> theta -= lr delta ->
    set_params_flat.  Returns (meanEnergy, varEnergy), one entry per iteration 0..numsteps like training.minimize_hamiltonian; the
    trained parameters are left in train_tfim.last_params.  The parameters keep the dtype of `params` (float32 models round every
    update to float32, as the Adam drivers do).  `solver` as in minsr_direction.
    device_steps=K (an integer >= 1): the numsteps + 1 iterations run on the device in chunks of at most K with one host
    synchronisation each (wf.sr_train_steps: the device solver, `solver` is ignored) - the same energies, variances and parameters,
    bit for bit, as solver="device" gives with the loop below."""
    device_steps = _check_device_steps(device_steps)
    _check_shift(diag_shift)
    _check_solver(solver)
    if int(numsteps) < 0 or int(numsamples) < 2:
        raise ValueError("numsteps must be >= 0 and numsamples >= 2, got %r and %r" % (numsteps, numsamples))
    jz = np.asarray(Jz, dtype=np.float64).ravel()
    if jz.size != wf.N:
        raise ValueError("Jz must have %d entries, got %d" % (wf.N, jz.size))
    couplings = np.concatenate([jz, [float(Bx)]])
    dtype = next(iter(params.values())).dtype
    theta = flatten_params(wf, params, scope).astype(dtype).astype(np.float64)
    wf.set_params_flat(theta)
    meanEnergy, varEnergy = [], []
    if device_steps:
        total = int(numsteps) + 1
        chunk = min(device_steps, 1024)                      # one call takes at most 1024 iterations
        for it in range(0, total, chunk):
            mom = wf.sr_train_steps(min(chunk, total - it), int(numsamples), seed, it, couplings, float(learningrate), float(diag_shift))
            for s1, s2, n, _ in mom:
                meanE = s1 / n
                meanEnergy.append(meanE)
                varEnergy.append(s2 / n - meanE ** 2)
        train_tfim.last_params = wf.get_params_dict(params, scope)
        return meanEnergy, varEnergy
    theta = _real_host_loop(wf, "", theta, dtype, couplings, numsteps, numsamples, learningrate, diag_shift, seed, solver, meanEnergy, varEnergy)
    train_tfim.last_params = unflatten_params(wf, theta, params, scope)
    return meanEnergy, varEnergy


# ---- the complex RNN (docs/sr_complex.md) ---------------------------------------------------------------------------------------
# psi = sqrt(P) e^{i phi} with real parameters: O = 1/2 d log P + i d phi, eps = E_loc - mean E complex,
#     S = Re(dO^H dO) / ns,  F = Re(dO^H eps) / ns,  delta = (S + lambda I)^-1 F = Obar^T (Obar Obar^T + ns lambda I)^-1 ebar
# for the stacked real Obar = [Re dO ; Im dO] (2 ns rows) and ebar = [Re eps ; Im eps]: the positive model's solve on order 2 ns.

def minsr_direction_complex(wf, diag_shift, solver="host"):
    """delta (num_params,) float64 on the resident batch of the complex RNN `wf`, flat order of wf._layout().  solver "host": the
    (2 ns, 2 ns) Gram matrix to the host, LAPACK Cholesky, sr_apply_complex; "device": wf.sr_direction_complex."""
    lam = _check_shift(diag_shift)
    if _check_solver(solver) == "device":
        return wf.sr_direction_complex(lam)
    gram, eps = wf.sr_gram_complex()
    ns = gram.shape[0] // 2
    if ns == 0:
        raise ValueError("minsr_direction_complex: no resident batch")
    # solve_shifted shifts by (order) x lambda; the system's shift is ns lambda = (2 ns) (lambda / 2)
    return wf.sr_apply_complex(solve_shifted(gram, eps, lam / 2.0))


def qgt_complex(wf):
    """S = Re(dO^H dO) / ns (num_params, num_params) float64 from the per-sample log-derivatives of the resident batch of the complex
    RNN: the quantum geometric tensor for real parameters.  For diagnostics and small models."""
    o = wf.log_derivatives_complex()
    d = o - o.mean(axis=0)
    return (d.real.T @ d.real + d.imag.T @ d.imag) / o.shape[0]


def train_j1j2(wf, J1, J2, Bz, params, numsteps=100, numsamples=500, learningrate=1e-2, diag_shift=1e-3, seed=111,
               scope="RNNwavefunction", Marshall_sign=False, solver="device"):
    """Minimise the open J1-J2 chain's energy of `wf` (a NativeWavefunction of CRNN_U1 with one layer, holding `params`) by minSR:
    the fused J1-J2 vmc_step (samples of the zero-magnetisation sector, complex local energies, moments; the batch stays resident) ->
    minsr_direction_complex -> theta -= lr delta -> set_params_flat, the host loop of train_tfim.  J1, J2, Bz: scalars or one entry
    per site.  `Marshall_sign` reaches the local energies exactly as training.run_J1J2 passes it on (through the reference's
    `periodic` slot: True selects the periodic chain without a Marshall sign).  Returns (meanEnergy, varEnergy) as run_J1J2 does,
    one entry per iteration 0..numsteps: meanEnergy complex, varEnergy the variance of the real part; the trained parameters are
    left in train_j1j2.last_params and keep the dtype of `params`."""
    _check_shift(diag_shift)
    _check_solver(solver)
    if int(numsteps) < 0 or int(numsamples) < 2:
        raise ValueError("numsteps must be >= 0 and numsamples >= 2, got %r and %r" % (numsteps, numsamples))
    N = wf.N
    j1, j2, bz = (np.broadcast_to(np.asarray(v, dtype=np.float64), (N,)) for v in (J1, J2, Bz))
    periodic = 1.0 if Marshall_sign else 0.0          # run_J1J2's couplings: [J1 | J2 | Bz | periodic, marshall = 0]
    couplings = np.concatenate([j1, j2, bz, [periodic, 0.0]])
    dtype = next(iter(params.values())).dtype
    theta = flatten_params(wf, params, scope).astype(dtype).astype(np.float64)
    wf.set_params_flat(theta)
    meanEnergy, varEnergy = [], []
    for it in range(int(numsteps) + 1):
        s1, s2, n, si = wf.vmc_step(int(numsamples), seed, it, couplings)["moments"]
        meanEnergy.append(complex(s1 / n, si / n))
        varEnergy.append(s2 / n - (s1 / n) ** 2)
        theta = (theta - learningrate * minsr_direction_complex(wf, diag_shift, solver)).astype(dtype).astype(np.float64)
        wf.set_params_flat(theta)
    train_j1j2.last_params = unflatten_params(wf, theta, params, scope)
    return meanEnergy, varEnergy


# ---- the 2D RNN (docs/sr_2d.md) ---------------------------------------------------------------------------------------------------
# psi = sqrt(P) real and positive on the zig-zag path of the square lattice: the positive model's formulas and solve, on the
# rnnwf_*_2d entries of an MDRNN2D handle.

def minsr_direction_2d(wf, diag_shift, solver="host"):
    """delta (num_params,) float64 on the resident batch of the 2D RNN `wf`, flat order of wf._layout().  solver "host": the Gram
    matrix to the host, LAPACK Cholesky, sr_apply_2d; "device": wf.sr_direction_2d."""
    return _real_direction(wf, "_2d", diag_shift, solver)


def qgt_2d(wf):
    """S = dO^T dO / ns (num_params, num_params) float64 from the per-sample log-derivatives of the resident batch of the 2D RNN.
    For diagnostics and small models."""
    return _real_qgt(wf.log_derivatives_2d())


def train_tfim2d(wf, Jz, Bx, params, numsteps=100, numsamples=500, learningrate=1e-2, diag_shift=1e-3, seed=111, scope="RNNwavefunction",
                 solver="device"):
    """Minimise the square-lattice TFIM energy of `wf` (a NativeWavefunction of MDRNN2D holding `params`) by minSR, the host loop of
    train_tfim: vmc_step (samples, local energies, moments; the batch stays resident) -> minsr_direction_2d -> theta -= lr delta ->
    set_params_flat.  Jz: a scalar or one entry per site in the order of vmc_step's couplings.  The batches are drawn as
    training.run_2DTFIM_2DRNN draws them (seed, step = iteration), so iteration 0 has that driver's moments from the same seed.
    Returns (meanEnergy, varEnergy), one entry per iteration 0..numsteps; the trained parameters are left in
    train_tfim2d.last_params and keep the dtype of `params`."""
    _check_shift(diag_shift)
    _check_solver(solver)
    if int(numsteps) < 0 or int(numsamples) < 2:
        raise ValueError("numsteps must be >= 0 and numsamples >= 2, got %r and %r" % (numsteps, numsamples))
    N = wf.N                                            # Nx Ny sites
    if np.size(Jz) not in (1, N):
        raise ValueError("Jz must be a scalar or have %d entries, got %d" % (N, np.size(Jz)))
    jz = np.broadcast_to(np.asarray(Jz, dtype=np.float64).ravel(), (N,))
    couplings = np.concatenate([jz, [float(Bx)]])
    dtype = next(iter(params.values())).dtype
    theta = flatten_params(wf, params, scope).astype(dtype).astype(np.float64)
    wf.set_params_flat(theta)
    meanEnergy, varEnergy = [], []
    theta = _real_host_loop(wf, "_2d", theta, dtype, couplings, numsteps, numsamples, learningrate, diag_shift, seed, solver, meanEnergy, varEnergy)
    train_tfim2d.last_params = unflatten_params(wf, theta, params, scope)
    return meanEnergy, varEnergy


# ---- the LSTM wave function (docs/sr_lstm.md) -------------------------------------------------------------------------------------
# psi = sqrt(P) real and positive on the raster path: the positive model's formulas and solve, on the rnnwf_*_lstm entries of an
# LSTM1D_F64 handle.  Its resident batch comes from wf.lstm_load_batch or wf.sr_step_lstm: vmc_step leaves an LSTM handle none.

def minsr_direction_lstm(wf, diag_shift, solver="host"):
    """delta (num_params,) float64 on the resident batch of the LSTM wave function `wf` (lstm_load_batch / sr_step_lstm), flat
    order of wf._layout().  solver "host": the Gram matrix to the host, LAPACK Cholesky, sr_apply_lstm; "device": wf.sr_direction_lstm."""
    return _real_direction(wf, "_lstm", diag_shift, solver)


def qgt_lstm(wf):
    """S = dO^T dO / ns (num_params, num_params) float64 from the per-sample log-derivatives of the resident batch of the LSTM wave
    function.  For diagnostics and small models."""
    return _real_qgt(wf.log_derivatives_lstm())


def train_tfim_lstm(wf, Jz, Bx, params, numsteps=100, numsamples=500, learningrate=1e-2, diag_shift=1e-3, seed=111, scope="RNNwavefunction",
                    solver="device"):
    """Minimise the square-lattice TFIM energy of `wf` (a NativeWavefunction of LSTM1D_F64 holding `params`) by minSR, with
    train_tfim2d's semantics: per iteration 0..numsteps a batch drawn at (seed, step = iteration), the minSR direction on it,
    theta -= lr delta, set_params_flat.  solver "device": one wf.sr_step_lstm per iteration (the fused step and the whole direction
    with one host synchronisation).  solver "host": wf.vmc_step with its samples and energies returned, wf.lstm_load_batch, the
    Gram matrix to the host, LAPACK Cholesky, sr_apply_lstm.  Both see the same batches.  Jz: a scalar or one entry per site in the
    order of vmc_step's couplings.  Returns (meanEnergy, varEnergy), one entry per iteration; the trained parameters are left in
    train_tfim_lstm.last_params and keep the dtype of `params`.  Whole iterations without the host (sr_train_steps) are not
    implemented for the LSTM: there is no device_steps argument."""
    lam = _check_shift(diag_shift)
    _check_solver(solver)
    if int(numsteps) < 0 or int(numsamples) < 2:
        raise ValueError("numsteps must be >= 0 and numsamples >= 2, got %r and %r" % (numsteps, numsamples))
    N = wf.N                                            # Nx Ny sites
    if np.size(Jz) not in (1, N):
        raise ValueError("Jz must be a scalar or have %d entries, got %d" % (N, np.size(Jz)))
    jz = np.broadcast_to(np.asarray(Jz, dtype=np.float64).ravel(), (N,))
    couplings = np.concatenate([jz, [float(Bx)]])
    dtype = next(iter(params.values())).dtype
    theta = flatten_params(wf, params, scope).astype(dtype).astype(np.float64)
    wf.set_params_flat(theta)
    meanEnergy, varEnergy = [], []
    for it in range(int(numsteps) + 1):
        if solver == "device":
            out = wf.sr_step_lstm(int(numsamples), seed, it, couplings, lam)
            delta = out["direction"]
        else:
            out = wf.vmc_step(int(numsamples), seed, it, couplings, want_samples=True, want_eloc=True)
            wf.lstm_load_batch(out["samples"], out["eloc"])
            delta = _real_direction(wf, "_lstm", lam, "host")
        s1, s2, n, _ = out["moments"]
        meanE = s1 / n
        meanEnergy.append(meanE)
        varEnergy.append(s2 / n - meanE ** 2)
        theta = (theta - learningrate * delta).astype(dtype).astype(np.float64)
        wf.set_params_flat(theta)
    train_tfim_lstm.last_params = unflatten_params(wf, theta, params, scope)
    return meanEnergy, varEnergy
