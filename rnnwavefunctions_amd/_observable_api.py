"""The one implementation behind the Pauli, Renyi and minimize wrappers of observables.py, observables_stack.py, observables_2d.py,
observables_complex.py, observables_lstm.py and training.minimize_hamiltonian.  A Family names what differs between the wave-function families - the
NativeWavefunction methods, the shape caller samples take, the centre site, two wordings -; the functions below take one and a
NativeWavefunction that the calling module's guard (_native, _native_stack, ...) has already accepted.  Private: the public names,
signatures and docstrings live in the calling modules."""
from collections import namedtuple

import numpy as np

from . import observables as O
from . import training as T

# step, train_steps, regions: names of the NativeWavefunction methods; chain_shape(nat): the shape of one chain of caller samples;
# centre(nat): the default centre site of correlations; label: what check_device_steps calls the driver; sites: the pairs error's noun;
# fused: name of a method that runs step AND the gradient of the cost in one call (dict with "moments" and "grads"), for a family whose
# batch vmc_gradient does not serve; None: step, then training.cost_gradient
Family = namedtuple("Family", "step train_steps regions chain_shape centre label sites fused", defaults=(None,))


def _chain(nat):
    return (nat.N,)


GRU = Family("pauli_step", "pauli_train_steps", "renyi2_regions", _chain, None, "minimize_hamiltonian", None)
STACK = Family("pauli_step_stack", "pauli_train_steps_stack", "renyi2_regions_stack", _chain, lambda nat: nat.N // 2,
               "observables_stack.minimize_hamiltonian", "sites")
LATTICE = Family("pauli_step_2d", "pauli_train_steps_2d", "renyi2_regions_2d", lambda nat: (nat.nx, nat.ny),
                 lambda nat: (nat.nx // 2) * nat.ny + nat.ny // 2, "observables_2d.minimize_hamiltonian", "lattice sites")
COMPLEX = Family("pauli_step_complex", "pauli_train_steps_complex", "renyi2_regions_complex", _chain, None, "minimize_hamiltonian", None)
# the LSTM cell (observables_lstm.py): its minimize loop takes the fused step and keeps refusing device_steps (the device-resident loop
# is training_lstm.minimize_hamiltonian_device)
LSTM = Family("pauli_step_lstm", None, "renyi2_regions_lstm", _chain, lambda nat: nat.N // 2, "observables_lstm.minimize_hamiltonian", "sites",
              "lstm_pauli_gradient_step")


def chains(fam, nat, samples, rows):
    """caller samples as `rows` chains in the family's shape; None (a device draw) stays None"""
    return None if samples is None else np.asarray(samples).reshape((int(rows),) + fam.chain_shape(nat))


def check_sites(nat, ham):
    if ham.N != nat.N:
        raise ValueError("the Hamiltonian has %d sites, the wave function %d" % (ham.N, nat.N))


def pauli_expectations(fam, nat, strings, numsamples, seed, step, samples):
    flip, sign, factor = O.pauli_terms(strings, nat.N)
    value, err = np.zeros(len(factor)), np.zeros(len(factor))
    real = np.flatnonzero(factor.imag == 0.0)
    if real.size:
        out = getattr(nat, fam.step)(flip[real], sign[real], np.ones(real.size), int(numsamples), samples=chains(fam, nat, samples, numsamples),
                                     seed=seed, step=step)
        mean, e = O.pauli_from_sums(out["term_sums"], numsamples)
        value[real], err[real] = factor.real[real] * mean, e
    return {"value": value, "err": err}


def local_energies(fam, nat, ham, numsamples, seed, step, samples, want_eloc):
    """the family's step on the terms of `ham`: its dict, with the moments of the local energies"""
    return getattr(nat, fam.step)(ham.flip, ham.sign, ham.coeff, int(numsamples), samples=chains(fam, nat, samples, numsamples), seed=seed, step=step,
                                  want_eloc=want_eloc)


def energy(fam, nat, ham, numsamples, seed, step, samples, want_eloc):
    check_sites(nat, ham)
    out = local_energies(fam, nat, ham, numsamples, seed, step, samples, want_eloc)
    m = out["moments"]
    mean = m[0] / m[2]
    var = max(m[1] / m[2] - mean * mean, 0.0)
    res = {"mean": mean, "var": var, "err": float(np.sqrt(var / m[2]))}
    if want_eloc:
        res["eloc"] = out["eloc"]
    return res


def correlations(fam, nat, numsamples, pairs, seed, step, samples):
    N, n = nat.N, int(numsamples)
    if pairs is None:
        c = fam.centre(nat)
        pairs = [(c, k) for k in range(N) if k != c]
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    if np.any(pairs < 0) or np.any(pairs >= N) or np.any(pairs[:, 0] == pairs[:, 1]):
        raise ValueError("pairs must name two distinct %s in 0..%d each" % (fam.sites, N - 1))
    npair = len(pairs)
    flip = np.zeros((N + npair, N), dtype=np.int32)
    flip[np.arange(N), np.arange(N)] = 1
    for k, (a, b) in enumerate(pairs):
        flip[N + k, [a, b]] = 1
    out = getattr(nat, fam.step)(flip, np.zeros_like(flip), np.ones(len(flip)), n, samples=chains(fam, nat, samples, n), seed=seed, step=step,
                                 want_log_ratio=True, want_samples=True)
    _, index = O.group_by_mask(flip)                     # (a, b) and (b, a) share a row
    r = np.exp(out["log_ratio"])[index]                  # (N + P, n)
    s = 2.0 * out["samples"].reshape(n, N).T - 1.0       # (N, n)

    def stats(v):
        return v.mean(axis=-1), v.std(axis=-1) / np.sqrt(n)

    a, b = pairs[:, 0], pairs[:, 1]
    res = {"pairs": pairs}
    res["z"], res["z_err"] = stats(s)
    res["x"], res["x_err"] = stats(r[:N])
    res["zz"], res["zz_err"] = stats(s[a] * s[b])
    res["xx"], res["xx_err"] = stats(r[N:])
    z, x = res["z"], res["x"]
    res["zz_c"] = res["zz"] - z[a] * z[b]
    res["xx_c"] = res["xx"] - x[a] * x[b]
    res["zz_c_err"] = stats(s[a] * s[b] - z[b][:, None] * s[a] - z[a][:, None] * s[b])[1]
    res["xx_c_err"] = stats(r[N:] - x[b][:, None] * r[a] - x[a][:, None] * r[b])[1]
    return res


def regions(fam, nat, masks, numpairs, seed, step, samples, **log_ratio):
    """the family's regions method on 2 numpairs chains: (its dict, the caller's chains as handed to it)"""
    s = chains(fam, nat, samples, 2 * int(numpairs))
    return getattr(nat, fam.regions)(masks, int(numpairs), samples=s, seed=seed, step=step, **log_ratio), s


def renyi2_regions(fam, nat, masks, numpairs, seed, step, samples):
    return O.renyi2_from_sums(regions(fam, nat, masks, numpairs, seed, step, samples)[0]["sums"], numpairs)


def mutual_log_ratios(fam, nat, a, b, numpairs, seed, step, samples):
    """per-pair log r of A, B and A u B (disjoint masks a, b) on the same pairs, one call"""
    return regions(fam, nat, np.stack([a, b, a | b]), numpairs, seed, step, samples, log_ratio=True)[0]["log_ratio"]


def renyi2_mutual_information(fam, nat, a, b, numpairs, seed, step, samples):
    return O.mutual_information2_from_log_ratios(*mutual_log_ratios(fam, nat, a, b, numpairs, seed, step, samples))


def minimize_loop(step, train_steps, mean_of, nat, ham, params, scope, numsteps, numsamples, learningrate, seed, opt, device_steps, verbose,
                  fused=None, lr_of_it=None):
    """Iterations 0..numsteps of  step (samples, local energies of `ham`, moments; the batch stays resident) -> training.cost_gradient ->
    opt.step -> set_params,  or - with device_steps - the same iterations through train_steps in chunks.  step, train_steps: bound
    NativeWavefunction methods; mean_of(s1, si, n): an entry of meanEnergy from the moments.  Returns (meanEnergy, varEnergy, params).
    fused: a bound method that takes step's place and training.cost_gradient's in one call (shapes= the tensors' shapes; its dict holds
    "moments" and the unscoped "grads").  lr_of_it(learningrate, it): the learning rate of iteration it; None: learningrate."""
    opt = opt or T.Adam()
    params = {k: np.array(v) for k, v in params.items()}
    nat.set_params(params, scope=scope)
    if device_steps:
        nat.adam_set_state(None, None, 0)
        meanEnergy, varEnergy = T.hamiltonian_steps_on_device(train_steps, ham, numsteps, numsamples, learningrate, seed, device_steps, verbose,
                                                              mean_of)
        return meanEnergy, varEnergy, nat.get_params_dict(params, scope)
    meanEnergy, varEnergy = [], []
    shapes = {k[len(scope) + 1:]: v.shape for k, v in params.items()}
    for it in range(numsteps + 1):
        if fused is not None:
            out = fused(ham.flip, ham.sign, ham.coeff, numsamples, seed=seed, step=it, shapes=shapes)
        else:
            out = step(ham.flip, ham.sign, ham.coeff, numsamples, seed=seed, step=it)
        s1, s2, n, si = out["moments"]
        meanE = mean_of(s1, si, n)
        varE = s2 / n - (s1 / n) ** 2
        meanEnergy.append(meanE)
        varEnergy.append(varE)
        if verbose and it % 10 == 0:
            print("mean(E): {0}, var(E): {1}, #samples {2}, #Step {3} \n\n".format(meanE, varE, numsamples, it))
        grads = T.cost_gradient(nat, params, scope, meanE, n) if fused is None else {scope + "/" + k: v for k, v in out["grads"].items()}
        params = opt.step(params, grads, learningrate if lr_of_it is None else lr_of_it(learningrate, it))
        nat.set_params(params, scope=scope)
    return meanEnergy, varEnergy, params


def minimize_family(fam, guard, wf, ham, params, numsteps, numsamples, learningrate, seed, scope, opt, comm, verbose, device_steps,
                    lr_of_it=None):
    """the drivers of the real families: their refusals in their order, then minimize_loop; guard(wf) gives the NativeWavefunction"""
    device_steps = T.check_device_steps(device_steps, opt, fam.label)
    if device_steps is not None and fam.train_steps is None:
        raise ValueError("%s: device_steps is not available for this family: it has no device-resident Adam (docs/lstm.md, \"Out of "
                         "scope\"); use the host loop (device_steps=None)" % fam.label)
    if comm is not None:
        raise ValueError("minimize_hamiltonian runs in one process on one GPU: no communicator (comm=%r)" % (comm,))
    nat = guard(wf)
    check_sites(nat, ham)
    return minimize_loop(getattr(nat, fam.step), getattr(nat, fam.train_steps) if fam.train_steps else None, lambda s1, si, n: s1 / n, nat, ham,
                         params, scope, numsteps, numsamples, learningrate, seed, opt, device_steps, verbose,
                         fused=getattr(nat, fam.fused) if fam.fused else None, lr_of_it=lr_of_it)
