"""GPU parity tests of the positive-RNN path: HIP kernels (through the C ABI) vs the CPU oracle.

Tolerances (fp32 cell, north_star: <E>/N within 1e-4 of the reference):
  log P(sigma)      : |hip - oracle| <= 2e-6 * N + 2e-6   (both are fp32 evaluations; the oracle in
                      fp64 differs from the fp32 oracle by about the same amount, asserted below)
  E_loc             : relative 2e-5 per sample
  samples           : identical rows except near-ties |u - p0| < 1e-5 (rare, counted)
"""
import os

import numpy as np
import pytest

from conftest import all_configs, golden_params
from oracle import estimators as E
from oracle import models as M
from oracle import philox
from rnnwavefunctions_amd import params as P

pytestmark = pytest.mark.gpu

SCOPE = "RNNwavefunction"


def make_wf(model, N, H, prm, ny=1):
    from rnnwavefunctions_amd import _lib
    wf = _lib.NativeWavefunction(model, N, ny, (H,))
    wf.set_params(prm, scope=SCOPE)
    return wf


def trained_like(H, seed, dtype=np.float32, heads=("wf_dense",)):
    return P.randomize_biases(P.scale_kernels(P.init_gru_params([H], seed=seed, dtype=dtype, heads=heads), 2.0), seed + 1)


@pytest.mark.parametrize("N,H,B", [(10, 12, 37), (33, 20, 200), (40, 36, 64), (70, 50, 130), (20, 64, 48), (24, 100, 40),
                                   (12, 101, 24), (12, 128, 24), (9, 133, 20), (8, 200, 20), (6, 256, 17), (5, 260, 16)])     # > 100 units: the image is read through L2
def test_log_prob_matches_oracle(N, H, B):
    from rnnwavefunctions_amd import _lib
    prm = trained_like(H, seed=H)
    wf = make_wf(_lib.MODEL_GRU1D, N, H, prm)
    s = np.random.RandomState(N).randint(0, 2, (B, N)).astype(np.int32)
    got = wf.log_prob(s)
    ref = M.prnn_log_probability(prm, s)
    prm64 = {k: v.astype(np.float64) for k, v in prm.items()}
    ref64 = M.prnn_log_probability(prm64, s, dtype=np.float64)
    err = np.abs(got - ref).max()
    err64 = np.abs(got - ref64).max()
    oracle_gap = np.abs(ref - ref64).max()
    print("N=%d H=%d: |hip-oracle32|=%.2e |hip-oracle64|=%.2e |oracle32-oracle64|=%.2e" % (N, H, err, err64, oracle_gap))
    assert err <= 2e-6 * N + 2e-6
    assert err64 <= 2e-6 * N + 2e-6


def test_normalisation_on_gpu():
    from rnnwavefunctions_amd import _lib
    N, H = 12, 20
    prm = trained_like(H, seed=3)
    wf = make_wf(_lib.MODEL_GRU1D, N, H, prm)
    lp = wf.log_prob(all_configs(N))
    assert abs(np.exp(lp).sum() - 1) < 2e-5


def test_empty_and_bad_inputs():
    from rnnwavefunctions_amd import _lib
    prm = trained_like(10, seed=1)
    wf = make_wf(_lib.MODEL_GRU1D, 8, 10, prm)
    assert wf.log_prob(np.zeros((0, 8), dtype=np.int32)).shape == (0,)
    with pytest.raises(ValueError):
        wf.log_prob(np.zeros((4, 9), dtype=np.int32))
    with pytest.raises(ValueError):
        wf.set_params({"wf_dense/bias": np.zeros(3, dtype=np.float32)})
    with pytest.raises(ValueError):
        _lib.NativeWavefunction(_lib.MODEL_GRU1D, 8, 1, (10, 10, 10, 10, 10))   # more than four layers: loud refusal
    wf2 = _lib.NativeWavefunction(_lib.MODEL_GRU1D, 8, 1, (10,))
    with pytest.raises(_lib.RnnwfError):
        wf2.log_prob(np.zeros((4, 8), dtype=np.int32))                   # parameters never committed


def test_tfim_eloc_matches_reference_golden(golden_estimators):
    """G4a: the reference's own Ising_local_energies driven by the oracle log-probs (N=10, 2 chunks)."""
    from rnnwavefunctions_amd import _lib
    g = golden_estimators
    prm = golden_params(g, "g4a")
    N = g["g4a_samples"].shape[1]
    wf = make_wf(_lib.MODEL_GRU1D, N, 12, prm)
    ns = g["g4a_samples"].shape[0]
    lp = np.zeros((N + 1) * ns)
    e = wf.tfim_eloc(g["g4a_samples"], g["g4a_Jz"], float(g["g4a_Bx"]), log_probs=lp)
    print("G4a: max|lp diff|=%.2e  max rel E diff=%.2e" % (np.abs(lp - g["g4a_logp"]).max(),
                                                        np.abs(e / g["g4a_eloc"] - 1).max()))
    assert np.allclose(lp, g["g4a_logp"], rtol=0, atol=3e-5)
    assert np.allclose(e, g["g4a_eloc"], rtol=2e-5, atol=2e-5)
    e0 = wf.tfim_eloc(g["g4a_samples"][:50], g["g4a_Jz"], 0.0)
    assert np.allclose(e0, g["g4a_eloc_bx0"], atol=1e-12)          # Bx = 0: diagonal only, exact


@pytest.mark.parametrize("N,H,ns", [(33, 20, 50), (65, 50, 21), (16, 100, 17), (12, 128, 21), (9, 196, 17), (8, 256, 17)])
def test_tfim_eloc_fused_equals_reference_formulation(N, H, ns):
    from rnnwavefunctions_amd import _lib
    prm = trained_like(H, seed=N)
    wf = make_wf(_lib.MODEL_GRU1D, N, H, prm)
    rng = np.random.RandomState(5)
    s = rng.randint(0, 2, (ns, N)).astype(np.int32)
    Jz = 1.0 + 0.1 * rng.standard_normal(N)
    lp = np.zeros((N + 1) * ns)
    e = wf.tfim_eloc(s, Jz, 1.3, log_probs=lp)
    e_ref, lp_ref = E.ising_local_energies(Jz, 1.3, s, lambda x: M.prnn_log_probability(prm, x), return_log_probs=True)
    print("N=%d H=%d: max|lp diff|=%.2e max rel E diff=%.2e" % (N, H, np.abs(lp - lp_ref.ravel()).max(),
                                                               np.abs(e / e_ref - 1).max()))
    assert np.allclose(lp, lp_ref.ravel(), rtol=0, atol=2e-6 * N + 2e-6)
    assert np.allclose(e, e_ref, rtol=2e-5)
    # the same numbers through the un-fused route: every flipped configuration scored from site 0
    queue = np.repeat(s[None], N + 1, axis=0)
    for i in range(N):
        queue[i + 1, :, i] ^= 1
    lp_full = wf.log_prob(queue.reshape(-1, N))
    # prefix reuse changes nothing but f32 rounding: the base and the flip kernel are separate instantiations
    # of the same step, and hipcc may associate their f32 sums differently (1 ulp per site)
    assert np.allclose(lp, lp_full, rtol=0, atol=3e-7 * N + 1e-6)


def test_sampling_matches_oracle_stream():
    from rnnwavefunctions_amd import _lib
    N, H, ns = 40, 20, 1000
    prm = trained_like(H, seed=9)
    wf = make_wf(_lib.MODEL_GRU1D, N, H, prm)
    s, lg = wf.sample(ns, seed=111, step=7, sample_offset=0, return_log=True)
    u = philox.uniforms(111, 7, 0, ns, N)
    s_ref, lg_ref = M.prnn_sample(prm, N, u)
    bad = np.where((s != s_ref).any(axis=1))[0]
    print("sampler: %d of %d rows differ from the oracle" % (len(bad), ns))
    assert len(bad) <= 2
    probs = M.prnn_site_probs(prm, s_ref)
    for b in bad:                                                   # a differing row must be a near-tie
        n0 = np.argmax(s[b] != s_ref[b])
        assert abs(u[b, n0] - probs[b, n0, 0]) < 1e-5
    good = np.setdiff1d(np.arange(ns), bad)
    assert np.allclose(lg[good], lg_ref[good], rtol=0, atol=2e-6 * N + 2e-6)
    # shard invariance: two half batches with the right sample_offset reproduce the full batch
    a = wf.sample(600, seed=111, step=7, sample_offset=0)
    b = wf.sample(400, seed=111, step=7, sample_offset=600)
    assert np.array_equal(np.concatenate([a, b]), s)
    # a different step gives a different batch
    assert not np.array_equal(wf.sample(ns, seed=111, step=8), s)


def test_parity_symmetric_model():
    from rnnwavefunctions_amd import _lib
    N, H, ns = 12, 20, 40
    prm = trained_like(H, seed=4)
    wf = make_wf(_lib.MODEL_GRU1D_PARITY, N, H, prm)
    s = np.random.RandomState(1).randint(0, 2, (ns, N)).astype(np.int32)
    lp = wf.log_prob(s)
    ref = M.prnn_paritysym_log_probability(prm, s)
    assert np.allclose(lp, ref, rtol=0, atol=5e-5)
    # the combine is symmetric in the two directions: what is left is a few ulp of its exp and log (tests/parity_reference.py: bound)
    assert np.all(np.abs(lp - wf.log_prob(s[:, ::-1])) <= 8 * 2.0 ** -52 * np.maximum(1.0, np.abs(lp)))
    Jz = np.ones(N)
    e = wf.tfim_eloc(s, Jz, 1.0)
    e_ref = E.ising_local_energies(Jz, 1.0, s, lambda x: M.prnn_paritysym_log_probability(prm, x))
    assert np.allclose(e, e_ref, rtol=5e-5)


def test_gru_f64_on_2d_lattice_matches_reference_golden(golden_estimators):
    """G4c: 2DTFIM_1DRNN estimator (reference code) driven by the f64 oracle."""
    from rnnwavefunctions_amd import _lib
    g = golden_estimators
    prm = golden_params(g, "g4c")
    Nx, Ny = (int(v) for v in g["g4c_shape"])
    wf = make_wf(_lib.MODEL_GRU1D_F64, Nx, 7, prm, ny=Ny)
    s = g["g4c_samples"]
    lp = np.zeros((Nx * Ny + 1) * s.shape[0])
    e = wf.tfim_eloc(s, g["g4c_Jz"], float(g["g4c_Bx"]), log_probs=lp)
    print("G4c: max|lp diff|=%.2e" % np.abs(lp - g["g4c_logp"]).max())
    assert np.allclose(lp, g["g4c_logp"], rtol=0, atol=1e-10)
    assert np.allclose(e, g["g4c_eloc"], rtol=1e-10)


@pytest.mark.parametrize("Nx,Ny,H,L", [(3, 4, 7, 2), (4, 4, 20, 2), (3, 3, 36, 2), (4, 3, 10, 3), (3, 3, 20, 3), (4, 3, 36, 3),
                                       (3, 3, 37, 2), (4, 4, 50, 2), (3, 3, 68, 2), (4, 3, 50, 3), (3, 2, 68, 3),      # 37..68 units: upper images through L2
                                       (3, 3, 20, 4), (3, 2, 50, 4)])
def test_stacked_gru_f64_on_2d_lattice_matches_oracle(Nx, Ny, H, L):
    """2DTFIM_1DRNN with units=[num_units]*num_layers (Training1DRNN_2DTFIM.py:94): log-probabilities, the sampler's
    stream and the 2D local energies against the float64 oracle."""
    from rnnwavefunctions_amd import _lib
    N = Nx * Ny
    prm = P.randomize_biases(P.scale_kernels(P.init_gru_params([H] * L, seed=H + L, dtype=np.float64), 1.5), H)
    wf = _lib.NativeWavefunction(_lib.MODEL_GRU1D_F64, Nx, Ny, (H,) * L)
    wf.set_params(prm, scope=SCOPE)
    rng = np.random.RandomState(H)
    s = rng.randint(0, 2, size=(37, N))
    lp = wf.log_prob(s)
    ref = M.prnn_log_probability(prm, s, dtype=np.float64)
    print("stacked f64 L=%d H=%d: max |lp - oracle| = %.2e" % (L, H, np.abs(lp - ref).max()))
    assert np.allclose(lp, ref, rtol=0, atol=1e-11 * N)
    smp = wf.sample(200, seed=9, step=1).reshape(200, N)
    assert np.allclose(wf.log_prob(smp), M.prnn_log_probability(prm, smp, dtype=np.float64), rtol=0, atol=1e-11 * N)
    Jz = np.ones((Nx, Ny))
    e = wf.tfim_eloc(smp, Jz, 2.0)
    e_ref = E.ising2d_local_energies(Jz, 2.0, Nx, Ny, smp, lambda x: M.prnn_log_probability(prm, x, dtype=np.float64))
    assert np.allclose(e, e_ref, rtol=1e-9)


def test_vmc_step_is_sample_plus_eloc_plus_moments():
    from rnnwavefunctions_amd import _lib
    N, H, ns = 30, 50, 333
    prm = trained_like(H, seed=2)
    wf = make_wf(_lib.MODEL_GRU1D, N, H, prm)
    Jz = np.ones(N)
    out = wf.vmc_step(ns, seed=5, step=3, couplings=np.append(Jz, 1.0), want_samples=True, want_eloc=True)
    assert np.array_equal(out["samples"], wf.sample(ns, seed=5, step=3))
    e = wf.tfim_eloc(out["samples"], Jz, 1.0)
    assert np.allclose(out["eloc"], e, rtol=1e-12)
    m = out["moments"]
    assert m[2] == ns
    assert np.isclose(m[0] / ns, e.mean(), rtol=1e-12)
    assert np.isclose(m[1] / ns - (m[0] / ns) ** 2, e.var(), rtol=1e-9)
    assert wf.allreduce_moments(m).tolist() == m.tolist()           # single rank: identity


def test_headline_config_energy_per_site_within_north_star():
    """BASELINE config 2 (N=80, h=50, ns=10000): the WHOLE batch against the oracle on the same sample matrix - the C
    restatement of the reference formulation (81 x 10 000 chains scored from site 0 in <= 25 000-row chunks, oracle/c) -
    north_star's acceptance statement (<E>/N within 1e-4 of the reference), held to 1e-5 here, per sample and for the mean;
    plus the NumPy oracle on a subset (the two oracles are separate restatements) and size-independent properties."""
    from oracle import cport
    from rnnwavefunctions_amd import _lib
    N, H, ns = 80, 50, 10000
    prm = P.init_gru_params([H], seed=111)
    wf = make_wf(_lib.MODEL_GRU1D, N, H, prm)
    Jz = np.ones(N)
    out = wf.vmc_step(ns, seed=111, step=0, couplings=np.append(Jz, 1.0), want_samples=True, want_eloc=True)
    s, e, m = out["samples"], out["eloc"], out["moments"]
    assert wf.engine_name() == "bf16x3"
    assert s.shape == (ns, N) and set(np.unique(s)) <= {0, 1}
    assert np.all(np.isfinite(e))
    e_ref = cport.ising_local_energies(prm, Jz, 1.0, s)
    per_site = np.abs(e - e_ref).max() / N
    d_mean = abs(e.mean() - e_ref.mean()) / N
    print("cfg2, all %d samples: max |E_loc - oracle| / N = %.2e ; |<E> - <E>_oracle| / N = %.2e ; <E>/N = %.6f" %
          (ns, per_site, d_mean, e.mean() / N))
    assert per_site < 1e-5
    assert d_mean < 1e-5                                           # north_star asks for 1e-4
    assert abs(m[0] / m[2] - e_ref.mean()) / N < 1e-5              # the moments the step returns are those of this batch
    sub = np.arange(0, ns, ns // 64)[:64]
    e_np = E.ising_local_energies(Jz, 1.0, s[sub], lambda x: M.prnn_log_probability(prm, x))
    assert np.abs(e[sub] - e_np).max() / N < 1e-5
    # off-diagonal part is a sum of N positive terms times -Bx: E_loc <= diagonal energy
    diag = -(np.where(s[:, :-1] == s[:, 1:], 1.0, -1.0)).sum(axis=1)
    assert np.all(e < diag)
    # the same batch on the f32-input MFMA: the two engines agree per sample far inside the tolerance
    import os
    os.environ["RNNWF_ENGINE"] = "f32"
    try:
        wf32 = make_wf(_lib.MODEL_GRU1D, N, H, prm)
    finally:
        del os.environ["RNNWF_ENGINE"]
    e32 = wf32.tfim_eloc(s, Jz, 1.0)
    print("cfg2: max |E_loc(bf16x3) - E_loc(f32 MFMA)| / N = %.2e" % (np.abs(e - e32).max() / N))
    assert np.abs(e32 - e_ref).max() / N < 1e-5 and np.abs(e - e32).max() / N < 1e-5


def test_rccl_all_reduce_single_rank():
    """The RCCL transport end to end with a one-rank communicator (the multi-rank case needs several GPUs
    and is run by the driver's scaling bench; its host logic is covered by tests/test_distributed_cpu.py)."""
    from rnnwavefunctions_amd import _lib
    prm = trained_like(10, seed=1)
    wf = make_wf(_lib.MODEL_GRU1D, 8, 10, prm)
    uid = wf.comm_unique_id()
    assert len(uid) == _lib.UNIQUE_ID_BYTES
    wf.comm_init(uid, 0, 1)
    m = np.array([1.5, -2.0, 64.0, 0.25])
    assert np.array_equal(wf.allreduce_moments(m), m)
    assert wf.comm_info() == {"nranks": 1, "rank": 0, "device": 0}        # ncclCommCount / ncclCommUserRank
    # the in-step form: the all-reduce runs on the stream inside rnnwf_vmc_step
    c = np.append(np.ones(8), 1.0)
    m0 = wf.vmc_step(64, seed=3, step=0, couplings=c)["moments"]
    wf.comm_reduce_in_step(True)
    assert np.array_equal(wf.vmc_step(64, seed=3, step=0, couplings=c)["moments"], m0)
    # the gradient's two collectives, walked with the one-rank communicator (a sum over one rank changes nothing): rnnwf_allreduce_grads
    # on the device-side flat gradient, and the in-stream all-reduce inside rnnwf_train_steps
    shapes = {k[len(SCOPE) + 1:]: v.shape for k, v in prm.items()}
    g0 = wf.vmc_gradient(m0[0] / m0[2], m0[2], shapes)
    g1 = wf.vmc_gradient(m0[0] / m0[2], m0[2], shapes, allreduce=True)           # rnnwf_allreduce_grads
    for k in g0:
        assert np.array_equal(g0[k], g1[k]), k
    plain = make_wf(_lib.MODEL_GRU1D, 8, 10, prm)
    lrs = [5e-3] * 10
    ma = wf.train_steps(64, 3, 0, c, lrs)
    mb = plain.train_steps(64, 3, 0, c, lrs)
    assert np.array_equal(ma, mb) and ma[0][0] != ma[-1][0]
    pa, pb = wf.get_params_dict(prm, SCOPE), plain.get_params_dict(prm, SCOPE)
    for k in prm:
        assert np.array_equal(pa[k], pb[k]), k
    with pytest.raises(ValueError):
        wf.comm_init(uid, 3, 2)


def _rccl_rank(rank, world, port, out):
    import os
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), GLOO_SOCKET_IFNAME="lo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    from rnnwavefunctions_amd import _lib
    from rnnwavefunctions_amd import distributed as D
    wf = _lib.NativeWavefunction(_lib.MODEL_GRU1D, 16, 1, (20,), device=rank)      # one rank per GPU
    wf.set_params(trained_like(20, seed=1), scope=SCOPE)
    r, w = D.init_rccl_from_env(wf)
    info = wf.comm_info()
    ns = 300
    m = wf.vmc_step(ns, seed=7, step=0, couplings=np.append(np.ones(16), 1.0), sample_offset=rank * ns)["moments"]
    g = wf.allreduce_moments(m)
    wf.comm_reduce_in_step(True)          # the same sum, taken on the stream inside the step
    g2 = wf.vmc_step(ns, seed=7, step=0, couplings=np.append(np.ones(16), 1.0), sample_offset=rank * ns)["moments"]
    assert np.allclose(g2, g, rtol=1e-14)
    if rank == 0:
        np.save(out, np.concatenate([g, [info["nranks"], info["rank"], info["device"], w]]))
    import torch.distributed as dist
    dist.barrier()
    dist.destroy_process_group()


def test_rccl_all_reduce_over_two_gpus(tmp_path):
    """Two ranks, one GPU each, through rnnwf_comm_unique_id -> launcher broadcast -> rnnwf_comm_init (ncclCommInitRank
    with nranks = 2) -> rnnwf_allreduce_moments: the reduced moments equal those of the single-device batch of both
    shards.  Skipped where fewer than two GPUs are visible (RCCL refuses two ranks on one device)."""
    import socket
    from rnnwavefunctions_amd import _lib
    _lib.load_library()                 # the product library (and /opt/rocm's HIP runtime) before torch's bundled copies
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs (this box has %d)" % torch.cuda.device_count())
    import torch.multiprocessing as mp
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    out = str(tmp_path / "g.npy")
    mp.spawn(_rccl_rank, args=(2, port, out), nprocs=2, join=True)
    g = np.load(out)
    assert list(g[4:]) == [2, 0, 0, 2]                      # ncclCommCount = 2, rank 0 on device 0
    wf = make_wf(_lib.MODEL_GRU1D, 16, 20, trained_like(20, seed=1))
    m = wf.vmc_step(600, seed=7, step=0, couplings=np.append(np.ones(16), 1.0))["moments"]
    assert g[2] == 600 and np.allclose(g[:4], m, rtol=1e-12)


def test_bench_launcher_flow_with_two_ranks():
    """The driver's multi-GPU command line (`python -m torch.distributed.run --nproc-per-node N bench.py --gpus N`) with
    two ranks.  On a one-GPU box both ranks sit on device 0 (--same-device): RCCL refuses that, every rank must then take
    the gloo road for the 32-byte all-reduce and the line must say so; with two GPUs the line carries rccl_nranks = 2.
    Either way: rendezvous, barriers, max-over-ranks timing, the sharded config-5 leg and ONE JSON line from rank 0."""
    import json
    import socket
    import subprocess
    import sys
    import torch
    two = torch.cuda.device_count() >= 2
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
           "--no-cpu-baseline", "--no-alt-engine", "--numsamples", "2000"] + ([] if two else ["--same-device"])
    if not two:
        # a scaling run that silently measured gloo is worse than none: without --allow-fallback the job exits 3 (every rank),
        # the line - with the reason - is still printed
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=root)
        assert r.returncode != 0 and "RCCL communicator could not be created" in r.stderr, r.stderr[-2000:]
        d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
        assert d["exit_code"] == 3 and "gloo" in d["transport_fallback"] and d["rccl_nranks"] is None
        cmd.append("--allow-fallback")
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["config"]["global_numsamples"] == 4000 and d["value"] > 0
    assert [x["rank"] for x in d["ranks"]] == [0, 1]
    if two:                         # RCCL itself is test_rccl_all_reduce_over_two_gpus' business; here: the line says which road it took
        assert (d["rccl_nranks"] == 2 and d["transport_fallback"] is None) or "gloo" in (d["transport_fallback"] or "")
        print("two GPUs: rccl_nranks", d["rccl_nranks"], "fallback", d["transport_fallback"])
    else:
        assert d["rccl_nranks"] is None and "gloo" in d["transport_fallback"]


@pytest.mark.parametrize("N,H,ns", [(1, 10, 5), (2, 10, 1), (32, 20, 17), (33, 20, 16), (64, 36, 31), (200, 100, 19)])
def test_edge_sizes(N, H, ns):
    """Ragged batches (ns not a multiple of the 16-chain tile, down to one sample), chain lengths around the 32-bit
    word boundaries of the packed spins, the largest BASELINE chain (N=200, num_units=100)."""
    from rnnwavefunctions_amd import _lib
    prm = trained_like(H, seed=N + H)
    wf = make_wf(_lib.MODEL_GRU1D, N, H, prm)
    out = wf.vmc_step(ns, seed=1, step=0, couplings=np.append(np.ones(N), 0.7), want_samples=True, want_eloc=True)
    s, e = out["samples"], out["eloc"]
    assert s.shape == (ns, N)
    e_ref = E.ising_local_energies(np.ones(N), 0.7, s, lambda x: M.prnn_log_probability(prm, x))
    assert np.allclose(e, e_ref, rtol=3e-5, atol=3e-5)
    assert np.allclose(wf.log_prob(s), M.prnn_log_probability(prm, s), atol=2e-6 * N + 2e-6)
    u = philox.uniforms(1, 0, 0, ns, N)
    s_ref, _ = M.prnn_sample(prm, N, u)
    assert (s != s_ref).any(axis=1).sum() <= 1


@pytest.mark.parametrize("N,H,ns", [(20, 10, 100), (33, 20, 50), (40, 36, 64), (65, 50, 37), (30, 64, 33), (25, 44, 40),
                                     (25, 49, 40), (25, 52, 40), (25, 37, 33), (18, 17, 33), (18, 21, 33),
                                     (20, 100, 40), (14, 70, 33), (12, 85, 70),           # > 68 units: w3 fragments through L2
                                     # both sides of every width-class boundary of the bf16x3 engine (split.hip / split_stream.hip):
                                     # flat <= 36 | aligned + special 37..50 | padded 51..52 | riders, LDS-resident 53..68 | streamed 69..100
                                     (21, 51, 33), (22, 53, 40), (19, 60, 33), (23, 68, 37), (21, 69, 40), (17, 96, 33), (15, 99, 21)])
def test_both_flip_engines_agree_with_the_f64_oracle(N, H, ns, monkeypatch):
    """The flip pass runs on the bf16x3 engine by default (three-way exact bf16 split of both operands, f32
    accumulate; csrc/split_core.h) and on the f32-input MFMA with RNNWF_ENGINE=f32.  Both must match the float64
    oracle to the same f32-level tolerance, and each other."""
    from rnnwavefunctions_amd import _lib
    prm = trained_like(H, seed=2 * N + H)
    prm64 = {k: v.astype(np.float64) for k, v in prm.items()}
    rng = np.random.RandomState(7)
    s = rng.randint(0, 2, (ns, N)).astype(np.int32)
    Jz = 1.0 + 0.1 * rng.standard_normal(N)
    e64, lp64 = E.ising_local_energies(Jz, 1.1, s, lambda x: M.prnn_log_probability(prm64, x, dtype=np.float64),
                                       return_log_probs=True)
    got = {}
    for engine in ("f32", "bf16x3"):
        monkeypatch.setenv("RNNWF_ENGINE", engine)
        wf = make_wf(_lib.MODEL_GRU1D, N, H, prm)            # the environment is read once, at rnnwf_create
        lp = np.zeros((N + 1) * ns)
        e = wf.tfim_eloc(s, Jz, 1.1, log_probs=lp)
        assert wf.engine_name() == ("bf16x3" if engine == "bf16x3" else "f32mfma")   # RNNWF_ENGINE pins the engine
        got[engine] = (e, lp)
        err_lp = np.abs(lp - lp64.ravel()).max()
        err_e = np.abs(e / e64 - 1).max()
        print("N=%d H=%d %-6s: max|lp - f64| = %.2e   max rel E err = %.2e" % (N, H, engine, err_lp, err_e))
        assert err_lp <= 2e-6 * N + 2e-6
        assert err_e <= 2e-5
    assert np.allclose(got["f32"][0], got["bf16x3"][0], rtol=2e-5)
    # without RNNWF_ENGINE a batch this small (fewer 32-chain tiles than two waves per SIMD) takes the 16-chain f32 flip kernel
    # (its base pass is then the default one - bf16 cooperative up to 52 units - where RNNWF_ENGINE=f32 pins the f32 base pass too)
    monkeypatch.delenv("RNNWF_ENGINE")
    wf = make_wf(_lib.MODEL_GRU1D, N, H, prm)
    e = wf.tfim_eloc(s, Jz, 1.1)
    assert wf.engine_name() == "f32mfma" and np.allclose(e, got["f32"][0], rtol=2e-5)
    monkeypatch.setenv("RNNWF_BASE", "f32")
    wf = make_wf(_lib.MODEL_GRU1D, N, H, prm)
    monkeypatch.delenv("RNNWF_BASE")
    assert np.array_equal(wf.tfim_eloc(s, Jz, 1.1), got["f32"][0])


def test_release_library_refuses_engine_switches_it_does_not_hold(monkeypatch):
    """The measured negatives of rounds 1-3 (four alternative bf16x3 engines and the 2D RNN's prefetching flip kernel, once selected
    through the values below) are gone from every build; the library holds one kernel per model and width class and
    refuses a value it does not know instead of silently running something else."""
    from rnnwavefunctions_amd import _lib
    for bad in ("bf16x3-n16", "bf16x3-serial", "bf16x3-hipcc", "bf16x3-asm32", "fp8"):
        monkeypatch.setenv("RNNWF_ENGINE", bad)
        with pytest.raises((ValueError, _lib.RnnwfError), match="RNNWF_ENGINE"):
            _lib.NativeWavefunction(_lib.MODEL_GRU1D, 8, 1, (50,))
    monkeypatch.setenv("RNNWF_ENGINE", "f32")
    _lib.NativeWavefunction(_lib.MODEL_GRU1D, 8, 1, (50,))


# ---- stacked layers (units = [h] * num_layers, 1DTFIM/TrainingRNN_1DTFIM.py:98; MultiRNNCell, RNNwavefunction.py:32) ----

def stacked_like(H, L, seed):
    return P.randomize_biases(P.scale_kernels(P.init_gru_params([H] * L, seed=seed), 1.6), seed + 1)


def make_stacked(model, N, H, L, prm):
    from rnnwavefunctions_amd import _lib
    wf = _lib.NativeWavefunction(model, N, 1, (H,) * L)
    wf.set_params(prm, scope=SCOPE)
    return wf


@pytest.mark.parametrize("N,H,L,B", [(12, 20, 2, 40), (9, 10, 3, 33), (20, 50, 2, 24), (7, 36, 3, 17), (10, 4, 2, 16),
                                      (16, 52, 2, 16), (20, 50, 3, 24), (9, 52, 3, 70),      # 3 x 50: top layer's image read through L2
                                      (8, 53, 2, 20), (9, 64, 2, 33), (7, 68, 3, 17), (6, 69, 2, 20), (8, 100, 2, 24), (6, 100, 3, 18),   # 53..100 units: upper images through L2
                                      (8, 20, 4, 24), (7, 50, 4, 20), (6, 100, 4, 16)])      # four layers
def test_stacked_layers_log_prob_and_eloc_match_oracle(N, H, L, B):
    from rnnwavefunctions_amd import _lib
    prm = stacked_like(H, L, seed=H + L)
    assert M.num_gru_layers(prm) == L
    wf = make_stacked(_lib.MODEL_GRU1D, N, H, L, prm)
    assert wf.num_params() == P.count_params(prm)
    rng = np.random.RandomState(N)
    s = rng.randint(0, 2, (B, N)).astype(np.int32)
    got = wf.log_prob(s)
    prm64 = {k: v.astype(np.float64) for k, v in prm.items()}
    ref64 = M.prnn_log_probability(prm64, s, dtype=np.float64)
    print("L=%d N=%d H=%d: |hip-oracle64|=%.2e" % (L, N, H, np.abs(got - ref64).max()))
    assert np.abs(got - ref64).max() <= 2e-6 * N * L + 2e-6
    Jz = 1.0 + 0.1 * rng.standard_normal(N)
    lp = np.zeros((N + 1) * B)
    e = wf.tfim_eloc(s, Jz, 0.9, log_probs=lp)
    e_ref, lp_ref = E.ising_local_energies(Jz, 0.9, s, lambda x: M.prnn_log_probability(prm64, x, dtype=np.float64),
                                           return_log_probs=True)
    assert np.allclose(lp, lp_ref.ravel(), rtol=0, atol=2e-6 * N * L + 2e-6)
    assert np.allclose(e, e_ref, rtol=3e-5)


def test_stacked_layers_sampling_vmc_step_and_parity_model():
    from rnnwavefunctions_amd import _lib
    N, H, L, ns = 14, 20, 2, 600
    prm = stacked_like(H, L, seed=4)
    wf = make_stacked(_lib.MODEL_GRU1D, N, H, L, prm)
    s, lg = wf.sample(ns, seed=11, step=2, return_log=True)
    u = philox.uniforms(11, 2, 0, ns, N)
    s_ref, lg_ref = M.prnn_sample(prm, N, u)
    bad = np.where((s != s_ref).any(axis=1))[0]
    assert len(bad) <= 2
    good = np.setdiff1d(np.arange(ns), bad)
    assert np.allclose(lg[good], lg_ref[good], rtol=0, atol=4e-6 * N + 2e-6)
    lp_all = wf.log_prob(all_configs(N))
    assert abs(np.exp(lp_all).sum() - 1) < 3e-5                     # normalised over the 2^14 configurations
    out = wf.vmc_step(ns, seed=11, step=2, couplings=np.append(np.ones(N), 1.0), want_samples=True, want_eloc=True)
    assert np.array_equal(out["samples"], s)
    assert np.allclose(out["eloc"], wf.tfim_eloc(s, np.ones(N), 1.0), rtol=1e-12)
    assert wf.engine_name() == "f32mfma"                            # no bf16x3 image for stacked layers
    wfp = make_stacked(_lib.MODEL_GRU1D_PARITY, N, H, L, prm)
    sp = s[:64].astype(np.int32)
    ref = M.prnn_paritysym_log_probability(prm, sp)
    assert np.allclose(wfp.log_prob(sp), ref, rtol=0, atol=4e-6 * N + 2e-6)


@pytest.mark.parametrize("N,H,L,B", [(20, 50, 2, 70), (12, 37, 2, 33), (9, 44, 3, 40), (7, 50, 4, 20), (16, 50, 3, 97), (33, 49, 2, 64), (2, 50, 2, 5)])
def test_stacked_layers_on_both_engines(N, H, L, B, monkeypatch):
    """Stacked layers of 37..50 units on the bf16x3 engine (a pipeline of one ping-pong kernel per layer, csrc/split_kernels.h:
    prnn_flip_pp_kernel<.., STACK> -> prnn_flip_pp_upper_kernel) and on the f32-input MFMA: log-probability queue and local
    energies of both against the float64 oracle, same tolerances; the two engines agree far inside them."""
    from rnnwavefunctions_amd import _lib
    prm = stacked_like(H, L, seed=H + L)
    prm64 = {k: v.astype(np.float64) for k, v in prm.items()}
    rng = np.random.RandomState(N + H)
    s = rng.randint(0, 2, (B, N)).astype(np.int32)
    Jz = 1.0 + 0.1 * rng.standard_normal(N)
    e_ref, lp_ref = E.ising_local_energies(Jz, 0.9, s, lambda x: M.prnn_log_probability(prm64, x, dtype=np.float64), return_log_probs=True)
    got = {}
    for engine in ("bf16x3", "f32"):
        monkeypatch.setenv("RNNWF_ENGINE", engine)
        wf = make_stacked(_lib.MODEL_GRU1D, N, H, L, prm)
        lp = np.zeros((N + 1) * B)
        e = wf.tfim_eloc(s, Jz, 0.9, log_probs=lp)
        assert wf.engine_name() == ("bf16x3" if engine == "bf16x3" else "f32mfma")
        print("L=%d N=%d H=%d %s: max |lp - oracle64| = %.2e, max rel dE = %.2e" %
              (L, N, H, engine, np.abs(lp - lp_ref.ravel()).max(), np.abs(e / e_ref - 1).max()))
        assert np.allclose(lp, lp_ref.ravel(), rtol=0, atol=2e-6 * N * L + 2e-6)
        assert np.allclose(e, e_ref, rtol=3e-5)
        got[engine] = (lp, e)
    assert np.allclose(got["bf16x3"][0], got["f32"][0], rtol=0, atol=2e-6 * N * L + 2e-6)
    # the parity-symmetric class on the same stack: both directions through the pipeline
    monkeypatch.setenv("RNNWF_ENGINE", "bf16x3")
    wfp = make_stacked(_lib.MODEL_GRU1D_PARITY, N, H, L, prm)
    ep = wfp.tfim_eloc(s, Jz, 0.9)
    ep_ref = E.ising_local_energies(Jz, 0.9, s, lambda x: M.prnn_paritysym_log_probability(prm64, x, dtype=np.float64))
    assert wfp.engine_name() == "bf16x3" and np.allclose(ep, ep_ref, rtol=3e-5)


def test_stacked_layers_bf16x3_vmc_step_at_speed_size():
    """The layer pipeline at a batch large enough to be chosen by default (no RNNWF_ENGINE): N=40, units=[50,50], 4 096 samples;
    256 of them against the float64 oracle, shard invariance bit for bit, copies of one configuration get identical values."""
    from rnnwavefunctions_amd import _lib
    N, H, L, ns = 40, 50, 2, 4096
    prm = stacked_like(H, L, seed=7)
    prm64 = {k: v.astype(np.float64) for k, v in prm.items()}
    wf = make_stacked(_lib.MODEL_GRU1D, N, H, L, prm)
    c = np.append(np.ones(N), 1.0)
    out = wf.vmc_step(ns, seed=5, step=1, couplings=c, want_samples=True, want_eloc=True)
    assert wf.engine_name() == "bf16x3"
    s, e = out["samples"], out["eloc"]
    sub = np.arange(0, ns, 16)
    e_ref = E.ising_local_energies(np.ones(N), 1.0, s[sub], lambda x: M.prnn_log_probability(prm64, x, dtype=np.float64))
    assert np.allclose(e[sub], e_ref, rtol=3e-5)
    lo = wf.vmc_step(ns // 2, seed=5, step=1, couplings=c, want_eloc=True)
    hi = wf.vmc_step(ns // 2, seed=5, step=1, couplings=c, sample_offset=ns // 2, want_eloc=True)
    assert np.array_equal(np.concatenate([lo["eloc"], hi["eloc"]]), e)
    rep = np.repeat(s[:3], 100, axis=0).astype(np.int32)
    er = wf.tfim_eloc(rep, np.ones(N), 1.0)
    assert all(len(set(er[k * 100:(k + 1) * 100].tolist())) == 1 for k in range(3))


@pytest.mark.parametrize("N,units,B", [(12, (20, 10), 40), (10, (10, 20), 33), (9, (36, 50, 20), 24), (8, (50, 7, 33), 17), (7, (64, 20), 20),
                                        (6, (30, 100), 16), (9, (20, 10, 36, 12), 24)])
def test_stacked_layers_of_unequal_width(N, units, B):
    """`units` is any list in the reference's constructor (1DTFIM/RNNwavefunction.py:32: MultiRNNCell([cell(units[n]) ...])).  Layers
    narrower than the widest are held zero-padded inside the library (a padded unit stays exactly 0 and feeds nothing); the caller
    sees the reference's shapes.  log P and local energies against the float64 oracle; the library's own initialiser gives
    params.init_gru_params' values."""
    from rnnwavefunctions_amd import _lib
    prm = P.randomize_biases(P.scale_kernels(P.init_gru_params(list(units), seed=sum(units)), 1.6), 5)
    wf = _lib.NativeWavefunction(_lib.MODEL_GRU1D, N, 1, units)
    wf.set_params(prm, scope=SCOPE)
    assert wf.num_params() == P.count_params(prm)
    for k, v in prm.items():
        assert np.array_equal(wf.get_param(k[len(SCOPE) + 1:], v.shape, np.float32), v), k
    rng = np.random.RandomState(N)
    s = rng.randint(0, 2, (B, N)).astype(np.int32)
    prm64 = {k: v.astype(np.float64) for k, v in prm.items()}
    ref64 = M.prnn_log_probability(prm64, s, dtype=np.float64)
    got = wf.log_prob(s)
    print("units=%s N=%d: |hip-oracle64|=%.2e" % (units, N, np.abs(got - ref64).max()))
    assert np.abs(got - ref64).max() <= 2e-6 * N * len(units) + 2e-6
    Jz = 1.0 + 0.1 * rng.standard_normal(N)
    e = wf.tfim_eloc(s, Jz, 0.8)
    e64 = E.ising_local_energies(Jz, 0.8, s, lambda x: M.prnn_log_probability(prm64, x, dtype=np.float64))
    assert np.abs(e - e64).max() <= 3e-5 * max(1.0, np.abs(e64).max())        # (a local energy may sit near zero)
    wf2 = _lib.NativeWavefunction(_lib.MODEL_GRU1D, N, 1, units)
    wf2.init_params(77)
    ini = P.init_gru_params(list(units), seed=77)
    for k, v in ini.items():
        assert np.array_equal(wf2.get_param(k[len(SCOPE) + 1:], v.shape, np.float32), v), k
    drawn = wf2.sample(50, seed=1, step=0)
    assert np.allclose(wf2.log_prob(drawn), M.prnn_log_probability(ini, drawn), rtol=0, atol=1e-4)


def test_stacked_layers_limits_and_facade():
    from rnnwavefunctions_amd import _lib
    from rnnwavefunctions_amd.TFIM1D.RNNwavefunction import RNNwavefunction
    _lib.NativeWavefunction(_lib.MODEL_GRU1D, 10, 1, (20, 10))          # unequal widths: padded to the widest layer inside the library
    _lib.NativeWavefunction(_lib.MODEL_GRU1D, 10, 1, (64, 64))          # above 52 units the upper layers' images are read through L2
    with pytest.raises(ValueError, match="num_units <= 100"):
        _lib.NativeWavefunction(_lib.MODEL_GRU1D, 10, 1, (104, 104))
    with pytest.raises(ValueError, match="num_units too large"):
        _lib.NativeWavefunction(_lib.MODEL_GRU1D, 10, 1, (261,))
    _lib.NativeWavefunction(_lib.MODEL_GRU1D, 10, 1, (260,))            # above 100 units the image is read through L2
    with pytest.raises(ValueError, match="one layer"):          # the reference: "num_layers is not supported yet"
        _lib.NativeWavefunction(_lib.MODEL_MDRNN2D, 4, 4, (10, 10))
    _lib.NativeWavefunction(_lib.MODEL_GRU1D_F64, 4, 4, (40, 40))       # likewise above 36 units in float64
    with pytest.raises(ValueError, match="float64 layers"):
        _lib.NativeWavefunction(_lib.MODEL_GRU1D_F64, 4, 4, (72, 72))
    _lib.NativeWavefunction(_lib.MODEL_GRU1D, 20, 1, (50, 50, 50))      # run_1dTFIM.py's width with num_layers = 3
    wf = RNNwavefunction(10, cell="CudnnCompatibleGRUCell", units=[10, 10], seed=111)
    # layer 0: 12*20 + 20 + 2*10 + 10 + 10*10 + 10 = 400; layer 1: 20*20 + 20 + 10*10 + 10 + 10*10 + 10 = 640; head 22
    assert wf.num_params() == 400 + 640 + 22
    prm = wf.get_params()
    smp = wf._native.sample(50, seed=111, step=0)
    lp = wf._native.log_prob(smp)
    assert np.allclose(lp, M.prnn_log_probability(prm, smp), rtol=0, atol=1e-4)
    wf = RNNwavefunction(10, cell="CudnnCompatibleGRUCell", units=[20, 10], seed=111)       # any list, as in the reference
    prm = wf.get_params()
    assert prm[SCOPE + "/multi_rnn_cell/cell_1/cudnn_compatible_gru_cell/gates/kernel"].shape == (30, 20)
    smp = wf._native.sample(50, seed=111, step=0)
    assert np.allclose(wf._native.log_prob(smp), M.prnn_log_probability(prm, smp), rtol=0, atol=1e-4)


@pytest.mark.parametrize("H", [10, 20, 36, 37, 44, 50, 51, 52, 53, 60, 64, 68, 69, 85, 100])
def test_copies_of_one_configuration_get_identical_values(H, monkeypatch):
    """96 copies of one spin configuration must give 96 bit-identical local energies on either engine, launch after
    launch: chains differ only in lane / wave / workgroup, so any difference is a scheduling hazard (round 2 found one this
    way: an inline-asm conversion in front of an MFMA that hipcc gave no wait states)."""
    from rnnwavefunctions_amd import _lib
    N = 24
    prm = trained_like(H, seed=H)
    rng = np.random.RandomState(H)
    one = rng.randint(0, 2, (1, N)).astype(np.int32)
    s = np.repeat(one, 96, axis=0)
    for engine in ("bf16x3", "f32"):
        monkeypatch.setenv("RNNWF_ENGINE", engine)
        wf = make_wf(_lib.MODEL_GRU1D, N, H, prm)
        lp = np.zeros((N + 1) * 96)
        e0 = wf.tfim_eloc(s, np.ones(N), 1.0, log_probs=lp)
        assert np.unique(e0).size == 1, (engine, np.unique(e0).size)
        assert all(np.unique(lp.reshape(N + 1, 96)[r]).size == 1 for r in range(N + 1))
        for _ in range(3):
            assert np.array_equal(wf.tfim_eloc(s, np.ones(N), 1.0), e0)


def test_stream_engine_edge_cases(monkeypatch):
    """The bf16x3 engine above 68 units (w3 fragments through L2): ragged batches (ns not a multiple of 32 or 16), the
    shortest chains (N = 2, 3), the parity-symmetric model, and a multi-pass call - all against the float64 oracle, and
    multi-pass == single pass bit for bit."""
    from rnnwavefunctions_amd import _lib
    rng = np.random.RandomState(5)
    monkeypatch.setenv("RNNWF_ENGINE", "bf16x3")
    for N, H, ns, model in ((2, 100, 33, _lib.MODEL_GRU1D), (3, 96, 1, _lib.MODEL_GRU1D), (17, 100, 47, _lib.MODEL_GRU1D),
                            (9, 72, 95, _lib.MODEL_GRU1D_PARITY)):
        prm = trained_like(H, seed=N + H)
        prm64 = {k: v.astype(np.float64) for k, v in prm.items()}
        wf = make_wf(model, N, H, prm)
        s = rng.randint(0, 2, (ns, N)).astype(np.int32)
        Jz = 1.0 + 0.1 * rng.standard_normal(N)
        e = wf.tfim_eloc(s, Jz, 0.8)
        assert wf.engine_name() == "bf16x3"
        fn = M.prnn_paritysym_log_probability if model == _lib.MODEL_GRU1D_PARITY else M.prnn_log_probability
        e64 = E.ising_local_energies(Jz, 0.8, s, lambda x: fn(prm64, x, dtype=np.float64))
        err = np.abs(e - e64).max() / max(1.0, np.abs(e64).max())
        print("stream engine N=%d H=%d ns=%d model=%d: max rel E err %.2e" % (N, H, ns, model, err))
        assert err < 2e-5
    N, H, ns = 20, 100, 1500                                  # checkpoints: 19 * 94 * 25 KB = 45 MB
    prm = trained_like(H, seed=9)
    s = rng.randint(0, 2, (ns, N)).astype(np.int32)
    wf = make_wf(_lib.MODEL_GRU1D, N, H, prm)
    e1 = wf.tfim_eloc(s, np.ones(N), 1.0)
    monkeypatch.setenv("RNNWF_STATE_BUDGET_MB", "4")
    wf = make_wf(_lib.MODEL_GRU1D, N, H, prm)
    monkeypatch.delenv("RNNWF_STATE_BUDGET_MB")
    e2 = wf.tfim_eloc(s, np.ones(N), 1.0)
    assert wf.engine_name() == "bf16x3" and np.array_equal(e1, e2)


def test_multi_pass_estimators_equal_the_single_pass(monkeypatch):
    """Batches larger than the hidden-state budget run in several passes (RNNWF_STATE_BUDGET_MB, read at rnnwf_create,
    shrinks the budget so that this happens at test sizes); results must not depend on the pass boundaries."""
    from rnnwavefunctions_amd import _lib
    rng = np.random.RandomState(0)
    N, H, ns = 24, 20, 3000                                   # checkpoints: 23 * 188 * 5 KB = 24 MB
    prm = trained_like(H, seed=1)
    for model in (_lib.MODEL_GRU1D, _lib.MODEL_GRU1D_PARITY):
        wf = make_wf(model, N, H, prm)
        s = rng.randint(0, 2, (ns, N)).astype(np.int32)
        lp1 = np.zeros((N + 1) * ns)
        e1 = wf.tfim_eloc(s, np.ones(N), 1.0, log_probs=lp1)
        monkeypatch.setenv("RNNWF_STATE_BUDGET_MB", "1")
        wf = make_wf(model, N, H, prm)
        monkeypatch.delenv("RNNWF_STATE_BUDGET_MB")
        lp2 = np.zeros((N + 1) * ns)
        e2 = wf.tfim_eloc(s, np.ones(N), 1.0, log_probs=lp2)
        out = wf.vmc_step(100, seed=1, step=0, couplings=np.append(np.ones(N), 1.0), want_eloc=True)
        shapes = {"wf_dense/kernel": (H, 2), "wf_dense/bias": (2,)}
        g1 = wf.vmc_gradient(out["eloc"].mean(), 100, shapes)
        with pytest.raises(_lib.RnnwfError, match="split the batch"):
            wf.vmc_step(ns, seed=1, step=0, couplings=np.append(np.ones(N), 1.0))
        g2 = wf.vmc_gradient(out["eloc"].mean(), 100, shapes)      # the refused step left the batch before it resident
        assert np.array_equal(e1, e2) and np.array_equal(lp1, lp2)
        assert all(np.array_equal(g1[nm], g2[nm]) for nm in shapes)
    # 2D MDRNN and the complex RNN take the same route
    from rnnwavefunctions_amd import params as PP
    wf = _lib.NativeWavefunction(_lib.MODEL_MDRNN2D, 4, 4, (20,))
    wf.set_params(PP.init_mdrnn_params(20, seed=3), scope=SCOPE)
    s2 = rng.randint(0, 2, (2000, 4, 4)).astype(np.int32)
    e1 = wf.tfim_eloc(s2, np.ones((4, 4)), 2.0)
    lp1 = wf.log_prob(s2)
    monkeypatch.setenv("RNNWF_STATE_BUDGET_MB", "1")                 # 16 sites x 3 KB per 16 chains: 336 chains per pass
    wf = _lib.NativeWavefunction(_lib.MODEL_MDRNN2D, 4, 4, (20,))
    monkeypatch.delenv("RNNWF_STATE_BUDGET_MB")
    wf.set_params(PP.init_mdrnn_params(20, seed=3), scope=SCOPE)
    e2 = wf.tfim_eloc(s2, np.ones((4, 4)), 2.0)
    lp2 = wf.log_prob(s2)                                             # its base pass keeps the states too: several passes
    assert np.array_equal(e1, e2) and np.array_equal(lp1, lp2)
    with pytest.raises(_lib.RnnwfError, match="split"):
        wf.sample(2000, seed=1)
    wfc = _lib.NativeWavefunction(_lib.MODEL_CRNN_U1, 12, 1, (20,))
    prmc = trained_like(20, seed=5, heads=("wf_dense_ampl", "wf_dense_phase"))
    wfc.set_params(prmc, scope=SCOPE)
    sc = wfc.sample(3000, seed=2, step=0)
    e1 = wfc.j1j2_eloc(sc, np.ones(12), 0.5 * np.ones(12), np.zeros(12))
    monkeypatch.setenv("RNNWF_STATE_BUDGET_MB", "1")
    wfc = _lib.NativeWavefunction(_lib.MODEL_CRNN_U1, 12, 1, (20,))
    monkeypatch.delenv("RNNWF_STATE_BUDGET_MB")
    wfc.set_params(prmc, scope=SCOPE)
    e2 = wfc.j1j2_eloc(sc, np.ones(12), 0.5 * np.ones(12), np.zeros(12))
    assert e1[1] == e2[1] and np.allclose(e1[0], e2[0], rtol=1e-6, atol=1e-6)


def test_log_prob_beyond_one_device_chunk():
    """log_probability uploads 2^20 rows per pass; a larger batch must come back in order."""
    from rnnwavefunctions_amd import _lib
    N, H = 4, 6
    prm = trained_like(H, seed=2)
    wf = make_wf(_lib.MODEL_GRU1D, N, H, prm)
    cfgs = all_configs(N)                                       # 16 configurations
    B = (1 << 20) + 4097
    idx = np.random.RandomState(1).randint(0, 16, B)
    lp = wf.log_prob(cfgs[idx])
    assert np.array_equal(lp, wf.log_prob(cfgs)[idx])


@pytest.mark.parametrize("N,H,ns", [(20, 10, 100), (33, 36, 333), (80, 50, 1000), (12, 64, 50), (7, 20, 16)])
def test_cooperative_base_pass_is_bit_identical(N, H, ns, monkeypatch):
    """The two f32-input-MFMA base kernels - one wave per 16-chain block (prnn_base_kernel) and NFULL+1 waves per block
    (prnn_base_coop_kernel) - agree in every bit, draws included.  Up to 52 units the default base pass is a third kernel
    (the cooperative pass on the bf16 matrix core, next test); RNNWF_BASE=f32 selects the f32 pair here."""
    from rnnwavefunctions_amd import _lib
    prm = trained_like(H, seed=N)
    monkeypatch.setenv("RNNWF_BASE", "f32")                  # read once, at rnnwf_create
    wf = make_wf(_lib.MODEL_GRU1D, N, H, prm)
    s1, lg1 = wf.sample(ns, seed=9, step=1, return_log=True)
    lp1 = wf.log_prob(s1)
    e1 = wf.tfim_eloc(s1, np.ones(N), 1.0)
    monkeypatch.setenv("RNNWF_NO_COOP", "1")
    wf = make_wf(_lib.MODEL_GRU1D, N, H, prm)
    monkeypatch.delenv("RNNWF_NO_COOP")
    monkeypatch.delenv("RNNWF_BASE")
    s2, lg2 = wf.sample(ns, seed=9, step=1, return_log=True)
    lp2 = wf.log_prob(s1)
    e2 = wf.tfim_eloc(s1, np.ones(N), 1.0)
    assert np.array_equal(s1, s2) and np.array_equal(lg1, lg2)
    assert np.array_equal(lp1, lp2) and np.array_equal(e1, e2)


@pytest.mark.parametrize("N,H,ns", [(20, 10, 100), (33, 20, 777), (33, 36, 333), (80, 50, 1000), (40, 44, 5000), (21, 52, 130), (7, 21, 16),
                                     (64, 50, 40000)])
def test_bf16_cooperative_base_pass_against_the_f32_kernels_and_the_oracle(N, H, ns, monkeypatch):
    """Up to 52 units the base pass (sample / log_probability / the checkpoints the flip pass starts from) runs NFULL+1 waves per
    16-chain block on the bf16 matrix core with bf16x3 operands (gru_kernels.h: coop_base_pass_bf), three blocks per workgroup,
    for EVERY batch size.  Against the f32-input-MFMA kernels (RNNWF_BASE=f32): log-probabilities within the f32 tolerance, the
    same draws except near-ties; against the float64 oracle: the same tolerance as every f32 path; shards reproduce the batch
    bit for bit (ragged last workgroup, several rounds at 40 000 samples)."""
    from rnnwavefunctions_amd import _lib
    prm = trained_like(H, seed=N + 1)
    prm64 = {k: v.astype(np.float64) for k, v in prm.items()}
    wf = make_wf(_lib.MODEL_GRU1D, N, H, prm)
    s1, lg1 = wf.sample(ns, seed=9, step=1, return_log=True)
    sub = np.arange(0, ns, max(1, ns // 400))[:400]
    ref64 = M.prnn_log_probability(prm64, s1[sub], dtype=np.float64)
    assert np.abs(lg1[sub] - ref64).max() <= 2e-6 * N + 2e-6
    lp1 = wf.log_prob(s1)
    assert np.array_equal(lp1, lg1)                          # teacher-forced on its own draws: the same kernel, the same numbers
    cut = (ns // 3) | 1
    a = wf.sample(cut, seed=9, step=1)
    b = wf.sample(ns - cut, seed=9, step=1, sample_offset=cut)
    assert np.array_equal(np.concatenate([a, b]), s1)        # shard invariance
    e1 = wf.tfim_eloc(s1[sub], np.ones(N), 1.0)
    monkeypatch.setenv("RNNWF_BASE", "f32")
    wf32 = make_wf(_lib.MODEL_GRU1D, N, H, prm)
    monkeypatch.delenv("RNNWF_BASE")
    s2, lg2 = wf32.sample(ns, seed=9, step=1, return_log=True)
    bad = np.where((s1 != s2).any(axis=1))[0]
    print("N=%d H=%d ns=%d: %d rows drawn differently by the bf16 and the f32 base pass" % (N, H, ns, len(bad)))
    assert len(bad) <= max(2, ns // 2000)
    u = philox.uniforms(9, 1, 0, ns, N)
    for r in bad[:8]:                                        # a differing row must be a near-tie
        n0 = np.argmax(s1[r] != s2[r])
        p0 = M.prnn_site_probs(prm, s2[r:r + 1])[0, n0, 0]
        assert abs(u[r, n0] - p0) < 1e-5
    good = np.setdiff1d(np.arange(ns), bad)
    assert np.abs(lg1[good] - lg2[good]).max() <= 2e-6 * N + 2e-6
    e2 = wf32.tfim_eloc(s1[sub], np.ones(N), 1.0)
    assert np.allclose(e1, e2, rtol=2e-5)


def test_config5_shard_at_full_size():
    """BASELINE config 5, one GPU's shard (N=200, h=100, 32 768 samples; bf16x3 engine with the w3 fragments read
    through L2, csrc/split_stream.hip): the per-site energy
    against the oracle on a subset of the same samples, and the size-independent properties - the two half shards
    drawn with their sample offsets are the full shard (samples AND local energies, bit for bit), the moments are the
    sums of the local energies."""
    from rnnwavefunctions_amd import _lib
    N, H, ns = 200, 100, 32768
    prm = P.init_gru_params([H], seed=111)
    wf = make_wf(_lib.MODEL_GRU1D, N, H, prm)
    Jz = np.ones(N)
    c = np.append(Jz, 1.0)
    out = wf.vmc_step(ns, seed=111, step=2, couplings=c, want_samples=True, want_eloc=True)
    s, e, m = out["samples"], out["eloc"], out["moments"]
    assert wf.engine_name() == "bf16x3"
    assert np.all(np.isfinite(e)) and m[2] == ns
    assert np.isclose(m[0], e.sum(), rtol=1e-12) and np.isclose(m[1], (e * e).sum(), rtol=1e-12)
    lo = wf.vmc_step(ns // 2, seed=111, step=2, couplings=c, want_samples=True, want_eloc=True)
    hi = wf.vmc_step(ns // 2, seed=111, step=2, couplings=c, sample_offset=ns // 2, want_samples=True, want_eloc=True)
    assert np.array_equal(np.concatenate([lo["samples"], hi["samples"]]), s)
    assert np.array_equal(np.concatenate([lo["eloc"], hi["eloc"]]), e)
    assert np.allclose(lo["moments"] + hi["moments"], m, rtol=1e-12)
    # 512 samples spread over the shard against the C oracle (201 x 512 chains of 200 sites from site 0: ~15 s of 16 cores),
    # 6 of them also against the NumPy oracle
    from oracle import cport
    sub = np.arange(0, ns, ns // 512)[:512]
    e_ref = cport.ising_local_energies(prm, Jz, 1.0, s[sub])
    per_site = np.abs(e[sub] - e_ref).max() / N
    d_mean = abs(e[sub].mean() - e_ref.mean()) / N
    print("cfg5 shard: <E>/N = %.6f, over 512 samples: max |E_loc - oracle|/N = %.2e, |mean diff|/N = %.2e" %
          (e.mean() / N, per_site, d_mean))
    assert per_site < 2e-5 and d_mean < 1e-5
    e_np = E.ising_local_energies(Jz, 1.0, s[sub[::86]], lambda x: M.prnn_log_probability(prm, x))
    assert np.abs(e[sub[::86]] - e_np).max() / N < 2e-5


def test_thousand_site_chain():
    """The longest chain the reference's tables mention (DMRG E0 for N=1000, Tutorial_1DTFIM.ipynb cell 24): 32 words of
    packed spins per sample, 999 checkpoints, half a million flip tiles."""
    from rnnwavefunctions_amd import _lib
    N, H, ns = 1000, 50, 96
    prm = P.init_gru_params([H], seed=111)
    wf = make_wf(_lib.MODEL_GRU1D, N, H, prm)
    out = wf.vmc_step(ns, seed=1, step=0, couplings=np.append(np.ones(N), 1.0), want_samples=True, want_eloc=True)
    s, e = out["samples"], out["eloc"]
    assert s.shape == (ns, N) and np.all(np.isfinite(e))
    sub = [0, ns - 1]
    e_ref = E.ising_local_energies(np.ones(N), 1.0, s[sub], lambda x: M.prnn_log_probability(prm, x))
    assert np.abs(e[sub] - e_ref).max() / N < 1e-5
    assert np.array_equal(wf.sample(ns, seed=1, step=0), s)
