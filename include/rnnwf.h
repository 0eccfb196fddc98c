/*
 * rnnwf.h - C ABI of librnnwf_hip.so: the MI355X-native VMC inner loop of RNN wave functions.
 *
 * The reference (MatteoMartinelli97/RNNWavefunctions) has no FFI: its boundary for this path is
 * the Python API of its RNNwavefunction classes and local-energy estimators, executed by
 * TensorFlow 1.13 through tf.Session.run.  Each entry point below names the reference interface
 * it stands in for (paths relative to the reference root).  The Python host code under
 * rnnwavefunctions_amd/ binds these symbols with ctypes and re-creates the reference's
 * signatures on top (INTEGRATION.md shows the binding).
 *
 * Conventions
 *   - plain C types only; all pointers are HOST pointers owned by the caller unless a name
 *     ends in _dev; the library owns all device memory inside the opaque handle;
 *   - every function returns 0 on success and a negative rnnwf_status otherwise; the message
 *     is available from rnnwf_last_error(); nothing aborts the process;
 *   - a handle is bound to one HIP device and one HIP stream; it is not thread-safe; calls are
 *     synchronous with respect to the host unless stated otherwise;
 *   - spin configurations are int32 arrays of 0/1, row-major (numsamples, N) for the 1D models
 *     and (numsamples, Nx, Ny) for the 2D MDRNN model, exactly as the reference feeds its
 *     placeholders (1DTFIM/TrainingRNN_1DTFIM.py:192).
 */
#ifndef RNNWF_H
#define RNNWF_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RNNWF_ABI_VERSION 1

typedef struct rnnwf_handle rnnwf_handle;

typedef enum {
    RNNWF_OK = 0,
    RNNWF_ERR_INVALID = -1,     /* bad argument / unsupported configuration            */
    RNNWF_ERR_HIP = -2,         /* a HIP runtime call failed                           */
    RNNWF_ERR_STATE = -3,       /* call order violated (e.g. parameters not committed) */
    RNNWF_ERR_COMM = -4,        /* RCCL failure                                        */
    RNNWF_ERR_NOMEM = -5,
    RNNWF_ERR_NUMERIC = -6      /* a factorisation met a pivot that is not positive and finite */
} rnnwf_status;

/* Which reference wave function the handle implements. */
typedef enum {
    RNNWF_MODEL_GRU1D = 0,       /* 1DTFIM/RNNwavefunction.py:7-118          pRNN, f32 cell, f64 log-sum   */
    RNNWF_MODEL_GRU1D_PARITY = 1,/* 1DTFIM/RNNwavefunction_paritysym.py:7-145 same sampler, symmetrised P   */
    RNNWF_MODEL_CRNN_U1 = 2,     /* J1J2/ComplexRNNwavefunction.py:15-169    cRNN, f32/complex64, U(1) mask */
    RNNWF_MODEL_GRU1D_F64 = 3,   /* 2DTFIM_1DRNN/RNNwavefunction.py:8-130    pRNN over a raster path, f64   */
    RNNWF_MODEL_MDRNN2D = 4,     /* 2DTFIM_2DRNN/RNNwavefunction.py:5-200 + MDRNNcell.py:6-66, f64          */
    RNNWF_MODEL_LSTM1D_F64 = 5   /* 2DTFIM_1DRNN/RNNwavefunction.py:9,37 with its default cell=LSTMCell:    */
                                 /* one LSTM layer over the raster path, f64; evaluation only (no gradient) */
} rnnwf_model;

typedef enum { RNNWF_F32 = 0, RNNWF_F64 = 1 } rnnwf_dtype;

#define RNNWF_MAX_LAYERS 4

typedef struct {
    int32_t abi_version;              /* RNNWF_ABI_VERSION                                        */
    int32_t model;                    /* rnnwf_model                                              */
    int32_t nx;                       /* systemsize (1D) or systemsize_x (2D)                     */
    int32_t ny;                       /* 1 for 1D models, systemsize_y for 2D                     */
    int32_t num_layers;               /* len(units) of the reference ctor: 1; 2..4 (any widths     */
                                      /* <= 100 units, float64: <= 68) for the GRU models          */
    int32_t units[RNNWF_MAX_LAYERS];  /* units[n]: one layer <= 260 (float GRU models; above 100 the */
                                      /* weight image is read through L2), <= 100 (float64 GRU;   */
                                      /* above 68 likewise), <= 84 (2D RNN), <= 68 (LSTM, one     */
                                      /* layer only)                                              */
    int32_t device;                   /* HIP device ordinal                                       */
    int32_t reserved[6];
} rnnwf_config;

/* ---- life cycle ------------------------------------------------------------------------------
 * rnnwf_create      <- RNNwavefunction.__init__ (1DTFIM/RNNwavefunction.py:8-33,
 *                      J1J2/ComplexRNNwavefunction.py:16-43, 2DTFIM_2DRNN/RNNwavefunction.py:6-33)
 *                      plus the tf.Session it would be run in (1DTFIM/TrainingRNN_1DTFIM.py:119-123). */
int rnnwf_create(const rnnwf_config* cfg, rnnwf_handle** out);
int rnnwf_destroy(rnnwf_handle* h);
/* Message of the last failure on this handle (h == NULL: of the last failed rnnwf_create). */
const char* rnnwf_last_error(const rnnwf_handle* h);
/* "hip-gfx950" */
const char* rnnwf_backend_name(void);
int rnnwf_abi_version(void);

/* ---- parameters ------------------------------------------------------------------------------
 * Stand in for the TF variables of the reference graph and for tf.train.Saver restore
 * (1DTFIM/TrainingRNN_1DTFIM.py:166,172-183).  `tf_name` is the TF variable name WITHOUT the scope
 * prefix, e.g. "multi_rnn_cell/cell_0/cudnn_compatible_gru_cell/gates/kernel", "wf_dense/bias",
 * "Wh_rnn_0".  `count` is the element count and must match the variable's shape; `dtype` is the
 * type of the caller's buffer (converted to the model's arithmetic type).
 * rnnwf_commit_params re-packs all parameters into the MFMA-fragment image the kernels stage in
 * LDS and uploads it; it must be called after the last rnnwf_set_param and before any compute. */
int rnnwf_set_param(rnnwf_handle* h, const char* tf_name, const void* data, int64_t count, int32_t dtype);
int rnnwf_get_param(rnnwf_handle* h, const char* tf_name, void* data, int64_t count, int32_t dtype);
int rnnwf_commit_params(rnnwf_handle* h);
/* rnnwf_init_params <- sess.run(tf.global_variables_initializer()) (1DTFIM/TrainingRNN_1DTFIM.py:168): glorot/xavier-
 * uniform kernels, gate bias 1, other biases 0 (MDRNN: all tensors xavier, MDRNNcell.py:21-35), drawn in the order
 * and with the generator of the Python side (numpy.random.RandomState(seed): MT19937, 53-bit doubles), so C and
 * Python callers start from identical weights; commits.  TensorFlow's own seeded draws are not reproducible outside
 * TF ("parity unpinned").  seed must fit 32 bits. */
int rnnwf_init_params(rnnwf_handle* h, uint64_t seed);
/* Number of scalar parameters (the count the reference prints, TrainingRNN_1DTFIM.py:127-136). */
int64_t rnnwf_num_params(const rnnwf_handle* h);

/* ---- wave function ---------------------------------------------------------------------------
 * rnnwf_sample   <- sess.run(wf.sample(numsamples, 2))   (1DTFIM/RNNwavefunction.py:35-74,
 *                   J1J2/ComplexRNNwavefunction.py:45-103, 2DTFIM_2DRNN/RNNwavefunction.py:35-118).
 *   Draws `numsamples` configurations.  The uniform of (global sample g = sample_offset + row,
 *   site n) is Philox4x32-10(key = seed, counter = (g, n/4, step))[n%4] >> 8, so shards of one
 *   batch drawn with different sample_offset on different devices are disjoint pieces of the
 *   same stream.  out_samples: (numsamples, N) int32; out_log (optional, may be NULL): the
 *   log-probability (f64) of each drawn configuration (2*Re log psi for the cRNN).            */
int rnnwf_sample(rnnwf_handle* h, int64_t numsamples, uint64_t seed, uint64_t step, int64_t sample_offset,
                 int32_t* out_samples, double* out_log);

/* rnnwf_log_prob <- sess.run(wf.log_probability(ph, 2), {ph: samples})
 *                   (1DTFIM/RNNwavefunction.py:76-118, RNNwavefunction_paritysym.py:80-145,
 *                    2DTFIM_1DRNN/RNNwavefunction.py:84-130, 2DTFIM_2DRNN/RNNwavefunction.py:120-200)
 *   out: (B,) f64.  For RNNWF_MODEL_CRNN_U1 it returns 2*Re log psi.                          */
int rnnwf_log_prob(rnnwf_handle* h, const int32_t* samples, int64_t B, double* out);

/* rnnwf_log_amp  <- sess.run(wf.log_amplitude(ph, 2), {ph: samples})
 *                   (J1J2/ComplexRNNwavefunction.py:105-169).  out_re_im: (B, 2) f32 = complex64. */
int rnnwf_log_amp(rnnwf_handle* h, const int32_t* samples, int64_t B, float* out_re_im);

/* ---- local-energy estimators -----------------------------------------------------------------
 * rnnwf_tfim_eloc <- Ising_local_energies(Jz, Bx, samples, queue_samples, log_probs_tensor,
 *                    samples_placeholder, log_probs, sess)   (1DTFIM/TrainingRNN_1DTFIM.py:13-75)
 *   Fused formulation: one teacher-forced pass that checkpoints the hidden state after every
 *   site, then every single-spin-flip configuration is scored from its flipped site onwards only;
 *   `queue_samples` is never materialised.  Jz: (N,) f64 (Jz[N-1] unused, as in the reference).
 *   eloc: (numsamples,) f64.  log_probs (optional): ((N+1)*numsamples,) f64, row 0 = log P(s),
 *   row i+1 = log P(s with spin i flipped) - the reference's `log_probs` scratch (:65,:70).   */
int rnnwf_tfim_eloc(rnnwf_handle* h, const int32_t* samples, int64_t numsamples, const double* Jz, double Bx,
                    double* eloc, double* log_probs);

/* rnnwf_tfim2d_eloc <- Ising2D_local_energies(Jz, Bx, Nx, Ny, samples, ...)
 *   (2DTFIM_2DRNN/Training2DRNN_2DTFIM.py:13-83 for RNNWF_MODEL_MDRNN2D, samples (ns, Nx, Ny);
 *    2DTFIM_1DRNN/Training1DRNN_2DTFIM.py:13-81 for RNNWF_MODEL_GRU1D_F64 and RNNWF_MODEL_LSTM1D_F64, samples (ns, Nx*Ny)).
 *   Jz: (Nx, Ny) f64 row-major.                                                                */
int rnnwf_tfim2d_eloc(rnnwf_handle* h, const int32_t* samples, int64_t numsamples, const double* Jz, double Bx,
                      double* eloc, double* log_probs);

/* rnnwf_j1j2_eloc <- J1J2Slices + chunked log_amplitude + E_loc loop
 *   (J1J2/TrainingRNN_J1J2.py:95-127, :255-279), with J1J2MatrixElements' `periodic` and
 *   `Marshall_sign` flags (:12) implemented as documented (the reference's J1J2Slices passes
 *   Marshall_sign into the `periodic` slot, :118; the Python facade reproduces that quirk).
 *   J1, J2, Bz: (N,) f64.  eloc_re_im: (numsamples, 2) f32.  n_connected (optional): total
 *   number of configurations scored (diagonal + off-diagonal), the reference's `len_sigmas`.  */
int rnnwf_j1j2_eloc(rnnwf_handle* h, const int32_t* samples, int64_t numsamples, const double* J1,
                    const double* J2, const double* Bz, int32_t periodic, int32_t marshall,
                    float* eloc_re_im, int64_t* n_connected);

/* ---- fused VMC step (sample + local energy + moments, nothing leaves HBM but the moments) -----
 * rnnwf_vmc_step <- one iteration of the loop at 1DTFIM/TrainingRNN_1DTFIM.py:199-207 /
 *   J1J2/TrainingRNN_J1J2.py:241-282 / the Training scripts of the two 2DTFIM folders, without the optimizer:
 *   samples = sess.run(samples_); local_energies = <estimator>(...); meanE; varE.
 *   `couplings` is model specific: TFIM1D: Jz (N) then Bx (1)              -> N+1 doubles
 *                                  TFIM2D: Jz (Nx*Ny) then Bx (1)          -> Nx*Ny+1 doubles
 *                                  J1J2  : J1 (N), J2 (N), Bz (N), periodic, marshall -> 3N+2 doubles
 *   moments[4] (out) = { sum Re E, sum (Re E)^2, n, sum Im E } over THIS handle's samples
 *   (combine across devices with rnnwf_allreduce_moments).  out_samples / out_eloc may be NULL
 *   (out_eloc is (numsamples,) f64 for TFIM, (numsamples,2) f32 for J1J2).                     */
int rnnwf_vmc_step(rnnwf_handle* h, int64_t numsamples, uint64_t seed, uint64_t step, int64_t sample_offset,
                   const double* couplings, int64_t n_couplings, int32_t* out_samples, void* out_eloc,
                   double* moments);

/* ---- gradient of the VMC cost (models GRU1D, GRU1D_PARITY, CRNN_U1 (f32), GRU1D_F64, MDRNN2D (f64)) ----
 * (For RNNWF_MODEL_LSTM1D_F64 these four and rnnwf_load_batch return RNNWF_ERR_INVALID; its gradient has entries of its
 * own, rnnwf_lstm_gradient and rnnwf_lstm_vmc_gradient_step below.)
 * rnnwf_vmc_gradient <- optimizer.compute_gradients(cost) with
 *   cost = mean(log_probs * Eloc) - mean(Eloc) * mean(log_probs)      (1DTFIM/TrainingRNN_1DTFIM.py:151-162)
 *   evaluated on the batch of the LAST rnnwf_vmc_step (its samples, per-site hidden states and E_loc are still
 *   resident):  grad = sum_s (E_s - mean_energy) / norm * d log P(s) / d theta.  Single device: mean_energy =
 *   moments[0]/moments[2], norm = numsamples; sharded: the all-reduced mean and the global sample count, then
 *   rnnwf_allreduce_grads.  Back-propagation through time on the MFMA + a TN GEMM for the weight gradients.
 *   Complex RNN: cost = 2 Re(mean(conj(log_amplitudes) Eloc) - conj(mean(log_amplitudes)) mean(Eloc))
 *   (J1J2/TrainingRNN_J1J2.py:197), i.e. grad = 2/norm sum_s [(Re E_s - mean_energy) d Re log psi +
 *   (Im E_s - mean_energy_im) d Im log psi]; mean_energy_im is ignored for the positive RNNs.
 *   The 2D drivers (2DTFIM_2DRNN/Training2DRNN_2DTFIM.py:163, 2DTFIM_1DRNN/Training1DRNN_2DTFIM.py:160) use the
 *   first cost in float64.  Every width rnnwf_create accepts (above 68 / 52 units the backward operand is read through
 *   L2 instead of LDS).  Stacked layers (len(units) 2..RNNWF_MAX_LAYERS, every GRU model): one backward pass per
 *   layer, top first.  GRU1D_PARITY (the import switch of 1DTFIM/TrainingRNN_1DTFIM.py:10): log P_sym =
 *   log(0.5 (P(s) + P(reversed s))), two backward passes weighted by each direction's share of P_sym.
 *   Every reduction has a fixed order: the same batch gives the same bits.
 * rnnwf_get_grad     <- the gradient of one TF variable (same names and shapes as rnnwf_set_param).
 * rnnwf_allreduce_grads: one RCCL all-reduce (sum) over all gradient arrays of the handle (flattened and summed on the
 *   device, in-stream, then copied to the host arrays; through pinned staging when the device-side map is unavailable).  */
int rnnwf_vmc_gradient(rnnwf_handle* h, double mean_energy, double mean_energy_im, double norm);
/* rnnwf_load_batch: the batch rnnwf_vmc_gradient works on, supplied by the caller instead of drawn by rnnwf_vmc_step -
 * what `sess.run(optstep, feed_dict={Eloc: local_energies, samp: samples, ...})` feeds (TrainingRNN_1DTFIM.py:221,
 * TrainingRNN_J1J2.py:286).  samples: int32 (ns, N) as for rnnwf_log_prob; eloc: float64[ns] (TFIM models) or
 * complex64[ns] as float pairs (complex RNN).  Runs the teacher-forced pass that stores the hidden-state checkpoints.  */
int rnnwf_load_batch(rnnwf_handle* h, const int32_t* samples, int64_t ns, const void* eloc);
int rnnwf_get_grad(rnnwf_handle* h, const char* tf_name, void* data, int64_t count, int32_t dtype);
/* One call per training iteration instead of one per tensor: every tensor in the reference's shapes, float64, concatenated in
 * the byte-wise order of the names (rnnwf_param_name(h, i, &count) lists them).  rnnwf_set_params_flat commits. */
int rnnwf_set_params_flat(rnnwf_handle* h, const double* flat, int64_t count);
/* Host only - needs no device and no handle: the two forms of the bf16x3 flip-pass image of a one-layer positive GRU of `units`
 * hidden units (37..50: the ping-pong kernel's class) with the parameters `flat` (order of rnnwf_set_params_flat), as the packer
 * builds them - img_h the form in h, img_g the form the kernel reads, whose state travels as g = (h + 1) / 2 - `cap` bytes each,
 * and layout[10] = {NT, NQ, NUP, NOUT, OFF_ASP, OFF_CI, OFF_XC, OFF_WD, OFF_BD, BYTES} (csrc/pack_split.h: GstateLayout).  For tests
 * of the packer on machines without a GPU.  Errors through rnnwf_last_error(NULL). */
int rnnwf_host_split_images(int32_t units, const double* flat, int64_t count, void* img_h, void* img_g, int64_t cap, int32_t* layout);
/* Host only, beside it: *bound = the image's range bound - the largest sum, over the units, of the bounds of the update gate's and the
 * candidate's exponent arguments over every state and both input spins (csrc/pack_split.h: gstate_range) - and *in_range = the word
 * the packer writes into img_g from it: 1 (bound <= 120, the flip kernel may take one reciprocal for update gate and candidate) or 0. */
int rnnwf_host_split_range(int32_t units, const double* flat, int64_t count, double* bound, int32_t* in_range);
int rnnwf_get_grads_flat(rnnwf_handle* h, double* flat, int64_t count);
const char* rnnwf_param_name(const rnnwf_handle* h, int32_t i, int64_t* count);
int rnnwf_allreduce_grads(rnnwf_handle* h);

/* ---- device-resident training iteration (every model of the four drivers) ----------------------------------------------
 * The reference's update is one `sess.run(optstep)` on the device (1DTFIM/TrainingRNN_1DTFIM.py:113,162,221;
 * J1J2/TrainingRNN_J1J2.py:164,286): tf.train.AdamOptimizer on the gradient of the cost, variables never leave the device.
 * rnnwf_device_training_supported: 1 when this handle can do the same (parameters, Adam moments and gradient resident on the
 *   device, the kernels' weight images rebuilt there after every update) - every GRU model, one layer or a stack, and the 2D
 *   RNN; 0 (a width without a packer table): keep the host optimizer (rnnwf_get_grads_flat / rnnwf_set_params_flat).
 * rnnwf_adam_step  <- optimizer.apply_gradients on the gradient the last rnnwf_vmc_gradient left on the device:
 *   t += 1; lr_t = lr sqrt(1 - beta2^t) / (1 - beta1^t); m = beta1 m + (1 - beta1) g; v = beta2 v + (1 - beta2) g^2;
 *   theta -= lr_t m / (sqrt(v) + epsilon) in float64, theta rounded to the model's type; then every weight image is rebuilt on the device.
 * rnnwf_train_steps <- K iterations of the loop at TrainingRNN_1DTFIM.py:199-227 (sample, local energies, moments, gradient,
 *   update) with ONE host synchronisation: iteration k draws with step index step0 + k and uses learning_rates[k];
 *   moments: [K][4] as rnnwf_vmc_step returns them (summed over the ranks when rnnwf_comm_reduce_in_step is on, as is the
 *   gradient: one in-stream RCCL all-reduce each).  1 <= K <= 1024.  Same arithmetic as the host optimizer, operation for
 *   operation: the trajectory is bit-identical.
 * rnnwf_adam_get_state / rnnwf_adam_set_state: Adam's m and v in the flat order of rnnwf_set_params_flat and the number of
 *   updates applied (what tf.train.Saver keeps as <var>/Adam, <var>/Adam_1 and the beta powers); NULL m/v in set: zeros.
 * rnnwf_get_param and rnnwf_commit_params see the device's parameters (they are copied back on demand).                    */
int rnnwf_device_training_supported(rnnwf_handle* h);
int rnnwf_adam_step(rnnwf_handle* h, double learning_rate, double beta1, double beta2, double epsilon);
int rnnwf_train_steps(rnnwf_handle* h, int32_t K, int64_t numsamples, uint64_t seed, uint64_t step0, int64_t sample_offset,
                      const double* couplings, int64_t n_couplings, const double* learning_rates, double beta1, double beta2,
                      double epsilon, double* moments);
int rnnwf_adam_get_state(rnnwf_handle* h, double* m_flat, double* v_flat, int64_t count, int64_t* t_steps);
int rnnwf_adam_set_state(rnnwf_handle* h, const double* m_flat, const double* v_flat, int64_t count, int64_t t_steps);

/* ---- entanglement: second Renyi entropy ------------------------------------------------------------
 * The reference README's "entanglement entropies", by the replica swap estimator (Hastings, Gonzalez, Kallin, Melko,
 * PRL 104, 157201 (2010)) on pairs (sigma, tau) drawn independently from |psi|^2 = P:
 *   r_l(sigma, tau) = psi(tau_A sigma_B) psi(sigma_A tau_B) / (psi(sigma) psi(tau)),   exp(-S2(l)) = E[r_l],
 * psi = sqrt(P).  Models GRU1D and GRU1D_F64, one layer; every other model and stacked layers: RNNWF_ERR_INVALID.
 * Swapped chains restart from the partner's hidden-state checkpoint at the cut: N (N - 1) cell evaluations per pair for
 * all cuts together (docs/renyi.md).  Runs in passes under the state budget (whole pairs per pass).  The sums of each
 * pass are reduced in a fixed order: a repeated call returns the same bits.  A pair with log r > 709 makes its cut's
 * sums +inf.  Overwrites the batch an earlier rnnwf_vmc_step left for rnnwf_vmc_gradient (a refused call does not).  */
/* Second Renyi entropy by the swap trick, cuts l = 0..N (A = first l sites; raster order for GRU1D_F64).
 *   samples      (2*npairs, N) int32, pair p = rows (2p, 2p+1); nullptr: draw them on the device exactly as
 *                rnnwf_sample(h, 2*npairs, seed, step, 2*pair_offset, ...) would (pair_offset ignored otherwise)
 *   sums         (N+1, 2) f64: sum_p r_l, sum_p r_l^2  (additive over shards)
 *   out_log_ratio(N+1, npairs) f64 or nullptr;  out_samples (2*npairs, N) int32 or nullptr (drawn chains)      */
int rnnwf_renyi2_swap(rnnwf_handle* h, const int32_t* samples, int64_t npairs, uint64_t seed, uint64_t step,
                      int64_t pair_offset, double* sums, double* out_log_ratio, int32_t* out_samples);

/* Second Renyi entropy of arbitrary regions (intervals, blocks, column cuts, disjoint pieces), by the same estimator with
 * A any site set (docs/renyi_regions.md):  r_A = psi(tau_A sigma_B) psi(sigma_A tau_B) / (psi(sigma) psi(tau)),
 * exp(-S2(A)) = E[r_A].  r_A = r_complement exactly, so each mask is normalised to site 0 not in A (complemented when
 * regions[r][0] == 1); a region that is then empty has log r = 0 exactly and costs nothing; otherwise, with f the first site
 * of A, the mixed chain (the partner's spins on A, the chain's own elsewhere) restarts from the chain's own checkpoint at
 * f - 1: N - f cell evaluations per chain and region.  Models, passes, fixed-order sums, +inf on log r > 709 and the
 * resident-batch rule as rnnwf_renyi2_swap.  RNNWF_ERR_INVALID, before any work: a refused model; nregions < 1 (or above
 * 65535); npairs < 1; null regions or sums; a mask entry other than 0 / 1; pair_offset < 0 with device-drawn samples.
 *   regions      (nregions, N) int32 of 0 / 1, 1 = site in A; sites in the model's order (raster ny * Nx + nx for GRU1D_F64)
 *   samples      (2*npairs, N) int32, pair p = rows (2p, 2p+1); nullptr: draw them on the device exactly as
 *                rnnwf_sample(h, 2*npairs, seed, step, 2*pair_offset, ...) would (pair_offset ignored otherwise)
 *   sums         (nregions, 2) f64: sum_p r_A, sum_p r_A^2  (additive over shards)
 *   out_log_ratio(nregions, npairs) f64 or nullptr;  out_samples (2*npairs, N) int32 or nullptr (drawn chains)      */
int rnnwf_renyi2_regions(rnnwf_handle* h, const int32_t* regions, int32_t nregions, const int32_t* samples, int64_t npairs,
                         uint64_t seed, uint64_t step, int64_t pair_offset, double* sums, double* out_log_ratio,
                         int32_t* out_samples);

/* rnnwf_renyi2_regions_2d: the same estimator for the 2D RNN (RNNWF_MODEL_MDRNN2D, float64; docs/renyi_2d.md).  Arguments, layouts and
 * outputs are rnnwf_renyi2_regions's, with N = Nx * Ny and one difference: the masks are indexed by the LATTICE index k = nx * Ny + ny,
 * the C-order flattening of samples (2*npairs, Nx, Ny) - the convention of rnnwf_pauli_step_2d - not by the position along the
 * zig-zag path; the driver maps them to visit order.  Each mask is normalised so that position 0 of the path (lattice site 0) is not
 * in A; a region that is then empty has log r = 0 exactly and costs nothing; otherwise, with f >= 1 the first position of A ALONG THE
 * PATH, the mixed chain (the partner's spins on A, the chain's own elsewhere) restarts from the chain's own state after position f,
 * takes position f's term from the head and recomputes the positions f+1..N-1: N - 1 - f cell evaluations per chain and region.
 * Passes, fixed-order sums, +inf on log r > 709 and the resident-batch rule as rnnwf_renyi2_swap.  RNNWF_ERR_INVALID, before any work
 * and without a launch: any model but MDRNN2D (rnnwf_renyi2_regions serves the GRU models); a width without a kernel; uncommitted
 * parameters; nregions < 1 (or above 65535); npairs < 1; null regions or sums; a mask entry other than 0 / 1; pair_offset < 0 with
 * device-drawn samples.
 *   regions      (nregions, Nx*Ny) int32 of 0 / 1, 1 = site in A, by lattice index
 *   samples      (2*npairs, Nx, Ny) int32, pair p = rows (2p, 2p+1); nullptr: draw them on the device exactly as
 *                rnnwf_sample(h, 2*npairs, seed, step, 2*pair_offset, ...) would (pair_offset ignored otherwise)
 *   sums         (nregions, 2) f64: sum_p r_A, sum_p r_A^2  (additive over shards)
 *   out_log_ratio(nregions, npairs) f64 or nullptr, rows under the caller's region index;  out_samples (2*npairs, Nx, Ny) int32 or
 *                nullptr (drawn chains)
 * Timing ids: 0 = base pass + site-term replay, 1 = paired masked-tail pass, 2 = log-ratio assembly + sums.  work[0] += sum over
 * non-empty regions of N - 1 - f per chain.                                                                                 */
int rnnwf_renyi2_regions_2d(rnnwf_handle* h, const int32_t* regions, int32_t nregions, const int32_t* samples, int64_t npairs,
                            uint64_t seed, uint64_t step, int64_t pair_offset, double* sums, double* out_log_ratio,
                            int32_t* out_samples);

/* rnnwf_renyi2_regions_complex: the same estimator for the complex RNN with the U(1) mask (RNNWF_MODEL_CRNN_U1, one layer;
 * docs/renyi_complex.md).  psi is complex, so is the estimator: with log psi the float64 sum of the per-site log-amplitudes and
 * phases (the imaginary part is never reduced modulo 2 pi)
 *   log r_A = [log psi(tau_A sigma_B) - log psi(sigma)] + [log psi(sigma_A tau_B) - log psi(tau)]   (no factor 1/2: log psi has it),
 *   r_A = exp(Re)(cos Im + i sin Im),   exp(-S2(A)) = E[Re r_A],   E[Im r_A] = 0 exactly.
 * Masks, normalisation (site 0 not in A), pairs (2p, 2p+1), device draws and the restart from the chain's own checkpoint at f - 1
 * (the U(1) count restarts from the ups of its own sites below f) as rnnwf_renyi2_regions.  Both chains of a pair lie in the
 * zero-magnetisation sector, so the two mixed chains do iff sigma and tau have the same number of ups in A; otherwise r_A = 0
 * exactly and the pair's out_log_ratio entry is (-inf, 0).  Only the surviving pairs are evaluated, compacted into full 16-chain
 * tiles: N - f cell evaluations per SURVIVING chain and non-empty region.  Passes under the state budget (whole pairs per pass),
 * fixed-order sums without float atomics (a repeated call returns the same bits) and the resident-batch rule as
 * rnnwf_renyi2_regions.  RNNWF_ERR_INVALID, before any work and without a launch: any model but CRNN_U1 (rnnwf_renyi2_regions serves
 * the GRU models, rnnwf_renyi2_regions_2d the 2D RNN); stacked layers; nregions < 1 (or above 65535); npairs < 1; null regions or
 * sums; a mask entry other than 0 / 1; pair_offset < 0 with device-drawn samples; a caller-supplied sample whose number of up spins
 * is not N / 2.  Uncommitted parameters: RNNWF_ERR_STATE.  rnnwf_renyi2_swap and rnnwf_renyi2_regions keep refusing this model.
 *   regions      (nregions, N) int32 of 0 / 1, 1 = site in A
 *   samples      (2*npairs, N) int32 in the sector, pair p = rows (2p, 2p+1); nullptr: draw them on the device exactly as
 *                rnnwf_sample(h, 2*npairs, seed, step, 2*pair_offset, ...) would (pair_offset ignored otherwise)
 *   sums         (nregions, 4) f64: sum Re r_A, sum Im r_A, sum (Re r_A)^2, sum (Im r_A)^2  (required, additive over shards)
 *   out_log_ratio(nregions, npairs, 2) f64 or nullptr: (Re, Im) of log r_A; (-inf, 0) for a pair outside the sector
 *   out_in_sector(nregions) int64 or nullptr: the surviving pairs of every region (additive over shards); npairs for a region that
 *                is empty or full
 *   out_samples  (2*npairs, N) int32 or nullptr (drawn chains)
 * Timing ids: 0 = base passes + site-term replay, 1 = survivor lists + paired tail pass, 2 = log-ratios, values and sums.  work[0]
 * += sum over non-empty regions of (N - f) x surviving chains; work[1] += the MFMA flops of the tiles run (padding included). */
int rnnwf_renyi2_regions_complex(rnnwf_handle* h, const int32_t* regions, int32_t nregions, const int32_t* samples, int64_t npairs,
                                 uint64_t seed, uint64_t step, int64_t pair_offset, double* sums, double* out_log_ratio,
                                 int64_t* out_in_sector, int32_t* out_samples);

/* ---- correlation functions -------------------------------------------------------------------------
 * The reference README's "correlation functions" of the positive one-layer GRU models (GRU1D, GRU1D_F64; every other model
 * and stacked layers: RNNWF_ERR_INVALID), psi = sqrt(P), samples sigma ~ P, s = 2 sigma - 1 (docs/correlations.md):
 *   <sz_i> = E[s_i],  <sz_i sz_j> = E[s_i s_j],
 *   <sx_i> = E[r_i],        log r_i  = 1/2 [log P(sigma with i flipped)       - log P(sigma)],
 *   <sx_i sx_j> = E[r_ij],  log r_ij = 1/2 [log P(sigma with i and j flipped) - log P(sigma)],  i < j, every pair.
 * Sites in the model's order (raster order ny * Nx + nx for GRU1D_F64).  Flipped chains restart from hidden-state checkpoints:
 * N(N-1)/2 + N(N-1)(N-2)/6 cell evaluations per chain.  Runs in passes under the state budget (whole 16-chain blocks per
 * pass; results do not depend on the pass size); sums are reduced in a fixed order: a repeated call returns the same bits.
 * A chain with log r > 709 makes the sums it enters +inf.  Overwrites the batch an earlier rnnwf_vmc_step left for
 * rnnwf_vmc_gradient (a refused call does not).
 *   samples      (ns, N) int32; nullptr: draw them on the device exactly as rnnwf_sample(h, ns, seed, step, sample_offset, ...)
 *                would (seed, step, sample_offset ignored otherwise)
 *   z_sums       (N) sum s_i;  zz_sums (N, N) sum s_i s_j, symmetric, diagonal ns
 *   x_sums       (N, 2) sum r_i, sum r_i^2
 *   xx_sums      (N, N, 5), entries i < j: sum r_ij, sum r_ij^2, sum r_ij r_i, sum r_ij r_j, sum r_i r_j; other entries 0
 *   all four are required and additive over shards
 *   out_log_ratio(N + N(N-1)/2, ns) f64 or nullptr: rows log r_i, then log r_ij in lexicographic order of (i, j)
 *   out_samples  (ns, N) int32 or nullptr (drawn chains)                                                        */
int rnnwf_correlations(rnnwf_handle* h, const int32_t* samples, int64_t ns, uint64_t seed, uint64_t step,
                       int64_t sample_offset, double* z_sums, double* zz_sums, double* x_sums, double* xx_sums,
                       double* out_log_ratio, int32_t* out_samples);

/* ---- correlation functions of the LSTM wave function ----------------------------------------------------
 * rnnwf_correlations for the LSTM cell over the raster path (LSTM1D_F64, one layer, 1..68 units, float64; every other model:
 * RNNWF_ERR_INVALID naming the entry that serves it, if one does) - docs/correlations_lstm.md.  The estimators, the arguments,
 * the layouts and shapes of the outputs, the pass rule (whole 16-chain blocks under the state budget, per-chain results
 * independent of the pass size, sums of the passes added on the host in pass order), the fixed-order reductions and the overflow
 * rule (a chain with log r > 709 makes the sums it enters +inf) are rnnwf_correlations'.  Sites are the chain position: the
 * column of `samples`, the raster index ny * Nx + nx.  Trunk i (spin i flipped) restarts from the base pass's state (h, c)
 * after site i and keeps its own states; branch (i, j) restarts from trunk i's state after site j:
 * N(N-1)/2 + N(N-1)(N-2)/6 cell evaluations per chain.  N = 1 runs no trunk kernel, N <= 2 no branch kernel.
 * Everything is validated before anything is touched: a refused call (another model, uncommitted parameters - RNNWF_ERR_STATE -,
 * ns < 1, a null sums array, sample_offset < 0 with drawn samples) leaves a batch of rnnwf_lstm_load_batch resident; a served
 * call overwrites it, and rnnwf_resident_samples is 0 afterwards.
 * Timing ids: 0 = base passes (the draw and the teacher-forced pass with checkpoints and both outcomes of every site),
 * 1 = trunk + branch passes, 2 = log-ratio assembly + sums.  work[0] += ns (N(N-1)/2 + N(N-1)(N-2)/6); work[1] += the MFMA flops
 * of those evaluations (per 16-chain block, padding included). */
int rnnwf_correlations_lstm(rnnwf_handle* h, const int32_t* samples, int64_t ns, uint64_t seed, uint64_t step,
                            int64_t sample_offset, double* z_sums, double* zz_sums, double* x_sums, double* xx_sums,
                            double* out_log_ratio, int32_t* out_samples);

/* ---- Pauli strings and arbitrary spin Hamiltonians ---------------------------------------------------
 * Expectation values of products of Pauli matrices and the local energy of any real-symmetric spin-1/2 Hamiltonian, for the
 * positive one-layer GRU models (GRU1D, GRU1D_F64; every other model and stacked layers: RNNWF_ERR_INVALID), psi = sqrt(P),
 * samples sigma ~ P, s = 2 sigma - 1 (docs/pauli.md).  Term k is O_k = (prod_{i in S_k} sz_i)(prod_{i in F_k} sx_i), sz to the left:
 *   v_k(sigma) = prod_{i in S_k} s_i(sigma) * exp(1/2 [log P(sigma ^ F_k) - log P(sigma)]),   E[v_k] = <psi|O_k|psi>,
 *   E_loc(sigma) = sum_k coeff_k v_k(sigma).
 * (sy = -i sz sx: a string with an even number of sy is +-1 times such a term; rnnwavefunctions_amd.observables.pauli_terms.)
 * Terms are grouped by flip mask: a mask shared by several terms is evaluated once, a term with empty F_k costs nothing, and order
 * and duplication of the terms change no per-term bit.  With f the first site of F, the flipped chain restarts from the chain's own
 * checkpoint at f - 1 (f = 0: from the zero state, all N sites): N - f cell evaluations per chain and distinct mask.  Runs in
 * passes of whole 16-chain blocks under the state budget (per-sample results do not depend on the pass size); sums are reduced in
 * a fixed order: a repeated call returns the same bits.  A chain with log r > 709 makes the sums it enters +inf.
 * A call that ran in ONE pass leaves its batch (spins, checkpoints, E_loc) resident as rnnwf_vmc_step does: rnnwf_vmc_gradient
 * then differentiates the VMC cost of this Hamiltonian.  A call in several passes leaves no batch; a refused call leaves an
 * earlier one usable.  RNNWF_ERR_INVALID, before any work: a refused model; nterms < 1; more than 65535 distinct non-empty flip
 * masks; ns < 1; null flip, sign, coeff or term_sums; a mask entry other than 0 / 1; sample_offset < 0 with device-drawn samples.
 *   flip, sign   (nterms, N) int32 of 0 / 1: F_k and S_k, indexed by the position p = 0..N-1 along the model's chain (the column of
 *                `samples`).  The pass attaches no geometry to p.  For GRU1D_F64 created with (nx, ny) rnnwf_tfim2d_eloc places lattice
 *                site (i, j), 0 <= i < nx, 0 <= j < ny, at p = i * ny + j (j runs fastest), and observables.tfim_hamiltonian does the
 *                same; "raster ny * Nx + nx" at the other observables names p by the fast and the slow index of the same chain
 *   coeff        (nterms) f64
 *   samples      (ns, N) int32; nullptr: draw them on the device exactly as rnnwf_sample(h, ns, seed, step, sample_offset, ...)
 *                would (seed, step, sample_offset ignored otherwise)
 *   term_sums    (nterms, 2) f64: sum v_k, sum v_k^2  (required, additive over shards)
 *   out_eloc     (ns) f64 or nullptr;  moments[4] or nullptr: {sum E_loc, sum E_loc^2, ns, 0} as rnnwf_vmc_step returns them
 *   out_log_ratio(nmasks, ns) f64 or nullptr: rows = the distinct non-empty flip masks in order of first appearance
 *   out_samples  (ns, N) int32 or nullptr (drawn chains)
 * Timing ids: 0 = base pass + site-term replay, 1 = flip-mask pass, 2 = log-ratios, term sums, E_loc and moments.  work[0] +=
 * sum over distinct masks of N - f per chain.                                                                             */
int rnnwf_pauli_step(rnnwf_handle* h, const int32_t* flip, const int32_t* sign, const double* coeff, int32_t nterms,
                     const int32_t* samples, int64_t ns, uint64_t seed, uint64_t step, int64_t sample_offset,
                     double* term_sums, double* out_eloc, double* moments, double* out_log_ratio, int32_t* out_samples);

/* rnnwf_pauli_step_2d: the same estimator for the 2D RNN (RNNWF_MODEL_MDRNN2D, float64; docs/pauli_2d.md).  Arguments, layouts and
 * outputs are rnnwf_pauli_step's, with N = Nx * Ny and one difference: the masks are indexed by the LATTICE index k = nx * Ny + ny,
 * the C-order flattening of samples (ns, Nx, Ny) - the convention of rnnwf_tfim2d_eloc's Jz - not by the position along the
 * zig-zag path; the driver maps them to visit order.  With f the first flipped position ALONG THE PATH, the flipped chain restarts
 * from the base pass's state after position f (which no spin at or behind f enters), takes position f's term from the head and
 * recomputes the positions f+1..N-1: N - 1 - f cell evaluations per chain and distinct mask.  Passes, fixed-order sums, the resident
 * batch (one pass: spins, states and E_loc stay as rnnwf_tfim2d_eloc's step leaves them, for rnnwf_vmc_gradient) and the
 * out_log_ratio rows (distinct non-empty masks in order of first appearance) as above.  RNNWF_ERR_INVALID, before any work and
 * without a launch: any model but MDRNN2D (rnnwf_pauli_step serves the GRU models); a width without a kernel; uncommitted
 * parameters; nterms < 1; ns < 1; null flip, sign, coeff or term_sums; a mask entry other than 0 / 1; more than 65535 distinct
 * non-empty flip masks; sample_offset < 0 with device-drawn samples.
 * Timing ids: 0 = base pass + site-term replay, 1 = masked-tail pass, 2 = log-ratios, term sums, E_loc and moments.  work[0] +=
 * sum over distinct masks of N - 1 - f per chain.                                                                          */
int rnnwf_pauli_step_2d(rnnwf_handle* h, const int32_t* flip, const int32_t* sign, const double* coeff, int32_t nterms,
                        const int32_t* samples, int64_t ns, uint64_t seed, uint64_t step, int64_t sample_offset,
                        double* term_sums, double* out_eloc, double* moments, double* out_log_ratio, int32_t* out_samples);

/* rnnwf_pauli_step_complex: the same estimator for the complex RNN with the U(1) mask (RNNWF_MODEL_CRNN_U1, one layer;
 * docs/pauli_complex.md).  psi is complex, so is the estimator: with d = log psi(sigma ^ F_k) - log psi(sigma) (complex, float64,
 * the unwrapped sum of the per-site log-amplitudes and phases; the imaginary part is never reduced modulo 2 pi)
 *   v_k(sigma) = prod_{i in S_k} s_i(sigma) * exp(Re d) (cos Im d + i sin Im d),   E[v_k] = <psi|O_k|psi>,
 *   E_loc(sigma) = sum_k coeff_k v_k(sigma)   with complex coeff_k: strings with an odd number of sy and terms with imaginary
 * matrix elements are legal here.  A flipped configuration outside the zero-magnetisation sector has psi = 0 exactly: its v is
 * exactly (0, 0), its out_log_ratio entry (-inf, 0), and no NaN appears.  Arguments as rnnwf_pauli_step, except:
 *   coeff_re_im   (nterms, 2) f64: complex coefficients
 *   term_sums     (nterms, 4) f64: sum Re v_k, sum Im v_k, sum (Re v_k)^2, sum (Im v_k)^2  (required, additive over shards)
 *   out_eloc_re_im(ns, 2) f32 = complex64 or nullptr (the type of rnnwf_j1j2_eloc and of rnnwf_vmc_step for this model)
 *   moments[4] or nullptr: {sum Re E, sum (Re E)^2, ns, sum Im E} of those complex64 values, as rnnwf_vmc_step returns them
 *   out_log_ratio (nmasks, ns, 2) f64 or nullptr: (Re d, Im d), rows = the distinct non-empty flip masks in order of first appearance
 * Grouping by flip mask, restart from the chain's own checkpoint at f - 1 (the U(1) count restarts from the ups of its own sites
 * below f), N - f cell evaluations per chain and distinct mask, passes under the state budget, fixed-order sums and the signs read
 * from the SAMPLED configuration as for rnnwf_pauli_step.  The checkpointed base pass always runs on the one-wave f32 kernel.
 * A call that ran in ONE pass leaves spins, checkpoints and complex64 E_loc resident as rnnwf_vmc_step does for this model:
 * rnnwf_vmc_gradient(mean_re, mean_im, ns) then differentiates the complex cost of this Hamiltonian.  A call in several passes
 * leaves no batch; a refused call leaves an earlier one usable.  RNNWF_ERR_INVALID, before any work and without a launch: any
 * model but CRNN_U1 (rnnwf_pauli_step serves the GRU models, rnnwf_pauli_step_2d the 2D RNN); stacked layers; nterms < 1; ns < 1;
 * null flip, sign, coeff_re_im or term_sums; a mask entry other than 0 / 1; more than 65535 distinct non-empty flip masks;
 * sample_offset < 0 with device-drawn samples; nterms x ceil(ns / 256) past the grid limit; a caller-supplied sample whose number
 * of up spins is not N / 2 (samples must lie in the zero-magnetisation sector: outside it their own log psi is -inf and the
 * ratio undefined; device-drawn chains always lie in it).  Uncommitted parameters:
 * RNNWF_ERR_STATE.  rnnwf_pauli_step and rnnwf_pauli_step_2d keep refusing this model.
 * Timing ids: 0 = base pass + site-term replay, 1 = flip-mask pass, 2 = log-ratios, term sums, E_loc and moments.  work[0] +=
 * sum over distinct masks of N - f per chain.                                                                             */
int rnnwf_pauli_step_complex(rnnwf_handle* h, const int32_t* flip, const int32_t* sign, const double* coeff_re_im, int32_t nterms,
                             const int32_t* samples, int64_t ns, uint64_t seed, uint64_t step, int64_t sample_offset,
                             double* term_sums, float* out_eloc_re_im, double* moments, double* out_log_ratio, int32_t* out_samples);

/* rnnwf_pauli_train_steps / rnnwf_pauli_train_steps_complex: K whole Adam iterations (1 <= K <= 1024) on the Hamiltonian
 * sum_k coeff_k O_k of the terms with ONE host synchronisation behind the last iteration: the counterpart of rnnwf_train_steps for the
 * Hamiltonians of rnnwf_pauli_step / rnnwf_pauli_step_complex (docs/pauli_train.md).  The models are those of the two entries (the
 * positive one-layer GRU1D and GRU1D_F64; the one-layer CRNN_U1).  The terms are checked, grouped and uploaded once per call.  Iteration
 * k = 0 .. K-1, all on the handle's stream: numsamples samples drawn with step index step0 + k as rnnwf_sample draws them; the base
 * pass, site terms and masked tails of the pauli entry; one amplitude ratio per (distinct flip mask, chain), read by E_loc and by the
 * per-term sums; the moments into row k of `moments` ([K][4], as the pauli entry returns them); the gradient of the VMC cost with
 * the mean energy read from those moments on the device; Adam with learning_rates[k] and bias correction number t + k + 1 (t the
 * count of rnnwf_adam_get_state) on the flat float64 parameters, rounded to the model's type; every weight image rebuilt on the
 * device.  The arithmetic is that of the host loop pauli entry -> rnnwf_vmc_gradient -> host Adam -> rnnwf_set_param, operation for
 * operation: moments, parameters and Adam's state equal that loop's bit for bit.
 * term_sums: NULL (the per-term kernels are then not launched), or [K][nterms][2] (complex: [K][nterms][4]): row k holds what the
 * pauli entry's term_sums holds for iteration k's batch.  out_eloc: NULL, or [numsamples] E_loc (complex64 for the complex entry) of
 * the LAST iteration's batch.
 * Afterwards, as after rnnwf_train_steps: no batch is resident, rnnwf_get_param and rnnwf_commit_params see the device's parameters,
 * Adam's step count has advanced by K.
 * Refused before anything is launched or changed, leaving parameters, Adam's state and the resident batch as they were:
 * RNNWF_ERR_INVALID "<entry>: <why>" for a model the pauli entry refuses, a handle with a communicator, K outside 1..1024, nterms < 1,
 * numsamples < 1, null flip, sign, coeff, learning_rates or moments, sample_offset < 0, a learning_rates[k] that is not finite, a mask
 * entry other than 0 / 1, more than 65535 distinct non-empty flip masks; RNNWF_ERR_STATE for uncommitted parameters; RNNWF_ERR_NOMEM
 * "<entry>: ... exceed the state budget of one pass; split the batch" for numsamples beyond one pass of the pauli entry.
 * Timing ids: 0 = base passes + site-term replay, 1 = masked-tail pass, 2 = ratios, [term sums,] E_loc and moments, 3 / 4 = gradient. */
int rnnwf_pauli_train_steps(rnnwf_handle* h, const int32_t* flip, const int32_t* sign, const double* coeff, int32_t nterms, int32_t K,
                            int64_t numsamples, uint64_t seed, uint64_t step0, int64_t sample_offset, const double* learning_rates,
                            double beta1, double beta2, double epsilon, double* moments, double* term_sums, double* out_eloc);
int rnnwf_pauli_train_steps_complex(rnnwf_handle* h, const int32_t* flip, const int32_t* sign, const double* coeff_re_im, int32_t nterms,
                                    int32_t K, int64_t numsamples, uint64_t seed, uint64_t step0, int64_t sample_offset,
                                    const double* learning_rates, double beta1, double beta2, double epsilon, double* moments,
                                    double* term_sums, float* out_eloc_re_im);

/* rnnwf_pauli_train_steps_2d: the same K iterations for the 2D RNN (RNNWF_MODEL_MDRNN2D, float64, 1..84 units) on the Hamiltonians of
 * rnnwf_pauli_step_2d (docs/pauli_train.md, "2D RNN").  Arguments, layouts, outputs, refusals and the state afterwards are
 * rnnwf_pauli_train_steps's, with N = Nx * Ny and that entry's one difference: the masks are indexed by the LATTICE index
 * k = nx * Ny + ny; the driver maps them to visit order, and a bad mask entry is named by its lattice index.  The sampling base pass
 * keeps every position's state and log P, so an iteration has no second pass in front of the site terms and masked tails.  moments
 * [K][4], term_sums NULL or [K][nterms][2], out_eloc NULL or [numsamples] float64 of the last iteration's batch.  Moments, per-term
 * sums, parameters and Adam's state equal the host loop rnnwf_pauli_step_2d -> rnnwf_vmc_gradient -> host Adam -> rnnwf_set_param bit
 * for bit.  RNNWF_ERR_INVALID for any model but MDRNN2D (rnnwf_pauli_train_steps serves the GRU models,
 * rnnwf_pauli_train_steps_complex the complex RNN, and both keep refusing this one); RNNWF_ERR_STATE for uncommitted parameters;
 * RNNWF_ERR_NOMEM "... split the batch" for numsamples beyond one pass of rnnwf_pauli_step_2d.  Timing ids as above, 0 being the one
 * sampling base pass + site-term replay.                                                                                         */
int rnnwf_pauli_train_steps_2d(rnnwf_handle* h, const int32_t* flip, const int32_t* sign, const double* coeff, int32_t nterms, int32_t K,
                               int64_t numsamples, uint64_t seed, uint64_t step0, int64_t sample_offset, const double* learning_rates,
                               double beta1, double beta2, double epsilon, double* moments, double* term_sums, double* out_eloc);

/* rnnwf_pauli_step_stack, rnnwf_pauli_train_steps_stack: rnnwf_pauli_step and rnnwf_pauli_train_steps for STACKED GRU layers
 * (RNNWF_MODEL_GRU1D float32 and RNNWF_MODEL_GRU1D_F64 float64 with 2..4 layers, every stack rnnwf_create accepts, layers of
 * unequal width included; docs/pauli_stack.md).  Arguments, layouts, outputs, passes, fixed-order sums, the resident-batch rule,
 * the state after the train entry and the refusals are those of the one-layer entries.  With f the first flipped site, the flipped
 * chain restarts ALL layers from the chain's own checkpoint of site f - 1 (f = 0: from the zero states) and recomputes the sites
 * f..N-1: N - f steps of the whole stack per chain and distinct mask, counted in work[0].  The checkpointed base pass always runs on
 * the one-wave MFMA stack kernel, whatever kernel rnnwf_vmc_step takes for the handle.  RNNWF_ERR_INVALID, before any work: a
 * one-layer handle (rnnwf_pauli_step / rnnwf_pauli_train_steps serve it, and keep refusing stacks); every other model, in
 * rnnwf_pauli_step's words.  Timing ids as rnnwf_pauli_step / rnnwf_pauli_train_steps.                                          */
int rnnwf_pauli_step_stack(rnnwf_handle* h, const int32_t* flip, const int32_t* sign, const double* coeff, int32_t nterms,
                           const int32_t* samples, int64_t ns, uint64_t seed, uint64_t step, int64_t sample_offset,
                           double* term_sums, double* out_eloc, double* moments, double* out_log_ratio, int32_t* out_samples);
int rnnwf_pauli_train_steps_stack(rnnwf_handle* h, const int32_t* flip, const int32_t* sign, const double* coeff, int32_t nterms, int32_t K,
                                  int64_t numsamples, uint64_t seed, uint64_t step0, int64_t sample_offset, const double* learning_rates,
                                  double beta1, double beta2, double epsilon, double* moments, double* term_sums, double* out_eloc);

/* rnnwf_renyi2_regions_stack: rnnwf_renyi2_regions for STACKED GRU layers (RNNWF_MODEL_GRU1D float32 and RNNWF_MODEL_GRU1D_F64 float64
 * with 2..4 layers, every stack rnnwf_create accepts, layers of unequal width included; docs/renyi_stack.md).  Arguments, layouts,
 * outputs, the normalisation of the masks (site 0 not in A; an empty or full region gives log r = 0 exactly at no cost), passes,
 * fixed-order sums and +inf on log r > 709 are rnnwf_renyi2_regions's.  With f >= 1 the first site of A, the mixed chain (the
 * partner's spins on A, the chain's own elsewhere) restarts ALL layers from the chain's own checkpoint of site f - 1 and recomputes
 * the sites f..N-1: N - f steps of the whole stack per chain and region, counted in work[0].  The checkpointed base pass always runs
 * on the one-wave MFMA stack kernel, whatever kernel rnnwf_vmc_step takes for the handle.  No batch is resident after a served call.
 * RNNWF_ERR_INVALID, before any work (a refused call leaves an earlier batch usable): a one-layer handle (rnnwf_renyi2_regions serves
 * it, and keeps refusing stacks); every other model, in rnnwf_renyi2_regions's words; the argument checks of rnnwf_renyi2_regions.
 * Timing ids: 0 = base pass + site-term replay, 1 = paired masked-tail pass, 2 = log-ratio assembly + sums.                      */
int rnnwf_renyi2_regions_stack(rnnwf_handle* h, const int32_t* regions, int32_t nregions, const int32_t* samples, int64_t npairs,
                               uint64_t seed, uint64_t step, int64_t pair_offset, double* sums, double* out_log_ratio,
                               int32_t* out_samples);

/* ---- stochastic reconfiguration (natural gradient, minSR; docs/sr.md) -------------------------------------------------------
 * psi = sqrt(P) real and positive:  O[s][k] = d log psi(sigma_s) / d theta_k = 1/2 d log P(sigma_s) / d theta_k, theta in the flat
 * order of rnnwf_set_params_flat;  dO = O - mean_s O;  eps_s = E_loc,s - mean E.  The minSR direction with diagonal shift lambda is
 *   delta = dO^T (dO dO^T + ns lambda I)^-1 eps  =  (S + lambda I)^-1 F,   S = dO^T dO / ns,  F = dO^T eps / ns
 * (2 F is the gradient rnnwf_vmc_gradient returns); the update is theta <- theta - lr delta.  The device does the per-sample
 * Jacobian, the centred Gram matrix and dO^T y; the ns x ns solve is the caller's (rnnwf_sr_gram, a host Cholesky as in
 * rnnwavefunctions_amd/sr.py, rnnwf_sr_apply) or the device's (rnnwf_sr_solve, rnnwf_sr_direction: blocked Cholesky in float64).
 * All five work on the RESIDENT batch of the last rnnwf_vmc_step / rnnwf_load_batch (RNNWF_ERR_STATE without one) and keep the
 * Jacobian on the device, image order, element type of the model, until the batch or the parameters change.
 * Models GRU1D and GRU1D_F64 with one layer of at most 68 units.  RNNWF_ERR_INVALID "<entry>: <why>", before any work: the parity
 * model, the complex RNN, the 2D RNN, the LSTM, stacked layers, wider layers, a handle with a communicator.  RNNWF_ERR_NOMEM
 * "... ns too large for the SR workspace": ns > 4096, or Jacobian + Gram matrix beyond the state budget (RNNWF_STATE_BUDGET_MB).
 * A refused call leaves the resident batch usable.  Every sum has a fixed order: the same batch gives the same bits.
 * rnnwf_log_derivatives: one backward pass with unit weights (per-sample head rows kept) and one N-row outer-product sum per
 *   sample on the MFMA.  out (ns, nparams) f64 = O, or NULL: build the device Jacobian only.  ns and nparams must be the resident
 *   batch's and rnnwf_num_params'.
 * rnnwf_sr_gram: gram (ns, ns) f64 = dO dO^T (f64 MFMA on operands converted and centred on the fly; exactly symmetric),
 *   eps (ns,) f64 from the resident local energies.  Builds the Jacobian when it is stale.
 * rnnwf_sr_apply: y (ns,) f64 -> out_direction (nparams,) f64 = dO^T y, one pass over the Jacobian.  Builds it when it is stale.
 * rnnwf_sr_solve, rnnwf_sr_direction: the solve on the device.  Both build the Jacobian when it is stale, rebuild the Gram matrix
 *   (no copy to the host), factorise gram + ns diag_shift I = L L^T by a blocked right-looking Cholesky in float64 (32 x 32 blocks,
 *   trailing update on the f64 MFMA) with eps, formed on the device from the resident local energies, carried as one more row, and
 *   finish with a blocked backward sweep.  rnnwf_sr_solve returns y (ns,) f64, the solution for the centred eps (not itself
 *   centred); rnnwf_sr_direction goes on with dO^T y on the device and returns delta (nparams,) f64: nparams doubles cross the bus.
 *   RNNWF_ERR_INVALID "<entry>: diag_shift must be positive and finite", before any work.  The workspace check counts the factor:
 *   Jacobian + 2 ns^2 doubles within the state budget.  RNNWF_ERR_NUMERIC "<entry>: pivot <index> ... (diag_shift ...)": a pivot that
 *   is not positive and finite (found at the call's one synchronisation; the resident batch stays usable).  */
int rnnwf_log_derivatives(rnnwf_handle* h, double* out, int64_t ns, int64_t nparams);
int rnnwf_sr_gram(rnnwf_handle* h, double* gram, double* eps);
int rnnwf_sr_apply(rnnwf_handle* h, const double* y, double* out_direction);
int rnnwf_sr_solve(rnnwf_handle* h, double diag_shift, double* y);
int rnnwf_sr_direction(rnnwf_handle* h, double diag_shift, double* out_direction);
/* samples of the resident batch (what sizes the five calls above), 0 without one */
int64_t rnnwf_resident_samples(const rnnwf_handle* h);
/* rnnwf_sr_train_steps: K whole minSR iterations (1 <= K <= 1024) with ONE host synchronisation, the counterpart of rnnwf_train_steps.
 * Iteration k = 0 .. K-1, all on the handle's stream: the fused VMC step of numsamples samples drawn with step index step0 + k (its
 * moments into row k of `moments`, [K][4] as rnnwf_vmc_step returns them); the Jacobian, the Gram matrix, the Cholesky solve with
 * diag_shifts[k] and dO^T y exactly as rnnwf_sr_direction runs them; theta_i <- theta_i - learning_rates[k] delta_i on the flat float64
 * parameters of the device (the product and the difference each rounded once, then rounded to float32 for GRU1D: the arithmetic of
 * rnnwavefunctions_amd/sr.py's train_tfim, so the trajectory equals that host loop's bit for bit); every weight image rebuilt on the device.
 * Afterwards, as after rnnwf_train_steps: no batch is resident, rnnwf_get_param and rnnwf_commit_params see the device's parameters,
 * Adam's moments and step count are untouched.
 * Refused before anything is launched or changed, leaving parameters, resident batch and Jacobian as they were: RNNWF_ERR_INVALID
 * "rnnwf_sr_train_steps: <why>" for the handles of the list above, bad arguments (K, numsamples < 1, a null pointer), the wrong number of
 * couplings, a diag_shifts[k] that is not positive and finite, a learning_rates[k] that is not finite; RNNWF_ERR_STATE for uncommitted
 * parameters; RNNWF_ERR_NOMEM "... ns too large for the SR workspace" for numsamples (the factor counted).
 * A pivot that is not positive and finite in iteration k: that iteration's update and all later ones are not stored (theta stays what it
 * was before iteration k, the later iterations sample it again), `moments` is filled for all K rows, and the call returns
 * RNNWF_ERR_NUMERIC "rnnwf_sr_train_steps: iteration <k>: pivot <index> ... (diag_shift ..., ... samples)" after its synchronisation.  */
int rnnwf_sr_train_steps(rnnwf_handle* h, int32_t K, int64_t numsamples, uint64_t seed, uint64_t step0, int64_t sample_offset,
                         const double* couplings, int64_t n_couplings, const double* learning_rates, const double* diag_shifts,
                         double* moments);

/* ---- stochastic reconfiguration for the complex RNN (CRNN_U1; docs/sr_complex.md) ------------------------------------------------
 * psi = sqrt(P) e^{i phi}, theta real:  O[s][k] = d log psi(sigma_s) / d theta_k = 1/2 d log P / d theta_k + i d phi / d theta_k,
 * eps_s = E_loc,s - mean E (complex).  S = Re(dO^H dO) / ns and F = Re(dO^H eps) / ns; with the stacked real matrix
 * Obar = [Re dO ; Im dO] (2 ns x nparams) and ebar = [Re eps ; Im eps], each half centred with its own mean, S = Obar^T Obar / ns,
 * F = Obar^T ebar / ns (2 F is the gradient rnnwf_vmc_gradient returns) and the minSR direction is
 *   delta = Obar^T (Obar Obar^T + ns lambda I)^-1 ebar  =  (S + lambda I)^-1 F:
 * the five calls above on a system of order 2 ns, rows [0, ns) the real parts and rows [ns, 2 ns) the imaginary parts.
 * rnnwf_log_derivatives_complex: out_re_im (2, ns, nparams) f64 = [Re O ; Im O] (not centred), or NULL.  rnnwf_sr_gram_complex: gram
 * (2 ns, 2 ns) f64 = Obar Obar^T, exactly symmetric; eps (2 ns,) f64 = ebar.  rnnwf_sr_apply_complex: y (2 ns,) -> Obar^T y (each half of y
 * is centred).  rnnwf_sr_solve_complex: y (2 ns,) of (gram + ns diag_shift I) y = ebar.  rnnwf_sr_direction_complex: delta (nparams,).
 * The complex RNN with one layer of at most 68 units; ns <= RNNWF_SR_COMPLEX_MAX_SAMPLES.  Refusals, state rules, workspace check (with
 * 2 ns rows), pivot status and error codes as for the five calls above; RNNWF_ERR_INVALID "<entry>: <why>" for every other model.  */
#define RNNWF_SR_COMPLEX_MAX_SAMPLES 2048
int rnnwf_log_derivatives_complex(rnnwf_handle* h, double* out_re_im, int64_t ns, int64_t nparams);
int rnnwf_sr_gram_complex(rnnwf_handle* h, double* gram, double* eps);
int rnnwf_sr_apply_complex(rnnwf_handle* h, const double* y, double* out_direction);
int rnnwf_sr_solve_complex(rnnwf_handle* h, double diag_shift, double* y);
int rnnwf_sr_direction_complex(rnnwf_handle* h, double diag_shift, double* out_direction);

/* ---- stochastic reconfiguration for the 2D RNN (MDRNN2D; docs/sr_2d.md) -----------------------------------------------------------
 * psi = sqrt(P) real and positive: the conventions, arguments, state rules, workspace check (ns <= 4096), pivot status and error
 * codes of the positive model's five calls, on the resident batch of the last rnnwf_vmc_step / rnnwf_load_batch of an MDRNN2D handle
 * at every width its gradient serves (up to 84 units).  O[s][k] = 1/2 d log P(sigma_s) / d theta_k in the flat order of
 * rnnwf_set_params_flat; 2 F = 2 dO^T eps / ns is the gradient rnnwf_vmc_gradient returns for this model.
 * RNNWF_ERR_INVALID "<entry>: only for the 2D RNN (RNNWF_MODEL_MDRNN2D)" for every other model; a handle with a communicator is
 * refused.  The positive model's and the complex RNN's entries keep refusing this model.                                        */
int rnnwf_log_derivatives_2d(rnnwf_handle* h, double* out, int64_t ns, int64_t nparams);
int rnnwf_sr_gram_2d(rnnwf_handle* h, double* gram, double* eps);
int rnnwf_sr_apply_2d(rnnwf_handle* h, const double* y, double* out_direction);
int rnnwf_sr_solve_2d(rnnwf_handle* h, double diag_shift, double* y);
int rnnwf_sr_direction_2d(rnnwf_handle* h, double diag_shift, double* out_direction);

/* ---- stochastic reconfiguration for the LSTM wave function (LSTM1D_F64; docs/sr_lstm.md) -----------------------------------------
 * psi = sqrt(P) real and positive: the conventions, arguments, state rules, workspace check (ns <= 4096), pivot status and error
 * codes of the positive model's five calls, on the resident batch of an LSTM1D_F64 handle (one layer, up to 68 units).  O[s][k] =
 * 1/2 d log P(sigma_s) / d theta_k in the flat order of rnnwf_set_params_flat; sum_s 2 w_s O_s is what rnnwf_lstm_gradient returns
 * for the weights w.
 * An LSTM handle has a resident batch only after one of two entries (rnnwf_vmc_step leaves it none and rnnwf_load_batch refuses it);
 * without one the five calls return RNNWF_ERR_STATE "<entry>: call rnnwf_lstm_load_batch or rnnwf_sr_step_lstm first".
 * rnnwf_lstm_load_batch: samples (ns, N) int32 and their local energies eloc (ns,) f64 become the resident batch (teacher-forced
 *     base pass); validates before it touches anything.
 * rnnwf_sr_step_lstm: one minSR iteration's device work with one host synchronisation - rnnwf_vmc_step's fused TFIM step at (seed,
 *     step, sample_offset) with couplings = [Jz (N) | Bx], moments (4,) as rnnwf_vmc_step returns them bit for bit, then the
 *     direction of rnnwf_sr_direction_lstm on that batch into out_direction (nparams,).  The batch and its Jacobian stay resident.
 * RNNWF_ERR_INVALID "<entry>: only for the LSTM wave function (RNNWF_MODEL_LSTM1D_F64)" for every other model; a handle with a
 * communicator is refused.  The other families' entries, rnnwf_sr_train_steps among them, keep refusing this model.              */
int rnnwf_log_derivatives_lstm(rnnwf_handle* h, double* out, int64_t ns, int64_t nparams);
int rnnwf_sr_gram_lstm(rnnwf_handle* h, double* gram, double* eps);
int rnnwf_sr_apply_lstm(rnnwf_handle* h, const double* y, double* out_direction);
int rnnwf_sr_solve_lstm(rnnwf_handle* h, double diag_shift, double* y);
int rnnwf_sr_direction_lstm(rnnwf_handle* h, double diag_shift, double* out_direction);
int rnnwf_lstm_load_batch(rnnwf_handle* h, const int32_t* samples, int64_t ns, const double* eloc);
int rnnwf_sr_step_lstm(rnnwf_handle* h, int64_t numsamples, uint64_t seed, uint64_t step, int64_t sample_offset, const double* couplings,
                       int64_t n_couplings, double diag_shift, double* moments, double* out_direction, int64_t nparams);

/* ---- multi-GPU: one RCCL all-reduce of the energy moments -------------------------------------
 * The reference is single-process; these add the one data-parallel collective of SURVEY.md 8e.
 * One process per GPU: rank 0 calls rnnwf_comm_unique_id and ships the 128 bytes to the other
 * ranks by any means (the Python host uses the launcher's store); every rank then calls
 * rnnwf_comm_init.  rnnwf_allreduce_moments sums `count` doubles in place over all ranks
 * (ncclAllReduce, ncclDouble, ncclSum on the handle's stream) - population mean/variance follow
 * as S1/n and S2/n - (S1/n)^2 (np.mean / np.var, TrainingRNN_1DTFIM.py:206-207).              */
#define RNNWF_UNIQUE_ID_BYTES 128
int rnnwf_comm_unique_id(void* id_out);
int rnnwf_comm_init(rnnwf_handle* h, const void* id, int32_t rank, int32_t nranks);
int rnnwf_allreduce_moments(rnnwf_handle* h, double* moments, int32_t count);
/* The same all-reduce for `count` doubles of any length (gradient partial sums held by the caller, histories ...):
 * host array -> pinned staging -> device -> ncclAllReduce(sum) on the handle's stream -> back; identity on one rank. */
int rnnwf_allreduce_f64(rnnwf_handle* h, double* data, int64_t count);
/* on != 0: rnnwf_vmc_step itself returns the moments summed over all ranks - the all-reduce runs on the handle's stream on
 * the device-resident moments, in front of the step's single host synchronisation (no second round trip per step).   */
int rnnwf_comm_reduce_in_step(rnnwf_handle* h, int32_t on);
/* The communicator's own answer (ncclCommCount, ncclCommUserRank) and the handle's device ordinal; 1 / 0 when no
 * communicator exists.  Reports print it, so that N one-rank runs cannot be mistaken for one N-rank run.    */
int rnnwf_comm_info(rnnwf_handle* h, int32_t* nranks, int32_t* rank, int32_t* device);
int rnnwf_comm_destroy(rnnwf_handle* h);

/* ---- gradient of the LSTM wave function (RNNWF_MODEL_LSTM1D_F64; docs/lstm.md, "Gradient") ------------------------
 * The entries above keep refusing an LSTM handle; these two are its gradient.  Both leave the tensors where rnnwf_get_grad,
 * rnnwf_get_grads_flat and rnnwf_allreduce_grads read them.  Any other model: RNNWF_ERR_INVALID; parameters not
 * committed: RNNWF_ERR_STATE; more samples than the state budget of one pass holds: RNNWF_ERR_NOMEM ("split the batch").
 *
 * rnnwf_lstm_gradient: d/dtheta sum_s weights[s] log P(samples[s]) for B caller-supplied configurations (B, N) int32
 *   (teacher-forced base pass with checkpoints, back-propagation through time, weight-gradient product).  With
 *   weights[s] = (E_s - mean E) / n it is the gradient of the reference's cost; several processes centre with the global mean.
 * rnnwf_lstm_vmc_gradient_step: rnnwf_vmc_step (same samples, E_loc and moments, bit for bit; couplings = Jz (Nx*Ny) then Bx)
 *   followed by the gradient with weights (E_s - moments[0] / moments[2]) * (1 / moments[2]) on the states that step left on
 *   the device: no second base pass, one host synchronisation.  Single process only (no communicator).              */
int rnnwf_lstm_gradient(rnnwf_handle* h, const int32_t* samples, int64_t B, const double* weights);
int rnnwf_lstm_vmc_gradient_step(rnnwf_handle* h, int64_t numsamples, uint64_t seed, uint64_t step, int64_t sample_offset,
                                 const double* couplings, double* moments, int32_t* out_samples, double* out_eloc);

/* ---- Pauli strings and generic Hamiltonians for the LSTM wave function (RNNWF_MODEL_LSTM1D_F64; docs/pauli_lstm.md) ----------
 * rnnwf_pauli_step_lstm: rnnwf_pauli_step for the LSTM cell (one layer, 1..68 units, float64).  Arguments, layouts, outputs, passes
 *   under RNNWF_STATE_BUDGET_MB, fixed-order sums, +inf on log r > 709 and the argument refusals (a mask entry that is not 0 or 1,
 *   nterms < 1, ns < 1, a negative sample_offset, more than 65 535 distinct flip masks, the grid of the term kernel) are
 *   rnnwf_pauli_step's; masks are indexed by the chain position, the column of `samples` (raster order).  A mask whose first flipped
 *   site is f >= 1 restarts the chain from its own checkpoint (h, c) of site f - 1: N - f cell evaluations per chain and mask,
 *   counted in work[0].  Terms without a flip alone run no recurrent kernel.  No batch is resident after a served call (the LSTM has
 *   no hook in rnnwf_vmc_gradient).  RNNWF_ERR_INVALID, before any work: every other model, by name, with the entry that serves it.
 *   rnnwf_pauli_step, _stack, _2d and _complex keep refusing the LSTM.  Timing ids: 0 = base pass with site terms, 1 = masked-tail
 *   pass, 2 = log-ratio assembly + sums.
 * rnnwf_lstm_pauli_gradient_step: rnnwf_lstm_vmc_gradient_step for the Hamiltonian sum_k coeff[k] (prod_sign sz)(prod_flip sx):
 *   one pass of rnnwf_pauli_step_lstm on numsamples drawn samples (same samples, E_loc, moments and term_sums, bit for bit), then
 *   the gradient with weights (E_s - moments[0] / moments[2]) * (1 / moments[2]) on the checkpoints that pass left on the device: no
 *   second base pass, one host synchronisation.  term_sums (nterms, 2), out_samples, out_eloc may be NULL.  Leaves the tensors where
 *   rnnwf_get_grad and rnnwf_get_grads_flat read them.  Refused before anything is touched (an earlier batch, the parameters and
 *   the gradient stay as they were): the refusals above; a handle with a communicator (single process only); RNNWF_ERR_NOMEM
 *   "... exceed the state budget of one pass; split the batch" for more samples than one pass holds.                           */
int rnnwf_pauli_step_lstm(rnnwf_handle* h, const int32_t* flip, const int32_t* sign, const double* coeff, int32_t nterms,
                          const int32_t* samples, int64_t ns, uint64_t seed, uint64_t step, int64_t sample_offset,
                          double* term_sums, double* out_eloc, double* moments, double* out_log_ratio, int32_t* out_samples);
int rnnwf_lstm_pauli_gradient_step(rnnwf_handle* h, const int32_t* flip, const int32_t* sign, const double* coeff, int32_t nterms,
                                   int64_t numsamples, uint64_t seed, uint64_t step, int64_t sample_offset, double* moments,
                                   double* term_sums, int32_t* out_samples, double* out_eloc);

/* rnnwf_renyi2_regions_lstm: rnnwf_renyi2_regions for the LSTM wave function (RNNWF_MODEL_LSTM1D_F64: one layer, 1..68 units, float64,
 * raster path; docs/renyi_lstm.md).  Arguments, layouts, outputs, the normalisation of the masks (site 0 not in A; an empty or full
 * region gives log r = 0 exactly at no cost), passes under RNNWF_STATE_BUDGET_MB, fixed-order sums and +inf on log r > 709 are
 * rnnwf_renyi2_regions's; masks are indexed by the chain position, the column of `samples` (raster index ny * Nx + nx).  With f >= 1
 * the first site of A, the mixed chain (the partner's spins on A, the chain's own elsewhere) restarts from the chain's own checkpoint
 * (h, c) of site f - 1 and recomputes the sites f..N-1: N - f cell evaluations per chain and region, counted in work[0].  A call
 * whose regions are all empty after normalisation (every call on a 1 x 1 lattice) runs no recurrent kernel.  No batch is resident
 * after a served call.  RNNWF_ERR_INVALID, before any work (a refused call touches nothing): every other model, by name, with the
 * region entry that serves it (rnnwf_renyi2_regions, _stack, _2d, _complex - which keep refusing the LSTM); the argument checks of
 * rnnwf_renyi2_regions.  RNNWF_ERR_STATE for uncommitted parameters.  Timing ids: 0 = base pass with site terms, 1 = paired
 * masked-tail pass, 2 = log-ratio assembly + sums.                                                                              */
int rnnwf_renyi2_regions_lstm(rnnwf_handle* h, const int32_t* regions, int32_t nregions, const int32_t* samples, int64_t npairs,
                              uint64_t seed, uint64_t step, int64_t pair_offset, double* sums, double* out_log_ratio,
                              int32_t* out_samples);

/* ---- device-resident Adam training of the LSTM wave function (RNNWF_MODEL_LSTM1D_F64; docs/lstm.md, "Device-resident training") ----
 * rnnwf_adam_step, rnnwf_train_steps, rnnwf_pauli_train_steps* and rnnwf_device_training_supported keep refusing an LSTM handle;
 * these two are its K iterations (1 <= K <= 1024) with ONE host synchronisation behind the last.  Both run, per iteration and
 * without a host visit, the kernels of the host loop's fused call, Adam in f64 on the device-resident flat parameters and the
 * re-pack of the forward image and of the backward operand from the recorded tables of their host packers: a trajectory equals the
 * host loop's (the fused call, the optimizer's arithmetic on the host, rnnwf_set_params_flat) bit for bit.
 * rnnwf_lstm_train_steps: rnnwf_train_steps's arguments and outputs; iteration k is rnnwf_lstm_vmc_gradient_step at step index
 *   step0 + k followed by the update with learning_rates[k].
 * rnnwf_lstm_pauli_train_steps: rnnwf_pauli_train_steps's arguments and outputs; iteration k is rnnwf_lstm_pauli_gradient_step.
 * Afterwards, as after rnnwf_train_steps: no batch is resident, rnnwf_get_param and rnnwf_commit_params see the device's
 * parameters, rnnwf_set_param / rnnwf_set_params_flat replace them, and Adam's moments and step count are read and set with
 * rnnwf_adam_get_state / rnnwf_adam_set_state (which serve an LSTM handle).  Refused before anything is touched: RNNWF_ERR_INVALID
 * for any other model ("needs an LSTM1D_F64 handle"), a handle with a communicator ("single process only"), K outside 1..1024, a
 * non-finite learning rate and the argument refusals of the entries they mirror; RNNWF_ERR_STATE for uncommitted parameters;
 * RNNWF_ERR_NOMEM "... exceed the state budget of one pass; split the batch".  An error inside the loop: the updates already
 * applied count in Adam's step count, and no batch or gradient is left.                                                          */
int rnnwf_lstm_train_steps(rnnwf_handle* h, int32_t K, int64_t numsamples, uint64_t seed, uint64_t step0, int64_t sample_offset,
                           const double* couplings, int64_t n_couplings, const double* learning_rates, double beta1, double beta2,
                           double epsilon, double* moments);
int rnnwf_lstm_pauli_train_steps(rnnwf_handle* h, const int32_t* flip, const int32_t* sign, const double* coeff, int32_t nterms,
                                 int32_t K, int64_t numsamples, uint64_t seed, uint64_t step0, int64_t sample_offset,
                                 const double* learning_rates, double beta1, double beta2, double epsilon, double* moments,
                                 double* term_sums, double* out_eloc);

/* ---- measurement ------------------------------------------------------------------------------
 * HIP-event timing of the kernels on the handle's stream (bench.py's roofline leg).
 * kernel ids: 0 = base pass (sample / teacher-forced + checkpoints), 1 = flip pass (dominant),
 *             2 = local-energy assembly + moments (rnnwf_renyi2_swap: 0 = base pass + site-term replay,
 *             1 = swap pass, 2 = log-ratio assembly + sums, and the same for rnnwf_renyi2_regions and
 *             rnnwf_renyi2_regions_2d (id 1 = its paired masked-tail pass); rnnwf_correlations: 0 = base pass + both-outcome replay, 1 = trunk +
 *             branch passes, 2 = log-ratio assembly + sums), 3 = back-propagation through time of rnnwf_vmc_gradient,
 *             4 = its weight-gradient GEMM.  total_ms / launches accumulate since the
 *             last rnnwf_timing_reset.  Stacked layers on the bf16x3 engine: id 1 brackets the whole
 *             pipeline of per-layer kernels as ONE launch.  work[] is the same for every id: work[0] =
 *             cell evaluations (all layers of a chain step count as one), work[1] = MFMA flops issued
 *             (padding included), both by the flip / swap pass (id 1) since the last reset.
 * rnnwf_timing_enable: on = 0 off, 1 all groups, 2 the dominant pass (id 1) only - two events per step instead of
 *             ten, which is what a throughput measurement wants beside its roofline figure.       */
int rnnwf_timing_enable(rnnwf_handle* h, int32_t on);
int rnnwf_timing_reset(rnnwf_handle* h);
int rnnwf_timing_get(rnnwf_handle* h, int32_t kernel_id, double* total_ms, int64_t* launches, double* work);
/* Which matrix engine the dominant (flip / swap) pass of this handle uses, decided at rnnwf_commit_params:
 *   "bf16x3"  - both operands held exactly as three bf16 parts, six bf16 MFMA products, f32 accumulate
 *               (f32 models up to 100 units; f32 accuracy, see csrc/split_core.h; above 68 units one weight part is read
 *               through L2; stacked layers of 37..50 units: one kernel per layer, csrc/split_kernels.h).  With one layer of
 *               37..52 units the base pass (sampling, log_probability) runs on the same engine (cooperative kernel);
 *   "f32mfma" - f32-input MFMA: forced with RNNWF_ENGINE=f32; above 100 units; stacked layers of other widths; batches too
 *               small to fill the chip with 32-chain tiles; every other base pass;
 *   "f64mfma" - the float64 models.                                                                     */
const char* rnnwf_engine_name(const rnnwf_handle* h);
/* hipDeviceSynchronize on the handle's device (bench.py brackets its timed region with it). */
int rnnwf_synchronize(rnnwf_handle* h);
/* Device properties for reports: cu_count, clock_mhz, hbm_bytes. */
int rnnwf_device_info(rnnwf_handle* h, int32_t* cu_count, int32_t* clock_mhz, int64_t* hbm_bytes, char* name64);

#ifdef __cplusplus
}
#endif
#endif /* RNNWF_H */
