// models.h - host-side entry points of each wave-function family (one .hip translation unit each) and
// the helpers they share (implemented in rnnwf_api.hip).
#pragma once
#include <vector>

#include "handle.h"

namespace rnnwf {

// ---- shared helpers (rnnwf_api.hip) --------------------------------------------------------------
int upload_samples(rnnwf_handle* h, const int32_t* samples, int64_t B);
int pack_device(rnnwf_handle* h, int64_t B, DevBuf& bits, int reverse, const int32_t* col_of_pos_dev);
int unpack_device(rnnwf_handle* h, const DevBuf& bits, int64_t B, const int32_t* pos_of_col_dev);
int upload_and_pack(rnnwf_handle* h, const int32_t* samples, int64_t B, DevBuf& bits, int reverse,
                    const int32_t* col_of_pos_dev);
int unpack_and_download(rnnwf_handle* h, const DevBuf& bits, int64_t B, int32_t* out, const int32_t* pos_of_col_dev);
int run_moments(rnnwf_handle* h, const void* eloc_dev, int64_t ns, bool complex_f32, double* moments_host);
int run_tfim_eloc(rnnwf_handle* h, const uint32_t* bits, const double* lpq, int64_t ns, int Nx, int Ny,
                  const int32_t* pos_of_site_dev, const double* Jz_dev, double Bx, double* eloc_dev);
int run_parity_combine(rnnwf_handle* h, const double* a, const double* b, int64_t n, double* out);
int run_parity_share(rnnwf_handle* h, double* lpF, double* lpR, int64_t n);      // in place: P_F / (P_F + P_R), P_R / (P_F + P_R)

// ---- one table per wave-function family -------------------------------------------------------------
// What the families' host code does differently.  The public compute entry points (rnnwf_api.hip) run one driver
// against it: chunk loop, copies back to the host, budget refusals and the resident-batch rule live there.
struct Draw { uint64_t seed, step; int64_t offset; };     // where an entry point takes a Draw, nullptr = teacher-forced
                                                          // on the spins the driver packed into h->bits
struct Gradient;
struct Family {
    const char* name;
    int (*pack_image)(rnnwf_handle* h, std::vector<char>& img);
    // the table of that image over Lin into the active PackTrace, from the same row of the family's shape table (shapes.h): what
    // device-resident training replays (train.hip); nullptr for a family without a gradient
    int (*pack_table)(rnnwf_handle* h);
    // base pass alone: log P of ns chains -> h->out_lp (spins drawn into h->bits when `draw`)
    int (*base)(rnnwf_handle* h, int64_t ns, const Draw* draw);
    // parity model: h->out_lp <- log P symmetrised over the reversed chains of the spins in h->samples_i32; nullptr for the others
    int (*symmetrise)(rnnwf_handle* h, int64_t ns);
    // checkpointed base pass -> flip / swap pass -> assembly: E_loc -> h->eloc (TFIM also the log-prob queue -> h->lpq).
    // couplings: the caller's whole vector; its per-site part is already on the device (h->coupl)
    int (*energy)(rnnwf_handle* h, int64_t ns, const Draw* draw, const double* couplings);
    int64_t (*max_chains_per_pass)(rnnwf_handle* h);
    // site order of the packed bits when it is not the caller's (MDRNN: the snake path); nullptr: the same
    int (*site_maps)(rnnwf_handle* h, const int32_t** col_of_pos, const int32_t** pos_of_site);
    void (*after_sync)(rnnwf_handle* h, int64_t ns);    // reads what the kernels left in pinned memory (cRNN: work totals); may be nullptr
    int coupl_per_site;        // couplings per site held on the device (TFIM: Jz; J1-J2: J1, J2, Bz) ...
    int coupl_tail;            // ... followed by this many scalars read on the host (TFIM: Bx; J1-J2: periodic, marshall)
    bool complex_eloc;         // complex64 E_loc (else float64)
    bool base_keeps_states;    // the base pass alone needs the state budget: log_prob runs in passes, sample refuses past it
    // the VMC-cost gradient; nullptr: none, and rnnwf_vmc_step leaves no batch resident for it
    const Gradient* gradient;
};

// ---- the VMC-cost gradient: one hook table per family that has one (grad.hip: the GRUs, mdrnn.hip: the 2D RNN) ---------------
// The driver (grad_device, grad.hip) checks the resident batch, scales the cost, packs and uploads the backward image when it is
// stale, allocates and clears h->gradW and calls `launch`.  rnnwf_vmc_gradient downloads the result and calls `unpack`; device
// training (train.hip) reads it on the device through a table probed from `unpack` (grad_flat_probe).
struct GradImage {
    bool f64;          // element type of h->gradW (else float)
    size_t count;      // elements of the result: the dW images and the head rows
    size_t alloc;      // elements allocated and cleared: count, plus the stacked GRU's scratch head row for its layer-0 pass
};
// w_s = (E_s - mean) * inv_norm; mom != nullptr: mean and norm are read from the step's moments on the device (GradArgs::mom)
struct GradCost { double mean_e, mean_im, inv_norm; const double* mom; };
struct Gradient {
    int (*layout)(rnnwf_handle* h, GradImage* out);
    // the backward image: img != nullptr: packed as doubles for upload; nullptr: its table over Lin into the active PackTrace
    int (*pack)(rnnwf_handle* h, std::vector<char>* img);
    // the backward kernels on the resident batch (h->bits, h->hck, h->eloc), adding into the cleared h->gradW
    int (*launch)(rnnwf_handle* h, const GradCost& cost);
    // a host copy of the h->gradW image -> h->grads
    void (*unpack)(rnnwf_handle* h, const void* img);
};
// the tables are static locals of host functions: hipcc would emit a namespace-scope const table for the device as well
const Family* gru_family();     // prnn.hip: GRU1D, GRU1D_PARITY, GRU1D_F64
const Family* crnn_family();    // crnn.hip: CRNN_U1
const Family* mdrnn_family();   // mdrnn.hip: MDRNN2D
const Family* lstm_family();    // lstm.hip: LSTM1D_F64
const Gradient* gru_gradient();   // grad.hip: the GRU hooks of gru_family and crnn_family (mdrnn.hip keeps the 2D RNN's)

// the fused VMC step behind rnnwf_vmc_step and rnnwf_train_steps (rnnwf_api.hip); out_samples, out_eloc, moments may be nullptr
int vmc_step(rnnwf_handle* h, int64_t ns, const Draw& draw, const double* couplings, int32_t* out_samples, void* out_eloc,
             double* moments);
// RNNWF_ERR_NOMEM "<what>: ... exceed the state budget of one pass" where vmc_step would refuse ns samples (rnnwf_api.hip)
int refuse_past_budget(rnnwf_handle* h, int64_t ns, const char* what);
// the batch just computed stays on the device (h->bits, h->hck, h->eloc) for rnnwf_vmc_gradient (rnnwf_api.hip): h->last_ns and
// h->sr_valid change together.  ns = 0: no batch is resident
void keep_resident(rnnwf_handle* h, int64_t ns);
// the name of an rnnwf_model value, for the refusals
inline const char* model_name(int model) {
    static const char* const names[] = {"GRU1D", "GRU1D_PARITY", "CRNN_U1", "GRU1D_F64", "MDRNN2D", "LSTM1D_F64"};
    return model >= 0 && model < (int)(sizeof names / sizeof *names) ? names[model] : "unknown";
}
// RNNWF_ERR_INVALID ("<what>: no gradient for the ...") for a family without one
int require_gradient(rnnwf_handle* h, const char* what);
// the gradient driver (grad.hip): result left in h->gradW, its layout in *im (may be nullptr).  mom_dev != nullptr (device
// training): mean energy and norm come from the step's moments on the device and the three doubles are unused
int grad_device(rnnwf_handle* h, double mean_energy, double mean_energy_im, double norm, const double* mom_dev, GradImage* im);
// sidx[i] = +-(1 + the h->gradW element flat parameter i is read from), 0: none (order of rnnwf_set_params_flat)
int grad_flat_probe(rnnwf_handle* h, std::vector<int32_t>& sidx, GradImage* im);

// complex RNN only (crnn.hip): amplitudes and J1-J2 local energies on caller-supplied samples
int crnn_log_amp(rnnwf_handle* h, const int32_t* samples, int64_t B, float* out_re_im, double* out_logp);
int crnn_j1j2_eloc(rnnwf_handle* h, const int32_t* samples, int64_t ns, const double* J1, const double* J2,
                   const double* Bz, int periodic, int marshall, float* eloc, int64_t* ncon);

// ---- bf16x3 engine (split.hip; compiled without SLP packing) -----------------------------------------
struct PrnnArgs;
struct CrnnArgs;
int prnn_split_flip(rnnwf_handle* h, const PrnnArgs& a);
double prnn_split_flops_per_step(rnnwf_handle* h);      // MFMA flops issued per 32-chain wave-step
int prnn_split_pack(rnnwf_handle* h, std::vector<char>& simg, std::vector<char>& simg_g);   // simg_g: the g-state form (pack_split.h), empty: none at this width
// split_stream.hip: the same pass at 53..100 units (the riders form; above 68 units the w3 fragments are read through L2)
int prnn_split_flip_stream(rnnwf_handle* h, const PrnnArgs& a, int kt16);
double prnn_split_stream_flops_per_step(rnnwf_handle* h);
int prnn_split_stream_pack(rnnwf_handle* h, std::vector<char>& simg);
int prnn_teacher_base(rnnwf_handle* h, int64_t ns, bool reversed, double* out_lp);   // prnn.hip
// prnn.hip, for the observable passes (observable.h): the base pass on the one-wave kernel only; its arguments; checkpoint bytes per 16 chains
int prnn_plain_base(rnnwf_handle* h, const PrnnArgs& a);
int prnn_stack_base(rnnwf_handle* h, const PrnnArgs& a);      // stacked layers (pauli_stack.hip): the one-wave MFMA stack kernel only
PrnnArgs prnn_base_args(rnnwf_handle* h, int64_t ns);
size_t prnn_hck_bytes_per_block(rnnwf_handle* h);
// lstm.hip, for the LSTM's gradient (lstm_grad.hip): teacher-forced base pass on h->bits that leaves the checkpoints in h->hck
int lstm_teacher_base(rnnwf_handle* h, int64_t ns);
// lstm_grad.hip, for the fused Pauli gradient step (lstm_pauli.hip): the LSTM's backward pass on the batch in h->bits / h->hck, weights
// from w_dev or (nullptr) from h->eloc and h->moments, the result queued into h->staging; after the caller's synchronisation
// lstm_grad_finish leaves the TF-named tensors in h->grads
// download = false (device-resident training): the result stays in h->gradW and nothing is queued into h->staging
int lstm_grad_queue(rnnwf_handle* h, const char* what, int64_t ns, const double* w_dev, bool download = true);
void lstm_grad_finish(rnnwf_handle* h);
// for the LSTM's builder of device-resident training (train.hip: train_prepare_lstm): the tables of h->wimg (lstm.hip) and of the
// backward operand h->wbwd (lstm_grad.hip) over Lin into the active PackTrace; the operand packed on the host when stale; and
// grad_flat_probe's table from the LSTM's own unpacker, *count the elements of its h->gradW image
int lstm_pack_table(rnnwf_handle* h);
int lstm_bwd_pack_table(rnnwf_handle* h);
int lstm_bwd_image(rnnwf_handle* h, const char* what);
int lstm_grad_flat_probe(rnnwf_handle* h, std::vector<int32_t>& sidx, size_t* count);
// lstm_grad.hip, for stochastic reconfiguration (sr.hip): lstm_bwd_kernel's unit-weight mode over the resident batch - the rows of P
// and Q into h->gradP / h->gradQ, every chain's head row into head_rows [ns][HEAD_ROW]
int lstm_sr_backward(rnnwf_handle* h, double* head_rows);
// crnn.hip, for the complex RNN's Pauli pass (crnn_pauli.hip): the same three for the one-layer complex RNN
int crnn_plain_base(rnnwf_handle* h, const CrnnArgs& a);
CrnnArgs crnn_base_args(rnnwf_handle* h, int64_t ns);
size_t crnn_hck_bytes_per_block(rnnwf_handle* h);
// split_stream.hip: the complex RNN's swap pass at 53..100 units
int crnn_split_swap_stream(rnnwf_handle* h, const CrnnArgs& a, int64_t max_tiles, int kt16);
double crnn_split_stream_flops_per_step(rnnwf_handle* h);
int crnn_split_stream_pack(rnnwf_handle* h, std::vector<char>& simg);
// stacked layers on the bf16x3 engine (split.hip; 37..50 units, ping-pong form): one kernel per layer over the same tiles, the new
// state of every step handed upward through h->xrec (split_core.h: SplitUpperLayout)
bool stack_split_available(const rnnwf_handle* h);
size_t stack_record_bytes_per_32_chains(const rnnwf_handle* h, int64_t steps);   // h->xrec bytes per 32-chain tile column with `steps` wave-steps
template <int NOUT> int stack_pack(rnnwf_handle* h);       // the layers' images; NOUT head rows: 1 (positive RNN), 3 (complex RNN)
int prnn_stack_flip(rnnwf_handle* h, const PrnnArgs& a);
int crnn_stack_swap(rnnwf_handle* h, const CrnnArgs& a, int64_t max_tiles, int64_t max_records);
double stack_split_flops_per_step(rnnwf_handle* h);
int crnn_split_swap(rnnwf_handle* h, const CrnnArgs& a, int64_t max_tiles);
double crnn_split_flops_per_step(rnnwf_handle* h);
int crnn_split_pack(rnnwf_handle* h, std::vector<char>& simg);
// cooperative base pass on the bf16 matrix core (gru_kernels.h: coop_base_pass_bf; f32 models, one layer, num_units <= 52):
// base_bf_available: this handle has the image (h->wbasebf); *_base_coop_bf: the launches; base_bf_pack: at commit
bool base_bf_available(const rnnwf_handle* h);
int base_bf_pack(rnnwf_handle* h);
int prnn_base_coop_bf(rnnwf_handle* h, const PrnnArgs& a);
int crnn_base_coop_bf(rnnwf_handle* h, const CrnnArgs& a);
// device-resident training (train.hip): the tables of the engine's images over Lin into the active PackTrace, from the rows of
// shapes.h their host packers take - h->wsplit of one layer; of a stack, layer 0 -> h->wsplit, l >= 1 -> h->wsplit_up[l - 1]; h->wbasebf
int split_pack_table(rnnwf_handle* h);
bool prnn_split_gstate_layout(const rnnwf_handle* h, int32_t* layout10);   // the ten fields of pack_split.h: GstateLayout; false: no g-state image at this width
bool prnn_split_gstate_range(const rnnwf_handle* h, const std::vector<char>& simg, const std::vector<char>& simg_g, double* bound, uint32_t* word);   // host: pack_split.h's gstate_range of the h image, the range word as the g image holds it
int split_gstate_refold(rnnwf_handle* h);      // behind a re-pack of h->wsplit: h->wsplit_g from it, on the stream (no-op without that image)
int stack_pack_table(rnnwf_handle* h, int layer);
int base_bf_pack_table(rnnwf_handle* h);

// ---- gradient (grad.hip) ---------------------------------------------------------------------------
// grad_wide.hip: the backward kernels of the wide one-layer shapes, compiled in their own translation unit - the rows of the GRU
// families' tables (shapes.h) that kGradWide picks: f32 from NFULL = 8 (101 units), f64 at NFULL = 6 (69..100 units).  Every
// gradient kernel of the GRUs runs kGradWaves waves per workgroup, whatever the forward kernels of its row run
struct GradArgs;
using GradKernel = void (*)(GradArgs);
constexpr int kGradWaves = 4;
template <typename T, int NFULL> constexpr bool kGradWide = sizeof(T) == 4 ? NFULL >= 8 : NFULL == 6;
GradKernel grad_wide_kernel(const rnnwf_handle* h);     // nullptr for another shape
int grad_bwd_image(rnnwf_handle* h);                    // grad.hip: the backward image, re-packed when stale
// mdrnn.hip, for stochastic reconfiguration (sr.hip): the 2D RNN's backward pass over the resident batch with unit weights - the rows
// of P and Q as the gradient leaves them (h->gradP, h->gradQ), every chain's two head rows into head_rows [ns][2][HEAD_ROW]
int mdrnn_sr_backward(rnnwf_handle* h, double* head_rows);
// ---- device-resident training (train.hip) ------------------------------------------------------------
void train_params_changed_on_host(rnnwf_handle* h);           // rnnwf_set_param / rnnwf_commit_params: the device copy is stale
int train_sync_params_to_host(rnnwf_handle* h);               // before the host reads its copy (rnnwf_get_param, checkpoints)
int train_allreduce_grads_device(rnnwf_handle* h);           // 1: gradient all-reduced in-stream on the device, 0: not available
// for rnnwf_sr_train_steps (sr.hip), whose iterations update the same flat parameters and re-pack the same images:
int train_prepare(rnnwf_handle* h);                          // the tables built and the flat parameters current on the device
// the same for an LSTM1D_F64 handle, through a builder of its own (the LSTM has no hook table: train_prepare keeps refusing it), for
// rnnwf_lstm_train_steps (lstm_grad.hip) and rnnwf_lstm_pauli_train_steps (lstm_pauli.hip)
int train_prepare_lstm(rnnwf_handle* h);
// theta_i <- round_T(theta_i - lr (+-col[|gidx_i| - 1])) unless *hold != 0 (both on the device), then the re-pack of every image
int train_apply_direction(rnnwf_handle* h, const double* col, size_t col_count, double lr, const long long* hold);
// for the Adam iterations of another local energy (pauli_driver.h: pauli_train_steps), behind train_prepare: the rows of the pinned
// moments table, iteration k's update as rnnwf_train_steps queues it, and the state that entry leaves after its one synchronisation
constexpr int kTrainMaxSteps = 1024;                         // iterations of one call: the rows of the pinned moments table
double* train_moments_row(rnnwf_handle* h, int k);           // device address of row k, for h->moments_direct
int train_adam_update(rnnwf_handle* h, int k, double lr, double beta1, double beta2, double epsilon);
void train_steps_done(rnnwf_handle* h, int K, double* moments);
// an error inside the LSTM entries' loop, behind their synchronisation: the `applied` updates count in Adam's bias correction and no
// batch or gradient is left claiming to belong to the new weights
void train_steps_failed(rnnwf_handle* h, int applied);
void grad_invalidate(rnnwf_handle* h);
// bytes of per-site hidden states one pass may hold; RNNWF_STATE_BUDGET_MB (read at rnnwf_create) overrides the
// default (tests use it to drive the multi-pass path at small sizes)
size_t state_budget_bytes(const rnnwf_handle* h, size_t dflt);
// RCCL sum of device-resident doubles on the handle's stream (comm.hip); no-op without a communicator
int comm_allreduce_device(rnnwf_handle* h, void* dev, size_t count);
// h->coupl <- n doubles; skipped when they are what the device already holds
int upload_couplings(rnnwf_handle* h, const double* src, size_t n);

}  // namespace rnnwf

extern "C" int rnnwf_comm_destroy(rnnwf_handle* h);
