// sr_solve_kernels.h - the ns x ns solve of stochastic reconfiguration on the device (docs/sr.md, "Solve on the device"):
//
//   (gram + ns lambda I) y = eps,   gram + ns lambda I = L L^T,   blocked right-looking Cholesky in f64, block width kSrNB = 32
//   (the blocks sr_gram_kernel produces), in the workspace F[ns + 1][ns]: rows < ns hold the blocks of L below the diagonal blocks,
//   row ns holds eps and is carried through the panel solve and the trailing update like any other row (the augmented form), so
//   that after the last panel it holds z = L^-1 eps.  The factors of the diagonal blocks go to Ld[nb][32][32] (rows past ns:
//   identity): every workgroup of a panel's launch loads the unfactorised diagonal block, so that launch cannot overwrite it.
//   The backward solve L^T y = z is one more blocked sweep, from the last panel to the first.
//
//   sr_centre_kernel       : out = in - mean(in) in a fixed order (eps from the local energies, y - mean y for J^T y); clears the
//                            pivot status word when given one.
//   sr_chol_panel_kernel   : panel k.  Every workgroup factorises the 32 x 32 diagonal block in LDS in plain f64 arithmetic (the same
//                            instructions on the same data: the same bits in every workgroup; the shift is added as the block is
//                            loaded), then solves its block of 32 rows below it against L_kk^T, one lane per row.
//   sr_chol_update_kernel  : A_ij -= L_ik L_jk^T for the blocks k < j <= i of the lower triangle and of the eps row, one workgroup
//                            per block, one 16 x 16 tile of v_mfma_f64_16x16x4_f64 per wave.
//   sr_chol_back_kernel    : panel k of the backward sweep.  Every workgroup solves y_k = L_kk^-T z_k (again the same bits), workgroup
//                            j < k then takes z_j -= L_kj^T y_k and workgroup k stores y_k.
//   Panel 0 reads the Gram matrix itself (`src`), every later panel the workspace: the Gram matrix is never written.
//   Block row nb = ceil(ns / 32) is the eps row: one valid row, stored behind the matrix.
// Every sum has a fixed order (no atomics).  A pivot that is not positive and finite is recorded (the first one, its index + 1) and
// replaced by 1: nothing later takes the root of or divides by it, and no result is ever an address or a loop bound.
#pragma once
#include "device.h"

namespace rnnwf {

constexpr int kSrNB = 32;

// out[s] = (in[s] - in[0]) - mean_s (in[s] - in[0]): a constant vector gives exact zeros.  One workgroup of 256 threads: thread t adds
// the elements t, t + 256, ... in order, then a fixed tree over the 256 partial sums.
__global__ void __launch_bounds__(256) sr_centre_kernel(const double* __restrict__ in, int64_t n, double* __restrict__ out,
                                                        long long* __restrict__ status) {
    __shared__ double part[256];
    const int t = threadIdx.x;
    const double ref = in[0];
    double v = 0.0;
    for (int64_t s = t; s < n; s += 256) v += in[s] - ref;
    part[t] = v;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (t < w) part[t] += part[t + w];
        __syncthreads();
    }
    const double mean = part[0] / (double)n;
    for (int64_t s = t; s < n; s += 256) out[s] = (in[s] - ref) - mean;
    if (status && t == 0) *status = 0;
}

// The complex RNN's stacked eps (docs/sr_complex.md): workgroup b = 0 / 1 takes the real / imaginary parts of the ns resident
// float2 local energies and writes out[b ns + s], centred with that half's own mean in the order and the arithmetic of
// sr_centre_kernel (reference element subtracted first: a constant E_loc gives exact zeros); workgroup 0 clears the status word.
__global__ void __launch_bounds__(256) sr_centre_complex_kernel(const float2* __restrict__ in, int64_t ns, double* __restrict__ out,
                                                                long long* __restrict__ status) {
    __shared__ double part[256];
    const int t = threadIdx.x;
    const bool im = blockIdx.x != 0;
    auto at = [&](int64_t s) { return (double)(im ? in[s].y : in[s].x); };
    const double ref = at(0);
    double v = 0.0;
    for (int64_t s = t; s < ns; s += 256) v += at(s) - ref;
    part[t] = v;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (t < w) part[t] += part[t + w];
        __syncthreads();
    }
    const double mean = part[0] / (double)ns;
    for (int64_t s = t; s < ns; s += 256) out[(im ? ns : 0) + s] = (at(s) - ref) - mean;
    if (status && t == 0 && !im) *status = 0;
}

// the 32 x 32 diagonal block of panel k, shifted, into LDS (rows past ns: identity) and its Cholesky factor in place (lower triangle)
__device__ __forceinline__ void sr_factor_diagonal(const double* src, int64_t ns, int64_t c0, double shift, bool record,
                                                   long long* __restrict__ status, double (*Ls)[kSrNB + 1]) {
    const int t = threadIdx.x;
    for (int e = t; e < kSrNB * kSrNB; e += 256) {
        const int r = e >> 5, c = e & 31;
        const bool ok = c0 + r < ns && c <= r;
        const double v = ok ? src[(c0 + r) * ns + c0 + c] : 0.0;
        Ls[r][c] = r == c ? (ok ? v + shift : 1.0) : v;
    }
    const int r = t >> 3;
    for (int j = 0; j < kSrNB; ++j) {
        __syncthreads();
        double d = Ls[j][j];
        const bool good = d > 0.0 && d < __builtin_inf();      // false for a NaN too
        if (!good) {
            if (record && t == 0 && *status == 0) *status = (long long)(c0 + j) + 1;
            d = 1.0;
        }
        const double root = sqrt(d);
        __syncthreads();
        if (t < kSrNB && t >= j) Ls[t][j] = t == j ? root : Ls[t][j] / root;
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int c = (t & 7) + 8 * q;
            if (c > j && c <= r) Ls[r][c] -= Ls[r][j] * Ls[c][j];
        }
    }
    __syncthreads();
}

// Items: the block rows k + 1 .. nb below the diagonal block (nb: the eps row).  X L_kk^T = B by forward substitution along the row.
__global__ void __launch_bounds__(256) sr_chol_panel_kernel(const double* src, double* F, int64_t ns, int k,
                                                            double shift, double* __restrict__ Ld, long long* __restrict__ status) {
    __shared__ double Ls[kSrNB][kSrNB + 1];
    __shared__ double Bs[kSrNB][kSrNB + 1];
    const int t = threadIdx.x;
    const int nb = (int)((ns + kSrNB - 1) / kSrNB);
    const int64_t c0 = (int64_t)kSrNB * k;
    const double* zsrc = F + ns * ns;                           // the eps row lives in the workspace from the start
    sr_factor_diagonal(src, ns, c0, shift, blockIdx.x == 0, status, Ls);
    if (blockIdx.x == 0)                                        // not in place: the other workgroups of this launch still load the block
        for (int e = t; e < kSrNB * kSrNB; e += 256) Ld[(int64_t)k * kSrNB * kSrNB + e] = Ls[e >> 5][e & 31];
    for (int i = k + 1 + blockIdx.x; i <= nb; i += gridDim.x) {
        for (int e = t; e < kSrNB * kSrNB; e += 256) {
            const int r = e >> 5, c = e & 31;
            const int64_t gr = (int64_t)kSrNB * i + r;
            const bool ok = (i < nb ? gr < ns : r == 0) && c0 + c < ns;
            Bs[r][c] = ok ? (i < nb ? src[gr * ns + c0 + c] : zsrc[c0 + c]) : 0.0;
        }
        __syncthreads();
        if (t < kSrNB) {
            double x[kSrNB];
#pragma unroll
            for (int c = 0; c < kSrNB; ++c) {
                double v = Bs[t][c];
#pragma unroll
                for (int j = 0; j < c; ++j) v -= x[j] * Ls[c][j];
                x[c] = v / Ls[c][c];
            }
#pragma unroll
            for (int c = 0; c < kSrNB; ++c) Bs[t][c] = x[c];
        }
        __syncthreads();
        for (int e = t; e < kSrNB * kSrNB; e += 256) {
            const int r = e >> 5, c = e & 31;
            const int64_t gr = (int64_t)kSrNB * i + r;
            const bool ok = (i < nb ? gr < ns : r == 0) && c0 + c < ns;
            if (ok) F[(i < nb ? gr : ns) * ns + c0 + c] = Bs[r][c];
        }
        __syncthreads();
    }
}

// Items: with m = nb - k - 1 block columns behind panel k, the m (m + 1) / 2 blocks (i, j), k < j <= i < nb, row by row, then the m
// blocks of the eps row.  Wave w owns the 16 x 16 tile (w >> 1, w & 1); a lane loads eight consecutive elements of its row of either
// panel block, element q is k-step q for both operands (the order of the sum over k is the same for every element of the block).
__global__ void __launch_bounds__(256) sr_chol_update_kernel(const double* src, double* F, int64_t ns, int k,
                                                             int64_t nitems) {
    typedef double V4 __attribute__((ext_vector_type(4)));
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int li = lane & 15, lk = lane >> 4;
    const int x = wave >> 1, y = wave & 1;
    const int nb = (int)((ns + kSrNB - 1) / kSrNB);
    const int m = nb - k - 1;
    const int64_t tri = (int64_t)m * (m + 1) / 2;
    const int64_t c0 = (int64_t)kSrNB * k;
    for (int64_t item = blockIdx.x; item < nitems; item += gridDim.x) {
        int ii = m, jj = (int)(item - tri);
        if (item < tri) {
            ii = 0;
            while ((int64_t)(ii + 1) * (ii + 2) / 2 <= item) ++ii;
            jj = (int)(item - (int64_t)ii * (ii + 1) / 2);
        }
        const int i = k + 1 + ii, j = k + 1 + jj;
        const bool epsrow = i == nb;
        // operand rows: A from block row i of panel k, B from block row j (always a matrix row block)
        const int64_t ra = (int64_t)kSrNB * i + 16 * x + li, rb = (int64_t)kSrNB * j + 16 * y + li;
        const bool aok = epsrow ? 16 * x + li == 0 : ra < ns;
        const bool bok = rb < ns;
        const double* ap = F + (epsrow ? ns : (aok ? ra : 0)) * ns + c0 + 8 * lk;       // rows past ns are read from row 0 and zeroed
        const double* bp = F + (bok ? rb : 0) * ns + c0 + 8 * lk;
        double av[8], bv[8];                                   // an update follows full panels only: the eight columns exist
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            av[q] = aok ? ap[q] : 0.0;
            bv[q] = bok ? bp[q] : 0.0;
        }
        V4 acc = V4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int q = 0; q < 8; ++q) acc = Frag<double>::mfma(av[q], bv[q], acc);
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const int lr = 16 * x + lk + 4 * rr;                  // f64 C/D fragment: row lk + 4 rr, column li
            const int64_t r = (int64_t)kSrNB * i + lr, c = (int64_t)kSrNB * j + 16 * y + li;
            const bool ok = c < ns && (epsrow ? lr == 0 : (r < ns && c <= r));
            if (ok) {
                const int64_t at = (epsrow ? ns : r) * ns + c;
                const double old = epsrow ? F[at] : src[at];
                F[at] = old - acc[rr];
            }
        }
    }
}

// Panel k of L^T y = z, from k = nb - 1 down to 0: workgroups 0 .. k of 64 threads.  y_k by column-oriented back substitution in wave 0
// (lane c owns z_c); workgroup j < k: z_j[c] -= sum_r L[32 k + r][32 j + c] y_k[r], r ascending; workgroup k stores y_k.
__global__ void __launch_bounds__(64) sr_chol_back_kernel(double* F, const double* __restrict__ Ld, int64_t ns, int k, double* __restrict__ y) {
    __shared__ double Ls[kSrNB][kSrNB + 1];
    __shared__ double ys[kSrNB];
    const int t = threadIdx.x;
    const int64_t c0 = (int64_t)kSrNB * k;
    double* z = F + ns * ns;
    for (int e = t; e < kSrNB * kSrNB; e += 64) Ls[e >> 5][e & 31] = Ld[(int64_t)k * kSrNB * kSrNB + e];
    double zr = t < kSrNB && c0 + t < ns ? z[c0 + t] : 0.0;
    __syncthreads();
    for (int c = kSrNB - 1; c >= 0; --c) {
        const double yc = __shfl(zr, c) / Ls[c][c];
        if (t == c) zr = yc;
        else if (t < c) zr -= Ls[c][t] * yc;
    }
    if (t < kSrNB) ys[t] = zr;
    __syncthreads();
    for (int j = blockIdx.x; j <= k; j += gridDim.x) {
        if (t >= kSrNB) continue;
        if (j == k) {
            if (c0 + t < ns) y[c0 + t] = ys[t];
            continue;
        }
        const int64_t c = (int64_t)kSrNB * j + t;              // j < k: a full block of columns
        double v = z[c];
        for (int r = 0; r < kSrNB && c0 + r < ns; ++r) v -= F[(c0 + r) * ns + c] * ys[r];
        z[c] = v;
    }
}

}  // namespace rnnwf
