// smooth.hpp -- the two steps of crsdr_doa that sit between its kernels: spatial smoothing / forward-backward averaging of the covariance
// (k_doa_cov_reduce -> here -> k_doa_subspace) and the source count from the singular values (k_doa_subspace -> here -> k_doa_scan).
//
// Smoothing.  URA of mx x my elements in the order iy * mx + ix, sub-arrays of sx x sy elements (ms = sx sy), P = (mx - sx + 1)(my - sy + 1) of
// them; sub-array (px, py) selects sel_p(iy * sx + ix) = (iy + py) * mx + ix + px.  For a <= b, in fp64 from the fp32 rxx, p running px
// fastest, then py:
//     acc[a][b] = sum_p rxx[sel_p(a)][sel_p(b)]
//     rs[a][b]  = acc[a][b] / P                                                without CRSDR_SMOOTH_FB
//     rs[a][b]  = (acc[a][b] + conj(acc[ms-1-a][ms-1-b])) / (2 P)              with it
// rounded once to fp32, rs[b][a] written as its conjugate.  Index reversal is the centro-symmetry of a URA in this element order: the
// backward image J conj(R) J of the covariance of steering vectors is again one of steering vectors (of conjugated ones alike, which is
// what the X^H X convention of k_covariance produces).
//
// Order.  M singular values sv (fp32, descending), N snapshots, in fp64:  lambda_i = max(sv[i], sv[0] 2^-40);  for k in [kmin, kmax],
// n = M - k:  T_k = n log((1/n) sum_{i >= k} lambda_i) - sum_{i >= k} log lambda_i;
//     MDL_k = N T_k + k (2M - k) log(N) / 2,     AIC_k = 2 N T_k + 2 k (2M - k);
// the estimate is the argmin, the smallest k on a tie; sv[0] = 0: kmin and all values 0.
//
// Each is one device function per matrix, called by the batched kernel (grid = estimates) and by the per-op one (one workgroup), so that
// both are the same instruction sequence per matrix -- as herm_subspace and pmusic2d_point are.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "music.hpp"

namespace crsdr {
namespace smooth {

constexpr int SM_THREADS = 256;
constexpr int MAX_M = music::MAX_M;
constexpr uint32_t FLAG_FB = 1u;            // CRSDR_SMOOTH_FB
constexpr int ORDER_MDL = 1, ORDER_AIC = 2; // CRSDR_ORDER_*

// acc[a][b] of the definition; sr = the raw covariance [m][m] (LDS), npx = mx - sx + 1, npy = my - sy + 1
__device__ __forceinline__ double2 smooth_acc(const float2 *sr, int m, int mx, int sx, int npx, int npy, int a, int b)
{
    const int ia = (a / sx) * mx + a % sx, ib = (b / sx) * mx + b % sx;      // sel_0
    double re = 0.0, im = 0.0;
    for (int py = 0; py < npy; ++py)
        for (int px = 0; px < npx; ++px) {
            const int o = py * mx + px;
            const float2 v = sr[(size_t)(ia + o) * m + ib + o];
            re += (double)v.x;
            im += (double)v.y;
        }
    return make_double2(re, im);
}

// One matrix, the whole workgroup (SM_THREADS threads) calling together: rxx [m][m] -> rs [ms][ms], both cf32 row-major, m = mx my <= 64.
__device__ __forceinline__ void smooth_covariance(const float2 *__restrict__ rxx, int mx, int my, int sx, int sy, uint32_t flags,
                                                  float2 *__restrict__ rs)
{
    __shared__ float2 sr[MAX_M * MAX_M];      // 32 KiB: every entry is read up to P times (2 P with FB)
    const int m = mx * my, ms = sx * sy, npx = mx - sx + 1, npy = my - sy + 1, tid = threadIdx.x;
    for (int i = tid; i < m * m; i += SM_THREADS) sr[i] = rxx[i];
    __syncthreads();
    const double div = (double)(npx * npy) * ((flags & FLAG_FB) ? 2.0 : 1.0);
    for (int i = tid; i < ms * ms; i += SM_THREADS) {
        const int a = i / ms, b = i - a * ms;
        if (a > b) continue;
        double2 acc = smooth_acc(sr, m, mx, sx, npx, npy, a, b);
        if (flags & FLAG_FB) {
            const double2 back = smooth_acc(sr, m, mx, sx, npx, npy, ms - 1 - a, ms - 1 - b);
            acc.x += back.x;
            acc.y -= back.y;
        }
        const float re = (float)(acc.x / div), im = (float)(acc.y / div);
        rs[(size_t)a * ms + b] = make_float2(re, im);
        if (a != b) rs[(size_t)b * ms + a] = make_float2(re, -im);
    }
}

// grid (nest): rxx [nest][m][m] -> rs [nest][ms][ms]
__global__ __launch_bounds__(SM_THREADS) void k_doa_smooth(const float2 *__restrict__ rxx, int mx, int my, int sx, int sy, uint32_t flags,
                                                           float2 *__restrict__ rs)
{
    const size_t e = blockIdx.x, mm = (size_t)(mx * my) * (mx * my), ss = (size_t)(sx * sy) * (sx * sy);
    smooth_covariance(rxx + e * mm, mx, my, sx, sy, flags, rs + e * ss);
}

__global__ __launch_bounds__(SM_THREADS) void k_smooth_covariance(const float2 *__restrict__ rxx, int mx, int my, int sx, int sy, uint32_t flags,
                                                                  float2 *__restrict__ rs)
{
    smooth_covariance(rxx, mx, my, sx, sy, flags, rs);
}

// One estimate, one wave (64 lanes) calling together: sv [M] -> *k_out, crit [kmax - kmin + 1].  1 <= kmin <= kmax < M <= 64.
__device__ __forceinline__ void source_order(const float *__restrict__ sv, int M, double N, int criterion, int kmin, int kmax,
                                             int32_t *__restrict__ k_out, float *__restrict__ crit)
{
    __shared__ double s_lam[MAX_M + 1], s_log[MAX_M + 1];      // suffix sums of lambda and of log lambda; [M] = 0
    const int lane = threadIdx.x;
    const double top = (double)sv[0];
    if (lane < M) {
        const double lam = fmax((double)sv[lane], top * 0x1p-40);
        s_lam[lane] = lam;
        s_log[lane] = log(lam);
    }
    __syncthreads();
    if (lane == 0) {      // once: at most 64 additions each, last value first
        double a = 0.0, b = 0.0;
        s_lam[M] = 0.0; s_log[M] = 0.0;
        for (int i = M - 1; i >= 0; --i) {
            a += s_lam[i]; b += s_log[i];
            s_lam[i] = a; s_log[i] = b;
        }
    }
    __syncthreads();
    const int k = kmin + lane;
    const bool live = k <= kmax;
    double v = 0.0;
    if (live && top > 0.0) {
        const double n = (double)(M - k), pen = (double)k * (double)(2 * M - k);
        const double T = n * log(s_lam[k] / n) - s_log[k];
        v = criterion == ORDER_AIC ? 2.0 * N * T + 2.0 * pen : N * T + 0.5 * pen * log(N);
    }
    if (live) crit[lane] = (float)v;
    // argmin over the live lanes, the smallest k on a tie (a NaN never wins: every comparison with it is false)
    double bv = live ? v : __longlong_as_double(0x7FF0000000000000ll);
    int bk = live ? k : 0x7FFFFFFF;
    if (bv != bv) { bv = __longlong_as_double(0x7FF0000000000000ll); bk = 0x7FFFFFFF; }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double ov = music::shfl_xor_f64(bv, off);
        const int ok = __shfl_xor(bk, off, 64);
        if (ov < bv || (ov == bv && ok < bk)) { bv = ov; bk = ok; }
    }
    if (lane == 0) *k_out = bk > kmax ? kmin : bk;
}

// grid (nest), one wave: sv [nest][M] -> k [nest], crit [nest][kmax - kmin + 1]
__global__ __launch_bounds__(64) void k_doa_order(const float *__restrict__ sv, int M, double N, int criterion, int kmin, int kmax,
                                                  int32_t *__restrict__ k, float *__restrict__ crit)
{
    const size_t e = blockIdx.x;
    source_order(sv + e * M, M, N, criterion, kmin, kmax, k + e, crit + e * (size_t)(kmax - kmin + 1));
}

} // namespace smooth
} // namespace crsdr
