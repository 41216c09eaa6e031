// augment.hpp -- co-array augmentation of the covariance, the step of crsdr_doa that takes smoothing's place between its kernels
// (k_doa_cov_reduce -> here -> k_doa_subspace) for arrays with absent receivers: thinned on purpose, or with dead ones.
//
// Physical array mx x my, element i = iy * mx + ix, m = mx my <= 64; bit i of `mask` set: element i is present (the host resolves "0 = all"
// before the launch).  Virtual array vx x vy, 1 <= vx <= mx, 1 <= vy <= my, mv = vx vy >= 2, element j = jy * vx + jx.  A lag u = (ux, uy)
// of the half-plane has uy > 0, or uy == 0 and ux >= 0, with |ux| < vx and uy < vy: vx + (vy - 1)(2 vx - 1) of them, at most 113 for
// mv <= 64.  P(u) = the pairs (p, q) of present elements with (ix_q - ix_p, iy_q - iy_p) = u, by ascending p (q is then determined and
// q >= p: only the upper triangle of rxx is read), c(u) = |P(u)| >= 1 (the host refuses a mask that leaves a lag uncovered).  In fp64
// from the fp32 rxx, in that order:
//     r(u)     = (1 / c(u)) sum_{(p, q) in P(u)} rxx[p][q]
//     ra[a][b] = r(pos_b - pos_a)          for a <= b
// rounded once to fp32, the diagonal's imaginary part exactly 0, ra[b][a] written as the conjugate.  Rows and columns of absent elements
// are never read in the arithmetic: they may hold anything.
//
// One device function per matrix, called by the batched kernel (grid = matrices) and by the per-op one (one workgroup), so that both are
// the same instruction sequence per matrix -- as smooth_covariance is.  Mapping: stage 1 is one thread per lag (its whole fp64 sum, so
// the order is pinned by a plain loop), stage 2 every thread on the mv^2 entries.  At most 64 fp64 additions per thread and 113 threads
// at work: nothing against the subspace kernel behind it, so nothing here is tuned.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "music.hpp"

namespace crsdr {
namespace augment {

constexpr int AG_THREADS = 256;
constexpr int MAX_M = music::MAX_M;
constexpr int MAX_LAGS = 128;               // >= vx + (vy - 1)(2 vx - 1) for every vx vy <= 64 (113 at 8 x 8)

// half-plane lags of a vx x vy array, and the index of (ux, uy) among them: row uy = 0 holds ux = 0 .. vx - 1, every row behind it
// ux = -(vx - 1) .. vx - 1
__host__ __device__ __forceinline__ int lag_count(int vx, int vy) { return vx + (vy - 1) * (2 * vx - 1); }
__host__ __device__ __forceinline__ int lag_index(int vx, int ux, int uy) { return uy == 0 ? ux : vx + (uy - 1) * (2 * vx - 1) + ux + vx - 1; }

// One matrix, the whole workgroup (AG_THREADS threads) calling together: rxx [m][m] -> ra [mv][mv], both cf32 row-major.
__device__ __forceinline__ void augment_covariance(const float2 *__restrict__ rxx, int mx, int my, int vx, int vy, uint64_t mask,
                                                   float2 *__restrict__ ra)
{
    __shared__ float2 sr[MAX_M * MAX_M];      // 32 KiB: an entry is read once, but by whichever thread owns its lag
    __shared__ double2 lag[MAX_LAGS];         // r(u)
    const int m = mx * my, mv = vx * vy, nlags = lag_count(vx, vy), tid = threadIdx.x;
    for (int i = tid; i < m * m; i += AG_THREADS) sr[i] = rxx[i];
    __syncthreads();
    if (tid < nlags) {
        int ux = tid, uy = 0;
        if (tid >= vx) {
            const int t = tid - vx, w = 2 * vx - 1;
            uy = 1 + t / w;
            ux = t - (uy - 1) * w - (vx - 1);
        }
        double re = 0.0, im = 0.0;
        int c = 0;
        for (int p = 0; p < m; ++p) {
            const int ixq = p % mx + ux, iyq = p / mx + uy;
            if (ixq < 0 || ixq >= mx || iyq >= my) continue;
            const int q = iyq * mx + ixq;
            if (!((mask >> p) & 1u) || !((mask >> q) & 1u)) continue;
            const float2 v = sr[p * m + q];
            re += (double)v.x;
            im += (double)v.y;
            ++c;
        }
        const double div = (double)(c > 0 ? c : 1);      // (c = 0: refused on the host)
        lag[tid] = make_double2(re / div, im / div);
    }
    __syncthreads();
    for (int i = tid; i < mv * mv; i += AG_THREADS) {
        const int a = i / mv, b = i - a * mv;
        if (a > b) continue;
        const double2 r = lag[lag_index(vx, b % vx - a % vx, b / vx - a / vx)];
        const float re = (float)r.x, im = a == b ? 0.f : (float)r.y;
        ra[(size_t)a * mv + b] = make_float2(re, im);
        if (a != b) ra[(size_t)b * mv + a] = make_float2(re, -im);
    }
}

// grid (nmat): rxx [nmat][m][m] -> ra [nmat][mv][mv].  (Templates, as refine.hpp's and esprit.hpp's kernels are: instantiated at their
// first use, at the end of the translation unit, they follow every older kernel in the code object.)
template <int NT>
__global__ __launch_bounds__(NT) void k_doa_augment(const float2 *__restrict__ rxx, int mx, int my, int vx, int vy, uint64_t mask,
                                                    float2 *__restrict__ ra)
{
    const size_t e = blockIdx.x, mm = (size_t)(mx * my) * (mx * my), vv = (size_t)(vx * vy) * (vx * vy);
    static_assert(NT == AG_THREADS, "augment_covariance strides by AG_THREADS");
    augment_covariance(rxx + e * mm, mx, my, vx, vy, mask, ra + e * vv);
}

template <int NT>
__global__ __launch_bounds__(NT) void k_augment_covariance(const float2 *__restrict__ rxx, int mx, int my, int vx, int vy, uint64_t mask,
                                                           float2 *__restrict__ ra)
{
    augment_covariance(rxx, mx, my, vx, vy, mask, ra);
}

} // namespace augment
} // namespace crsdr
