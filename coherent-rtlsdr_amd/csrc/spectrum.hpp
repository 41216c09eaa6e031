// spectrum.hpp -- the two power maps beside the MUSIC pseudo-spectrum (crsdr_doa_set_spectrum, crsdr_spectrum2d), over the same grid and
// with the same steering vector a(cx, cy) as music::pmusic2d_point:
//     y_r = v_r^H a = sum_i conj(vec[i][r]) a[i]   for ALL columns r = 0 .. M-1,       S = sum_r w_r |y_r|^2
//     Bartlett   w_r = sv[r] / M^2,                                   pm = S       (= a^H R a / M^2: what a delay-and-sum beam receives)
//     Capon      w_r = 1 / (sv[r] + delta), delta = loading * sv[0],  pm = 1 / S   (= 1 / a^H (R + delta I)^-1 a: the MVDR beam's power)
// The weights are fp64 from the published fp32 sv, rounded once (what k_doa_beam_weights does at its few directions); everything else is
// fp32.  sv[0] == 0 (an all-zero estimate): pm = 0 everywhere.  Otherwise w_r >= 0 with w_0 > 0 (Capon: every w_r > 0 and sum_r |y_r|^2 = M,
// so S > 0 and 1 / S is finite; Bartlett on a rank-deficient estimate has w_r = 0 behind the rank and S = 0 where a is orthogonal to the
// signal columns): S >= 0, pm is never negative or NaN from finite input and doa.hpp's peak keys order it like MUSIC's.
//
// Shape.  As the MUSIC scan: one wave per workgroup, one grid point per lane, the lane's steering vector in LDS as A[i][lane].  The work
// is M^2 complex MACs per point (MUSIC: M (M - k)).  pmusic2d_point reads one element of U (a broadcast) and one of A (per lane) for every
// 4 FMAs; here the columns are taken four at a time: per element i one read of a[i] and two 16-byte broadcasts of U serve 16 FMAs on eight
// independent accumulators.  For that the columns of vec lie in LDS block by block: block b holds columns 4b .. 4b + nc - 1 (nc = 4, the
// last block M mod 4 if that is not 0) as [i][nc], at 4 b M.  Every column is summed over ascending i and S over ascending r, so the
// result does not depend on the blocking.  Plain fmaf (the Makefile's note on packed fp32).
//   LDS: U [M][M] cf32 + A [M][64] cf32 + w [M] float = 65 792 bytes at M = 64: above the 64 KiB default, the callers raise the limit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "doa.hpp"

namespace crsdr {
namespace spectrum {

enum { KIND_MUSIC = 0, KIND_BARTLETT = 1, KIND_CAPON = 2 };
constexpr int PT = music::PT, COLS = 4;

__host__ __device__ constexpr size_t lds_bytes(int M) { return sizeof(float2) * ((size_t)M * M + (size_t)M * PT) + sizeof(float) * (size_t)M; }

// NC columns of one block: U [M][NC] of the block, A + lane, w of the block's first column.  Returns S with the block's terms added.
template <int NC>
__device__ __forceinline__ float block_cols(const float2 *__restrict__ U, const float2 *__restrict__ A, const float *__restrict__ w, int M, float S)
{
    float yr[NC], yi[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) yr[c] = yi[c] = 0.f;
#pragma unroll 4
    for (int i = 0; i < M; ++i) {
        const float2 a = A[(size_t)i * PT];
        float2 u[NC];
        if constexpr (NC == 4) {
            const float4 p = reinterpret_cast<const float4 *>(U + i * 4)[0], q = reinterpret_cast<const float4 *>(U + i * 4)[1];
            u[0] = make_float2(p.x, p.y); u[1] = make_float2(p.z, p.w); u[2] = make_float2(q.x, q.y); u[3] = make_float2(q.z, q.w);
        } else if constexpr (NC == 2) {
            const float4 p = reinterpret_cast<const float4 *>(U + i * 2)[0];
            u[0] = make_float2(p.x, p.y); u[1] = make_float2(p.z, p.w);
        } else {
#pragma unroll
            for (int c = 0; c < NC; ++c) u[c] = U[i * NC + c];
        }
#pragma unroll
        for (int c = 0; c < NC; ++c) {                  // y += conj(u) a
            yr[c] = fmaf(u[c].y, a.y, fmaf(u[c].x, a.x, yr[c]));
            yi[c] = fmaf(-u[c].y, a.x, fmaf(u[c].x, a.y, yi[c]));
        }
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) S = fmaf(w[c], fmaf(yr[c], yr[c], yi[c] * yi[c]), S);
    return S;
}

// pm of grid point g = blockIdx.x * PT + threadIdx.x (live: g inside the grid), the whole workgroup (PT threads) calling together.
// vec [M][M] cf32 row-major (column r = v_r), sv [M]; kind BARTLETT or CAPON.  Shared by k_spectrum2d and k_doa_spectrum.
__device__ __forceinline__ float spectrum2d_point(const float2 *__restrict__ vec, const float *__restrict__ sv, int M, int kind, float loading, float d,
                                                  int Mx, int My, int Cx, int Cy, int g, bool live)
{
    extern __shared__ __attribute__((aligned(16))) float2 ssm[];
    float2 *U = ssm;                                     // the column blocks, M * M in all
    float2 *A = ssm + (size_t)M * M;                     // [M][PT]: this thread's steering vector, conflict-free by lane
    float *w = reinterpret_cast<float *>(A + (size_t)M * PT);      // [M]
    const int tid = threadIdx.x;
    const float s0 = sv[0];
    if (s0 == 0.f) return 0.f;                           // workgroup-uniform: an all-zero estimate (Capon would divide by zero)
    for (int e = tid; e < M * M; e += PT) {
        const int i = e / M, r = e - i * M, b = r / COLS, nc = min(COLS, M - COLS * b);
        U[(size_t)COLS * b * M + i * nc + (r - COLS * b)] = vec[e];
    }
    if (tid < M) {
        const double sr = (double)sv[tid];
        w[tid] = kind == KIND_CAPON ? (float)(1.0 / (sr + (double)loading * (double)s0)) : (float)(sr / ((double)M * (double)M));
    }
    // the steering vector: the expressions of music::pmusic2d_point in their order, so that a grid point is the same direction in every map
    const int cx = live ? g / Cy : 0, cy = live ? g - (g / Cy) * Cy : 0;
    const float pi = 3.14159274101257324f;
    const float alpha = (float)cx * pi / (float)Cx, beta = (float)cy * pi / (float)Cy;
    const float ca = cosf(alpha), sb = sinf(beta), cb = cosf(beta);
    for (int iy = 0, rc = 0; iy < My; ++iy) {
        const float py = 2.0f * pi * (float)iy * d * cb;
        float sy, cyv;
        sincosf(py, &sy, &cyv);
        for (int ix = 0; ix < Mx; ++ix, ++rc) {
            const float px = 2.0f * pi * (float)ix * d * ca * sb;
            float sx, cxv;
            sincosf(px, &sx, &cxv);
            A[(size_t)rc * PT + tid] = make_float2(cxv * cyv - sx * sy, cxv * sy + sx * cyv);
        }
    }
    __syncthreads();
    float S = 0.f;
    const int full = M / COLS;
    for (int b = 0; b < full; ++b) S = block_cols<COLS>(U + (size_t)COLS * b * M, A + tid, w + COLS * b, M, S);
    const float2 *Ut = U + (size_t)COLS * full * M;
    const float *wt = w + COLS * full;
    switch (M - COLS * full) {                           // the last, narrower block
    case 1: S = block_cols<1>(Ut, A + tid, wt, M, S); break;
    case 2: S = block_cols<2>(Ut, A + tid, wt, M, S); break;
    case 3: S = block_cols<3>(Ut, A + tid, wt, M, S); break;
    default: break;
    }
    return kind == KIND_CAPON ? 1.0f / S : S;
}

// crsdr_spectrum2d: pm [Cx][Cy] row-major.  grid (ceil(Cx Cy / PT)), PT threads, lds_bytes(M) of dynamic LDS.
__global__ __launch_bounds__(PT) void k_spectrum2d(const float2 *__restrict__ vec, const float *__restrict__ sv, int M, int kind, float loading, float d, int Mx,
                                                   int My, int Cx, int Cy, float *__restrict__ pm)
{
    const int g = blockIdx.x * PT + threadIdx.x;
    const bool live = g < Cx * Cy;
    const float v = spectrum2d_point(vec, sv, M, kind, loading, d, Mx, My, Cx, Cy, g, live);
    if (live) pm[g] = v;
}

// The batched scan, in the place and shape of doa::k_doa_scan: grid (ceil(Cx Cy / PT), nmat), one wave.  vec [nmat][M][M], sv [nmat][M];
// pm [nmat][Cx][Cy] or NULL; wgbest [nmat][gridDim.x]: the workgroup's best key, for k_doa_peak and the local-peak kernels behind it.
__global__ __launch_bounds__(PT) void k_doa_spectrum(const float2 *__restrict__ vec, const float *__restrict__ sv, int M, int kind, float loading, float d, int Mx,
                                                     int My, int Cx, int Cy, float *__restrict__ pm, unsigned long long *__restrict__ wgbest)
{
    static_assert(PT == 64, "the workgroup's peak is reduced with wave shuffles");
    const size_t e = blockIdx.y;
    const int g = blockIdx.x * PT + threadIdx.x;
    const bool live = g < Cx * Cy;
    const float v = spectrum2d_point(vec + e * M * M, sv + e * M, M, kind, loading, d, Mx, My, Cx, Cy, g, live);
    if (pm && live) pm[e * Cx * Cy + g] = v;
    unsigned long long key = live ? doa::peak_key(v, g) : 0ull;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned long long o = doa::shfl_xor_u64(key, off);
        key = o > key ? o : key;
    }
    if (threadIdx.x == 0) wgbest[e * gridDim.x + blockIdx.x] = key;
}

} // namespace spectrum
} // namespace crsdr
