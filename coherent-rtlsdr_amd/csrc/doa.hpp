// doa.hpp -- the beamformer chain of covariance.hpp / music.hpp in its batched form (crsdr_doa): one estimate per F consecutive
// packets of a plan's batch, every step one launch over all estimates, nothing per estimate on the host.
//
//   k_doa_cov         grid (K slice, estimate): the m <= 64 signal rows are one or two 32-row operand blocks, so Rxx is 1 or 3
//                     v_mfma_i32_32x32x32_i8 tiles on / above the diagonal.  A workgroup's four waves split its K slice, add their
//                     exact int32 partials in LDS and leave them in a workspace.
//   k_doa_cov_reduce  grid (tile, estimate): adds the slices' partials in 64 bits and applies the fp64 epilogue of k_covariance /
//                     k_cov_reduce with L = F * blocksize / 2.  Integer sums: whatever the split, the bits of crsdr_covariance.
//   k_doa_subspace    music::herm_subspace per estimate (one workgroup each, as k_herm_subspace).
//   k_doa_scan        music::pmusic2d_point per grid point and estimate; the workgroup's largest pm leaves as one 64-bit key.
//   k_doa_peak        grid (estimate): the largest key -> (cx, cy) and its value.
// With crsdr_doa_set_smoothing the subspace works on the smoothed covariance (smooth.hpp: k_doa_smooth behind the reducer), with
// crsdr_doa_set_order the scan takes every estimate's source count from k_doa_order's output (k_doa_scan<true>).
//
// Peak order: pm = (a2 / den)^2 is never negative, so the bit pattern of the float orders like the value; the key is
// (value bits << 32) | (0xFFFFFFFF - row-major index): its maximum is the largest value at the LOWEST index, whatever order the keys are
// combined in.  A NaN pm (a NaN in the subspace: never from the division, a2 = m > 0) is canonicalised to 0x7FC00000, above +inf: NaN counts
// as the largest value and the first NaN wins, which is what numpy's argmax does with the same spectrum.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "covariance.hpp"
#include "music.hpp"

namespace crsdr {
namespace doa {

using cov::v16i;
using cov::v4i;

constexpr int COV_WAVES = 4, COV_THREADS = 64 * COV_WAVES;
constexpr int TILE = 32, TILE_ELEMS = TILE * TILE;      // one MFMA tile; a tile's partial = two planes of TILE_ELEMS int32
constexpr int MAX_ROWS = 64;                            // = music::MAX_M: two operand blocks

__host__ __device__ constexpr int cov_tiles(int nt) { return nt * (nt + 1) / 2; }

__device__ __forceinline__ v4i as_v4i(const uint4 w) { return v4i{(int)w.x, (int)w.y, (int)w.z, (int)w.w}; }
__device__ __forceinline__ v4i swapnot4(const v4i a) { return v4i{cov::swapnot16(a.x), cov::swapnot16(a.y), cov::swapnot16(a.z), cov::swapnot16(a.w)}; }

// Packet t of the batch at packets + t * packet_stride, its matrix [nrows][B] int8 at + matrix_off (4-byte aligned).  Estimate e stacks
// packets e * frames .. e * frames + frames - 1 along K.  grid (frames * spb, nest): slice z = (frame z / spb, part z % spb of its B / 32
// MFMA steps); a part is at most 65536 bytes (the host picks spb >= B / 65536), so every int32 sum is exact (|sum| <= 2^30).
//   partial [nest][S][tiles][2][16 regs][64 lanes] int32 in the MFMA's C/D layout: plane 0 = sum (I_a I_b + Q_a Q_b),
//                                                  plane 1 = sum (Q_a I_b - I_a Q_b) - sum Q_b   (A' = (Q, ~I): see covariance.hpp)
//   psum    [nest][S][MAX_ROWS] int2: the slice's sums of I and Q per signal row
template <int NT>
__global__ __launch_bounds__(COV_THREADS) void k_doa_cov(const int8_t *__restrict__ packets, size_t packet_stride, size_t matrix_off, int nrows, int B,
                                                         int frames, int spb, int *__restrict__ partial, int2 *__restrict__ psum)
{
    constexpr int NTRI = cov_tiles(NT);
    __shared__ int red[NTRI * 2 * TILE_ELEMS];
    __shared__ int rsum[NT * TILE * 2];
    const int m = nrows - 1, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int e = blockIdx.y, z = blockIdx.x, S = gridDim.x;
    const int f = z / spb, part = z - f * spb;
    const int8_t *matrix = packets + (size_t)(e * frames + f) * packet_stride + matrix_off;
    const int steps = B / 32;
    const int s_lo = (int)(((long long)steps * part) / spb), s_hi = (int)(((long long)steps * (part + 1)) / spb);
    const int n = s_hi - s_lo, w_lo = s_lo + n * wave / COV_WAVES, w_hi = s_lo + n * (wave + 1) / COV_WAVES;
    for (int i = tid; i < NTRI * 2 * TILE_ELEMS; i += COV_THREADS) red[i] = 0;
    if (tid < NT * TILE * 2) rsum[tid] = 0;
    __syncthreads();
    // operand fragment of the 32x32x32 int8 MFMA: lane -> row lane & 31, the 16 K bytes of half lane >> 5 (both operands alike)
    const int r = lane & 31;
    const int8_t *p0 = matrix + (size_t)(1 + min(r, m - 1)) * B + 16 * (lane >> 5);            // clamp: padded rows are masked by the reducer
    const int8_t *p1 = matrix + (size_t)(1 + min(TILE + r, m - 1)) * B + 16 * (lane >> 5);
    v16i g1[NTRI] = {}, g2[NTRI] = {};
    int si0 = 0, sq0 = 0, si1 = 0, sq1 = 0;
    // four steps (128 bytes of every row: one cache line) loaded before their MFMAs, so that a wave has eight 16-byte loads in flight
#define DOA_COV_STEP(w0, w1)                                                                                         \
    do {                                                                                                             \
        const v4i a0 = as_v4i(w0), n0 = swapnot4(a0);                                                                \
        cov::cov_iq_sums(w0, si0, sq0);                                                                              \
        g1[0] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a0, a0, g1[0], 0, 0, 0);                                       \
        g2[0] = __builtin_amdgcn_mfma_i32_32x32x32_i8(n0, a0, g2[0], 0, 0, 0);                                       \
        if constexpr (NT == 2) {                                                                                     \
            const v4i a1 = as_v4i(w1), n1 = swapnot4(a1);                                                            \
            cov::cov_iq_sums(w1, si1, sq1);                                                                          \
            g1[1] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a0, a1, g1[1], 0, 0, 0);                                   \
            g2[1] = __builtin_amdgcn_mfma_i32_32x32x32_i8(n0, a1, g2[1], 0, 0, 0);                                   \
            g1[2] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a1, a1, g1[2], 0, 0, 0);                                   \
            g2[2] = __builtin_amdgcn_mfma_i32_32x32x32_i8(n1, a1, g2[2], 0, 0, 0);                                   \
        }                                                                                                            \
    } while (0)
    int s = w_lo;
    for (; s + 4 <= w_hi; s += 4) {
        uint4 w0[4], w1[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            w0[k] = cov::cov_load16(p0 + (size_t)(s + k) * 32);
            w1[k] = NT == 2 ? cov::cov_load16(p1 + (size_t)(s + k) * 32) : w0[k];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) DOA_COV_STEP(w0[k], w1[k]);
    }
    for (; s < w_hi; ++s) {
        const uint4 w0 = cov::cov_load16(p0 + (size_t)s * 32);
        const uint4 w1 = NT == 2 ? cov::cov_load16(p1 + (size_t)s * 32) : w0;
        DOA_COV_STEP(w0, w1);
    }
#undef DOA_COV_STEP
    // waves -> workgroup: integer adds in LDS (order cannot change an exact sum); lanes of a register are consecutive words
#pragma unroll
    for (int u = 0; u < NTRI; ++u)
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            atomicAdd(&red[(2 * u) * TILE_ELEMS + k * 64 + lane], g1[u][k]);
            atomicAdd(&red[(2 * u + 1) * TILE_ELEMS + k * 64 + lane], g2[u][k]);
        }
    si0 += __shfl_xor(si0, 32, 64); sq0 += __shfl_xor(sq0, 32, 64);      // the two K halves of a row
    si1 += __shfl_xor(si1, 32, 64); sq1 += __shfl_xor(sq1, 32, 64);
    if (lane < 32) {
        atomicAdd(&rsum[2 * r], si0); atomicAdd(&rsum[2 * r + 1], sq0);
        if constexpr (NT == 2) { atomicAdd(&rsum[2 * (TILE + r)], si1); atomicAdd(&rsum[2 * (TILE + r) + 1], sq1); }
    }
    __syncthreads();
    int *pt = partial + ((size_t)e * S + z) * (NTRI * 2 * TILE_ELEMS);
    for (int i = tid; i < NTRI * 2 * TILE_ELEMS; i += COV_THREADS) pt[i] = red[i];
    if (tid < NT * TILE) psum[((size_t)e * S + z) * MAX_ROWS + tid] = make_int2(rsum[2 * tid], rsum[2 * tid + 1]);
}

// grid (tiles, nest), 256 threads: four elements of the tile per thread.  rxx [nest][m][m] cf32, both triangles.
__global__ __launch_bounds__(256) void k_doa_cov_reduce(const int *__restrict__ partial, const int2 *__restrict__ psum, int S, int ntri, int nrows, int B,
                                                        int frames, float2 *__restrict__ rxx)
{
    __shared__ double2 srow[TILE], scol[TILE];
    const int m = nrows - 1, tid = threadIdx.x, u = blockIdx.x, e = blockIdx.y;
    const int ti = u == 2 ? 1 : 0, tj = u == 0 ? 0 : 1;                  // tiles in the order (0,0), (0,1), (1,1)
    if (tid < 2 * TILE) {
        const int row = tid < TILE ? ti * TILE + tid : tj * TILE + tid - TILE;
        const int2 *ps = psum + (size_t)e * S * MAX_ROWS + row;
        long long a = 0, b = 0;
        for (int z = 0; z < S; ++z) { const int2 v = ps[(size_t)z * MAX_ROWS]; a += v.x; b += v.y; }
        (tid < TILE ? srow[tid] : scol[tid - TILE]) = make_double2((double)a, (double)b);
    }
    const size_t zs = (size_t)ntri * 2 * TILE_ELEMS;
    const int *p0 = partial + (size_t)e * S * zs + (size_t)u * 2 * TILE_ELEMS + tid;
    long long s1[4] = {}, s2[4] = {};
    // the loads of four slices are issued before the first add (a rolled loop waits out one round trip per slice)
    for (int z0 = 0; z0 < S; z0 += 4) {
        int v1[4][4], v2[4][4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int *q = p0 + (size_t)min(z0 + k, S - 1) * zs;
#pragma unroll
            for (int j = 0; j < 4; ++j) { v1[k][j] = q[256 * j]; v2[k][j] = q[TILE_ELEMS + 256 * j]; }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (z0 + k < S) {
#pragma unroll
                for (int j = 0; j < 4; ++j) { s1[j] += v1[k][j]; s2[j] += v2[k][j]; }
            }
    }
    __syncthreads();
    const double L = (double)frames * (double)(B / 2), scale = 1.0 / (127.0 * 127.0);
    float2 *out = rxx + (size_t)e * m * m;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        // C/D layout of the 32 x 32 MFMA: element reg * 64 + lane -> col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
        const int i = tid + 256 * j, reg = i >> 6, lane = i & 63;
        const int lrow = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5), lcol = lane & 31;
        const int row = ti * TILE + lrow, col = tj * TILE + lcol;
        if (row < m && col < m) {
            const double2 sa = srow[lrow], sb = scol[lcol];
            // (1/L) sum conj(x_a) x_b - conj(mean_a) mean_b,   x = (I + jQ)/127      (the expression of k_covariance / k_cov_reduce)
            const double re = ((double)s1[j] / L - (sa.x * sb.x + sa.y * sb.y) / (L * L)) * scale;
            const long long s_im = -(s2[j] + (long long)sb.y);      // I_a Q_b - Q_a I_b: the tiles left sum (Q_a I_b - I_a Q_b - Q_b)
            const double im = ((double)s_im / L - (sa.x * sb.y - sa.y * sb.x) / (L * L)) * scale;
            out[(size_t)row * m + col] = make_float2((float)re, (float)im);
            if (ti != tj) out[(size_t)col * m + row] = make_float2((float)re, -(float)im);      // the tile below the diagonal
        }
    }
}

// grid (nest): rxx [nest][M][M] -> sv [nest][M], vec [nest][M][M], info [nest][2] (sweeps, converged)
__global__ __launch_bounds__(music::JT) void k_doa_subspace(const float2 *__restrict__ rxx, int M, float *__restrict__ sv, float2 *__restrict__ vec,
                                                            int *__restrict__ info)
{
    const size_t e = blockIdx.x;
    music::herm_subspace(rxx + e * M * M, M, sv + e * M, vec + e * M * M, info + 2 * e);
}

__device__ __forceinline__ unsigned long long peak_key(float v, int g)
{
    const uint32_t bits = v != v ? 0x7FC00000u : __float_as_uint(v);
    return ((unsigned long long)bits << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)g);
}
__device__ __forceinline__ unsigned long long shfl_xor_u64(unsigned long long v, int mask)
{
    const int lo = __shfl_xor((int)(uint32_t)v, mask, 64), hi = __shfl_xor((int)(uint32_t)(v >> 32), mask, 64);
    return ((unsigned long long)(uint32_t)hi << 32) | (uint32_t)lo;
}

// grid (ceil(Cx Cy / PT), nest), PT threads = one wave.  vec [nest][M][M]; pm [nest][Cx][Cy] or NULL; wgbest [nest][gridDim.x].
// PER_EST (crsdr_doa_set_order): estimate e takes its source count from korder [nest] (in [kmin, M - 1]: the dynamic LDS covers
// M - kmin noise vectors) instead of k; pmusic2d_point is the same either way, so its pm has the bits of a fixed-k = korder[e] scan.
template <bool PER_EST>
__global__ __launch_bounds__(music::PT) void k_doa_scan(const float2 *__restrict__ vec, int M, int k, float d, int Mx, int My, int Cx, int Cy,
                                                        float *__restrict__ pm, unsigned long long *__restrict__ wgbest,
                                                        const int32_t *__restrict__ korder)
{
    static_assert(music::PT == 64, "the workgroup's peak is reduced with wave shuffles");
    const size_t e = blockIdx.y;
    const int g = blockIdx.x * music::PT + threadIdx.x;
    const bool live = g < Cx * Cy;
    if constexpr (PER_EST) k = korder[e];
    const float v = music::pmusic2d_point(vec + e * M * M, M, M, k, M - k, d, Mx, My, Cx, Cy, g, live);
    if (pm && live) pm[e * Cx * Cy + g] = v;
    unsigned long long key = live ? peak_key(v, g) : 0ull;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned long long o = shfl_xor_u64(key, off);
        key = o > key ? o : key;
    }
    if (threadIdx.x == 0) wgbest[e * gridDim.x + blockIdx.x] = key;
}

// grid (nest), 256 threads: peak [nest][2] = (cx, cy), peak_value [nest]
__global__ __launch_bounds__(256) void k_doa_peak(const unsigned long long *__restrict__ wgbest, int nwg, int Cy, int32_t *__restrict__ peak,
                                                  float *__restrict__ peak_value)
{
    __shared__ unsigned long long wred[4];
    const size_t e = blockIdx.x;
    unsigned long long key = 0;
    for (int i = threadIdx.x; i < nwg; i += 256) { const unsigned long long o = wgbest[e * nwg + i]; key = o > key ? o : key; }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned long long o = shfl_xor_u64(key, off);
        key = o > key ? o : key;
    }
    if ((threadIdx.x & 63) == 0) wred[threadIdx.x >> 6] = key;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) key = wred[w] > key ? wred[w] : key;
        const int g = (int)(0xFFFFFFFFu - (uint32_t)key);
        peak[2 * e] = g / Cy;
        peak[2 * e + 1] = g - (g / Cy) * Cy;
        peak_value[e] = __uint_as_float((uint32_t)(key >> 32));
    }
}

// ---- several directions per estimate (crsdr_doa_set_peaks): the `count` largest local maxima of each spectrum ----
// Point g is a local peak if its key beats every other key in the (2r+1) x (2r+1) window around it, clipped at the grid's edges.  Keys
// are unique, so that is "its key is the window's maximum", and the maximum of a rectangle is the maximum over its rows of each row's
// maximum: 2 (2r + 1) comparisons per point instead of (2r + 1)^2.  Key 0 would need index 0xFFFFFFFF (grids hold at most 2^24 points):
// it stands for "no point", both outside the grid and in an empty candidate slot.
constexpr int LP_TX = 16, LP_TY = 64, LP_THREADS = 256, LP_PER_THREAD = LP_TX * LP_TY / LP_THREADS;      // a tile: 16 rows of 64 points
constexpr int MAX_PEAKS = 16, MAX_RADIUS = 16;

__host__ __device__ constexpr int lp_tiles(int Cx, int Cy) { return ((Cx + LP_TX - 1) / LP_TX) * ((Cy + LP_TY - 1) / LP_TY); }
__host__ __device__ constexpr size_t lp_lds(int r)
{
    return sizeof(unsigned long long) * ((size_t)(LP_TX + 2 * r) * (LP_TY + 2 * r) + (size_t)(LP_TX + 2 * r) * LP_TY);
}

// the largest `key` of the workgroup (LP_THREADS threads), in every thread; red [LP_THREADS / 64] is free again on return
__device__ __forceinline__ unsigned long long lp_block_max(unsigned long long key, unsigned long long *red)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned long long o = shfl_xor_u64(key, off);
        key = o > key ? o : key;
    }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = key;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < LP_THREADS / 64; ++w) key = red[w] > key ? red[w] : key;
    __syncthreads();
    return key;
}

// Rounds of max-and-remove over the keys a thread holds: round i takes the largest key below the one taken in round i - 1 (keys are
// unique), thread i keeps it.  Ends early once nothing is left (the round's maximum is the same in every thread).  Returns the number taken.
template <int N>
__device__ __forceinline__ int lp_top(const unsigned long long (&keys)[N], int count, unsigned long long *red, unsigned long long &mine)
{
    unsigned long long last = ~0ull;
    int n = 0;
    mine = 0;
    for (; n < count; ++n) {
        unsigned long long best = 0;
#pragma unroll
        for (int u = 0; u < N; ++u) best = keys[u] < last && keys[u] > best ? keys[u] : best;
        best = lp_block_max(best, red);
        if (best == 0) break;
        if ((int)threadIdx.x == n) mine = best;
        last = best;
    }
    return n;
}

// grid (lp_tiles(Cx, Cy), nest), LP_THREADS threads, lp_lds(r) bytes of dynamic LDS.  pm [nest][Cx][Cy];
// cand [nest][tiles][count]: the tile's local peaks, the `count` largest keys in descending order, then 0.
__global__ __launch_bounds__(LP_THREADS) void k_doa_local_peaks(const float *__restrict__ pm, int Cx, int Cy, int r, int count,
                                                                unsigned long long *__restrict__ cand)
{
    extern __shared__ unsigned long long lpk[];
    __shared__ unsigned long long red[LP_THREADS / 64];
    const int tid = threadIdx.x, tiles_y = (Cy + LP_TY - 1) / LP_TY;
    const size_t e = blockIdx.y;
    const int x0 = (int)(blockIdx.x / tiles_y) * LP_TX, y0 = (int)(blockIdx.x % tiles_y) * LP_TY;
    const int HX = LP_TX + 2 * r, HY = LP_TY + 2 * r;
    unsigned long long *key = lpk;                  // [HX][HY]: the keys of the tile and its r-wide halo, 0 outside the grid
    unsigned long long *hmax = lpk + HX * HY;       // [HX][LP_TY]: the largest key of each row's window
    const float *p = pm + e * Cx * Cy;
    // row segments of the halo'd tile: consecutive threads read consecutive points of a row
    for (int i = tid; i < HX * HY; i += LP_THREADS) {
        const int hx = i / HY, cx = x0 - r + hx, cy = y0 - r + (i - hx * HY);
        key[i] = cx >= 0 && cx < Cx && cy >= 0 && cy < Cy ? peak_key(p[(size_t)cx * Cy + cy], cx * Cy + cy) : 0ull;
    }
    __syncthreads();
    for (int i = tid; i < HX * LP_TY; i += LP_THREADS) {
        const int hx = i / LP_TY;
        const unsigned long long *row = key + hx * HY + (i - hx * LP_TY);
        unsigned long long m = row[0];
        for (int j = 1; j <= 2 * r; ++j) m = row[j] > m ? row[j] : m;
        hmax[i] = m;
    }
    __syncthreads();
    unsigned long long mine[LP_PER_THREAD];
#pragma unroll
    for (int u = 0; u < LP_PER_THREAD; ++u) {
        const int i = tid + u * LP_THREADS, x = i / LP_TY, y = i - x * LP_TY;
        const unsigned long long k = key[(x + r) * HY + y + r];
        unsigned long long m = hmax[x * LP_TY + y];
        for (int j = 1; j <= 2 * r; ++j) m = hmax[(x + j) * LP_TY + y] > m ? hmax[(x + j) * LP_TY + y] : m;
        mine[u] = m == k ? k : 0ull;                 // (k = 0: a point of the tile outside the grid)
    }
    unsigned long long top;
    lp_top(mine, count, red, top);
    if (tid < count) cand[(e * gridDim.x + blockIdx.x) * count + tid] = top;
}

// grid (nest), LP_THREADS threads: the `count` largest of the ncand = tiles * count candidates of an estimate ->
// found [nest], peaks [nest][count][2] = (cx, cy), values [nest][count]; the slots after found hold (-1, -1) and -1.
// cap [nest] or NULL: at most cap[e] of them (crsdr_doa_set_order with limit_directions: the estimate's source count).
__global__ __launch_bounds__(LP_THREADS) void k_doa_peaks_merge(const unsigned long long *__restrict__ cand, int ncand, int Cy, int count,
                                                                int32_t *__restrict__ found, int32_t *__restrict__ peaks,
                                                                float *__restrict__ values, const int32_t *__restrict__ cap)
{
    __shared__ unsigned long long red[LP_THREADS / 64];
    const size_t e = blockIdx.x;
    const unsigned long long *c = cand + e * ncand;
    const int tid = threadIdx.x;
    // most grids leave at most a few candidates per thread (100 x 100: 14 tiles); a larger one is folded down to LP_MERGE keys per thread
    // first, each thread keeping the largest LP_MERGE of its strided share -- which holds every one of its keys that can be among the
    // workgroup's `count` largest only if LP_MERGE >= count, so LP_MERGE = MAX_PEAKS
    constexpr int LP_MERGE = MAX_PEAKS;
    unsigned long long keys[LP_MERGE];
#pragma unroll
    for (int u = 0; u < LP_MERGE; ++u) keys[u] = 0;
    for (int j = tid; j < ncand; j += LP_THREADS) {
        unsigned long long o = c[j];
#pragma unroll
        for (int u = 0; u < LP_MERGE; ++u) {      // insertion into the descending list keys[]
            const unsigned long long hi = keys[u] > o ? keys[u] : o, lo = keys[u] > o ? o : keys[u];
            keys[u] = hi; o = lo;
        }
    }
    unsigned long long mine;
    const int take = cap ? min(count, max(cap[e], 0)) : count;
    const int n = lp_top(keys, take, red, mine);
    if (tid < count) {
        const int g = (int)(0xFFFFFFFFu - (uint32_t)mine);
        const size_t s = e * count + tid;
        peaks[2 * s] = mine ? g / Cy : -1;
        peaks[2 * s + 1] = mine ? g - (g / Cy) * Cy : -1;
        values[s] = mine ? __uint_as_float((uint32_t)(mine >> 32)) : -1.0f;
    }
    if (tid == 0) found[e] = n;
}

} // namespace doa
} // namespace crsdr
