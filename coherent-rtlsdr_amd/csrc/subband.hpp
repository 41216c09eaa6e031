// subband.hpp -- one covariance per (estimate, frequency band): crsdr_doa_set_subbands / crsdr_subband_covariance.
//
// Definition (tests/doa_subband_model.py is the fp64 statement of it).  A signal row c of a packet holds L = B / 2 complex samples
// x_c[n] = (I + jQ) / 127.  Each row is cut into J = L / N segments of N = nfft samples (never across packets), segment j is
// transformed with the window w,  X_c[j][f] = sum_n w[n] x_c[jN + n] exp(-2 pi i f n / N),  and per bin
//     R_f[a][b] = 1 / (J' N sum_n w[n]^2) * sum_j conj(X_a[j][f]) X_b[j][f],      J' = frames * J   (the X^H X convention of crsdr_covariance).
// Band i is the sum of R_f over the bins (first + i width + u) mod N, u < width.  No mean is removed: a DC offset stays in bin 0 (Hann:
// bins 0 and +-1).
//
//   k_doa_subband_cov     grid (K slice of segments, unit group, estimate), 256 threads.  A unit is (8 x 8 block of R on or above the
//                         diagonal, bin); a thread keeps its unit's 64 complex sums in registers over the slice's segments.  Per chunk
//                         of segments the workgroup loads the rows its blocks touch (16-byte loads of the int8 packets), applies the
//                         window, runs the N-point transform in LDS in one or two register passes (fft_lds.hpp butterflies) and then
//                         every thread reads its 16 spectra values per segment from LDS: 16 LDS reads for 256 fmaf.
//                         Plain VALU, by measurement: the f32 MFMA (32 x 32 x 2, real and imaginary plane as k) runs at the vector
//                         rate and computes both triangles of a 32 x 32 tile; a variant on it took 211 us against 147 us (21 rows,
//                         nfft 64, 64 packets of 16384 bytes per row: DESIGN.md).
//   k_doa_subband_reduce  grid (band, estimate): adds the slices' fp32 partials in fp64 in slice order, bin after bin, scales in fp64,
//                         rounds once, writes both triangles (the lower one as the conjugate, the diagonal's imaginary part 0) and the
//                         band's power Re trace / m.
// The split (subband_spb) is a function of (B, N) alone, and a unit's sums run over its slice's segments in order: an estimate has the
// same bits wherever it sits in a batch.
//
// Transform: N = FA * FB.  Pass 1 is an FA-point DFT over n1 (n = n1 FB + n2) and the twiddle W_N^(n2 k1), pass 2 an FB-point DFT over
// n2; both in place, so bin f = k1 + FA k2 ends in slot k1 FB + k2 = (f mod FA) FB + f / FA.  Slots, not bins, index the partials.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "covariance.hpp"
#include "fft_lds.hpp"

namespace crsdr {
namespace subband {

constexpr int SB_THREADS = 256, SB_BLOCK = 8, SB_UNIT = SB_BLOCK * SB_BLOCK;      // a unit's partial: SB_UNIT float2
constexpr int SB_MAX_ROWS = 64, SB_MIN_LOG2 = 3, SB_MAX_LOG2 = 8;
constexpr int SB_LDS_POINTS = 7168;                    // float2 of spectra per chunk (56 KiB); a segment of a workgroup's rows is at most 4096
constexpr int SB_SLICE_SEGMENTS = 64, SB_MAX_SPB = 16; // a K slice has at least 64 segments (or the packet's all), a packet at most 16 slices
constexpr int WINDOW_RECT = 0, WINDOW_HANN = 1;

__host__ __device__ constexpr int sb_fa_log2(int lg) { return lg <= 4 ? lg : (lg == 5 || lg == 6) ? 3 : 4; }      // 8 16 | 8x4 8x8 | 16x8 16x16
__host__ __device__ constexpr int sb_blocks(int m) { return ((m + SB_BLOCK - 1) / SB_BLOCK) * ((m + SB_BLOCK - 1) / SB_BLOCK + 1) / 2; }
__host__ __device__ constexpr int sb_block_index(int nb, int bi, int bj) { return bi * nb - bi * (bi - 1) / 2 + (bj - bi); }
// K slices per packet: from (B, N) alone
__host__ __device__ constexpr int subband_spb(int B, int N)
{
    const int J = B / (2 * N), s = J / SB_SLICE_SEGMENTS;
    return s < 1 ? 1 : s > SB_MAX_SPB ? SB_MAX_SPB : s;
}
__host__ __device__ constexpr int subband_groups(int m, int N) { return (sb_blocks(m) * N + SB_THREADS - 1) / SB_THREADS; }
// float2 of partials per (estimate, slice)
__host__ __device__ constexpr size_t subband_partial(int m, int N) { return (size_t)sb_blocks(m) * N * SB_UNIT; }

// ---- the front end of a chunk, shared with subband_beams.hpp: both kernels stage the same spectra because they run these four ----
// the workgroup's tables: tw[t] = W_N^t, win[t] = the window
template <int LOG2N>
__device__ __forceinline__ void sb_fill_tables(float2 *tw, float *win, int window)
{
    constexpr int N = 1 << LOG2N;
    for (int t = threadIdx.x; t < N; t += SB_THREADS) {
        double s, c;
        sincospi(2.0 * (double)t / (double)N, &s, &c);
        tw[t] = make_float2((float)c, (float)-s);
        win[t] = window == WINDOW_HANN ? (float)(0.5 - 0.5 * c) : 1.0f;
    }
}
// one 16-byte piece = 8 samples (I, Q int8) from sample n0 of the segment on -> dst[0 .. 7] = win[n0 + n] (I + jQ)
__device__ __forceinline__ void sb_unpack_window(const uint4 wd, const float *win, int n0, float2 *dst)
{
    const uint32_t w4[4] = {wd.x, wd.y, wd.z, wd.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float w0 = win[n0 + 2 * k], w1 = win[n0 + 2 * k + 1];
        dst[2 * k] = make_float2(w0 * (float)(int8_t)(w4[k] & 0xFF), w0 * (float)(int8_t)((w4[k] >> 8) & 0xFF));
        dst[2 * k + 1] = make_float2(w1 * (float)(int8_t)((w4[k] >> 16) & 0xFF), w1 * (float)(int8_t)(w4[k] >> 24));
    }
}
// a pass-1 item: the FA-point DFT of the points at p + k FB, then W_N^(n2 k1); p = the segment's row + n2
template <int LOG2N>
__device__ __forceinline__ void sb_pass1(float2 *p, const float2 *tw, int n2)
{
    constexpr int LA = sb_fa_log2(LOG2N), FA = 1 << LA, LB = LOG2N - LA, FB = 1 << LB;
    float2 v[FA];
#pragma unroll
    for (int k = 0; k < FA; ++k) v[k] = p[k << LB];
    dft<FA, -1>(v);
    if constexpr (FB > 1) {
#pragma unroll
        for (int k = 1; k < FA; ++k) v[k] = cmul(v[k], tw[n2 * k]);
    }
#pragma unroll
    for (int k = 0; k < FA; ++k) p[k << LB] = v[k];
}
// a pass-2 item: the FB-point DFT of the consecutive points at p = the segment's row + k1 FB
template <int LOG2N>
__device__ __forceinline__ void sb_pass2(float2 *p)
{
    constexpr int FB = 1 << (LOG2N - sb_fa_log2(LOG2N));
    float2 v[FB];
#pragma unroll
    for (int k = 0; k < FB; ++k) v[k] = p[k];
    dft<FB, -1>(v);
#pragma unroll
    for (int k = 0; k < FB; ++k) p[k] = v[k];
}

// Packet t of the batch at packets + t * packet_stride, its matrix [nrows][B] int8 at + matrix_off (4-byte aligned).  Estimate e stacks
// packets e * frames .. + frames - 1.  grid (frames * spb, groups, nest): slice z = (frame z / spb, part z % spb of its J segments).
//   partial [nest][S][blocks][N slots][8][8] float2 = sum_j conj(X'_a) X'_b over the slice, X' the transform of w (I + jQ)
template <int LOG2N>
__global__ __launch_bounds__(SB_THREADS) void k_doa_subband_cov(const int8_t *__restrict__ packets, size_t packet_stride, size_t matrix_off, int nrows, int B,
                                                                int frames, int spb, int window, float2 *__restrict__ partial)
{
    constexpr int N = 1 << LOG2N, LA = sb_fa_log2(LOG2N), FA = 1 << LA, LB = LOG2N - LA, FB = 1 << LB;
    __shared__ float2 A[SB_LDS_POINTS];          // [segment of the chunk][row of the workgroup][N]
    __shared__ float2 tw[N];                     // W_N^t
    __shared__ float win[N];
    __shared__ int rows[SB_MAX_ROWS], rslot[SB_MAX_ROWS], nrow_s;
    const int m = nrows - 1, tid = threadIdx.x, nb = (m + SB_BLOCK - 1) / SB_BLOCK, nblk = nb * (nb + 1) / 2;
    const int z = blockIdx.x, S = gridDim.x, e = blockIdx.z;
    const int f = z / spb, part = z - f * spb, J = B / (2 * N);
    const int seg_lo = (int)(((long long)J * part) / spb), seg_hi = (int)(((long long)J * (part + 1)) / spb);
    const int8_t *matrix = packets + (size_t)(e * frames + f) * packet_stride + matrix_off;
    // this thread's unit, and the rows the workgroup's blocks touch
    const int unit = blockIdx.y * SB_THREADS + tid, blk = unit >> LOG2N, slot = unit & (N - 1);
    const bool active = blk < nblk;
    int bi = 0, bj = 0;
    {
        int left = active ? blk : nblk - 1;
        while (left >= nb - bi) { left -= nb - bi; ++bi; }
        bj = bi + left;
    }
    sb_fill_tables<LOG2N>(tw, win, window);
    if (tid == 0) {
        const int b_lo = (blockIdx.y * SB_THREADS) >> LOG2N, b_hi = min((blockIdx.y * SB_THREADS + SB_THREADS - 1) >> LOG2N, nblk - 1);
        unsigned long long mask = 0;
        int i = 0, j = 0;
        for (int b = 0; b <= b_hi; ++b) {
            if (b >= b_lo) mask |= (0xFFull << (SB_BLOCK * i)) | (0xFFull << (SB_BLOCK * j));
            if (++j == nb) { ++i; j = i; }
        }
        int n = 0;
        for (int c = 0; c < m; ++c) {
            rslot[c] = n;
            if ((mask >> c) & 1) rows[n++] = c;
        }
        nrow_s = n;
    }
    __syncthreads();
    const int R = nrow_s, SC = min(SB_LDS_POINTS / (R * N), seg_hi - seg_lo);      // segments per chunk (R * N <= 4096)
    int ra[SB_BLOCK], rb[SB_BLOCK];              // offsets of the unit's rows in a segment of A (rows past m: clamped, the reducer never reads them)
#pragma unroll
    for (int i = 0; i < SB_BLOCK; ++i) {
        ra[i] = rslot[min(SB_BLOCK * bi + i, m - 1)] * N + slot;
        rb[i] = rslot[min(SB_BLOCK * bj + i, m - 1)] * N + slot;
    }
    float2 acc[SB_BLOCK][SB_BLOCK];
#pragma unroll
    for (int i = 0; i < SB_BLOCK; ++i)
#pragma unroll
        for (int j = 0; j < SB_BLOCK; ++j) acc[i][j] = make_float2(0.f, 0.f);

    for (int s0 = seg_lo; s0 < seg_hi; s0 += SC) {
        const int sc = min(SC, seg_hi - s0);
        // load: 16 bytes = 8 samples per item; a row's chunk is contiguous
        const int ppr = sc * N / 8;              // pieces per row
        for (int it = tid; it < R * ppr; it += SB_THREADS) {
            const int r = it / ppr, piece = it - r * ppr;
            const uint4 wd = cov::cov_load16(matrix + (size_t)(1 + rows[r]) * B + (size_t)s0 * 2 * N + (size_t)piece * 16);
            const int jj = (piece * 8) >> LOG2N, n0 = (piece * 8) & (N - 1);
            sb_unpack_window(wd, win, n0, A + (jj * R + r) * N + n0);
        }
        __syncthreads();
        // pass 1: FA-point DFTs at stride FB, then W_N^(n2 k1)
        for (int it = tid; it < sc * R * FB; it += SB_THREADS) {
            const int n2 = it & (FB - 1);
            sb_pass1<LOG2N>(A + (it >> LB) * N + n2, tw, n2);
        }
        __syncthreads();
        if constexpr (FB > 1) {
            // pass 2: FB-point DFTs of consecutive points
            for (int it = tid; it < sc * R * FA; it += SB_THREADS) sb_pass2<LOG2N>(A + it * FB);
            __syncthreads();
        }
        if (active) {
            for (int jj = 0; jj < sc; ++jj) {
                const float2 *Aj = A + jj * R * N;
                float2 xa[SB_BLOCK], xb[SB_BLOCK];
#pragma unroll
                for (int i = 0; i < SB_BLOCK; ++i) { xa[i] = Aj[ra[i]]; xb[i] = Aj[rb[i]]; }
#pragma unroll
                for (int i = 0; i < SB_BLOCK; ++i)
#pragma unroll
                    for (int j = 0; j < SB_BLOCK; ++j) {
                        // conj(xa) xb
                        acc[i][j].x = fmaf(xa[i].y, xb[j].y, fmaf(xa[i].x, xb[j].x, acc[i][j].x));
                        acc[i][j].y = fmaf(-xa[i].y, xb[j].x, fmaf(xa[i].x, xb[j].y, acc[i][j].y));
                    }
            }
        }
        __syncthreads();
    }
    if (active) {
        float4 *pt = reinterpret_cast<float4 *>(partial + ((((size_t)e * S + z) * nblk + blk) * N + slot) * SB_UNIT);
#pragma unroll
        for (int i = 0; i < SB_BLOCK; ++i)
#pragma unroll
            for (int j = 0; j < SB_BLOCK; j += 2) pt[(i * SB_BLOCK + j) / 2] = make_float4(acc[i][j].x, acc[i][j].y, acc[i][j + 1].x, acc[i][j + 1].y);
    }
}

// grid (nbands, nest), 256 threads.  rbands [nest][nbands][m][m] cf32, power [nest][nbands].
__global__ __launch_bounds__(256) void k_doa_subband_reduce(const float2 *__restrict__ partial, int S, int nrows, int B, int frames, int log2n, int first, int width,
                                                            int window, float2 *__restrict__ rbands, float *__restrict__ power)
{
    __shared__ double sdiag[SB_MAX_ROWS];
    const int m = nrows - 1, N = 1 << log2n, la = sb_fa_log2(log2n), lb = log2n - la;
    const int nb = (m + SB_BLOCK - 1) / SB_BLOCK, nblk = nb * (nb + 1) / 2;
    const int band = blockIdx.x, nbands = gridDim.x, e = blockIdx.y;
    // sum w^2: N (rect), 3 N / 8 (periodic Hann, N >= 4)
    const double sw2 = window == WINDOW_HANN ? 0.375 * (double)N : (double)N;
    const double scale = 1.0 / (127.0 * 127.0 * (double)frames * (double)(B / (2 * N)) * (double)N * sw2);
    float2 *out = rbands + ((size_t)e * nbands + band) * m * m;
    for (int idx = threadIdx.x; idx < m * m; idx += 256) {
        const int a = idx / m, b = idx - a * m;
        if (a > b) continue;
        const int blk = sb_block_index(nb, a / SB_BLOCK, b / SB_BLOCK), el = (a % SB_BLOCK) * SB_BLOCK + (b % SB_BLOCK);
        double sr = 0.0, si = 0.0;
        for (int u = 0; u < width; ++u) {
            const int f = (first + band * width + u) & (N - 1), slot = ((f & ((1 << la) - 1)) << lb) + (f >> la);
            const float2 *p = partial + (((size_t)e * S * nblk + blk) * N + slot) * SB_UNIT + el;
            for (int z = 0; z < S; ++z) {
                const float2 v = p[(size_t)z * nblk * N * SB_UNIT];
                sr += (double)v.x; si += (double)v.y;
            }
        }
        sr *= scale; si *= scale;
        if (a == b) { si = 0.0; sdiag[a] = sr; }
        out[(size_t)a * m + b] = make_float2((float)sr, (float)si);
        if (a != b) out[(size_t)b * m + a] = make_float2((float)sr, -(float)si);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int a = 0; a < m; ++a) t += sdiag[a];
        power[(size_t)e * nbands + band] = (float)(t / (double)m);
    }
}

} // namespace subband
} // namespace crsdr
