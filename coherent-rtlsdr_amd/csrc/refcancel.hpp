// refcancel.hpp -- the reference-noise canceller of digital-mode plans (include/crsdr.h, crsdr_plan_set_refcancel / crsdr_refcancel).
// Per owned row and block: y = the row shifted by its lag (the row the phase path uses), r_j = the block's reference row delayed by
// j samples, j = -K .. K, zero-filled.  g solves the normal equations G g = c of the least-squares fit of y by the r_j from exact
// integer sums; the row written is clip(rint(p (y - sum_j g_j r_j))).
//   k_refcancel_gram    one workgroup per block: the 45 integer sums G_ij of the 9 x 9 Gram (taps -4 .. 4; fewer taps use its centre),
//                       then one lane factors the centre taps x taps part in fp64 (Cholesky) -- once per block, every row shares it
//   k_refcancel_dots    one workgroup per (row, block): c_j and E = sum |y|^2 by dot4 on byte-aligned reference words, workgroup
//                       reduction, one lane substitutes through the factor and publishes g (fp32), the residual share and the status
//   k_refcancel_apply   one workgroup per (row, block): eight samples per thread and step, taps complex multiply-adds per sample on
//                       reference samples converted to float once, rotation, round-half-even and saturation as rotq_word does them
// The reference window of a step -- samples 8 i - 4 .. 8 i + 11, whatever the tap count -- is eight words: two 16-byte loads at an
// 8-byte aligned address inside the row, word-wise with zero fill at the row's two ends (and for rows that are only 4-byte aligned).
#pragma once
#include "kernels.hpp"
#include "refcancel_solve.hpp"

namespace crsdr {
namespace rc {

constexpr int kThreads = 256;

struct CancelArgs {
    const int8_t *rows;        // batch base: block t at rows + t * block_stride, layout [nrows][B], row 0 = reference
    size_t block_stride;
    int8_t *orows;             // row `row` of block t goes to orows + t * orows_stride + (row - orow_first) * B
    size_t orows_stride;
    int orow_first;
    const int32_t *lag;        // [T][nrows] the lags the rows are shifted by
    const float2 *phasor;      // [T][nrows]
    float2 *coef;              // [T][nrows][coef_pitch] g_j, j ascending
    int coef_pitch;
    float *residual;           // [T][nrows]
    int32_t *status;           // [T][nrows]
    int32_t *gram;             // [T][GRAM_INTS]
    cd *chol;                  // [T][GRAM_PAIRS] the factor of the block's Gram
    int32_t *block_status;     // [T] 0 or STATUS_SINGULAR
    int nrows, B, row_begin, taps;
    uint32_t xor80;
};

struct __attribute__((packed, aligned(8))) u4_aligned8 { uint32_t x, y, z, w; };

// words 4 i - 2 .. 4 i + 5 of the reference row (samples 8 i - 4 .. 8 i + 11), zero outside the row
template <bool VEC>
__device__ __forceinline__ void ref_window(uint32_t (&w)[8], const int8_t *__restrict__ rrow, int i, int nw, uint32_t xor80)
{
    const int w0 = 4 * i - 2;
    if (VEC && w0 >= 0 && w0 + 8 <= nw) {
        const u4_aligned8 lo = *reinterpret_cast<const u4_aligned8 *>(rrow + 4 * (ptrdiff_t)w0);
        const u4_aligned8 hi = *reinterpret_cast<const u4_aligned8 *>(rrow + 4 * (ptrdiff_t)w0 + 16);
        w[0] = lo.x ^ xor80; w[1] = lo.y ^ xor80; w[2] = lo.z ^ xor80; w[3] = lo.w ^ xor80;
        w[4] = hi.x ^ xor80; w[5] = hi.y ^ xor80; w[6] = hi.z ^ xor80; w[7] = hi.w ^ xor80;
    } else {
        const uint32_t *r32 = reinterpret_cast<const uint32_t *>(rrow);
#pragma unroll
        for (int q = 0; q < 8; ++q) w[q] = ((unsigned)(w0 + q) < (unsigned)nw) ? (r32[w0 + q] ^ xor80) : 0u;
    }
}

// the eight samples 8 i .. 8 i + 7 of the row shifted by d, as k_align_quant reads them
template <bool VEC>
__device__ __forceinline__ uint4 row_vec(const int8_t *__restrict__ srow, int i, int nvec, int d, int L, uint32_t xor80)
{
    if constexpr (VEC) {
        uint4 sv[1];
        shifted_vecs<1>(sv, srow, i, kThreads, nvec, d, L, xor80);
        return sv[0];
    } else {
        const uint32_t *s32 = reinterpret_cast<const uint32_t *>(srow);
        return make_uint4(shifted_word(s32, 4 * i, d, L, xor80), shifted_word(s32, 4 * i + 1, d, L, xor80), shifted_word(s32, 4 * i + 2, d, L, xor80),
                          shifted_word(s32, 4 * i + 3, d, L, xor80));
    }
}

// a lag outside [-L, L] shifts everything out, as -L and L do (the plan's lags are inside; the per-op call takes the caller's)
__device__ __forceinline__ int clamp_lag(int d, int L) { return d < -L ? -L : (d > L ? L : d); }

template <bool VEC>
__global__ __launch_bounds__(kThreads) void k_refcancel_gram(CancelArgs a)
{
    __shared__ int sred[kThreads / 64][GRAM_INTS];
    __shared__ int32_t sg[GRAM_INTS];
    __shared__ cd sL[GRAM_PAIRS];
    const int tid = threadIdx.x, t = blockIdx.x;
    const int nvec = a.B / 16, nw = a.B / 4;
    const int8_t *rrow = a.rows + (size_t)t * a.block_stride;
    int acc[GRAM_INTS];
#pragma unroll
    for (int v = 0; v < GRAM_INTS; ++v) acc[v] = 0;
    for (int i = tid; i < nvec; i += kThreads) {
        uint32_t w[8];
        ref_window<VEC>(w, rrow, i, nw, a.xor80);
        int I[16], Q[16];
#pragma unroll
        for (int s = 0; s < 16; ++s) { I[s] = sext8(w[s >> 1], 2 * (s & 1)); Q[s] = sext8(w[s >> 1], 2 * (s & 1) + 1); }
        // sample n = 8 i + k: r_j[n] = r[n - j] is window sample 4 + k - j; with index = tap + 4 that is 8 + k - index
#pragma unroll
        for (int k = 0; k < 8; ++k)
#pragma unroll
            for (int i9 = 0; i9 < MAX_TAPS; ++i9)
#pragma unroll
                for (int j9 = i9; j9 < MAX_TAPS; ++j9) {
                    const int x = 8 + k - i9, y = 8 + k - j9, v = 2 * gram_index(i9, j9);
                    acc[v] += I[x] * I[y] + Q[x] * Q[y];          // conj(r_i) r_j
                    acc[v + 1] += I[x] * Q[y] - Q[x] * I[y];
                }
    }
#pragma unroll
    for (int v = 0; v < GRAM_INTS; ++v) {
        const int s = wave_sum_lane63(acc[v]);
        if ((tid & 63) == 63) sred[tid >> 6][v] = s;
    }
    __syncthreads();
    if (tid < GRAM_INTS) {
        int s = 0;
        for (int wv = 0; wv < kThreads / 64; ++wv) s += sred[wv][tid];
        sg[tid] = s;
        a.gram[(size_t)t * GRAM_INTS + tid] = s;
    }
    __syncthreads();
    if (tid == 0) {
        const bool ok = chol_factor(sg, a.taps, sL);
        a.block_status[t] = ok ? 0 : STATUS_SINGULAR;
    }
    __syncthreads();
    if (tid < GRAM_PAIRS) a.chol[(size_t)t * GRAM_PAIRS + tid] = sL[tid];     // (entries beyond the factor's taps are never read)
}

template <int TAPS, bool VEC>
__global__ __launch_bounds__(kThreads) void k_refcancel_dots(CancelArgs a)
{
    constexpr int K = (TAPS - 1) / 2, NV = 2 * TAPS + 1;
    __shared__ int sred[kThreads / 64][NV];
    const int tid = threadIdx.x, t = blockIdx.y;
    const int row = a.row_begin + (int)blockIdx.x;
    const int B = a.B, L = B >> 1, nvec = B / 16, nw = B / 4;
    const int8_t *blk = a.rows + (size_t)t * a.block_stride;
    const int8_t *srow = blk + (size_t)row * B;
    const size_t o = (size_t)t * a.nrows + row;
    const int d = clamp_lag(a.lag[o], L);
    int re[TAPS], cr[TAPS], nq[TAPS], E = 0;
#pragma unroll
    for (int j = 0; j < TAPS; ++j) re[j] = cr[j] = nq[j] = 0;
    for (int i = tid; i < nvec; i += kThreads) {
        const uint4 sv = row_vec<VEC>(srow, i, nvec, d, L, a.xor80);
        const uint32_t s[4] = {sv.x, sv.y, sv.z, sv.w};
        uint32_t w[8], od[7];
        ref_window<VEC>(w, blk, i, nw, a.xor80);
        // the reference word under signal word q for tap j starts at window sample 4 + 2 q - j: an even start is a window word, an odd
        // one the two-byte alignment of two neighbours
#pragma unroll
        for (int q = 0; q < 7; ++q) od[q] = __builtin_amdgcn_alignbyte(w[q + 1], w[q], 2);
#pragma unroll
        for (int q = 0; q < 4; ++q) E = __builtin_amdgcn_sdot4((int)s[q], (int)s[q], E, false);
#pragma unroll
        for (int jj = 0; jj < TAPS; ++jj)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int m = 2 * q - (jj - K);
                const uint32_t rw = (m & 1) ? od[2 + (m - 1) / 2] : w[2 + m / 2];
                dot_word3(s[q], rw, re[jj], cr[jj], nq[jj]);
            }
    }
    // c_j = (re, cr - 2 nq) and E, summed over the workgroup: each below 2^29 in magnitude, exact in int32
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        const int x = v == 2 * TAPS ? E : ((v & 1) ? cr[v >> 1] - 2 * nq[v >> 1] : re[v >> 1]);
        const int s = wave_sum_lane63(x);
        if ((tid & 63) == 63) sred[tid >> 6][v] = s;
    }
    __syncthreads();
    if (tid == 0) {
        cd c[TAPS], y[TAPS], g[TAPS];
        for (int j = 0; j < TAPS; ++j) {
            long long sr = 0, si = 0;
            for (int wv = 0; wv < kThreads / 64; ++wv) { sr += sred[wv][2 * j]; si += sred[wv][2 * j + 1]; }
            c[j] = y[j] = cd{(double)sr, (double)si};
            g[j] = cd{0.0, 0.0};
        }
        long long e = 0;
        for (int wv = 0; wv < kThreads / 64; ++wv) e += sred[wv][2 * TAPS];
        const int st = a.block_status[t];
        if (!st) chol_solve(a.chol + (size_t)t * GRAM_PAIRS, TAPS, y, g);
        float2 *co = a.coef + o * (size_t)a.coef_pitch;
        for (int j = 0; j < TAPS; ++j) co[j] = make_float2((float)g[j].re, (float)g[j].im);
        a.residual[o] = (float)residual_share((double)e, g, c, TAPS);
        a.status[o] = st;
    }
}

// clip(rint(v), -128, 127) + 128 into byte BYTE of `out`: the magic-constant round-half-even and v_cvt_pk_u8_f32 of rotq_word.  The
// constant needs |v| < 2^22, and the coefficients are the caller's in the per-op call: v is clamped to +-256 first (no byte changes).
template <int BYTE>
__device__ __forceinline__ void quant_byte(uint32_t &out, float v)
{
    v = __builtin_amdgcn_fmed3f(v, -256.0f, 256.0f);
    const float u = (v + 12582912.0f) - 12582784.0f;
    if (BYTE == 0) asm("v_cvt_pk_u8_f32 %0, %1, 0, %1" : "=v"(out) : "v"(u));
    else asm("v_cvt_pk_u8_f32 %0, %1, %2, %0" : "+v"(out) : "v"(u), "n"(BYTE));
}

template <int TAPS, bool VEC>
__global__ __launch_bounds__(kThreads) void k_refcancel_apply(CancelArgs a)
{
    constexpr int K = (TAPS - 1) / 2;
    const int tid = threadIdx.x, t = blockIdx.y;
    const int row = a.row_begin + (int)blockIdx.x;
    const int B = a.B, L = B >> 1, nvec = B / 16, nw = B / 4;
    const int8_t *blk = a.rows + (size_t)t * a.block_stride;
    const int8_t *srow = blk + (size_t)row * B;
    int8_t *orow = a.orows + (size_t)t * a.orows_stride + (size_t)(row - a.orow_first) * B;
    const size_t o = (size_t)t * a.nrows + row;
    const int d = clamp_lag(a.lag[o], L);
    const float2 p = a.phasor[o];
    float2 g[TAPS];
#pragma unroll
    for (int j = 0; j < TAPS; ++j) g[j] = a.coef[o * (size_t)a.coef_pitch + j];
    for (int i = tid; i < nvec; i += kThreads) {
        const uint4 sv = row_vec<VEC>(srow, i, nvec, d, L, a.xor80);
        const uint32_t s[4] = {sv.x, sv.y, sv.z, sv.w};
        uint32_t w[8];
        ref_window<VEC>(w, blk, i, nw, a.xor80);
        float rI[16], rQ[16];                              // window samples 4 - K .. 11 + K, each converted once
#pragma unroll
        for (int x = 4 - K; x < 12 + K; ++x) { rI[x] = (float)sext8(w[x >> 1], 2 * (x & 1)); rQ[x] = (float)sext8(w[x >> 1], 2 * (x & 1) + 1); }
        uint32_t ow[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int k = 2 * q + h;
                float zr = (float)sext8(s[q], 2 * h), zi = (float)sext8(s[q], 2 * h + 1);
#pragma unroll
                for (int jj = 0; jj < TAPS; ++jj) {        // z -= g_j r[n - j]
                    const int x = 4 + k - (jj - K);
                    zr = fmaf(-g[jj].x, rI[x], zr); zr = fmaf(g[jj].y, rQ[x], zr);
                    zi = fmaf(-g[jj].x, rQ[x], zi); zi = fmaf(-g[jj].y, rI[x], zi);
                }
                const float wr = fmaf(-p.y, zi, p.x * zr), wi = fmaf(p.y, zr, p.x * zi);
                if (h == 0) { quant_byte<0>(ow[q], wr); quant_byte<1>(ow[q], wi); }
                else { quant_byte<2>(ow[q], wr); quant_byte<3>(ow[q], wi); }
            }
            ow[q] ^= 0x80808080u;
        }
        if constexpr (VEC) reinterpret_cast<uint4 *>(orow)[i] = make_uint4(ow[0], ow[1], ow[2], ow[3]);
        else {
            uint32_t *o32 = reinterpret_cast<uint32_t *>(orow) + 4 * i;
            o32[0] = ow[0]; o32[1] = ow[1]; o32[2] = ow[2]; o32[3] = ow[3];
        }
    }
}

// a batch the pass does not run for (submitted without CRSDR_REFNOISE_ENABLED): status 2, g = 0, residual 1 for the owned rows
__global__ void k_refcancel_idle(CancelArgs a, int row_count)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x, t = blockIdx.y;
    if (i >= row_count) return;
    const size_t o = (size_t)t * a.nrows + a.row_begin + i;
    for (int j = 0; j < a.coef_pitch; ++j) a.coef[o * (size_t)a.coef_pitch + j] = make_float2(0.0f, 0.0f);
    a.residual[o] = 1.0f;
    a.status[o] = STATUS_IDLE;
}

// row 0 of the per-op call's output: the reference row as the packets carry it (two's complement)
__global__ void k_refcancel_row0(uint32_t *__restrict__ out, const uint32_t *__restrict__ in, int nwords, uint32_t xor80)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nwords) out[i] = in[i] ^ xor80;
}

template <int TAPS>
static hipError_t launch_rows(hipStream_t s, const CancelArgs &a, int row_count, int nblocks, bool vec)
{
    const dim3 grid((unsigned)row_count, (unsigned)nblocks), block(kThreads);
    if (vec) hipLaunchKernelGGL((k_refcancel_dots<TAPS, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((k_refcancel_dots<TAPS, false>), grid, block, 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (vec) hipLaunchKernelGGL((k_refcancel_apply<TAPS, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((k_refcancel_apply<TAPS, false>), grid, block, 0, s, a);
    return hipGetLastError();
}

// the three kernels for rows row_begin .. row_begin + row_count - 1 of nblocks blocks; vec: every row, input and output, 16-byte aligned
static hipError_t launch_refcancel(hipStream_t s, const CancelArgs &a, int row_count, int nblocks, bool vec)
{
    if (vec) hipLaunchKernelGGL(k_refcancel_gram<true>, dim3((unsigned)nblocks), dim3(kThreads), 0, s, a);
    else hipLaunchKernelGGL(k_refcancel_gram<false>, dim3((unsigned)nblocks), dim3(kThreads), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    switch (a.taps) {
    case 1: return launch_rows<1>(s, a, row_count, nblocks, vec);
    case 3: return launch_rows<3>(s, a, row_count, nblocks, vec);
    case 5: return launch_rows<5>(s, a, row_count, nblocks, vec);
    case 7: return launch_rows<7>(s, a, row_count, nblocks, vec);
    case 9: return launch_rows<9>(s, a, row_count, nblocks, vec);
    default: return hipErrorInvalidValue;
    }
}

} // namespace rc
} // namespace crsdr
