// spectra.hpp -- Welch auto-spectra, cross-spectra against row 0 and the alignment figures: crsdr_spectra / crsdr_welch.
//
// Definition (tests/spectra_model.py is the fp64 statement of it).  Row c of a packet's matrix [nrows][B] int8 holds L = B / 2 samples
// x_c[n] = (I + jQ) / 127, row 0 (the reference channel) included.  N = nfft, hop H = N (overlap 0) or N / 2 (overlap 1); a packet has
// J = (L - N) / H + 1 segments, segment j from sample jH on, never across packets; a line is `frames` consecutive packets, J' = frames J.
//     X_c[t][j][f] = sum_n w[n] x_c[jH + n] exp(-2 pi i f n / N)
//     P_c[f] = 1 / (J' N sum w^2) * sum_{t,j} |X_c[t][j][f]|^2
//     S_c[f] = 1 / (J' N sum w^2) * sum_{t,j} conj(X_0[t][j][f]) X_c[t][j][f]            S_0[f] = (P_0[f], 0)
// No mean is removed.  The alignment figures: spectra_align.hpp.
//
//   k_spectra_tables   tw[t] = W_N^t and the window, computed in fp64 and rounded once: at create, not per submit.
//   k_spectra<LG, 1>   grid (chunk, packet): the reference row's segment spectra, ref [nblocks][J][N] cf32 in slot order -- the
//                      project's K0 / K1 idiom: the row every other row is held against is transformed once.
//   k_spectra<LG, 0>   grid (row, line), 256 threads, ONE row per workgroup.  Per chunk of up to 4096 / N segments: 16-byte loads of the
//                      int8 row (4-byte aligned is enough: cov_load16), window, the N-point transform in LDS (fft_lds.hpp butterflies:
//                      radix 16, the remainder last), then every thread adds |X|^2 and conj(X_0) X of its slots into three fp32 sums per
//                      slot, the reference spectrum read from ref (coalesced, L2).  A thread owns slots tid + 256 k (N >= 256: N / 256
//                      slots, 48 floats at N = 4096) or slot tid mod N of lane tid / N (N < 256: 256 / N lanes take a chunk's segments
//                      round robin).  After SP_CHAIN segments per lane the fp32 sums are added into fp64 registers and start again:
//                      an fp32 chain is at most SP_CHAIN = 32 terms long, and where it is cut depends on (B, N, overlap) alone.  The
//                      fp64 sums go on over the packets of the line; at the end the lanes are added in lane order, the scale is
//                      applied in fp64 and psd / cross are rounded once and written at their bins.  No partials in memory, no reducer,
//                      no atomics: a line's bits depend on its own packets alone.
//   k_spectra_align    grid (row, line), one wave: spectra_align.hpp's sums, one part per lane, added by an xor butterfly.
//
// Transform: the decimation-in-frequency network of fft_lds.hpp, in place, so bin f ends in slot j with f = digit_reverse(j) (FftGeom);
// the reference and the row run the same network, so slot meets slot, and only the last write maps slots to bins.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "covariance.hpp"
#include "fft_lds.hpp"
#include "spectra_align.hpp"
#include "subband.hpp"

namespace crsdr {
namespace spectra {

constexpr int SP_THREADS = 256, SP_POINTS = 4096, SP_CHAIN = 32;
constexpr int SP_MIN_LOG2 = 4, SP_MAX_LOG2 = 12;
// A chunk's points in LDS, one float2 of padding behind every 16: a thread of the last pass owns 16 consecutive points, and without
// the padding the 32 lanes of a half wave meet on two of the 32 eight-byte bank pairs (stride 128 bytes); with it the stride is 136.
// Not at N = 4096: there the chunk and the twiddle table fill the 64 KiB of static LDS exactly, and a variant that made room by keeping
// half the table ran a third slower than the unpadded kernel: its workgroup is alone on its CU at 256 VGPRs either way.
template <int LOG2N>
__host__ __device__ constexpr int sp_pad(int p) { return LOG2N < SP_MAX_LOG2 ? p + (p >> 4) : p; }
template <int LOG2N>
constexpr int sp_lds_points() { return sp_pad<LOG2N>(SP_POINTS); }

__host__ __device__ constexpr int sp_hop(int N, int overlap) { return overlap ? N / 2 : N; }
__host__ __device__ constexpr int sp_segments(int B, int N, int overlap) { return (B / 2 - N) / sp_hop(N, overlap) + 1; }
// segments per chunk, lanes, and chunks per chain group (SP_CHAIN segments per lane)
__host__ __device__ constexpr int sp_spc(int N) { return SP_POINTS / N; }
__host__ __device__ constexpr int sp_lanes(int N) { return N < SP_THREADS ? SP_THREADS / N : 1; }
__host__ __device__ constexpr int sp_group_chunks(int N) { return SP_CHAIN * sp_lanes(N) / sp_spc(N); }

// grid ceil(N / 256)
__global__ __launch_bounds__(SP_THREADS) void k_spectra_tables(int N, int window, float2 *__restrict__ tw, float *__restrict__ win)
{
    const int t = blockIdx.x * SP_THREADS + threadIdx.x;
    if (t >= N) return;
    double s, c;
    sincospi(2.0 * (double)t / (double)N, &s, &c);
    tw[t] = make_float2((float)c, (float)-s);
    win[t] = window == subband::WINDOW_HANN ? (float)(0.5 - 0.5 * c) : 1.0f;
}

// pass P of the DIF network over the sc segments of a chunk at A: groups of R points at stride M, butterfly, then W_N^(n2 k 16^P)
template <int LOG2N, int P>
__device__ __forceinline__ void sp_pass(float2 *A, const float2 *tw, int sc, int tid)
{
    using G = FftGeom<LOG2N>;
    constexpr int LR = G::log2r(P), R = 1 << LR, LM = G::log2m(P), M = 1 << LM, LG_GROUPS = LOG2N - LR;
    for (int it = tid; it < (sc << LG_GROUPS); it += SP_THREADS) {
        const int seg = it >> LG_GROUPS, g = it & ((1 << LG_GROUPS) - 1), n2 = g & (M - 1);
        const int e0 = (seg << LOG2N) + ((g >> LM) << (LM + LR)) + n2;      // the group's first point; point i at e0 + i M
        float2 v[R];
#pragma unroll
        for (int i = 0; i < R; ++i) v[i] = A[sp_pad<LOG2N>(e0 + (i << LM))];
        dft<R, -1>(v);
        if constexpr (M > 1) {
#pragma unroll
            for (int k = 1; k < R; ++k) v[k] = cmul(v[k], tw[(n2 * k) << (4 * P)]);
        }
#pragma unroll
        for (int i = 0; i < R; ++i) A[sp_pad<LOG2N>(e0 + (i << LM))] = v[i];
    }
    __syncthreads();
    if constexpr (P + 1 < G::NPASS) sp_pass<LOG2N, P + 1>(A, tw, sc, tid);
}

// segments j0 .. j0 + sc - 1 of the row at `row` -> their spectra in A (point p at sp_pad<LOG2N>(p)), slot order; a barrier ends it
template <int LOG2N>
__device__ __forceinline__ void sp_chunk(const int8_t *row, int H, int j0, int sc, const float *__restrict__ win, const float2 *tw, float2 *A, int tid)
{
    constexpr int N = 1 << LOG2N, LP = LOG2N - 3;            // 2^LP pieces of 16 bytes = 8 samples per segment
    for (int it = tid; it < (sc << LP); it += SP_THREADS) {
        const int jj = it >> LP, n0 = (it & ((1 << LP) - 1)) * 8;
        const uint4 wd = cov::cov_load16(row + ((size_t)(j0 + jj) * H + n0) * 2);
        subband::sb_unpack_window(wd, win, n0, A + sp_pad<LOG2N>(jj * N + n0));      // (eight points from a multiple of 8 on: no padding among them)
    }
    __syncthreads();
    sp_pass<LOG2N, 0>(A, tw, sc, tid);
}

// Packet t of the batch at packets + t * packet_stride, its matrix [nrows][B] int8 at + matrix_off (4-byte aligned).
//   REF: grid (chunks of a packet, nblocks)  -> ref [nblocks][J][N] float2, slot order
//   else grid (nrows, nest); line e = packets e * frames .. + frames - 1 -> psd [nest][nrows][N], cross [nest][nrows][N] float2, bin order
template <int LOG2N, bool REF>
__global__ __launch_bounds__(SP_THREADS) void k_spectra(const int8_t *__restrict__ packets, size_t packet_stride, size_t matrix_off, int nrows, int B, int frames,
                                                        int overlap, int window, const float2 *__restrict__ tw_g, const float *__restrict__ win,
                                                        float2 *__restrict__ ref, float *__restrict__ psd, float2 *__restrict__ cross)
{
    constexpr int N = 1 << LOG2N, SPC = sp_spc(N), NL = sp_lanes(N), SLOTS = N >= SP_THREADS ? N / SP_THREADS : 1, CPG = sp_group_chunks(N);
    __shared__ float2 A[sp_lds_points<LOG2N>()];
    __shared__ float2 tw[N];
    const int tid = threadIdx.x, H = sp_hop(N, overlap), J = sp_segments(B, N, overlap);
    for (int t = tid; t < N; t += SP_THREADS) tw[t] = tw_g[t];      // (sp_chunk's first barrier is ahead of its first use)

    if constexpr (REF) {
        const int j0 = blockIdx.x * SPC, sc = min(SPC, J - j0), t = blockIdx.y;
        sp_chunk<LOG2N>(packets + (size_t)t * packet_stride + matrix_off, H, j0, sc, win, tw, A, tid);
        float2 *out = ref + ((size_t)t * J + j0) * N;
        for (int it = tid; it < sc * N; it += SP_THREADS) out[it] = A[sp_pad<LOG2N>(it)];
    } else {
        const int row = blockIdx.x, e = blockIdx.y, lane = tid >> (LOG2N < 8 ? LOG2N : 8), slot0 = tid & (N - 1), nchunks = (J + SPC - 1) / SPC;
        double dp[SLOTS], dr[SLOTS], di[SLOTS];
#pragma unroll
        for (int k = 0; k < SLOTS; ++k) dp[k] = dr[k] = di[k] = 0.0;
        for (int f = 0; f < frames; ++f) {
            const int t = e * frames + f;
            const int8_t *rowp = packets + (size_t)t * packet_stride + matrix_off + (size_t)row * B;
            const float2 *reft = ref + (size_t)t * J * N;
            float fp[SLOTS], fr[SLOTS], fi[SLOTS];
#pragma unroll
            for (int k = 0; k < SLOTS; ++k) fp[k] = fr[k] = fi[k] = 0.f;
            for (int q = 0; q < nchunks; ++q) {
                const int j0 = q * SPC, sc = min(SPC, J - j0);
                sp_chunk<LOG2N>(rowp, H, j0, sc, win, tw, A, tid);
#pragma unroll 4
                for (int jj = lane; jj < sc; jj += NL) {         // (unrolled: the reference loads of four segments are in flight together)
#pragma unroll
                    for (int k = 0; k < SLOTS; ++k) {
                        const int slot = slot0 + k * SP_THREADS;
                        const float2 x = A[sp_pad<LOG2N>(jj * N + slot)], r = reft[(size_t)(j0 + jj) * N + slot];
                        fp[k] = fmaf(x.y, x.y, fmaf(x.x, x.x, fp[k]));
                        fr[k] = fmaf(r.y, x.y, fmaf(r.x, x.x, fr[k]));      // conj(r) x
                        fi[k] = fmaf(-r.y, x.x, fmaf(r.x, x.y, fi[k]));
                    }
                }
                __syncthreads();
                if ((q + 1) % CPG == 0 || q + 1 == nchunks) {               // the end of an fp32 chain
#pragma unroll
                    for (int k = 0; k < SLOTS; ++k) {
                        dp[k] += (double)fp[k]; dr[k] += (double)fr[k]; di[k] += (double)fi[k];
                        fp[k] = fr[k] = fi[k] = 0.f;
                    }
                }
            }
        }
        if constexpr (NL > 1) {                  // the lanes' sums, in lane order
            double *D = reinterpret_cast<double *>(A);
            D[tid * 3] = dp[0]; D[tid * 3 + 1] = dr[0]; D[tid * 3 + 2] = di[0];
            __syncthreads();
            if (lane != 0) return;
            for (int l = 1; l < NL; ++l) { dp[0] += D[(l * N + slot0) * 3]; dr[0] += D[(l * N + slot0) * 3 + 1]; di[0] += D[(l * N + slot0) * 3 + 2]; }
        }
        // sum w^2: N (rect), 3 N / 8 (periodic Hann, N >= 4)
        const double sw2 = window == subband::WINDOW_HANN ? 0.375 * (double)N : (double)N;
        const double scale = 1.0 / (127.0 * 127.0 * (double)frames * (double)J * (double)N * sw2);
        const size_t o = ((size_t)e * nrows + row) * N;
#pragma unroll
        for (int k = 0; k < SLOTS; ++k) {
            const int bin = digit_reverse<LOG2N>(slot0 + k * SP_THREADS);
            const float p = (float)(dp[k] * scale);
            psd[o + bin] = p;
            cross[o + bin] = row == 0 ? make_float2(p, 0.f) : make_float2((float)(dr[k] * scale), (float)(di[k] * scale));
        }
    }
}

__device__ __forceinline__ double sp_wave_sum(double v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// grid (nrows, nest), 64 threads.  align [nest][nrows][4] = (delay, phase, gain, coherence) over the signed bins lo .. lo + K - 1
__global__ __launch_bounds__(64) void k_spectra_align(const float *__restrict__ psd, const float2 *__restrict__ cross, int nrows, int N, int lo, int K,
                                                      float *__restrict__ align)
{
    const int row = blockIdx.x, e = blockIdx.y, l = threadIdx.x;
    const float *p0 = psd + (size_t)e * nrows * N, *pc = p0 + (size_t)row * N;
    const float *sc = reinterpret_cast<const float *>(cross + ((size_t)e * nrows + row) * N);
    spa::Lag a = spa::lag_part(sc, N, lo, K, l, 64);
    a.re = sp_wave_sum(a.re); a.im = sp_wave_sum(a.im);
    const double delay = spa::delay_of(a, N);
    spa::Sums t = spa::sums_part(p0, pc, sc, N, lo, K, delay, l, 64);
    t.zre = sp_wave_sum(t.zre); t.zim = sp_wave_sum(t.zim); t.p0 = sp_wave_sum(t.p0); t.ss = sp_wave_sum(t.ss); t.pp = sp_wave_sum(t.pp);
    if (l == 0) spa::figures(delay, t, align + ((size_t)e * nrows + row) * 4);
}

} // namespace spectra
} // namespace crsdr
