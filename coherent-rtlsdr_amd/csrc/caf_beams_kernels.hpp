// caf_beams_kernels.hpp -- the two kernels of crsdr_caf's coherent beam maps (include/crsdr.h, section (w), "Beams"; the decisions
// themselves are caf_beams.hpp's).  With the detector's two between them: four launches whatever the batch size.
//
//   k_caf_beams      grid (ceil(cells / 128), line), 256 threads: a wave owns 32 consecutive cells of the line and forms every beam's
//                    sum at them on the fp32 matrix pipe.  One v_mfma_f32_32x32x2_f32 has K = 2, one element's (re, im): its B operand
//                    is one float a lane, lanes 0 .. 31 the re and lanes 32 .. 63 the im of the 32 cells -- together one coalesced
//                    256-byte read straight from chi's interleaved layout, no LDS staging.  Its A operand is, for the real parts of
//                    32 beams, (wr, -wi) over k, and for the imaginary parts (wi, wr): lane (beam, k) reads the beam's (wr, wi) of the
//                    element from an LDS table [m][32 NG] float2 (at most 32 KiB, built once per workgroup from the weights) and
//                    picks its two values with two selects.  Two MFMAs per element and group of 32 beams; the second group
//                    (NG = 2, nbeams > 32) reuses the B registers.  Eight elements' loads are in flight together: whole chunks of eight run
//                    without a condition, and the tail's loads are pinned ahead of its uniform branches.  The result is
//                    bit for bit the chain of bm::beam_sum, whatever the tile: a line has its bits wherever it sits.  The tail of
//                    `cells` is masked on the load (zeros) and on the store.  Epilogue: the fp64 square in the accumulators' layout
//                    (a lane holds 16 beams of one cell: row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)), one rounding, and stores
//                    that are 128-byte runs along the cells of a beam's map.
//   k_caf_beam_fuse  grid (line), 256 threads: the candidates of every beam's list into LDS (their places come from a prefix sum over
//                    the beams' counts, no atomics), suppression and rank by counting under bm::before, a strict total order, and
//                    the first K survivors' records.  At most 64 x 64 candidates, 48 KiB.
// Nothing depends on the order in which workgroups or atomics arrive, and nothing in a line on another line.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "caf_beams.hpp"

namespace crsdr {
namespace caf_beams {

constexpr int THREADS = 256, WAVE_CELLS = 32, WG_CELLS = (THREADS / 64) * WAVE_CELLS, INFLIGHT = 8;
typedef float acc16 __attribute__((ext_vector_type(16)));

__host__ __device__ constexpr int groups_of(int nbeams) { return (nbeams + bm::GROUP - 1) / bm::GROUP; }
__host__ __device__ constexpr size_t table_bytes(int m, int nbeams) { return sizeof(float2) * (size_t)m * (size_t)(groups_of(nbeams) * bm::GROUP); }

// element e into the accumulators of the wave's 32 cells: x is the lane's B operand, A[beam][k] is (wr, -wi) for re z and (wi, wr) for im z
template <int NG>
__device__ inline void beam_step(const float2 *tab, int e, int col, int k, float x, acc16 *re, acc16 *im)
{
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        const float2 t = tab[e * (NG * bm::GROUP) + g * bm::GROUP + col];
        const float are = k ? -t.y : t.x, aim = k ? t.x : t.y;
        re[g] = __builtin_amdgcn_mfma_f32_32x32x2f32(are, x, re[g], 0, 0, 0);
        im[g] = __builtin_amdgcn_mfma_f32_32x32x2f32(aim, x, im[g], 0, 0, 0);
    }
}

// chi [nest][nrows][cells] float2, w [nbeams][m][2] of line 0 and wstride floats from line to line (0: one set for every line;
// nbeams m 2: the adaptive weights of caf_adapt_kernels.hpp), bmap [nest][nbeams][cells]
template <int NG>
__global__ __launch_bounds__(THREADS) void k_caf_beams(const float2 *__restrict__ chi, const float *__restrict__ w0, size_t wstride, int nrows, int cells, int ref_row,
                                                       int nbeams, float *__restrict__ bmap)
{
    extern __shared__ float2 tab[];                                              // [m][32 NG]: (wr, wi) of beam b at element e; zeros past nbeams
    constexpr int NB = NG * bm::GROUP;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, m = nrows - 1, e_line = blockIdx.y;
    const float *w = w0 + (size_t)e_line * wstride;
    for (int x = tid; x < m * NB; x += THREADS) {
        const int e = x / NB, b = x - e * NB;
        tab[x] = b < nbeams ? make_float2(w[2 * ((size_t)b * m + e)], w[2 * ((size_t)b * m + e) + 1]) : make_float2(0.f, 0.f);
    }
    __syncthreads();

    const int col = lane & 31, k = lane >> 5, cell = blockIdx.x * WG_CELLS + wave * WAVE_CELLS + col;
    const bool in = cell < cells;
    // the lane's float of element e: re (k = 0) or im (k = 1) of its cell; cell 0 where the cell is past the end, and a zero chosen behind it
    const float *src = reinterpret_cast<const float *>(chi + (size_t)e_line * nrows * cells) + 2 * (size_t)(in ? cell : 0) + k;
    acc16 re[NG], im[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g)
#pragma unroll
        for (int r = 0; r < 16; ++r) { re[g][r] = 0.f; im[g][r] = 0.f; }

    // whole chunks: INFLIGHT loads issued together, nothing conditional between them and the MFMAs
    const int whole = m - m % INFLIGHT;
    for (int e0 = 0; e0 < whole; e0 += INFLIGHT) {
        float v[INFLIGHT];
#pragma unroll
        for (int u = 0; u < INFLIGHT; ++u) v[u] = src[2 * (size_t)brg::row_of(e0 + u, ref_row) * cells];
#pragma unroll
        for (int u = 0; u < INFLIGHT; ++u) beam_step<NG>(tab, e0 + u, col, k, in ? v[u] : 0.f, re, im);
    }
    // the tail: its loads are issued together as well (past m: element m - 1 again, not used) and pinned ahead of the uniform
    // branches, into which the compiler would otherwise sink each one beside its use
    if (whole < m) {
        float v[INFLIGHT];
#pragma unroll
        for (int u = 0; u < INFLIGHT; ++u) v[u] = src[2 * (size_t)brg::row_of(min(whole + u, m - 1), ref_row) * cells];
#pragma unroll
        for (int u = 0; u < INFLIGHT; ++u) asm volatile("" : "+v"(v[u]));
#pragma unroll
        for (int u = 0; u < INFLIGHT; ++u) {
            if (whole + u >= m) break;                                           // (the same for every lane)
            beam_step<NG>(tab, whole + u, col, k, in ? v[u] : 0.f, re, im);
        }
    }

    if (!in) return;
    float *out = bmap + (size_t)e_line * nbeams * cells + cell;
#pragma unroll
    for (int g = 0; g < NG; ++g)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int b = g * bm::GROUP + (r & 3) + 8 * (r >> 2) + 4 * k;
            if (b < nbeams) out[(size_t)b * cells] = bm::power(re[g][r], im[g][r]);
        }
}

// bdet [nest][nbeams][K][8], bcount [nest][nbeams] -> fused [nest][K][8], nfused [nest]
__global__ __launch_bounds__(THREADS) void k_caf_beam_fuse(const float *__restrict__ bdet, const int32_t *__restrict__ bcount, int nbeams, int K, int nd, int R,
                                                           float *__restrict__ fused, int32_t *__restrict__ nfused)
{
    __shared__ bm::Cand list[bm::MAX_CAND];
    __shared__ int first[bm::MAX_BEAMS + 1];
    __shared__ int total[THREADS];
    const int tid = threadIdx.x, line = blockIdx.x;
    const float *det = bdet + (size_t)line * nbeams * K * 8;
    const int32_t *cnt = bcount + (size_t)line * nbeams;

    if (tid == 0) {
        int at = 0;
        for (int b = 0; b < nbeams; ++b) { first[b] = at; at += bm::live_slots(cnt[b], K); }
        first[nbeams] = at;
    }
    __syncthreads();
    const int n = first[nbeams];
    // (a slot that names no cell of the map keeps its place with i < 0: it is no candidate, and the places depend on the counts alone)
    for (int x = tid; x < nbeams * K; x += THREADS) {
        const int b = x / K, q = x - b * K;
        if (q < first[b + 1] - first[b]) list[first[b] + q] = bm::candidate(det + (size_t)x * 8, b, q, nd, R);
    }
    __syncthreads();

    // suppression: the candidate's i goes to -2 - i only behind the barrier, so that every thread reads the same list
    constexpr int PER = bm::MAX_CAND / THREADS;
    unsigned dead = 0;
    int mine = 0;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const int x = tid + j * THREADS;
        if (x >= n || list[x].i < 0) { dead |= 1u << j; continue; }
        if (bm::suppressed(list, n, x, nd, R)) dead |= 1u << j; else mine += 1;
    }
    total[tid] = mine;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const int x = tid + j * THREADS;
        if (x < n && (dead & (1u << j)) && list[x].i >= 0) list[x].i = -2 - list[x].i;
    }
    for (int h = THREADS / 2; h >= 1; h >>= 1) {
        if (tid < h) total[tid] += total[tid + h];
        __syncthreads();
    }
    const int nf = total[0];

    float *out = fused + (size_t)line * K * 8;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const int x = tid + j * THREADS;
        if (x >= n || (dead & (1u << j))) continue;
        const bm::Cand c = list[x];
        int rank = 0;
        for (int y = 0; y < n; ++y) rank += list[y].i >= 0 && bm::before(list[y], c) ? 1 : 0;
        if (rank < K) bm::record(det + ((size_t)bm::beam_of(c) * K + bm::slot_of(c)) * 8, bm::beam_of(c), out + (size_t)rank * 8);
    }
    for (int x = min(nf, K) * 8 + tid; x < K * 8; x += THREADS) out[x] = 0.f;
    if (tid == 0) nfused[line] = nf;
}

} // namespace caf_beams
} // namespace crsdr
