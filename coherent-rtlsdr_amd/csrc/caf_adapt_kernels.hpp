// caf_adapt_kernels.hpp -- the two kernels of crsdr_caf's adaptive beams (include/crsdr.h, section (w), "Adaptive beams"; the decisions
// themselves are caf_adapt.hpp's).  Two launches whatever the batch size, ahead of k_caf_beams, which then reads a line's own weights.
//
//   k_caf_beam_cov    grid (tile of training cells, line), 256 threads.  A tile is tile_chunks(N) chunks of 64 cells.  Per chunk the
//                     workgroup brings its cells of the m rows into LDS as u = conj(chi): thread (e mod 4, c) reads cell c of rows
//                     e, e + 4, ..: a wave reads 64 consecutive training cells of one row, runs of r_n float2 along the lags.  The
//                     image is [16 ceil(m / 16)][132] floats: (re u, im u) of cell c at floats 2 c, 2 c + 1 of its row; rows past m are
//                     zeros, written once, and cells past the tile's end are zeros: the tails are masked on the operand.  The 16 x 16
//                     blocks (bi, bj), bj <= bi, of Q's lower triangle are dealt to the four waves in turn (at most 10 blocks, three a
//                     wave).  One v_mfma_f64_16x16x4_f64 has K = 4 = (re, im) of two cells; lane (r = lane & 15, k = lane >> 4) reads
//                     float 4 step + k of row 16 b + r -- a row stride of 132 floats puts the 64 lanes on 64 different banks.  Re Q_ij
//                     takes A = (ur_i, ui_i), Im Q_ij takes A = (ui_i, -ur_i), both with B = (ur_j, ui_j): one B operand for two
//                     MFMAs.  Every product of two fp32 values is exact in fp64.  Epilogue: the f64 form's C/D layout (col = lane & 15,
//                     row = (lane >> 4) + 4 reg), entries with col <= row < m to part [line][tile][pair] as double2, plain vector
//                     stores, no atomics; Im of the diagonal is written as 0.
//   k_caf_beam_adapt  grid (line), 256 threads: the tiles summed in ascending order, the trace, the loading, the factor and its inverse
//                     in LDS (two packed triangles, the beams' vectors and the figures' terms: 82 960 bytes, 81 KiB, at m = 64, above
//                     the default dynamic limit, which caf_lds_limits raises), the unloaded Q summed again into the factor's triangle
//                     once the inverse stands, then
//                     four beams a pass, a thread per (beam, element): y = Li v, g = Li^H y, the scaling, the rounding, the figures.
//                     A line that falls back copies the caller's weights and leaves.
// Nothing depends on the order in which workgroups arrive, and nothing in a line on another line.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "caf_adapt.hpp"

namespace crsdr {
namespace caf_adapt {

constexpr int THREADS = 256, WAVES = THREADS / 64, ROW_FLOATS = 2 * ad::CHUNK + 4, MAX_OWN = 3, PASS_BEAMS = THREADS / 64;
typedef double acc4 __attribute__((ext_vector_type(4)));

__host__ __device__ constexpr size_t align16(size_t n) { return (n + 15) & ~(size_t)15; }
__host__ __device__ constexpr size_t tri_bytes(int m) { return align16(sizeof(brg::cd) * (size_t)(m * (m + 1) / 2)); }
// two triangles, V, Y, G [PASS_BEAMS][m], the figures' terms [2][PASS_BEAMS][m], the factor's scalars
__host__ __device__ constexpr size_t adapt_lds_bytes(int m)
{
    return 2 * tri_bytes(m) + 3 * sizeof(brg::cd) * (size_t)(PASS_BEAMS * m) + 2 * sizeof(double) * (size_t)(PASS_BEAMS * m) + 16;
}

// chi [nest][nrows][nd R] float2 -> part [nest][tiles][m (m + 1) / 2] double2
__global__ __launch_bounds__(THREADS) void k_caf_beam_cov(const float2 *__restrict__ chi, int nrows, int nd, int R, int ref_row, ad::Params prm,
                                                          double2 *__restrict__ part)
{
    __shared__ __attribute__((aligned(16))) float img[ad::MAX_M * ROW_FLOATS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, m = nrows - 1, mb = (m + 15) / 16, nblk = mb * (mb + 1) / 2;
    const int N = ad::cells_of(prm), tc = ad::tile_cells(N), tile = blockIdx.x, line = blockIdx.y, tiles = gridDim.x;
    const int t_begin = tile * tc, t_end = t_begin + tc < N ? t_begin + tc : N;
    const size_t cells = (size_t)nd * (size_t)R;
    const float2 *X = chi + (size_t)line * nrows * cells;

    for (int x = m * ROW_FLOATS + tid; x < 16 * mb * ROW_FLOATS; x += THREADS) img[x] = 0.f;      // the rows past m, once

    int bi[MAX_OWN], bj[MAX_OWN];
    acc4 re[MAX_OWN], im[MAX_OWN];
#pragma unroll
    for (int s = 0; s < MAX_OWN; ++s) {
        const int q = wave + WAVES * s;
        brg::pair_of(q < nblk ? q : 0, &bi[s], &bj[s]);
#pragma unroll
        for (int r = 0; r < 4; ++r) { re[s][r] = 0.0; im[s][r] = 0.0; }
    }

    const int c = tid & 63, k = lane >> 4, r16 = lane & 15;
    for (int t0 = t_begin; t0 < t_end; t0 += ad::CHUNK) {
        __syncthreads();                                                         // the last chunk's readers are done
        const int t = t0 + c;
        const bool in = t < t_end;
        const size_t idx = (size_t)(in ? ad::cell_of(prm, nd, R, t) : 0);
        for (int e = tid >> 6; e < m; e += WAVES) {
            const float2 v = X[(size_t)brg::row_of(e, ref_row) * cells + idx];
            *reinterpret_cast<float2 *>(&img[e * ROW_FLOATS + 2 * c]) = in ? make_float2(v.x, -v.y) : make_float2(0.f, 0.f);
        }
        __syncthreads();
        const int left = t_end - t0, steps = ((left < ad::CHUNK ? left : ad::CHUNK) + 1) / 2;
        for (int step = 0; step < steps; ++step) {
            const int off = 4 * step + k, offp = 4 * step + (k ^ 1);
#pragma unroll
            for (int s = 0; s < MAX_OWN; ++s) {
                if (wave + WAVES * s >= nblk) break;                             // (the same for every lane of the wave)
                const float *ra = img + (16 * bi[s] + r16) * ROW_FLOATS;
                const double xa = (double)ra[off], ya = (double)ra[offp], xb = (double)img[(16 * bj[s] + r16) * ROW_FLOATS + off];
                re[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(xa, xb, re[s], 0, 0, 0);
                im[s] = __builtin_amdgcn_mfma_f64_16x16x4f64((k & 1) ? -ya : ya, xb, im[s], 0, 0, 0);
            }
        }
    }

    const int pairs = ad::pairs_of(m);
    double2 *out = part + ((size_t)line * tiles + tile) * pairs;
#pragma unroll
    for (int s = 0; s < MAX_OWN; ++s) {
        if (wave + WAVES * s >= nblk) break;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int I = 16 * bi[s] + (lane >> 4) + 4 * r, J = 16 * bj[s] + r16;
            if (I < m && J <= I) out[brg::chol_index(I, J)] = make_double2(re[s][r], I == J ? 0.0 : im[s][r]);
        }
    }
}

// part [nest][tiles][pairs] double2, w [nbeams][m][2] -> aw [nest][nbeams][m][2], ainfo [nest][nbeams][2], astat [nest]
__global__ __launch_bounds__(THREADS) void k_caf_beam_adapt(const double2 *__restrict__ part, const float *__restrict__ w, int m, int nbeams, ad::Params prm,
                                                            float *__restrict__ aw, float *__restrict__ ainfo, int32_t *__restrict__ astat)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char adapt_sm[];
    const int tid = threadIdx.x, line = blockIdx.x, pairs = ad::pairs_of(m), N = ad::cells_of(prm), tiles = ad::tiles_of(N);
    brg::cd *Lf = reinterpret_cast<brg::cd *>(adapt_sm);                                       // [pairs]: the sums, Q', its factor, then Q
    brg::cd *Li = reinterpret_cast<brg::cd *>(adapt_sm + tri_bytes(m));                        // [pairs]
    brg::cd *V = reinterpret_cast<brg::cd *>(adapt_sm + 2 * tri_bytes(m));                     // [PASS_BEAMS][m]
    brg::cd *Y = V + PASS_BEAMS * m, *G = Y + PASS_BEAMS * m;
    double *T = reinterpret_cast<double *>(G + PASS_BEAMS * m);                                // [2][PASS_BEAMS][m]
    double &inv_s = T[2 * PASS_BEAMS * m];
    int &bad = *reinterpret_cast<int *>(&inv_s + 1);
    const double *P = reinterpret_cast<const double *>(part + (size_t)line * tiles * pairs);
    float *lw = aw + (size_t)line * nbeams * m * 2, *li = ainfo + (size_t)line * nbeams * 2;

    for (int p = tid; p < pairs; p += THREADS) Lf[p] = ad::tile_sum(P, tiles, pairs, p);
    if (tid == 0) bad = 0;
    __syncthreads();
    const double tr = brg::trace_of(Lf, m);                                                    // (every thread the same sum)
    __syncthreads();                                                                           // read before the loading rewrites the diagonal
    int status = ad::trace_status(tr);
    if (!status) {
        for (int p = tid; p < pairs; p += THREADS) {
            int i, k;
            brg::pair_of(p, &i, &k);
            Lf[p] = brg::loaded_entry(Lf[p], i, k, N, tr, m, prm.loading);
        }
        __syncthreads();
        for (int k = 0; k < m; ++k) {                                                          // brg::factor, a column at a time
            if (tid == 0) {
                const double dv = cc::chol_pivot(Lf, Lf[brg::chol_index(k, k)].re, k);
                if (!(dv > 0.0)) bad = 1;
                const double lkk = sqrt(dv), inv = 1.0 / lkk;
                Lf[brg::chol_index(k, k)] = brg::cd{lkk, inv};
                inv_s = inv;
            }
            __syncthreads();
            if (bad) break;                                                                    // (the whole workgroup reads the same flag)
            for (int i = k + 1 + tid; i < m; i += THREADS) Lf[brg::chol_index(i, k)] = cc::chol_entry(Lf, Lf[brg::chol_index(i, k)], i, k, inv_s);
            __syncthreads();
        }
        if (bad) status = ad::STATUS_SOLVE;
    }
    if (status) {                                                                              // (workgroup-uniform) the caller's weights, bit for bit
        for (int x = tid; x < 2 * nbeams * m; x += THREADS) lw[x] = w[x];
        for (int x = tid; x < 2 * nbeams; x += THREADS) li[x] = 0.f;
        if (tid == 0) astat[line] = status;
        return;
    }
    if (tid < m) brg::inv_column(Lf, Li, m, tid);
    __syncthreads();
    for (int p = tid; p < pairs; p += THREADS) {                                               // the factor has served: the unloaded Q in its place
        int i, k;
        brg::pair_of(p, &i, &k);
        Lf[p] = ad::plain_entry(ad::tile_sum(P, tiles, pairs, p), i, k, N);
    }

    const int bb = tid >> 6, e = tid & 63;
    brg::cd *v = V + bb * m, *y = Y + bb * m, *g = G + bb * m;
    double *tw = T + bb * m, *tv = T + (PASS_BEAMS + bb) * m;
    for (int b0 = 0; b0 < nbeams; b0 += PASS_BEAMS) {
        const int b = b0 + bb;
        const bool live = b < nbeams && e < m;
        const float *vb = w + 2 * (size_t)(b < nbeams ? b : 0) * m;
        __syncthreads();                                                                       // Q stands; the last pass's readers are done
        if (e < m) v[e] = live ? ad::weight_of(vb, e) : brg::cd{0.0, 0.0};
        __syncthreads();
        if (e < m) y[e] = brg::fwd_entry(Li, v, e);
        __syncthreads();
        const double vv = brg::norm2(v, m), den = brg::norm2(y, m);                            // (every thread of the beam the same sums)
        if (e < m) g[e] = vv > 0.0 ? ad::scaled(brg::bwd_entry(Li, y, m, e), vv, den) : v[e];
        __syncthreads();
        if (e < m) { tw[e] = ad::quad_row(Lf, g, m, e); tv[e] = ad::quad_row(Lf, v, m, e); }
        if (live) {
            float *o = lw + 2 * ((size_t)b * m + e);
            if (vv > 0.0) { o[0] = (float)g[e].re; o[1] = (float)g[e].im; } else { o[0] = vb[2 * e]; o[1] = vb[2 * e + 1]; }
        }
        __syncthreads();
        if (live && e == 0) { li[2 * b] = (float)ad::sum_of(tw, m); li[2 * b + 1] = (float)ad::sum_of(tv, m); }
    }
    if (tid == 0) astat[line] = 0;
}

} // namespace caf_adapt
} // namespace crsdr
