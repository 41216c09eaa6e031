// caf_cfar_kernels.hpp -- the two kernels of crsdr_caf's CFAR detector (include/crsdr.h, section (w), "Detections"; the decisions
// themselves are caf_cfar.hpp's).  Two launches whatever the batch size.
//
//   k_caf_cfar        grid (entry * tiles + tile, line), 256 threads: ONE (line, entry, tile of 16 Doppler bins x 64 lags) per workgroup.
//                     Thread (l, g) owns lag l of the tile and the rows g, g + 4, ...: no division anywhere.  The tile and its halo (Hd
//                     rows either side, wrapped; Hr lags either side) go into LDS as fp64 P, 0 for a cell outside S or outside the
//                     lags, a thread's sixteen loads in flight together.  A horizontal pass leaves two sums per (halo row, tile lag):
//                     the wings gr < |b| <= Hr, and the wings plus the centre band |b| <= gr.  A vertical pass adds the wing sums of
//                     the rows |a| <= gd and the full sums of the rows gd < |a| <= Hd: Z, by additions only, in one fixed order.  In
//                     both passes a thread's rows go side by side under each offset, so that their LDS reads overlap.  N is
//                     cfar::train_count's closed form (integers), so no presence counts are kept.  Threshold and neighbourhood tests
//                     (cfar::detect; the neighbours come from global memory, so Hd = 0 and Hr = 0 need nothing of their own: few cells
//                     get that far).  The tile's detections are gathered in LDS, ranked by counting (cfar::before is a strict total
//                     order: the rank does not depend on where the LDS atomic put a detection) and the best kt = min(K, cells of a tile)
//                     written in order to the tile's slot, with the tile's count.
//                     LDS: P 32 x 96 x 8 = 24 KiB, sums 2 x 32 x 64 x 8 = 32 KiB (reused for the detections, 24 B x 1024): 56 KiB static.
//   k_caf_cfar_merge  grid (entry, line), 256 threads: the counts summed; the tiles' sorted lists merged K times over their heads (a
//                     tree over the threads' best, cfar::before); the figures (cfar::figures); for entry nrows the snapshot, chi of every
//                     row at the detection's cell, copied as 64-bit words.
// Nothing depends on the order in which workgroups or atomics arrive, and nothing in a line on another line.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "caf_cfar.hpp"

namespace crsdr {
namespace cfar {

constexpr int THREADS = 256, TILE_D = 16, TILE_L = 64, TILE_CELLS = TILE_D * TILE_L, PER = TILE_CELLS / THREADS;
constexpr int GROUPS = THREADS / TILE_L;                                         // thread (l, g): lag l of the tile, rows g, g + GROUPS, ...
constexpr int HALO_ROWS = TILE_D + 2 * MAX_HD, HALO_COLS = TILE_L + 2 * MAX_HR;
constexpr int MAX_TILES = (4096 / TILE_D) * (1024 / TILE_L);                     // nd <= 4096, R <= 1024

__host__ __device__ constexpr int tiles_d(int nd) { return (nd + TILE_D - 1) / TILE_D; }
__host__ __device__ constexpr int tiles_l(int R) { return (R + TILE_L - 1) / TILE_L; }
__host__ __device__ constexpr int tiles_of(int nd, int R) { return tiles_d(nd) * tiles_l(R); }
// candidates a tile keeps: no more than it has cells
__host__ __device__ constexpr int tile_keep(int K, int nd, int R)
{
    const int c = (nd < TILE_D ? nd : TILE_D) * (R < TILE_L ? R : TILE_L);
    return K < c ? K : c;
}

__device__ inline const float *entry_src(const float2 *chi, const float *map, int nrows, size_t cells, int e, int entry, int *comps)
{
    *comps = entry < nrows ? 2 : 1;
    return entry < nrows ? reinterpret_cast<const float *>(chi + ((size_t)e * nrows + entry) * cells) : map + (size_t)e * cells;
}

// The tile and its halo into P: hrows x hcols cells from (d0 - Hd, l0 - Hr) on, Doppler wrapped, 0 outside S or the lags.  Thread
// (l, g) takes the columns l and l + 64 of the rows g, g + 4, ...  Its loads are issued together, from cell 0 where the cell is not
// read, and the values chosen behind them: the loads' latencies overlap.
template <int COMPS>
__device__ inline void fill_halo(double *P, const float *__restrict__ src, int nd, int R, int guard, int d0, int l0, int Hd, int Hr, int hrows, int hcols, int l, int g)
{
    constexpr int ROWS = HALO_ROWS / GROUPS;
    static_assert(HALO_COLS <= 2 * TILE_L, "two columns a thread");
    double v[ROWS][2];
#pragma unroll
    for (int k = 0; k < ROWS; ++k) {
        const int hr = g + GROUPS * k, d = wrap(d0 - Hd + hr, nd);
        const bool row = hr < hrows && cafp::in_set(d, nd, guard);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int c = l + TILE_L * h, lag = l0 - Hr + c;
            const bool in = row && c < hcols && lag >= 0 && lag < R;
            const double p = cafp::power(src, COMPS, in ? d * R + lag : 0);
            v[k][h] = in ? p : 0.0;
        }
    }
#pragma unroll
    for (int k = 0; k < ROWS; ++k) {
        const int hr = g + GROUPS * k;
#pragma unroll
        for (int h = 0; h < 2; ++h)
            if (hr < hrows && l + TILE_L * h < hcols) P[hr * HALO_COLS + l + TILE_L * h] = v[k][h];
    }
}

// chi [nest][nrows][nd][R], map [nest][nd][R]; entries 0 .. entries - 1 of a line are searched (entry < nrows: that row's chi, else map).
// slots [nest][entries][tiles][kt], tcount [nest][entries][tiles]
__global__ __launch_bounds__(THREADS) void k_caf_cfar(const float2 *__restrict__ chi, const float *__restrict__ map, int nrows, int entries, int nd, int R, int guard,
                                                      Params q, int kt, Cand *__restrict__ slots, int32_t *__restrict__ tcount)
{
    __shared__ double P[HALO_ROWS * HALO_COLS];
    __shared__ double SUMS[2 * HALO_ROWS * TILE_L];
    __shared__ int nfound;
    static_assert(sizeof(Cand) * TILE_CELLS <= sizeof(double) * 2 * HALO_ROWS * TILE_L, "the detections reuse the sums");
    double *W = SUMS, *F = SUMS + HALO_ROWS * TILE_L;
    const int tid = threadIdx.x, l = tid & (TILE_L - 1), g = tid / TILE_L, tl_n = tiles_l(R), tiles = tiles_d(nd) * tl_n, entry = blockIdx.x / tiles, tile = blockIdx.x - entry * tiles, e = blockIdx.y;
    const int d0 = (tile / tl_n) * TILE_D, l0 = (tile % tl_n) * TILE_L, th = min(TILE_D, nd - d0), tw = min(TILE_L, R - l0);
    const int Hd = q.gd + q.td, Hr = q.gr + q.tr, hrows = th + 2 * Hd, hcols = tw + 2 * Hr;
    int comps;
    const float *src = entry_src(chi, map, nrows, (size_t)nd * R, e, entry, &comps);

    if (tid == 0) nfound = 0;
    if (comps == 2) fill_halo<2>(P, src, nd, R, guard, d0, l0, Hd, Hr, hrows, hcols, l, g);
    else fill_halo<1>(P, src, nd, R, guard, d0, l0, Hd, Hr, hrows, hcols, l, g);
    __syncthreads();
    // (a thread's rows side by side under each offset: their LDS reads are in flight together.  Rows past hrows and lags past tw are
    // read inside P and SUMS all the same, and dropped)
    constexpr int ROWS = HALO_ROWS / GROUPS;
    {
        double wings[ROWS] = {}, band[ROWS] = {};
        const double *p = P + g * HALO_COLS + l + Hr;                            // the tile lag's own column, the thread's first row
        for (int b = -Hr; b < -q.gr; ++b)
#pragma unroll
            for (int k = 0; k < ROWS; ++k) wings[k] += p[k * GROUPS * HALO_COLS + b];
        for (int b = q.gr + 1; b <= Hr; ++b)
#pragma unroll
            for (int k = 0; k < ROWS; ++k) wings[k] += p[k * GROUPS * HALO_COLS + b];
        for (int b = -q.gr; b <= q.gr; ++b)
#pragma unroll
            for (int k = 0; k < ROWS; ++k) band[k] += p[k * GROUPS * HALO_COLS + b];
#pragma unroll
        for (int k = 0; k < ROWS; ++k) {
            const int hr = g + GROUPS * k;
            if (hr < hrows && l < tw) { W[hr * TILE_L + l] = wings[k]; F[hr * TILE_L + l] = wings[k] + band[k]; }
        }
    }
    __syncthreads();

    Cand mine[PER];
    unsigned hits = 0;
    double z[PER] = {};
    for (int a = -Hd; a <= Hd; ++a) {
        const double *s = ((a < 0 ? -a : a) <= q.gd ? W : F) + (g + Hd + a) * TILE_L + l;
#pragma unroll
        for (int j = 0; j < PER; ++j) z[j] += s[j * GROUPS * TILE_L];
    }
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const int r = g + GROUPS * j;
        if (r >= th || l >= tw) continue;
        if (detect(src, comps, nd, R, guard, q, d0 + r, l0 + l, P[(r + Hd) * HALO_COLS + l + Hr], z[j], &mine[j])) hits |= 1u << j;
    }
    __syncthreads();                                                             // (the sums are read: the detections take their place)
    Cand *list = reinterpret_cast<Cand *>(SUMS);
#pragma unroll
    for (int j = 0; j < PER; ++j)
        if (hits & (1u << j)) list[atomicAdd(&nfound, 1)] = mine[j];
    __syncthreads();
    const int n = nfound;
    Cand *out = slots + (((size_t)e * entries + entry) * tiles + tile) * kt;
    for (int x = tid; x < n; x += THREADS) {
        const Cand c = list[x];
        int rank = 0;
        for (int y = 0; y < n; ++y) rank += before(list[y], c) ? 1 : 0;
        if (rank < kt) out[rank] = c;
    }
    for (int x = n + tid; x < kt; x += THREADS) out[x] = Cand{0.0, 0.0, -1, 0};
    if (tid == 0) tcount[((size_t)e * entries + entry) * tiles + tile] = n;
}

// det [nest][entries][K][8], count [nest][entries], snap [nest][K][nrows][2] (entry nrows only; may be NULL)
__global__ __launch_bounds__(THREADS) void k_caf_cfar_merge(const float2 *__restrict__ chi, const float *__restrict__ map, int nrows, int entries, int nd, int R, int guard,
                                                            Params q, int kt, const Cand *__restrict__ slots, const int32_t *__restrict__ tcount, float *__restrict__ det,
                                                            int32_t *__restrict__ count, float *__restrict__ snap)
{
    __shared__ unsigned char head[MAX_TILES];
    __shared__ Cand red[THREADS];
    __shared__ int redt[THREADS], total[THREADS];
    __shared__ Cand sel[MAX_DET];
    const int tid = threadIdx.x, entry = blockIdx.x, e = blockIdx.y, tiles = tiles_of(nd, R), K = q.max_det;
    const size_t cells = (size_t)nd * R, base = ((size_t)e * entries + entry) * tiles;
    int comps;
    const float *src = entry_src(chi, map, nrows, cells, e, entry, &comps);

    int mine = 0;
    for (int t = tid; t < tiles; t += THREADS) { head[t] = 0; mine += tcount[base + t]; }
    total[tid] = mine;
    __syncthreads();
    for (int h = THREADS / 2; h >= 1; h >>= 1) {
        if (tid < h) total[tid] += total[tid + h];
        __syncthreads();
    }
    int nsel = 0;
    for (; nsel < K; ++nsel) {
        Cand best{0.0, 0.0, -1, 0};
        int bt = -1;
        for (int t = tid; t < tiles; t += THREADS) {
            const int h = head[t];
            if (h >= min(tcount[base + t], kt)) continue;
            const Cand c = slots[(base + t) * kt + h];
            if (before(c, best)) { best = c; bt = t; }
        }
        red[tid] = best; redt[tid] = bt;
        __syncthreads();
        for (int h = THREADS / 2; h >= 1; h >>= 1) {
            if (tid < h && before(red[tid + h], red[tid])) { red[tid] = red[tid + h]; redt[tid] = redt[tid + h]; }
            __syncthreads();
        }
        const int wt = redt[0];
        if (wt < 0) break;                                                       // (the same for every thread)
        if (tid == 0) { sel[nsel] = red[0]; head[wt] += 1; }
        __syncthreads();
    }
    __syncthreads();

    if (tid < K) figures(src, comps, nd, R, guard, tid < nsel ? sel[tid] : Cand{0.0, 0.0, -1, 0}, det + (((size_t)e * entries + entry) * K + tid) * 8);
    if (tid == 0) count[(size_t)e * entries + entry] = total[0];
    if (entry == nrows && snap && nrows > 0) {
        const unsigned long long *c64 = reinterpret_cast<const unsigned long long *>(chi + (size_t)e * nrows * cells);
        unsigned long long *s64 = reinterpret_cast<unsigned long long *>(snap) + (size_t)e * K * nrows;
        for (int idx = tid; idx < K * nrows; idx += THREADS) {
            const int k = idx / nrows, row = idx - k * nrows;
            s64[idx] = k < nsel ? c64[(size_t)row * cells + sel[k].i] : 0ull;
        }
    }
}

} // namespace cfar
} // namespace crsdr
