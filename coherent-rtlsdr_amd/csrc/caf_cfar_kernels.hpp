// caf_cfar_kernels.hpp -- the kernels of crsdr_caf's CFAR detector (include/crsdr.h, section (w), "Detections" and "Estimators"; the
// decisions themselves are caf_cfar.hpp's).  Two launches whatever the batch size and the estimator: k_caf_cfar<EST> (cell averaging,
// greatest-of, smallest-of) or k_caf_cfar_os (ordered statistic; described where it stands), then k_caf_cfar_merge.
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

// The tile and its halo into P: hrows x hcols cells from (d0 - Hd, l0 - Hr) on, Doppler wrapped, `absent` (0 for the sums, a negative
// mark for the ordered statistic) outside S or the lags.  Thread
// (l, g) takes the columns l and l + 64 of the rows g, g + 4, ...  Its loads are issued together, from cell 0 where the cell is not
// read, and the values chosen behind them: the loads' latencies overlap.
template <int COMPS>
__device__ inline void fill_halo(double *P, const float *__restrict__ src, int nd, int R, int guard, int d0, int l0, int Hd, int Hr, int hrows, int hcols, int l, int g,
                                 double absent)
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
            v[k][h] = in ? p : absent;
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
template <int EST>
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
    if (comps == 2) fill_halo<2>(P, src, nd, R, guard, d0, l0, Hd, Hr, hrows, hcols, l, g, 0.0);
    else fill_halo<1>(P, src, nd, R, guard, d0, l0, Hd, Hr, hrows, hcols, l, g, 0.0);
    __syncthreads();
    constexpr int ROWS = HALO_ROWS / GROUPS;
    Cand mine[PER];
    unsigned hits = 0;
    if constexpr (EST == EST_CA) {
        // (a thread's rows side by side under each offset: their LDS reads are in flight together.  Rows past hrows and lags past tw are
        // read inside P and SUMS all the same, and dropped)
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
    } else {
        // GO and SO: the same two passes once per half.  Over lag (axis 0) a half's horizontal pass takes its own wing and its own side
        // of the centre band, and the vertical pass every row; over Doppler (axis 1) the horizontal pass is cell averaging's, run once,
        // and a half's vertical pass takes the rows on its side: row a = 0 goes to neither.  The order of the additions is fixed.
        double zh[2][PER] = {};
        for (int half = 0; half < 2; ++half) {
            if (q.axis == 0 || half == 0) {
                if (half) __syncthreads();                                       // (the lower half's sums are read)
                double wings[ROWS] = {}, band[ROWS] = {};
                const double *p = P + g * HALO_COLS + l + Hr;
                const int w0 = q.axis == 0 && half ? q.gr + 1 : -Hr, w1 = q.axis == 0 && !half ? -q.gr - 1 : Hr;
                const int b0 = q.axis == 0 && half ? 1 : -q.gr, b1 = q.axis == 0 && !half ? -1 : q.gr;
                for (int b = w0; b <= w1; ++b) {
                    if (b >= -q.gr && b <= q.gr) continue;
#pragma unroll
                    for (int k = 0; k < ROWS; ++k) wings[k] += p[k * GROUPS * HALO_COLS + b];
                }
                for (int b = b0; b <= b1; ++b)
#pragma unroll
                    for (int k = 0; k < ROWS; ++k) band[k] += p[k * GROUPS * HALO_COLS + b];
#pragma unroll
                for (int k = 0; k < ROWS; ++k) {
                    const int hr = g + GROUPS * k;
                    if (hr < hrows && l < tw) { W[hr * TILE_L + l] = wings[k]; F[hr * TILE_L + l] = wings[k] + band[k]; }
                }
                __syncthreads();
            }
            const int a0 = q.axis == 1 && half ? 1 : -Hd, a1 = q.axis == 1 && !half ? -1 : Hd;
            for (int a = a0; a <= a1; ++a) {
                const double *s = ((a < 0 ? -a : a) <= q.gd ? W : F) + (g + Hd + a) * TILE_L + l;
#pragma unroll
                for (int j = 0; j < PER; ++j) zh[half][j] += s[j * GROUPS * TILE_L];
            }
        }
        Params qe = q;
        qe.est = EST;
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const int r = g + GROUPS * j;
            if (r >= th || l >= tw) continue;
            if (detect_halves(src, comps, nd, R, guard, qe, d0 + r, l0 + l, P[(r + Hd) * HALO_COLS + l + Hr], zh[0][j], zh[1][j], &mine[j])) hits |= 1u << j;
        }
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

constexpr int WAVE = 64, WAVES = THREADS / WAVE;
constexpr int OS_PER_LANE = ((2 * MAX_HD + 1) * (2 * MAX_HR + 1) + WAVE - 1) / WAVE;    // 9: the largest window's cells a lane holds

__device__ inline int wave_sum(int v)
{
#pragma unroll
    for (int m = WAVE / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m, WAVE);
    return v;
}

// The 3 x 3 test of tile cell (r, l) on the halo, which holds every neighbour when Hd >= 1 and Hr >= 1: a neighbour outside the lags
// or outside S carries the negative mark and does not count.  cfar::local_max's answer, without its global reads.
__device__ inline bool local_max_lds(const double *P, int nd, int R, int d, int tau, int hr, int hc, double p)
{
    const int i = d * R + tau;
    bool ok = true;
#pragma unroll
    for (int a = -1; a <= 1; ++a)
#pragma unroll
        for (int b = -1; b <= 1; ++b) {
            if (a == 0 && b == 0) continue;
            const double pq = P[(hr + a) * HALO_COLS + hc + b];
            ok = ok && (pq < 0.0 || beats(p, i, pq, wrap(d + a, nd) * R + tau + b));
        }
    return ok;
}

// The ordered statistic.  Grid, tile, slots and tcount as k_caf_cfar's, so k_caf_cfar_merge follows it unchanged (Cand.noise: the
// order statistic, Cand.n: N).  The halo goes into LDS with absent cells marked -1, not zeroed: P >= 0 says "a member".  No sort:
// rounding is monotone, so with x_(k) the k-th smallest member, alpha x_(k) < P  <=>  #{j: alpha x_j < P} >= k, and x_(k) > 0  <=>
// #{j: x_j = 0} < k.
//   1  every cell's 3 x 3 test first (from the halo, or cfar::local_max where Hd = 0 or Hr = 0 leaves the halo without neighbours); the
//      survivors, about one cell in nine, are compacted into an LDS list
//   2  a wave takes the survivors w, w + 4, ...: its lanes stride the window, at most nine cells a lane, read once and held in
//      registers, and count the members with alpha x < P and the zeros, summed across the wave.  N is the closed form.
//   3  for the few that pass, x_(k) by bisection on the fp64 bit pattern (non-negative doubles order as their bits do): the smallest
//      v with #{j: x_j <= v} >= k, 63 counts at the most
//   4  the tile's detections ranked and written as k_caf_cfar does
// Neither list's order matters: a survivor's verdict is its own, and the ranking is by cfar::before.
// LDS: P 24 KiB, the survivors 2 B x 1024, the detections 24 B x 1024: 50 KiB static.
__global__ __launch_bounds__(THREADS) void k_caf_cfar_os(const float2 *__restrict__ chi, const float *__restrict__ map, int nrows, int entries, int nd, int R, int guard,
                                                         Params q, int kt, Cand *__restrict__ slots, int32_t *__restrict__ tcount)
{
    __shared__ double P[HALO_ROWS * HALO_COLS];
    __shared__ Cand list[TILE_CELLS];
    __shared__ unsigned short surv[TILE_CELLS];
    __shared__ int nsurv, nfound;
    const int tid = threadIdx.x, l = tid & (TILE_L - 1), g = tid / TILE_L, tl_n = tiles_l(R), tiles = tiles_d(nd) * tl_n, entry = blockIdx.x / tiles, tile = blockIdx.x - entry * tiles, e = blockIdx.y;
    const int d0 = (tile / tl_n) * TILE_D, l0 = (tile % tl_n) * TILE_L, th = min(TILE_D, nd - d0), tw = min(TILE_L, R - l0);
    const int Hd = q.gd + q.td, Hr = q.gr + q.tr, hrows = th + 2 * Hd, hcols = tw + 2 * Hr;
    int comps;
    const float *src = entry_src(chi, map, nrows, (size_t)nd * R, e, entry, &comps);

    if (tid == 0) { nsurv = 0; nfound = 0; }
    if (comps == 2) fill_halo<2>(P, src, nd, R, guard, d0, l0, Hd, Hr, hrows, hcols, l, g, -1.0);
    else fill_halo<1>(P, src, nd, R, guard, d0, l0, Hd, Hr, hrows, hcols, l, g, -1.0);
    __syncthreads();

    const bool halo_has_neighbours = Hd >= 1 && Hr >= 1;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const int r = g + GROUPS * j;
        if (r >= th || l >= tw) continue;
        const double p = P[(r + Hd) * HALO_COLS + l + Hr];
        if (p < 0.0) continue;                                                   // (the row is not in S)
        const bool top = halo_has_neighbours ? local_max_lds(P, nd, R, d0 + r, l0 + l, r + Hd, l + Hr, p) : local_max(src, comps, nd, R, guard, d0 + r, l0 + l, p);
        if (top) surv[atomicAdd(&nsurv, 1)] = (unsigned short)(r * TILE_L + l);
    }
    __syncthreads();

    const int lane = tid & (WAVE - 1), wave = tid / WAVE, ns = nsurv, wc = 2 * Hr + 1, cells = (2 * Hd + 1) * wc, nfull = full_count(q);
    for (int x = wave; x < ns; x += WAVES) {
        const int cell = surv[x], r = cell / TILE_L, lc = cell - r * TILE_L, d = d0 + r, tau = l0 + lc;
        const double p = P[(r + Hd) * HALO_COLS + lc + Hr];
        const int N = train_count(d, tau, nd, R, guard, q);
        if (N < 1 || N < q.min_train) continue;                                  // (the same for every lane of the wave)
        const int k = os_rank(q.rank, N, nfull);
        double v[OS_PER_LANE];
        int under = 0, zeros = 0;
#pragma unroll
        for (int u = 0; u < OS_PER_LANE; ++u) {
            const int idx = lane + WAVE * u, row = idx / wc, a = row - Hd, b = idx - row * wc - Hr;
            const bool in = idx < cells && !((a < 0 ? -a : a) <= q.gd && (b < 0 ? -b : b) <= q.gr);
            // (absent cells carry the mark already; + 0.0 turns a map's -0.0 into the 0.0 whose bits order with the rest)
            v[u] = in ? P[(r + Hd + a) * HALO_COLS + lc + Hr + b] + 0.0 : -1.0;
            const double t = (double)q.alpha * v[u];
            under += v[u] >= 0.0 && t < p ? 1 : 0;
            zeros += v[u] == 0.0 ? 1 : 0;
        }
        under = wave_sum(under);
        zeros = wave_sum(zeros);
        if (under < k || zeros >= k) continue;
        unsigned long long lo = 0ull, hi = 0x7ff0000000000000ull;                // x_(k) in (lo, hi] as bits: it is above 0, and finite or infinity
        while (hi - lo > 1ull) {
            const unsigned long long mid = lo + (hi - lo) / 2;
            int le = 0;
#pragma unroll
            for (int u = 0; u < OS_PER_LANE; ++u) le += v[u] >= 0.0 && (unsigned long long)__double_as_longlong(v[u]) <= mid ? 1 : 0;
            if (wave_sum(le) >= k) hi = mid; else lo = mid;
        }
        if (lane == 0) list[atomicAdd(&nfound, 1)] = Cand{p, __longlong_as_double((long long)hi), d * R + tau, N};
    }
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
