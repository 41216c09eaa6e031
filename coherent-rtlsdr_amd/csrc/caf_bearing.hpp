// caf_bearing.hpp -- the kernels of crsdr_caf's bearings (include/crsdr.h, section (w), "Bearings"; crsdr_caf_set_bearing,
// crsdr_bearing): a direction per detection of the array map from its snapshot across the rows.  The arithmetic is
// caf_bearing_solve.hpp's, fp64 throughout; three launches whatever the batch and whatever the counts, which the kernels read on the
// device.
//   k_bearing_slot    grid (K, lines): a workgroup per (line, slot).  The snapshot u; in the adaptive mode the training snapshots'
//                     covariance -- per Doppler bin of the window the (up to 2 Hr + 1) lags of every element, contiguous in chi, go to
//                     LDS once as published and every thread adds them to its entries of the packed triangle, so chi is read once --
//                     its loading, the Cholesky factor a column at a time (a thread per entry below the pivot), the factor's inverse
//                     (a thread per column), W u, u^H W u and the co-array coefficients of a^H W a (a thread per coefficient).  It
//                     leaves the slot's record (brg::REC doubles).  An empty slot writes a zero head and leaves.
//   k_bearing_scan    grid (tiles of TILE grid points, K, lines): a thread per grid point evaluates T from the record in LDS, writes
//                     spec where it is kept, and the tile's first maximum (value, then lower index) goes to tbest.
//   k_bearing_finish  grid (K, lines), one wave: merges the tiles' maxima under the same rule -- a strict total order, so the split
//                     and the order of the joins do not matter -- then the zoom search, a lane per lattice point and every lane the
//                     same walk, and the slot's eight figures.
// Nothing depends on the order of workgroups; no atomics.  Plain C++ with vector stores only.
//   LDS of k_bearing_slot: two packed triangles of m (m + 1) / 2 fp64 pairs (the second doubles as the staging area of the training
//   snapshots) and two vectors: 68 624 bytes at m = 64, above the 64 KiB default -- the callers raise the limit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "caf_bearing_solve.hpp"

namespace crsdr {
namespace bearing {

constexpr int THREADS = 256, TILE = 256, FIN_THREADS = 64;

struct Best { double v; int i, pad; };

__host__ __device__ constexpr size_t align16(size_t n) { return (n + 15) & ~(size_t)15; }
__host__ __device__ constexpr size_t tri_bytes(int m) { return sizeof(brg::cd) * (size_t)(m * (m + 1) / 2); }
// the second region: the inverse's triangle, or a Doppler bin's training snapshots [2 Hr + 1][m] as published
__host__ __device__ constexpr size_t second_bytes(int m, int Hr)
{
    return align16(tri_bytes(m) > sizeof(float2) * (size_t)((2 * Hr + 1) * m) ? tri_bytes(m) : sizeof(float2) * (size_t)((2 * Hr + 1) * m));
}
__host__ __device__ constexpr size_t slot_lds_bytes(int m, int Hr) { return align16(tri_bytes(m)) + second_bytes(m, Hr) + 2 * sizeof(brg::cd) * (size_t)m + 16; }

__host__ __device__ inline int tiles_of(int ncx, int ncy) { return (ncx * ncy + TILE - 1) / TILE; }

// chi [lines][nrows][nd][R]; det, count: the array map's entry of line 0, det_stride floats and count_stride ints from line to line
__global__ __launch_bounds__(THREADS) void k_bearing_slot(const float2 *__restrict__ chi, const float *__restrict__ det, size_t det_stride,
                                                          const int32_t *__restrict__ count, size_t count_stride, int nrows, int nd, int R, int ref_row, int guard,
                                                          cfar::Params cp, brg::Params bp, int K, double *__restrict__ rec)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char bsm[];
    const int m = bp.mx * bp.my, npairs = m * (m + 1) / 2, Hd = cp.gd + cp.td, Hr = cp.gr + cp.tr;
    brg::cd *Lf = reinterpret_cast<brg::cd *>(bsm);                                            // [npairs]
    brg::cd *Li = reinterpret_cast<brg::cd *>(bsm + align16(tri_bytes(m)));                    // [npairs]
    float2 *stage = reinterpret_cast<float2 *>(Li);                                            // [2 Hr + 1][m], before Li is made
    brg::cd *u = reinterpret_cast<brg::cd *>(bsm + align16(tri_bytes(m)) + second_bytes(m, Hr));   // [m]
    brg::cd *y = u + m;                                                                        // [m]
    double &inv_s = *reinterpret_cast<double *>(y + m);                                        // (in the dynamic region: its base stays 16-byte aligned)
    int &bad = *reinterpret_cast<int *>(&inv_s + 1);
    const int slot = blockIdx.x, line = blockIdx.y, tid = threadIdx.x;
    double *out = rec + ((size_t)line * K + slot) * brg::REC;
    const int cnt = count[(size_t)line * count_stride];
    const float *dt = det + (size_t)line * det_stride + (size_t)slot * 8;
    const int cell = slot < cnt ? brg::cell_of(dt, nd, R) : -1;
    if (cell < 0) {                                                                            // an empty slot, or no cell of the map (workgroup-uniform)
        if (tid < 4) out[tid] = tid == 1 && slot < cnt ? (double)brg::STATUS_CELL : 0.0;
        return;
    }
    const size_t cells = (size_t)nd * (size_t)R;
    const float *X = reinterpret_cast<const float *>(chi + (size_t)line * nrows * cells);
    const int d = cell / R, tau = cell - d * R;
    if (tid < m) u[tid] = brg::snap_elem(X, cells, ref_row, tid, cell);
    if (tid == 0) bad = 0;
    __syncthreads();
    const double uu = brg::norm2(u, m);                                                        // (every thread the same sum)
    if (uu == 0.0) {
        if (tid < 4) out[tid] = tid == 1 ? (double)brg::STATUS_ZERO : 0.0;
        return;
    }
    int status = 0;
    bool ident = bp.mode != brg::MODE_ADAPTIVE;
    if (!ident) {
        for (int p = tid; p < npairs; p += THREADS) Lf[p] = brg::cd{0.0, 0.0};
        int N = 0;
        const int lo = tau - Hr < 0 ? 0 : tau - Hr, hi = tau + Hr > R - 1 ? R - 1 : tau + Hr, nb = hi - lo + 1;
        for (int a = -Hd; a <= Hd; ++a) {
            const int dq = cfar::wrap(d + a, nd);
            if (!cafp::in_set(dq, nd, guard)) continue;                                        // (workgroup-uniform)
            __syncthreads();                                                                   // the last bin's readers are done
            for (int t = tid; t < m * nb; t += THREADS) {
                const int e = t / nb, j = t - e * nb;
                stage[j * m + e] = chi[((size_t)line * nrows + brg::row_of(e, ref_row)) * cells + (size_t)dq * R + lo + j];
            }
            __syncthreads();
            for (int j = 0; j < nb; ++j) N += cfar::trains(a, lo + j - tau, d, tau, nd, R, guard, cp) ? 1 : 0;
            for (int p = tid; p < npairs; p += THREADS) {
                int i, k;
                brg::pair_of(p, &i, &k);
                brg::cd acc = Lf[p];
                for (int j = 0; j < nb; ++j) {
                    if (!cfar::trains(a, lo + j - tau, d, tau, nd, R, guard, cp)) continue;
                    const float2 xi = stage[j * m + i], xk = stage[j * m + k];
                    brg::cov_add(&acc, brg::cd{(double)xi.x, -(double)xi.y}, brg::cd{(double)xk.x, -(double)xk.y});
                }
                Lf[p] = acc;
            }
        }
        __syncthreads();
        const double tr = brg::trace_of(Lf, m);                                                // (every thread the same sum)
        __syncthreads();                                                                       // read before the loading rewrites the diagonal
        if (N == 0 || !(tr > 0.0)) ident = true;
        else {
            for (int p = tid; p < npairs; p += THREADS) {
                int i, k;
                brg::pair_of(p, &i, &k);
                Lf[p] = brg::loaded_entry(Lf[p], i, k, N, tr, m, bp.loading);
            }
            __syncthreads();
            for (int k = 0; k < m; ++k) {                                                      // brg::factor, a column at a time
                if (tid == 0) {
                    const double dv = cc::chol_pivot(Lf, Lf[brg::chol_index(k, k)].re, k);
                    if (!(dv > 0.0)) bad = 1;
                    const double lkk = sqrt(dv), inv = 1.0 / lkk;
                    Lf[brg::chol_index(k, k)] = brg::cd{lkk, inv};
                    inv_s = inv;
                }
                __syncthreads();
                if (bad) break;                                                                // (the whole workgroup reads the same flag)
                for (int i = k + 1 + tid; i < m; i += THREADS) Lf[brg::chol_index(i, k)] = cc::chol_entry(Lf, Lf[brg::chol_index(i, k)], i, k, inv_s);
                __syncthreads();
            }
            if (bad) ident = true;
        }
        if (ident) status |= brg::STATUS_IDENTITY;
    }
    brg::cd *wu = reinterpret_cast<brg::cd *>(out + brg::REC_WU), *C = reinterpret_cast<brg::cd *>(out + brg::REC_COEF);
    if (ident) {
        if (tid < m) wu[tid] = u[tid];
        if (tid == 0) out[0] = uu;
    } else {
        if (tid < m) brg::inv_column(Lf, Li, m, tid);
        __syncthreads();
        if (tid < m) y[tid] = brg::fwd_entry(Li, u, tid);
        __syncthreads();
        if (tid < m) wu[tid] = brg::bwd_entry(Li, y, m, tid);
        if (tid == 0) out[0] = brg::norm2(y, m);
        const int w = 2 * bp.my - 1;
        for (int c = tid; c < brg::coefs(bp.mx, bp.my); c += THREADS) C[c] = brg::coef(Li, bp.mx, bp.my, c / w, c % w - (bp.my - 1));
    }
    if (tid == 0) { out[1] = (double)status; out[2] = 1.0; out[3] = ident ? 1.0 : 0.0; }
}

// spec [lines][K][ncx][ncy] or NULL; tbest [lines][K][tiles]
__global__ __launch_bounds__(THREADS) void k_bearing_scan(const double *__restrict__ rec, brg::Params bp, int K, float *__restrict__ spec, Best *__restrict__ tbest)
{
    __shared__ double r[brg::REC];
    __shared__ double bv[THREADS];
    __shared__ int bi[THREADS];
    const int tile = blockIdx.x, slot = blockIdx.y, line = blockIdx.z, tid = threadIdx.x, npts = bp.ncx * bp.ncy, g = tile * TILE + tid;
    const size_t s = (size_t)line * K + slot;
    const double *in = rec + s * brg::REC;
    if (in[2] == 0.0) {                                                                        // nothing to scan (workgroup-uniform): T = 0 everywhere
        if (spec && g < npts) spec[s * npts + g] = 0.f;
        return;
    }
    const int used = brg::REC_COEF + 2 * brg::coefs(bp.mx, bp.my);
    for (int i = tid; i < used; i += THREADS) r[i] = in[i];
    __syncthreads();
    double T = -1.0;
    if (g < npts) {
        T = brg::stat(r, bp.mx, bp.my, bp.d, bp.ncx, bp.ncy, (double)(g / bp.ncy), (double)(g % bp.ncy));
        if (spec) spec[s * npts + g] = (float)T;
    }
    bv[tid] = T; bi[tid] = g;
    __syncthreads();
    for (int h = THREADS / 2; h > 0; h >>= 1) {
        if (tid < h && (bv[tid + h] > bv[tid] || (bv[tid + h] == bv[tid] && bi[tid + h] < bi[tid]))) { bv[tid] = bv[tid + h]; bi[tid] = bi[tid + h]; }
        __syncthreads();
    }
    if (tid == 0) tbest[s * gridDim.x + tile] = Best{bv[0], bi[0], 0};
}

// dir [lines][K][8]
__global__ __launch_bounds__(FIN_THREADS) void k_bearing_finish(const double *__restrict__ rec, const Best *__restrict__ tbest, int tiles, brg::Params bp, int K,
                                                                float *__restrict__ dir)
{
    __shared__ double r[brg::REC];
    __shared__ double bv[FIN_THREADS];
    __shared__ int bi[FIN_THREADS];
    __shared__ double fval[FIN_THREADS];
    const int slot = blockIdx.x, line = blockIdx.y, tid = threadIdx.x;
    const size_t s = (size_t)line * K + slot;
    const double *in = rec + s * brg::REC;
    float *out = dir + s * 8;
    if (in[2] == 0.0) {                                                                        // (workgroup-uniform)
        if (tid == 0) brg::figures(in, 0, 0, 0.0, 0.0, 0.0, bp.ncx, bp.ncy, out);
        return;
    }
    const int used = brg::REC_COEF + 2 * brg::coefs(bp.mx, bp.my);
    for (int i = tid; i < used; i += FIN_THREADS) r[i] = in[i];
    double v = -1.0;
    int at = 0x7fffffff;
    for (int t = tid; t < tiles; t += FIN_THREADS) {
        const Best b = tbest[s * tiles + t];
        if (b.v > v || (b.v == v && b.i < at)) { v = b.v; at = b.i; }
    }
    bv[tid] = v; bi[tid] = at;
    __syncthreads();
    for (int h = FIN_THREADS / 2; h > 0; h >>= 1) {
        if (tid < h && (bv[tid + h] > bv[tid] || (bv[tid + h] == bv[tid] && bi[tid + h] < bi[tid]))) { bv[tid] = bv[tid + h]; bi[tid] = bi[tid + h]; }
        __syncthreads();
    }
    const int cx = bi[0] / bp.ncy, cy = bi[0] - cx * bp.ncy;
    const double tg = bv[0];
    double x = (double)cx, y = (double)cy, step = 0.5;
    for (int l = 0; l < bp.levels; ++l) {
        if (tid < brg::POINTS) {
            double px, py;
            brg::lattice_point(x, y, step, tid, bp.ncx, bp.ncy, &px, &py);
            fval[tid] = brg::stat(r, bp.mx, bp.my, bp.d, bp.ncx, bp.ncy, px, py);
        }
        __syncthreads();
        brg::zoom_pick(fval, step, bp.ncx, bp.ncy, &x, &y);                                    // the same walk in every lane
        __syncthreads();
        step *= 0.25;
    }
    if (tid == 0) brg::figures(r, cx, cy, tg, x, y, bp.ncx, bp.ncy, out);
}

} // namespace bearing
} // namespace crsdr
