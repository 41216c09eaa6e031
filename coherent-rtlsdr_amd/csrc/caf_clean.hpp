// caf_clean.hpp -- crsdr_caf's second cancellation stage: the strong detections of the first pass join the canceller's basis, the rows
// are solved jointly, and the maps and the detector run again on the residual (include/crsdr.h, section (w), "Cleaning",
// crsdr_caf_set_clean; tests/caf_clean_model.py is the fp64 statement of it; the arithmetic is caf_clean_solve.hpp's).  It reads what the
// first pass left -- the array map's detection list, the canceller's G, S, c, E and h -- and changes none of it.  Nine launches behind
// the detector's, all on the submit's stream, the same number whatever the batch and however many picks a line has:
//
//   k_clean_pick    grid (line), one wave: lane 0 walks the list (cl::pick_walk) and writes the member table (cl::build_table); the wave
//                   copies the picked records to tgt.
//   k_clean_g       grid (k, line): the reference's segment k and the R - 1 samples in front of it in LDS (zeros in front of the
//                   packet); a thread per (distinct member lag m, tau), G2[k][slot][tau] = sum_n X_r[s + n - m] conj(X_r[s + n - tau]),
//                   formed directly -- exact in int32, so the bits of k_cancel_g's recurrence where the two overlap.  Its first threads
//                   write the members' phases phi_g[k] for the later kernels.
//   k_clean_y       grid (ceil(nd slots / 256), row, line): y_c[k][m] at the member lags, a thread per (k, slot), directly.
//   k_clean_sums    grid (ceil(entries / 32), line), 32 entries x 8 parts as k_cancel_sums: the cross and target blocks of A and the
//                   target part of c in fp64, part q over k = q, q + 8, ..., the parts added in part order.
//   k_clean_solve   grid (line, 64 rows) as k_cancel_solve: the joint factor in LDS (2080 packed pairs, 32.5 KiB), whose leading
//                   block is stage 1's arithmetic and so its bits; then a thread per row solves its own equations.
//   k_caf<LG, 3>    caf.hpp: the rows again with the joint subtraction, into rchi.
//   k_caf_map, k_caf_cfar*, k_caf_cfar_merge as they are, on rchi.
// Nothing depends on the order of workgroups; no float atomics.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "caf.hpp"
#include "caf_cancel.hpp"
#include "caf_clean_solve.hpp"

namespace crsdr {
namespace clean {

constexpr int THREADS = 256, SUM_ENTRIES = 32, SUM_PARTS = THREADS / SUM_ENTRIES, SOLVE_ROWS = 64;
constexpr int G_SAMPLES = (1 << caf::CAF_MAX_SEG_LOG2) + caf::CAF_MAX_LAGS;         // a segment and its history: 10 KiB of int16

// det, count: the array map's entry of the first line.  tgt [nest][T][8], ntgt [nest]
__global__ __launch_bounds__(64) void k_clean_pick(const float *__restrict__ det, size_t det_stride, const int32_t *__restrict__ count, size_t count_stride, int Kdet, int nd,
                                                   int R, int taps, int dopp, cl::Params prm, cl::Table *__restrict__ tab, float *__restrict__ tgt, int32_t *__restrict__ ntgt)
{
    __shared__ int picked[cl::MAX_TARGETS];
    __shared__ int nt_s;
    const int e = blockIdx.x, lane = threadIdx.x;
    const float *d = det + (size_t)e * det_stride;
    if (lane == 0) {
        const int nt = cl::pick_walk(d, count[(size_t)e * count_stride], Kdet, nd, taps, dopp, prm, picked);
        cl::build_table(d, picked, nt, R, prm, tab + e);
        ntgt[e] = nt;
        nt_s = nt;
    }
    __syncthreads();
    for (int i = lane; i < prm.max_targets * 8; i += 64) {
        const int t = i >> 3;
        tgt[(size_t)e * prm.max_targets * 8 + i] = t < nt_s ? d[(size_t)picked[t] * 8 + (i & 7)] : 0.f;
    }
}

// G2 [nest][nd][slots][R], ph2 [nest][members][nd]; slots, members: as allocated
__global__ __launch_bounds__(THREADS) void k_clean_g(const int8_t *__restrict__ packets, size_t packet_stride, size_t matrix_off, int B, int frames, int lgseg, int nd, int R,
                                                     int ref_row, const cl::Table *__restrict__ tab, int slots, int members, int2 *__restrict__ G2,
                                                     double2 *__restrict__ ph2)
{
    __shared__ int16_t X[G_SAMPLES];
    const int k = blockIdx.x, e = blockIdx.y, tid = threadIdx.x;
    const cl::Table &t = tab[e];
    const int Ls = 1 << lgseg, J = (B >> 1) >> lgseg, f = k / J, s = (k - f * J) << lgseg, H = R - 1;
    const int16_t *x = reinterpret_cast<const int16_t *>(packets + (size_t)(e * frames + f) * packet_stride + matrix_off + (size_t)ref_row * B);
    for (int i = tid; i < t.nmem; i += THREADS) {
        const cc::cd p = cl::phase(t.g[i], k, nd);
        ph2[((size_t)e * members + i) * nd + k] = make_double2(p.re, p.im);
    }
    if (t.nslot == 0) return;                                         // (the whole workgroup)
    for (int i = tid; i < Ls + H; i += THREADS) {
        const int n = s + i - H;                                      // < L: s + Ls <= L
        X[i] = n >= 0 ? x[n] : (int16_t)0;
    }
    __syncthreads();
    int2 *out = G2 + ((size_t)e * nd + k) * (size_t)slots * R;
    for (int id = tid; id < t.nslot * R; id += THREADS) {
        const int sl = id / R, tau = id - sl * R, m = t.slot_lag[sl];
        const int16_t *a = X + H - m, *b = X + H - tau;
        int2 g = make_int2(0, 0);
        for (int n = 0; n < Ls; ++n) {
            const int va = a[n], vb = b[n];
            const int2 p = cancel::cancel_mulc(make_int2((int)(int8_t)(va & 0xff), va >> 8), make_int2((int)(int8_t)(vb & 0xff), vb >> 8));
            g.x += p.x; g.y += p.y;
        }
        out[(size_t)sl * R + tau] = g;
    }
}

// Y2 [nest][nrows][nd][slots]
__global__ __launch_bounds__(THREADS) void k_clean_y(const int8_t *__restrict__ packets, size_t packet_stride, size_t matrix_off, int nrows, int B, int frames, int lgseg,
                                                     int nd, int ref_row, const cl::Table *__restrict__ tab, int slots, int2 *__restrict__ Y2)
{
    const int id = blockIdx.x * THREADS + threadIdx.x, row = blockIdx.y, e = blockIdx.z;
    const cl::Table &t = tab[e];
    if (id >= nd * slots || row == ref_row) return;
    const int k = id / slots, sl = id - k * slots;
    if (sl >= t.nslot) return;
    const int Ls = 1 << lgseg, J = (B >> 1) >> lgseg, f = k / J, s = (k - f * J) << lgseg, m = t.slot_lag[sl];
    const int8_t *mat = packets + (size_t)(e * frames + f) * packet_stride + matrix_off;
    const int8_t *xc = mat + (size_t)row * B, *xr = mat + (size_t)ref_row * B;
    int2 y = make_int2(0, 0);
    for (int n = 0; n < Ls; ++n) {
        const int2 p = cancel::cancel_mulc(cancel::cancel_sample(xc, s + n), cancel::cancel_sample(xr, s + n - m));
        y.x += p.x; y.y += p.y;
    }
    Y2[(((size_t)e * nrows + row) * nd + k) * slots + sl] = y;
}

// entries of a line: n2max nmax of A2 (row i - n1, column j; j > i and rows past the line's members are left alone), then nrows n2max
// of C2 (row r's are left alone).  G: the canceller's [nest][nd][K][R]
__global__ __launch_bounds__(THREADS) void k_clean_sums(const int2 *__restrict__ G, const int2 *__restrict__ G2, const int2 *__restrict__ Y2,
                                                        const double2 *__restrict__ ph2, const cl::Table *__restrict__ tab, int nrows, int nd, int R, int K, int P,
                                                        int ref_row, int slots, int members, int n2max, int nmax, double2 *__restrict__ A2, double2 *__restrict__ C2)
{
    __shared__ double2 part[SUM_PARTS][SUM_ENTRIES];
    const int l = threadIdx.x % SUM_ENTRIES, q = threadIdx.x / SUM_ENTRIES, i = blockIdx.x * SUM_ENTRIES + l, e = blockIdx.y;
    const cl::Table &t = tab[e];
    const int n1 = K * (2 * P + 1), nA = n2max * nmax, nC = nrows * n2max;
    const int2 *src = nullptr;
    size_t step = 0;
    double turn = 0.0;                                                 // an entry of A: exp(2 pi i turn k / nd) * src[k * step]
    const double2 *tbl = nullptr;                                      // an entry of c: conj(tbl[k]) * src[k * step]
    double2 *dst = nullptr;
    if (i < nA) {
        const int i2 = i / nmax, j = i - i2 * nmax, ii = n1 + i2;
        if (i2 < t.nmem && j <= ii) {
            const int mi = t.lag[i2], mj = cl::member_lag(t, K, n1, j);
            src = j < n1 ? G + (size_t)e * nd * (size_t)K * R + (size_t)mj * R + mi : G2 + (size_t)e * nd * (size_t)slots * R + (size_t)t.slot[j - n1] * R + mi;
            step = j < n1 ? (size_t)K * R : (size_t)slots * R;
            turn = cl::member_doppler(t, K, P, n1, j) - t.g[i2];
            dst = A2 + (size_t)e * nA + i;
        }
    } else if (i < nA + nC) {
        const int j = i - nA, row = j / n2max, i2 = j - row * n2max;
        if (row != ref_row && i2 < t.nmem) {
            src = Y2 + ((size_t)e * nrows + row) * nd * (size_t)slots + t.slot[i2];
            step = (size_t)slots;
            tbl = ph2 + ((size_t)e * members + i2) * nd;
            dst = C2 + (size_t)e * nC + j;
        }
    }
    double sr = 0.0, si = 0.0;
    if (src)
        for (int k = q; k < nd; k += SUM_PARTS) {
            const int2 v = src[(size_t)k * step];
            cc::cd f;
            if (tbl) { const double2 w = tbl[k]; f = cc::cd{w.x, -w.y}; }
            else f = cl::phase(turn, k, nd);
            const double vr = (double)v.x, vi = (double)v.y;
            sr += f.re * vr - f.im * vi;
            si += f.re * vi + f.im * vr;
        }
    part[q][l] = make_double2(sr, si);
    __syncthreads();
    if (q != 0 || !dst) return;
    for (int k = 1; k < SUM_PARTS; ++k) { sr += part[k][l].x; si += part[k][l].y; }
    *dst = make_double2(sr, si);
}

// grid (nest, ceil(nrows / SOLVE_ROWS)).  S, C, E, h1: the canceller's (h1 its fp64 h).  Wj [nest][nrows][2][nmax]: a row's c and the
// solve's intermediate; hj [nest][nrows][nmax]; jstat [nest]; tcoef [nest][nrows][T][per][2]; tinfo [nest][nrows][2]
__global__ __launch_bounds__(THREADS) void k_clean_solve(const double2 *__restrict__ S, const double2 *__restrict__ C, const long long *__restrict__ E,
                                                         const double2 *__restrict__ h1, const double2 *__restrict__ A2, const double2 *__restrict__ C2,
                                                         const cl::Table *__restrict__ tab, int nrows, int K, int P, int ref_row, int n2max, int nmax, int per,
                                                         double2 *__restrict__ Wj, double2 *__restrict__ hj, int *__restrict__ jstat, float *__restrict__ tcoef,
                                                         float *__restrict__ tinfo)
{
    __shared__ cc::cd Lf[cl::MAX_PAIRS];
    __shared__ double inv_s;
    __shared__ int bad;
    const int e = blockIdx.x, tid = threadIdx.x, n1 = cc::basis(K, P), row = blockIdx.y * SOLVE_ROWS + tid;
    const cl::Table &t = tab[e];
    const int n = n1 + t.nmem;
    const cc::cd *Se = reinterpret_cast<const cc::cd *>(S) + (size_t)e * (4 * P + 1) * K * K;
    const cc::cd *Ae = reinterpret_cast<const cc::cd *>(A2) + (size_t)e * n2max * nmax;
    const double floor_ = cc::pivot_floor(Se, K, P);
    if (tid == 0) bad = 0;
    __syncthreads();
    for (int k = 0; k < n; ++k) {
        if (tid == 0) {
            const double d = cc::chol_pivot(Lf, cl::joint_entry(Se, Ae, K, P, n1, nmax, k, k).re, k);
            if (!(d > floor_)) bad = k < n1 ? cl::STATUS_SINGULAR : cl::STATUS_TARGET;
            const double lkk = sqrt(d), inv = 1.0 / lkk;
            Lf[cc::chol_index(k, k)] = cc::cd{lkk, inv};
            inv_s = inv;
        }
        __syncthreads();
        if (bad) break;                                               // (the whole workgroup reads the same flag)
        for (int i = k + 1 + tid; i < n; i += THREADS) Lf[cc::chol_index(i, k)] = cc::chol_entry(Lf, cl::joint_entry(Se, Ae, K, P, n1, nmax, i, k), i, k, inv_s);
        __syncthreads();
    }
    const int st = bad;
    if (tid == 0 && blockIdx.y == 0) jstat[e] = st;
    if (tid < SOLVE_ROWS && row < nrows) {
        const size_t r = (size_t)e * nrows + row;
        cc::cd *cr = reinterpret_cast<cc::cd *>(Wj) + r * 2 * nmax, *yr = cr + nmax, *hr = reinterpret_cast<cc::cd *>(hj) + r * nmax;
        const cc::cd *c1 = reinterpret_cast<const cc::cd *>(C) + r * n1, *c2 = reinterpret_cast<const cc::cd *>(C2) + r * n2max;
        const cc::cd *h1r = reinterpret_cast<const cc::cd *>(h1) + r * n1;
        for (int j = 0; j < nmax; ++j) hr[j] = cc::cd{0.0, 0.0};
        double share = 1.0;
        int used = n;
        if (row != ref_row) {
            for (int j = 0; j < n; ++j) cr[j] = j < n1 ? c1[j] : c2[j - n1];
            if (!st) cc::chol_solve(Lf, n, cr, yr, hr);
            else if (st == cl::STATUS_TARGET) { used = n1; for (int j = 0; j < n1; ++j) hr[j] = h1r[j]; }
            share = cc::residual_share((double)E[r], hr, cr, used);
        }
        float *tc = tcoef + r * (size_t)n2max * 2;
        for (int j = 0; j < n2max * 2; ++j) tc[j] = 0.f;
        for (int i = 0; i < t.nmem; ++i) {
            const int at = t.owner[i] * per + t.pos[i];
            tc[2 * at] = (float)hr[n1 + i].re; tc[2 * at + 1] = (float)hr[n1 + i].im;
        }
        tinfo[r * 2] = (float)share;
        tinfo[r * 2 + 1] = row != ref_row ? (float)st : 0.f;
    }
}

} // namespace clean
} // namespace crsdr
