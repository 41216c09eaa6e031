// caf_cancel.hpp -- crsdr_caf's least-squares canceller of the direct path and the clutter (include/crsdr.h, section (w),
// crsdr_caf_set_cancel; tests/caf_cancel_model.py is the fp64 statement of it).  It works in the lag domain on the range stage's exact
// integers: per line the reference's own sums G, per row the normal equations A h = c over the basis phi_p[k] X_r[n - m], and
//     y'_c[k][tau] = y_c[k][tau] - sum_(m,p) h_c,(m,p) phi_p[k] G[k][m][tau]
// in fp64 with one rounding, in front of the Doppler stage.  Five launches take k_caf's place, all on the submit's stream:
//
//   k_cancel_g      grid (ceil(nd (R + K - 1) / 256), line): a thread per (k, diagonal tau - m).  G[k][m][tau] = sum_{n < Ls}
//                   X_r[s + n - m] conj(X_r[s + n - tau]), s = j Ls.  The diagonal's first entry (m = 0 or tau = 0) is a sum over the
//                   segment; every further one follows from the one before it by two products,
//                       G[k][m][tau] = G[k][m-1][tau-1] + X_r[s-m] conj(X_r[s-tau]) - X_r[s+Ls-m] conj(X_r[s+Ls-tau]),
//                   exact because these are integers (|G| <= 2^15 Ls <= 2^27), with the zeros in front of the packet.
//   k_caf<LG, 1>         caf.hpp's range stage on the lags < K of every row but r: Y[k][m] = y_c[k][m] and E = sum |X_c|^2 (int64).
//   k_cancel_sums   grid (ceil(entries / 32), line), 32 entries x 8 parts as k_caf_map: the sums over k of S[q][m][m'] =
//                   sum_k phi_q[k] G[k][m][m'] (|q| <= 2 P) and c_(m',p') = sum_k conj(phi_p'[k]) Y[k][m'] in fp64, part q over
//                   k = q, q + 8, ..., the parts added in part order.  phi from a table exp(2 pi i j / nd) (k_cancel_phase), p k mod nd.
//                   For q = 0 every term and partial sum is an integer below 2^39, so fp64 holds it exactly.
//   k_cancel_solve  grid (line, 64 rows): the factor of caf_cancel_solve.hpp in LDS, a column at a time with a thread per entry below the
//                   pivot; then a thread per row solves its own equations from the factor.  h stays in fp64 for the subtraction; coef and cinfo
//                   are its published forms.  A singular line: h = 0, status bit 0.
//   k_caf<LG, 2>         k_caf with the subtraction between its stages.
// Nothing depends on the order of workgroups; no float atomics.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "caf.hpp"
#include "caf_cancel_solve.hpp"

namespace crsdr {
namespace cancel {

constexpr int THREADS = 256, SUM_ENTRIES = 32, SUM_PARTS = THREADS / SUM_ENTRIES, SOLVE_ROWS = 64;

__global__ __launch_bounds__(THREADS) void k_cancel_phase(int nd, double2 *__restrict__ ph)
{
    const int j = blockIdx.x * THREADS + threadIdx.x;
    if (j >= nd) return;
    double s, c;
    sincospi(2.0 * (double)j / (double)nd, &s, &c);
    ph[j] = make_double2(c, s);
}

// sample i of a row (its bytes I, Q), zero in front of the packet
__device__ __forceinline__ int2 cancel_sample(const int8_t *__restrict__ x, int i)
{
    if (i < 0) return make_int2(0, 0);
    const int v = reinterpret_cast<const int16_t *>(x)[i];
    return make_int2((int)(int8_t)(v & 0xff), v >> 8);
}

// a conj(b)
__device__ __forceinline__ int2 cancel_mulc(int2 a, int2 b) { return make_int2(a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y); }

__global__ __launch_bounds__(THREADS) void k_cancel_g(const int8_t *__restrict__ packets, size_t packet_stride, size_t matrix_off, int B, int frames, int lgseg, int nd,
                                                      int R, int K, int ref_row, int2 *__restrict__ G)
{
    const int diags = R + K - 1, id = blockIdx.x * THREADS + threadIdx.x, e = blockIdx.y;
    if (id >= nd * diags) return;
    const int k = id / diags, d = id - k * diags - (K - 1);           // d = tau - m
    const int Ls = 1 << lgseg, J = (B >> 1) >> lgseg, t = k / J, s = (k - t * J) << lgseg;
    const int8_t *x = packets + (size_t)(e * frames + t) * packet_stride + matrix_off + (size_t)ref_row * B;
    int m = d < 0 ? -d : 0, tau = d < 0 ? 0 : d;
    int2 g = make_int2(0, 0);
    for (int n = 0; n < Ls; ++n) {
        const int2 p = cancel_mulc(cancel_sample(x, s + n - m), cancel_sample(x, s + n - tau));
        g.x += p.x; g.y += p.y;
    }
    int2 *out = G + ((size_t)e * nd + k) * (size_t)K * R;
    out[(size_t)m * R + tau] = g;
    for (++m, ++tau; m < K && tau < R; ++m, ++tau) {
        const int2 a = cancel_mulc(cancel_sample(x, s - m), cancel_sample(x, s - tau));
        const int2 b = cancel_mulc(cancel_sample(x, s + Ls - m), cancel_sample(x, s + Ls - tau));      // (m, tau >= 1: inside the packet)
        g.x += a.x - b.x; g.y += a.y - b.y;
        out[(size_t)m * R + tau] = g;
    }
}

// entries of a line: (4 P + 1) K K of S, then nrows (2 P + 1) K of c (row r's are left alone)
__global__ __launch_bounds__(THREADS) void k_cancel_sums(const int2 *__restrict__ G, const int2 *__restrict__ Y, const double2 *__restrict__ ph, int nrows, int nd, int R,
                                                         int K, int P, int ref_row, double2 *__restrict__ S, double2 *__restrict__ C)
{
    __shared__ double2 part[SUM_PARTS][SUM_ENTRIES];
    const int l = threadIdx.x % SUM_ENTRIES, q = threadIdx.x / SUM_ENTRIES, i = blockIdx.x * SUM_ENTRIES + l, e = blockIdx.y;
    const int nS = (4 * P + 1) * K * K, n = K * (2 * P + 1), nC = nrows * n;
    const int2 *src = nullptr;
    size_t step = 0;
    int turn = 0;                                                      // the term is exp(2 pi i turn k / nd) * src[k * step]
    double2 *dst = nullptr;
    if (i < nS) {
        const int qq = i / (K * K), mm = i - qq * K * K;               // mm = m K + m'
        src = G + (size_t)e * nd * (size_t)K * R + (size_t)(mm / K) * R + mm % K;
        step = (size_t)K * R; turn = qq - 2 * P; dst = S + (size_t)e * nS + i;
    } else if (i < nS + nC) {
        const int j = i - nS, row = j / n, b = j - row * n;            // b = (p' + P) K + m'
        if (row != ref_row) {
            src = Y + ((size_t)e * nrows + row) * nd * (size_t)K + b % K;
            step = (size_t)K; turn = -(b / K - P); dst = C + (size_t)e * nC + j;
        }
    }
    double sr = 0.0, si = 0.0;
    if (src)
        for (int k = q; k < nd; k += SUM_PARTS) {
            const int2 v = src[(size_t)k * step];
            const double2 f = ph[(turn * k) & (nd - 1)];
            const double vr = (double)v.x, vi = (double)v.y;
            sr += f.x * vr - f.y * vi;
            si += f.x * vi + f.y * vr;
        }
    part[q][l] = make_double2(sr, si);
    __syncthreads();
    if (q != 0 || !dst) return;
    for (int k = 1; k < SUM_PARTS; ++k) { sr += part[k][l].x; si += part[k][l].y; }
    *dst = make_double2(sr, si);
}

// grid (nest, ceil(nrows / SOLVE_ROWS)): every workgroup factors the line's matrix for itself (the same arithmetic, so the same bits) and
// solves SOLVE_ROWS rows -- one workgroup per line left a line of 1025 rows to five rounds of solves, 105 us.  S [nest][(4 P + 1) K K], C, W (the solves' intermediates), h [nest][nrows][n] as cc::cd; E [nest][nrows]
__global__ __launch_bounds__(THREADS) void k_cancel_solve(const double2 *__restrict__ S, const double2 *__restrict__ C, const long long *__restrict__ E, int nrows, int K,
                                                          int P, int ref_row, double2 *__restrict__ W, double2 *__restrict__ h, int *__restrict__ status,
                                                          float *__restrict__ coef, float *__restrict__ cinfo)
{
    __shared__ cc::cd Lf[cc::MAX_PAIRS];
    __shared__ double inv_s;
    __shared__ int bad;
    const int e = blockIdx.x, tid = threadIdx.x, n = cc::basis(K, P), row = blockIdx.y * SOLVE_ROWS + tid;
    const cc::cd *Se = reinterpret_cast<const cc::cd *>(S) + (size_t)e * (4 * P + 1) * K * K;
    const double floor_ = cc::pivot_floor(Se, K, P);
    if (tid == 0) bad = 0;
    __syncthreads();
    for (int k = 0; k < n; ++k) {
        if (tid == 0) {
            const double d = cc::chol_pivot(Lf, cc::gram_entry(Se, K, P, k, k).re, k);
            if (!(d > floor_)) bad = 1;
            const double lkk = sqrt(d), inv = 1.0 / lkk;
            Lf[cc::chol_index(k, k)] = cc::cd{lkk, inv};
            inv_s = inv;
        }
        __syncthreads();
        if (bad) break;                                               // (the whole workgroup reads the same flag)
        for (int i = k + 1 + tid; i < n; i += THREADS) Lf[cc::chol_index(i, k)] = cc::chol_entry(Lf, cc::gram_entry(Se, K, P, i, k), i, k, inv_s);
        __syncthreads();
    }
    const int st = bad ? cc::STATUS_SINGULAR : 0;
    if (tid == 0 && blockIdx.y == 0) status[e] = st;
    if (tid < SOLVE_ROWS && row < nrows) {
        const size_t at = ((size_t)e * nrows + row) * n;
        cc::cd *hr = reinterpret_cast<cc::cd *>(h) + at;
        const cc::cd *cr = reinterpret_cast<const cc::cd *>(C) + at;
        for (int j = 0; j < n; ++j) hr[j] = cc::cd{0.0, 0.0};
        double share = 1.0;
        if (row != ref_row) {
            if (!st) cc::chol_solve(Lf, n, cr, reinterpret_cast<cc::cd *>(W) + at, hr);
            share = cc::residual_share((double)E[(size_t)e * nrows + row], hr, cr, n);
        }
        for (int j = 0; j < n; ++j) { coef[(at + j) * 2] = (float)hr[j].re; coef[(at + j) * 2 + 1] = (float)hr[j].im; }
        cinfo[((size_t)e * nrows + row) * 2] = (float)share;
        cinfo[((size_t)e * nrows + row) * 2 + 1] = row != ref_row ? (float)st : 0.f;
    }
}

} // namespace cancel
} // namespace crsdr
