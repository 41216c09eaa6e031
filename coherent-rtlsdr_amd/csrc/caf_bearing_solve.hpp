// caf_bearing_solve.hpp -- the fp64 arithmetic of crsdr_caf's bearings (include/crsdr.h, section (w), "Bearings"; crsdr_caf_set_bearing,
// crsdr_bearing): its limits, which row is which element, the training snapshots' covariance and its loading, the Cholesky factor and
// its inverse, W u and u^H W u, the co-array coefficients of a^H W a, the statistic T at a point and one level of the zoom search.
// Plain C++ that both the kernels of caf_bearing.hpp and a CPU program compile (tools/caf_bearing_cpu.cc; tests/test_host_caf_bearing.py
// runs these very functions under the sanitizers).  tests/caf_bearing_model.py is the fp64 statement.
//
// Elements e = 0 .. m - 1 are the rows c != ref_row in ascending order, e = iy mx + ix (crsdr_pmusic2d's order).  u_e = conj(chi_c) of
// the cell.  The training set is the detector's (cfar::trains), N its size:
//     Qs = sum_train u_t u_t^H (cells in the order a ascending, b ascending),  tr = sum_e Qs_ee,
//     Q' = Qs / N + loading ((tr / N) / m) I = L L^H,   Li = L^-1,   y = Li u,   W u = Li^H y,   u^H W u = sum |y_e|^2
//     W_ef = sum_{k >= max(e, f)} conj(Li_ke) Li_kf
// Packed lower triangles: entry (i, k), k <= i, at cc::chol_index(i, k); the factor's diagonal holds (L_kk, 1 / L_kk).
// a^H W a on the URA: with C[p][q] = sum of W_ef over the pairs with (fx - ex, fy - ey) = (p, q),
//     a^H W a = C[0][0] + 2 Re sum_{p > 0, or p = 0 and q > 0} C[p][q] exp(i 2 pi d (p cos(alpha) sin(beta) + q cos(beta)))
// since C[-p][-q] = conj(C[p][q]): mx (2 my - 1) coefficients, p = 0 .. mx - 1, q = -(my - 1) .. my - 1, at p (2 my - 1) + q + my - 1.
//
// A slot's record (REC doubles) carries all of this from the per-slot kernel to the scan and the zoom:
//     [0] u^H W u   [1] status   [2] 1: scan it (0: an empty slot, an all-zero snapshot or a cell outside the map)   [3] 1: W = I
//     [4 ..] W u [MAX_M] (re, im)   [4 + 2 MAX_M ..] C [MAX_COEF] (re, im)
#pragma once
#include <math.h>
#include <stdint.h>

#include "caf_cancel_solve.hpp"
#include "caf_cfar.hpp"

namespace crsdr {
namespace brg {

using cc::cd;
using cc::chol_index;

constexpr int MAX_M = 64, MIN_NC = 2, MAX_NC = 512, MAX_LEVELS = 8, SIDE = 7, POINTS = SIDE * SIDE;
constexpr int MAX_COEF = 2 * MAX_M;                            // mx (2 my - 1) < 2 m
constexpr int REC_WU = 4, REC_COEF = REC_WU + 2 * MAX_M, REC = REC_COEF + 2 * MAX_COEF;
constexpr long long MAX_SPEC = 1ll << 24;                      // (max_batch / frames) * K * ncx * ncy floats of spec
constexpr int MODE_CONVENTIONAL = 1, MODE_ADAPTIVE = 2;
constexpr unsigned KEEP_SPECTRUM = 1u;
constexpr int STATUS_ZERO = 1, STATUS_IDENTITY = 2, STATUS_CELL = 4;

struct Params { int mx, my, ncx, ncy; float d; int mode; float loading; int levels; unsigned flags; };

// 0, or the number of the limit of section (w) that fails (caf_engine.hpp words them)
CAFP_HD int bad_limit(int nrows, long long lines, int K, const Params &q)
{
    if (q.mx < 1 || q.my < 1) return 1;
    const long long m = (long long)q.mx * (long long)q.my;
    if (m < 2 || m > MAX_M || m != (long long)nrows - 1) return 2;
    if (q.ncx < MIN_NC || q.ncx > MAX_NC || q.ncy < MIN_NC || q.ncy > MAX_NC) return 3;
    if (!(q.d > 0.f) || !(q.d <= 3.402823466e+38f)) return 4;             // (NaN fails the first, infinity the second)
    if (q.mode != MODE_CONVENTIONAL && q.mode != MODE_ADAPTIVE) return 5;
    if (q.mode == MODE_ADAPTIVE && !(q.loading >= 1e-6f && q.loading <= 1.f)) return 6;
    if (q.levels < 0 || q.levels > MAX_LEVELS) return 7;
    if (q.flags & ~KEEP_SPECTRUM) return 8;
    if ((q.flags & KEEP_SPECTRUM) && lines * K * q.ncx * q.ncy > MAX_SPEC) return 9;
    return 0;
}

CAFP_HD int row_of(int e, int ref_row) { return e < ref_row ? e : e + 1; }
CAFP_HD int coefs(int mx, int my) { return mx * (2 * my - 1); }
CAFP_HD int coef_index(int p, int q, int my) { return p * (2 * my - 1) + q + my - 1; }

// u_e at cell i of a line's chi [nrows][cells][2]
CAFP_HD cd snap_elem(const float *chi, size_t cells, int ref_row, int e, int i)
{
    const float *p = chi + 2 * ((size_t)row_of(e, ref_row) * cells + (size_t)i);
    return cd{(double)p[0], -(double)p[1]};
}

// packed entry p -> (i, k), k <= i
CAFP_HD void pair_of(int p, int *i, int *k)
{
    int r = (int)((sqrt(8.0 * (double)p + 1.0) - 1.0) * 0.5);
    while ((r + 1) * (r + 2) / 2 <= p) ++r;
    while (r * (r + 1) / 2 > p) --r;
    *i = r;
    *k = p - r * (r + 1) / 2;
}

// acc += u_i conj(u_k)
CAFP_HD void cov_add(cd *acc, cd ui, cd uk)
{
    acc->re += ui.re * uk.re + ui.im * uk.im;
    acc->im += ui.im * uk.re - ui.re * uk.im;
}

// Qs of the cell (d, tau), every entry summed over the training cells in the order a ascending, b ascending; returns N
CAFP_HD int train_cov(const float *chi, int m, int nd, int R, int ref_row, int guard, const cfar::Params &cp, int d, int tau, cd *Qs)
{
    const int Hd = cp.gd + cp.td, Hr = cp.gr + cp.tr;
    const size_t cells = (size_t)nd * (size_t)R;
    for (int p = 0; p < m * (m + 1) / 2; ++p) Qs[p] = cd{0.0, 0.0};
    int N = 0;
    for (int a = -Hd; a <= Hd; ++a)
        for (int b = -Hr; b <= Hr; ++b) {
            if (!cfar::trains(a, b, d, tau, nd, R, guard, cp)) continue;
            const int i = cfar::wrap(d + a, nd) * R + tau + b;
            ++N;
            for (int r = 0; r < m; ++r)
                for (int k = 0; k <= r; ++k) cov_add(&Qs[chol_index(r, k)], snap_elem(chi, cells, ref_row, r, i), snap_elem(chi, cells, ref_row, k, i));
        }
    return N;
}

CAFP_HD double trace_of(const cd *Qs, int m)
{
    double t = 0.0;
    for (int e = 0; e < m; ++e) t += Qs[chol_index(e, e)].re;
    return t;
}

// entry (i, k) of Q' from the sums
CAFP_HD cd loaded_entry(cd s, int i, int k, int N, double tr, int m, float loading)
{
    const double n = (double)N;
    cd q{s.re / n, s.im / n};
    if (i == k) { q.re += (double)loading * ((tr / n) / (double)m); q.im = 0.0; }
    return q;
}

// Q' = L L^H in place; false: a pivot that is not > 0 (only non-finite input gives one)
CAFP_HD bool factor(cd *Lf, int m)
{
    for (int k = 0; k < m; ++k) {
        const double d = cc::chol_pivot(Lf, Lf[chol_index(k, k)].re, k);
        if (!(d > 0.0)) return false;
        const double lkk = sqrt(d), inv = 1.0 / lkk;
        Lf[chol_index(k, k)] = cd{lkk, inv};
        for (int i = k + 1; i < m; ++i) Lf[chol_index(i, k)] = cc::chol_entry(Lf, Lf[chol_index(i, k)], i, k, inv);
    }
    return true;
}

// column j of Li = L^-1 (entries i >= j), each from the ones above it
CAFP_HD void inv_column(const cd *Lf, cd *Li, int m, int j)
{
    Li[chol_index(j, j)] = cd{Lf[chol_index(j, j)].im, 0.0};
    for (int i = j + 1; i < m; ++i) {
        cd s{0.0, 0.0};
        for (int k = j; k < i; ++k) {
            const cd a = Lf[chol_index(i, k)], x = Li[chol_index(k, j)];
            s.re += a.re * x.re - a.im * x.im;
            s.im += a.re * x.im + a.im * x.re;
        }
        const double inv = Lf[chol_index(i, i)].im;
        Li[chol_index(i, j)] = cd{-s.re * inv, -s.im * inv};
    }
}

// y_i = sum_{k <= i} Li_ik u_k
CAFP_HD cd fwd_entry(const cd *Li, const cd *u, int i)
{
    cd s{0.0, 0.0};
    for (int k = 0; k <= i; ++k) {
        const cd a = Li[chol_index(i, k)], x = u[k];
        s.re += a.re * x.re - a.im * x.im;
        s.im += a.re * x.im + a.im * x.re;
    }
    return s;
}

// (W u)_k = sum_{i >= k} conj(Li_ik) y_i
CAFP_HD cd bwd_entry(const cd *Li, const cd *y, int m, int k)
{
    cd s{0.0, 0.0};
    for (int i = k; i < m; ++i) {
        const cd a = Li[chol_index(i, k)], x = y[i];
        s.re += a.re * x.re + a.im * x.im;
        s.im += a.re * x.im - a.im * x.re;
    }
    return s;
}

CAFP_HD double norm2(const cd *y, int m)
{
    double t = 0.0;
    for (int e = 0; e < m; ++e) t += y[e].re * y[e].re + y[e].im * y[e].im;
    return t;
}

CAFP_HD cd w_entry(const cd *Li, int m, int e, int f)
{
    cd s{0.0, 0.0};
    for (int k = e > f ? e : f; k < m; ++k) {
        const cd a = Li[chol_index(k, e)], b = Li[chol_index(k, f)];
        s.re += a.re * b.re + a.im * b.im;
        s.im += a.re * b.im - a.im * b.re;
    }
    return s;
}

// C[p][q], p >= 0: the pairs in the order of e
CAFP_HD cd coef(const cd *Li, int mx, int my, int p, int q)
{
    cd s{0.0, 0.0};
    for (int ey = 0; ey < my; ++ey) {
        const int fy = ey + q;
        if (fy < 0 || fy >= my) continue;
        for (int ex = 0; ex + p < mx; ++ex) {
            const cd w = w_entry(Li, mx * my, ey * mx + ex, fy * mx + ex + p);
            s.re += w.re;
            s.im += w.im;
        }
    }
    return s;
}

// everything of one slot behind its snapshot, for the CPU program (the kernel spreads the same calls over its threads).
// Qs: the sums, factored in place; Li, y: scratch; rec [REC].  N and Qs as train_cov left them (conventional: unused).
CAFP_HD void solve_slot(const Params &bp, const cd *u, cd *Qs, int N, cd *Li, cd *y, double *rec)
{
    const int m = bp.mx * bp.my;
    for (int i = 0; i < REC; ++i) rec[i] = 0.0;
    const double uu = norm2(u, m);
    if (uu == 0.0) { rec[1] = (double)STATUS_ZERO; return; }
    int status = 0;
    bool ident = bp.mode != MODE_ADAPTIVE;
    if (!ident) {
        const double tr = trace_of(Qs, m);
        if (N == 0 || !(tr > 0.0)) ident = true;
        else {
            for (int i = 0; i < m; ++i)
                for (int k = 0; k <= i; ++k) Qs[chol_index(i, k)] = loaded_entry(Qs[chol_index(i, k)], i, k, N, tr, m, bp.loading);
            if (!factor(Qs, m)) ident = true;
        }
        if (ident) status |= STATUS_IDENTITY;
    }
    cd *wu = reinterpret_cast<cd *>(rec + REC_WU), *C = reinterpret_cast<cd *>(rec + REC_COEF);
    if (ident) {
        for (int e = 0; e < m; ++e) wu[e] = u[e];
        rec[0] = uu;
    } else {
        for (int j = 0; j < m; ++j) inv_column(Qs, Li, m, j);
        for (int i = 0; i < m; ++i) y[i] = fwd_entry(Li, u, i);
        for (int k = 0; k < m; ++k) wu[k] = bwd_entry(Li, y, m, k);
        rec[0] = norm2(y, m);
        for (int c = 0; c < coefs(bp.mx, bp.my); ++c) C[c] = coef(Li, bp.mx, bp.my, c / (2 * bp.my - 1), c % (2 * bp.my - 1) - (bp.my - 1));
    }
    rec[1] = (double)status; rec[2] = 1.0; rec[3] = ident ? 1.0 : 0.0;
}

CAFP_HD void sin_cos(double ph, double *s, double *c)
{
#if defined(__HIP_DEVICE_COMPILE__)
    sincos(ph, s, c);
#else
    *s = sin(ph); *c = cos(ph);
#endif
}

// T at the cell coordinates (x, y) from a slot's record
CAFP_HD double stat(const double *rec, int mx, int my, float d, int ncx, int ncy, double x, double y)
{
    if (rec[2] == 0.0) return 0.0;
    const double pi = 3.14159265358979323846;
    const double alpha = x * pi / (double)ncx, beta = y * pi / (double)ncy;
    const double ca = cos(alpha), sb = sin(beta), cb = cos(beta);
    const bool ident = rec[3] != 0.0;
    const double *wu = rec + REC_WU, *C = rec + REC_COEF;
    double nr = 0.0, ni = 0.0, den = ident ? (double)(mx * my) : C[2 * coef_index(0, 0, my)];
    for (int iy = 0; iy < my; ++iy)
        for (int ix = 0; ix < mx; ++ix) {
            const int e = iy * mx + ix;
            const double ph = 2.0 * pi * (double)d * ((double)ix * ca * sb + (double)iy * cb);
            double s, c;
            sin_cos(ph, &s, &c);
            nr += c * wu[2 * e] + s * wu[2 * e + 1];                 // conj(a_e) (W u)_e
            ni += c * wu[2 * e + 1] - s * wu[2 * e];
            if (!ident && e > 0) { const double *k = C + 2 * coef_index(ix, iy, my); den += 2.0 * (k[0] * c - k[1] * s); }
        }
    if (!ident)
        for (int iy = 1; iy < my; ++iy)
            for (int ix = 1; ix < mx; ++ix) {
                const double ph = 2.0 * pi * (double)d * ((double)ix * ca * sb - (double)iy * cb);
                double s, c;
                sin_cos(ph, &s, &c);
                const double *k = C + 2 * coef_index(ix, -iy, my);
                den += 2.0 * (k[0] * c - k[1] * s);
            }
    return (nr * nr + ni * ni) / (den * rec[0]);
}

// lattice point q of a level around (x, y)
CAFP_HD void lattice_point(double x, double y, double step, int q, int ncx, int ncy, double *px, double *py)
{
    *px = fmin(fmax(x + (double)(q / SIDE - SIDE / 2) * step, 0.0), (double)ncx);
    *py = fmin(fmax(y + (double)(q % SIDE - SIDE / 2) * step, 0.0), (double)ncy);
}

// one level's walk over f [POINTS]: the centre keeps ties, a NaN never wins, the lowest index wins equal values
CAFP_HD void zoom_pick(const double *f, double step, int ncx, int ncy, double *x, double *y)
{
    const double c = f[POINTS / 2];
    double best = c, bx = *x, by = *y;
    for (int q = 0; q < POINTS; ++q) {
        if (q == POINTS / 2) continue;
        const double v = f[q];
        if (v > c && v > best) { best = v; lattice_point(*x, *y, step, q, ncx, ncy, &bx, &by); }
    }
    *x = bx; *y = by;
}

// the eight figures of a slot
CAFP_HD void figures(const double *rec, int cx, int cy, double tg, double x, double y, int ncx, int ncy, float *out)
{
    if (rec[2] == 0.0) { for (int k = 0; k < 7; ++k) out[k] = 0.f; out[7] = (float)rec[1]; return; }
    const double pi = 3.14159265358979323846;
    out[0] = (float)cx; out[1] = (float)cy; out[2] = (float)tg;
    out[3] = (float)(x - (double)cx); out[4] = (float)(y - (double)cy);
    out[5] = (float)(x * pi / (double)ncx); out[6] = (float)(y * pi / (double)ncy);
    out[7] = (float)rec[1];
}

// the cell a detection names, or -1 where its figures lie outside the map
CAFP_HD int cell_of(const float *det, int nd, int R)
{
    const float lag = det[0], dop = det[1];
    if (!(lag >= 0.f && lag < (float)R) || !(dop >= (float)(-nd / 2) && dop < (float)(nd / 2))) return -1;
    const int tau = (int)lag, s = (int)dop;
    return cfar::wrap(s, nd) * R + tau;
}

} // namespace brg
} // namespace crsdr
