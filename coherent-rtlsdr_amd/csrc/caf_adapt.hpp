// caf_adapt.hpp -- the decisions of crsdr_caf's adaptive beams (include/crsdr.h, section (w), "Adaptive beams"; crsdr_caf_set_beam_adapt,
// crsdr_beam_adapt): the limits, the enumeration of a line's training cells and of their tiles, the order of the partial sums, the
// line's solve on the bearings' fp64 Cholesky pieces (caf_bearing_solve.hpp), the figures and the fallback.  Plain C++ that both the
// kernels of caf_adapt_kernels.hpp and a CPU program compile (tools/caf_adapt_cpu.cc; tests/test_host_caf_adapt.py runs these very
// functions under the sanitizers).  tests/caf_adapt_model.py is the fp64 statement.
//
// Elements e = 0 .. m - 1 are the rows c != ref_row in ascending order (brg::row_of), u_e = conj(chi_c(e)[cell]) (brg::snap_elem).
// Training cell t = 0 .. N - 1, N = d_n r_n:  a = t / r_n, b = t % r_n,  Doppler (d_lo + a) mod nd, lag r_lo + b.
// Tiles: the cells are cut into chunks of CHUNK; a tile is tile_chunks(N) consecutive chunks, so that there are at most MAX_TILES
// tiles, and their number depends on N alone.  The sums of a tile are formed in any order (every product of two fp32 values is exact
// in fp64); the tiles' sums are added in ascending order:
//     Qs = sum_tiles (sum_{t in tile} u_t u_t^H)      packed lower triangle, entry (i, k), k <= i, at chol_index(i, k); Im Qs_ii = 0
//     tr = sum_e Qs_ee,   Q = Qs / N,   Q' = Q + loading ((tr / N) / m) I = L L^H,   Li = L^-1
// Per beam b with the caller's v (fp64 from its fp32 parts):
//     y = Li v,  g = Li^H y = Q'^-1 v,  den = v^H g = |y|^2,  w = (v^H v / den) g        aw = (float) w, each part rounded once
//     ainfo = ((float)(w^H Q w), (float)(v^H Q v)),  x^H Q x = sum_i Re(conj(x_i) sum_j Q_ij x_j), i ascending
// A beam whose v is all zero keeps it.  Fallback of a line (aw = v bit for bit, ainfo = 0): tr == 0: STATUS_ZERO; tr not finite or a
// pivot not > 0: STATUS_SOLVE.
#pragma once
#include <math.h>
#include <stdint.h>

#include "caf_bearing_solve.hpp"

namespace crsdr {
namespace ad {

using brg::cd;
using brg::chol_index;

constexpr int MAX_M = 64, CHUNK = 64, MAX_TILES = 64;
constexpr int STATUS_ZERO = 1, STATUS_SOLVE = 2;

struct Params { int d_lo, d_n, r_lo, r_n; float loading; unsigned flags; };

// 0, or the number of the limit of section (w) that fails (caf_engine.hpp words them)
CAFP_HD int bad_limit(int nrows, int nd, int R, const Params &q)
{
    if (nrows - 1 < 1 || nrows - 1 > MAX_M) return 1;
    if (q.d_lo < 0 || q.d_lo >= nd) return 2;
    if (q.d_n < 1 || q.d_n > nd) return 3;
    if (q.r_lo < 0) return 4;
    if (q.r_n < 1) return 5;
    if ((long long)q.r_lo + (long long)q.r_n > (long long)R) return 6;
    if (!(q.loading >= 1e-6f && q.loading <= 1.f)) return 7;                // (NaN fails both)
    if (q.flags) return 8;
    return 0;
}

CAFP_HD int cells_of(const Params &q) { return q.d_n * q.r_n; }
CAFP_HD int tile_chunks(int N) { return ((N + CHUNK - 1) / CHUNK + MAX_TILES - 1) / MAX_TILES; }
CAFP_HD int tile_cells(int N) { return tile_chunks(N) * CHUNK; }
CAFP_HD int tiles_of(int N) { return (N + tile_cells(N) - 1) / tile_cells(N); }
CAFP_HD int pairs_of(int m) { return m * (m + 1) / 2; }

// training cell t -> its index d R + tau in the line's map
CAFP_HD int cell_of(const Params &q, int nd, int R, int t)
{
    const int a = t / q.r_n, b = t - a * q.r_n;
    int d = q.d_lo + a;
    if (d >= nd) d -= nd;
    return d * R + q.r_lo + b;
}

// the sums of one tile, P [pairs_of(m)]: chi [nrows][cells][2] of the line
CAFP_HD void tile_cov(const float *chi, int m, int nd, int R, int ref_row, const Params &q, int tile, cd *P)
{
    const size_t cells = (size_t)nd * (size_t)R;
    const int N = cells_of(q), tc = tile_cells(N), t0 = tile * tc, t1 = t0 + tc < N ? t0 + tc : N;
    for (int p = 0; p < pairs_of(m); ++p) P[p] = cd{0.0, 0.0};
    for (int t = t0; t < t1; ++t) {
        const int i = cell_of(q, nd, R, t);
        for (int r = 0; r < m; ++r)
            for (int k = 0; k <= r; ++k) brg::cov_add(&P[chol_index(r, k)], brg::snap_elem(chi, cells, ref_row, r, i), brg::snap_elem(chi, cells, ref_row, k, i));
    }
    for (int r = 0; r < m; ++r) P[chol_index(r, r)].im = 0.0;
}

// entry p of Qs: the tiles' sums in ascending order; part [tiles][pairs][2]
CAFP_HD cd tile_sum(const double *part, int tiles, int pairs, int p)
{
    cd s{0.0, 0.0};
    for (int t = 0; t < tiles; ++t) { s.re += part[2 * ((size_t)t * pairs + p)]; s.im += part[2 * ((size_t)t * pairs + p) + 1]; }
    return s;
}

// 0, or the fallback that the trace alone decides (a non-finite sum anywhere in Qs makes a diagonal entry non-finite)
CAFP_HD int trace_status(double tr)
{
    if (tr == 0.0) return STATUS_ZERO;
    return tr > 0.0 && tr <= 1.7976931348623157e308 ? 0 : STATUS_SOLVE;
}

// entry (i, k) of the unloaded Q from the sums
CAFP_HD cd plain_entry(cd s, int i, int k, int N)
{
    const double n = (double)N;
    return cd{s.re / n, i == k ? 0.0 : s.im / n};
}

CAFP_HD cd weight_of(const float *v, int e) { return cd{(double)v[2 * e], (double)v[2 * e + 1]}; }

// w_e from g_e
CAFP_HD cd scaled(cd g, double vv, double den)
{
    const double s = vv / den;
    return cd{s * g.re, s * g.im};
}

// Re(conj(x_i) sum_j Q_ij x_j), Q the packed lower triangle of a Hermitian matrix
CAFP_HD double quad_row(const cd *Q, const cd *x, int m, int i)
{
    cd s{0.0, 0.0};
    for (int j = 0; j < m; ++j) {
        const cd a = j <= i ? Q[chol_index(i, j)] : cd{Q[chol_index(j, i)].re, -Q[chol_index(j, i)].im};
        s.re += a.re * x[j].re - a.im * x[j].im;
        s.im += a.re * x[j].im + a.im * x[j].re;
    }
    return x[i].re * s.re + x[i].im * s.im;
}

CAFP_HD double sum_of(const double *t, int m)
{
    double s = 0.0;
    for (int e = 0; e < m; ++e) s += t[e];
    return s;
}

// the fallback of a line: the caller's weights bit for bit, no figures
CAFP_HD void keep_line(const float *v, int m, int nbeams, float *aw, float *ainfo)
{
    for (int k = 0; k < 2 * nbeams * m; ++k) aw[k] = v[k];
    for (int k = 0; k < 2 * nbeams; ++k) ainfo[k] = 0.f;
}

// everything of one line behind its tiles' sums, for the CPU program (the kernel spreads the same calls over its threads).
// part [tiles][pairs][2]; v [nbeams][m][2]; Lf, Li, Q: pairs_of(m) each; x: 3 m; t: 2 m.  Returns the line's status.
inline int solve_line(const Params &q, int m, int nbeams, const double *part, const float *v, cd *Lf, cd *Li, cd *Q, cd *x, double *t, float *aw, float *ainfo)
{
    const int N = cells_of(q), tiles = tiles_of(N), pairs = pairs_of(m);
    for (int p = 0; p < pairs; ++p) Lf[p] = tile_sum(part, tiles, pairs, p);
    const double tr = brg::trace_of(Lf, m);
    int status = trace_status(tr);
    if (!status) {
        for (int i = 0; i < m; ++i)
            for (int k = 0; k <= i; ++k) {
                Q[chol_index(i, k)] = plain_entry(Lf[chol_index(i, k)], i, k, N);
                Lf[chol_index(i, k)] = brg::loaded_entry(Lf[chol_index(i, k)], i, k, N, tr, m, q.loading);
            }
        if (!brg::factor(Lf, m)) status = STATUS_SOLVE;
    }
    if (status) { keep_line(v, m, nbeams, aw, ainfo); return status; }
    for (int j = 0; j < m; ++j) brg::inv_column(Lf, Li, m, j);
    cd *V = x, *Y = x + m, *G = x + 2 * m;
    for (int b = 0; b < nbeams; ++b) {
        const float *vb = v + 2 * (size_t)b * m;
        for (int e = 0; e < m; ++e) V[e] = weight_of(vb, e);
        for (int e = 0; e < m; ++e) Y[e] = brg::fwd_entry(Li, V, e);
        const double vv = brg::norm2(V, m), den = brg::norm2(Y, m);
        for (int e = 0; e < m; ++e) G[e] = vv > 0.0 ? scaled(brg::bwd_entry(Li, Y, m, e), vv, den) : V[e];
        for (int e = 0; e < m; ++e) {
            float *o = aw + 2 * ((size_t)b * m + e);
            if (vv > 0.0) { o[0] = (float)G[e].re; o[1] = (float)G[e].im; } else { o[0] = vb[2 * e]; o[1] = vb[2 * e + 1]; }
            t[e] = quad_row(Q, G, m, e);
            t[m + e] = quad_row(Q, V, m, e);
        }
        ainfo[2 * b] = (float)sum_of(t, m);
        ainfo[2 * b + 1] = (float)sum_of(t + m, m);
    }
    return 0;
}

} // namespace ad
} // namespace crsdr
