// caf_cfar.hpp -- the decision arithmetic of the cell-averaging CFAR detector of crsdr_caf (include/crsdr.h, section (w), "Detections"):
// which cells train a cell's noise estimate and how many they are, the threshold test, the 3 x 3 neighbourhood test, the order of the
// detections and the eight figures of one.  Plain C++ on the footing of caf_peak.hpp, whose map P, signed bin s(d), searched set S and
// linear index i = d R + tau it takes over: the kernels of caf_cfar_kernels.hpp call these functions and tools/caf_cfar_cpu.cc compiles
// them for the CPU (tests/test_host_caf_cfar.py runs them under the sanitizers).  tests/caf_cfar_model.py is the fp64 statement.
// The other noise estimates (greatest-of, smallest-of, ordered statistic) are at the end: tools/caf_cfar_est_cpu.cc compiles those for the
// CPU, and tests/caf_cfar_est_model.py is their fp64 statement.
//
// Parameters: guard half-widths gd, gr over Doppler and lag, training half-widths td, tr beyond them, Hd = gd + td, Hr = gr + tr.
// Training set of a cell (d, tau) of S: the cells (d + a mod nd, tau + b) with |a| <= Hd and |b| <= Hr, not (|a| <= gd and |b| <= gr),
// 0 <= tau + b < R, and the Doppler bin in S.  Doppler wraps, lag does not.  N is the set's size, Z the fp64 sum of P over it, in any
// order but never by subtraction.
//     detected  <=>  N >= min_train,  Z > 0,  P > t  with  noise = Z / (double)N,  t = (double)alpha * noise,
//                    and P beats its (up to) eight neighbours: against q, P > P_q, or P == P_q and i < i_q; neighbours outside the lags
//                    or outside S do not count.
// det[8] = (lag, doppler = s(d), power = P, snr = P / noise, noise, dlag, ddop, ntrain = N), each rounded once to fp32; dlag and ddop are
// cafp::vertex on the same cells and with the same edge rules as caf_peak.hpp's.
// Detections are ordered by (P descending, i ascending): a strict total order, so the best K of any split of the map, joined in any
// order, are the same K.
#pragma once
#include "caf_peak.hpp"

namespace crsdr {
namespace cfar {

constexpr int MAX_HD = 8, MAX_HR = 16, MAX_DET = 64;

enum { EST_CA = 0, EST_GO = 1, EST_SO = 2, EST_OS = 3 };

// est, axis, rank: the noise estimate (below, "Estimators"); zeros are cell averaging, so seven initialisers still say what they said
struct Params { int gd, gr, td, tr; float alpha; int min_train, max_det; int est, axis, rank; };

// a candidate of one tile: everything the figures need but the neighbours' powers.  i < 0: an empty slot
struct Cand { double p, noise; int i, n; };

// 0, or the number of the limit of section (w) that (nd, prm) misses -- the messages are the caller's
CAFP_HD int bad_limit(int nd, const Params &q)
{
    if (q.gd < 0 || q.gr < 0 || q.td < 0 || q.tr < 0) return 1;
    if (q.gd > MAX_HD || q.td > MAX_HD || q.gd + q.td > MAX_HD) return 2;
    if (q.gr > MAX_HR || q.tr > MAX_HR || q.gr + q.tr > MAX_HR) return 3;
    if (q.td + q.tr < 1) return 4;
    if (2 * (q.gd + q.td) + 1 > nd) return 5;
    if (!(q.alpha > 0.f) || !(q.alpha <= 3.402823466e+38f)) return 6;      // (NaN fails the first, infinity the second)
    if (q.min_train < 1) return 7;
    if (q.max_det < 1 || q.max_det > MAX_DET) return 8;
    return 0;
}

CAFP_HD int wrap(int d, int nd) { return (d + nd) & (nd - 1); }           // nd a power of two, d >= -nd

// is (d + a mod nd, tau + b) one of the training cells of (d, tau)?
CAFP_HD bool trains(int a, int b, int d, int tau, int nd, int R, int guard, const Params &q)
{
    const int aa = a < 0 ? -a : a, bb = b < 0 ? -b : b;
    if (aa > q.gd + q.td || bb > q.gr + q.tr) return false;
    if (aa <= q.gd && bb <= q.gr) return false;
    if (tau + b < 0 || tau + b >= R) return false;
    return cafp::in_set(wrap(d + a, nd), nd, guard);
}

// the Doppler bins of S among d - h .. d + h (2 h + 1 <= nd: no bin twice), and the lags of 0 .. R - 1 among tau - h .. tau + h
CAFP_HD int bins_within(int d, int h, int nd, int guard)
{
    int n = 0;
    for (int a = -h; a <= h; ++a) n += cafp::in_set(wrap(d + a, nd), nd, guard) ? 1 : 0;
    return n;
}
CAFP_HD int lags_within(int tau, int h, int R)
{
    const int lo = tau - h < 0 ? 0 : tau - h, hi = tau + h > R - 1 ? R - 1 : tau + h;
    return hi - lo + 1;
}
// N: the window's cells less the guard block's, both products of a count over Doppler and one over lag.  Integers: exact.
CAFP_HD int train_count(int d, int tau, int nd, int R, int guard, const Params &q)
{
    return bins_within(d, q.gd + q.td, nd, guard) * lags_within(tau, q.gr + q.tr, R) - bins_within(d, q.gd, nd, guard) * lags_within(tau, q.gr, R);
}

// Z by the definition, a cell at a time (the CPU program; the kernel forms the same sum from row sums)
CAFP_HD double train_sum(const float *src, int comps, int nd, int R, int guard, const Params &q, int d, int tau)
{
    double z = 0.0;
    for (int a = -(q.gd + q.td); a <= q.gd + q.td; ++a)
        for (int b = -(q.gr + q.tr); b <= q.gr + q.tr; ++b)
            if (trains(a, b, d, tau, nd, R, guard, q)) z += cafp::power(src, comps, wrap(d + a, nd) * R + tau + b);
    return z;
}

// the threshold test; *noise is written whenever n >= 1
CAFP_HD bool over_threshold(double p, double z, int n, const Params &q, double *noise)
{
    if (n < 1) { *noise = 0.0; return false; }
    *noise = z / (double)n;
    if (n < q.min_train || !(z > 0.0)) return false;
    const double t = (double)q.alpha * *noise;
    return p > t;
}

CAFP_HD bool beats(double p, int i, double pq, int iq) { return p > pq || (p == pq && i < iq); }

// the 3 x 3 neighbourhood test of cell (d, tau), P = p
CAFP_HD bool local_max(const float *src, int comps, int nd, int R, int guard, int d, int tau, double p)
{
    const int i = d * R + tau;
    for (int a = -1; a <= 1; ++a) {
        const int dq = wrap(d + a, nd);
        if (!cafp::in_set(dq, nd, guard)) continue;
        for (int b = -1; b <= 1; ++b) {
            const int tq = tau + b;
            if ((a == 0 && b == 0) || tq < 0 || tq >= R) continue;
            const int iq = dq * R + tq;
            if (!beats(p, i, cafp::power(src, comps, iq), iq)) return false;
        }
    }
    return true;
}

// the order of the detections; an empty slot loses to everything
CAFP_HD bool before(const Cand &x, const Cand &y) { return x.i >= 0 && (y.i < 0 || beats(x.p, x.i, y.p, y.i)); }

// one cell, all of it: is (d, tau), of power p and training sum z, a detection, and if so its candidate
CAFP_HD bool detect(const float *src, int comps, int nd, int R, int guard, const Params &q, int d, int tau, double p, double z, Cand *c)
{
    if (!cafp::in_set(d, nd, guard)) return false;
    c->i = d * R + tau;
    c->p = p;
    c->n = train_count(d, tau, nd, R, guard, q);
    if (!over_threshold(p, z, c->n, q, &c->noise)) return false;
    return local_max(src, comps, nd, R, guard, d, tau, p);
}

CAFP_HD void figures(const float *src, int comps, int nd, int R, int guard, const Cand &c, float *out)
{
    if (c.i < 0) { for (int k = 0; k < 8; ++k) out[k] = 0.f; return; }
    const int d = c.i / R, tau = c.i - d * R;
    double dlag = 0.0, ddop = 0.0;
    if (tau > 0 && tau < R - 1) dlag = cafp::vertex(cafp::power(src, comps, c.i - 1), c.p, cafp::power(src, comps, c.i + 1));
    const int dm = wrap(d - 1, nd), dp = wrap(d + 1, nd);
    if (cafp::in_set(dm, nd, guard) && cafp::in_set(dp, nd, guard)) ddop = cafp::vertex(cafp::power(src, comps, dm * R + tau), c.p, cafp::power(src, comps, dp * R + tau));
    out[0] = (float)tau;
    out[1] = (float)cafp::signed_bin(d, nd);
    out[2] = (float)c.p;
    out[3] = (float)(c.p / c.noise);                  // (noise > 0: Z > 0 was required)
    out[4] = (float)c.noise;
    out[5] = (float)dlag;
    out[6] = (float)ddop;
    out[7] = (float)c.n;
}

// ---- Estimators (crsdr_cfar_est_desc).  Only noise and ntrain change with them: the training set, the threshold rule P > t with
// t = (double)alpha * noise, the neighbourhood test, the order and the figures are the ones above.
//   GO, SO   the set split in two halves by the sign of b (axis 0, lag) or of a (axis 1, Doppler); the centre line trains neither.  A half
//            counts iff its size N_h >= min_train; its mean is Z_h / (double)N_h, Z_h by additions only.  noise is the larger (GO) or
//            smaller (SO) mean of the halves that count, the lower half on equal means, and ntrain that half's N_h.  noise > 0 or
//            no detection.
//   OS       with N >= min_train, noise is the k-th smallest P of the set, k = max(1, ceil(rank N / Nfull)): a value of the map.
//            Only cells of the set take part: a cell outside the lags or S is absent, not a zero; a cell of S with P = 0 is present.

// Nfull: the training cells of a cell far from every edge
CAFP_HD int full_count(const Params &q) { return (2 * (q.gd + q.td) + 1) * (2 * (q.gr + q.tr) + 1) - (2 * q.gd + 1) * (2 * q.gr + 1); }

// 0, or which field of the estimator misses its limit (1 est, 2 axis, 3 rank)
CAFP_HD int bad_estimator(const Params &q)
{
    if (q.est < EST_CA || q.est > EST_OS) return 1;
    if ((q.est == EST_GO || q.est == EST_SO) && (q.axis < 0 || q.axis > 1)) return 2;
    if (q.est == EST_OS && (q.rank < 1 || q.rank > full_count(q))) return 3;
    return 0;
}

// the half a window offset belongs to: -1 the lower, +1 the upper, 0 the centre line
CAFP_HD int half_of(int a, int b, int axis)
{
    const int v = axis == 0 ? b : a;
    return v < 0 ? -1 : v > 0 ? 1 : 0;
}

// the Doppler bins of S among d - h .. d - 1 (side < 0) or d + 1 .. d + h, and the lags of 0 .. R - 1 among tau - h .. tau - 1 or tau + 1 .. tau + h
CAFP_HD int bins_beside(int d, int h, int side, int nd, int guard)
{
    int n = 0;
    for (int a = 1; a <= h; ++a) n += cafp::in_set(wrap(d + side * a, nd), nd, guard) ? 1 : 0;
    return n;
}
CAFP_HD int lags_beside(int tau, int h, int side, int R)
{
    const int room = side < 0 ? tau : R - 1 - tau;
    return h < room ? h : room;
}
// N_h of the half on `side` (-1, +1): as train_count, the window's cells of that half less the guard block's.  Integers: exact.
CAFP_HD int half_count(int d, int tau, int nd, int R, int guard, const Params &q, int side)
{
    if (q.axis == 0)
        return bins_within(d, q.gd + q.td, nd, guard) * lags_beside(tau, q.gr + q.tr, side, R) - bins_within(d, q.gd, nd, guard) * lags_beside(tau, q.gr, side, R);
    return bins_beside(d, q.gd + q.td, side, nd, guard) * lags_within(tau, q.gr + q.tr, R) - bins_beside(d, q.gd, side, nd, guard) * lags_within(tau, q.gr, R);
}

// Z_h by the definition, a cell at a time
CAFP_HD double half_sum(const float *src, int comps, int nd, int R, int guard, const Params &q, int d, int tau, int side)
{
    double z = 0.0;
    for (int a = -(q.gd + q.td); a <= q.gd + q.td; ++a)
        for (int b = -(q.gr + q.tr); b <= q.gr + q.tr; ++b)
            if (half_of(a, b, q.axis) == side && trains(a, b, d, tau, nd, R, guard, q)) z += cafp::power(src, comps, wrap(d + a, nd) * R + tau + b);
    return z;
}

// the half means and their choice: false with no counting half or a chosen mean that is not above 0
CAFP_HD bool choose_half(double zlo, int nlo, double zhi, int nhi, const Params &q, double *noise, int *n)
{
    const bool lo = nlo >= q.min_train && nlo >= 1, hi = nhi >= q.min_train && nhi >= 1;
    *noise = 0.0; *n = 0;
    if (!lo && !hi) return false;
    const double mlo = lo ? zlo / (double)nlo : 0.0, mhi = hi ? zhi / (double)nhi : 0.0;
    const bool upper = !lo || (hi && (q.est == EST_GO ? mhi > mlo : mhi < mlo));          // (equal means: the lower half)
    *noise = upper ? mhi : mlo;
    *n = upper ? nhi : nlo;
    return *noise > 0.0;
}

// one cell under GO or SO, all of it, as detect is under cell averaging
CAFP_HD bool detect_halves(const float *src, int comps, int nd, int R, int guard, const Params &q, int d, int tau, double p, double zlo, double zhi, Cand *c)
{
    if (!cafp::in_set(d, nd, guard)) return false;
    c->i = d * R + tau;
    c->p = p;
    if (!choose_half(zlo, half_count(d, tau, nd, R, guard, q, -1), zhi, half_count(d, tau, nd, R, guard, q, 1), q, &c->noise, &c->n)) return false;
    const double t = (double)q.alpha * c->noise;
    return p > t && local_max(src, comps, nd, R, guard, d, tau, p);
}

// k of the ordered statistic at a cell that trains on N of the Nfull cells (rank N <= 560 * 560: an int holds it)
CAFP_HD int os_rank(int rank, int N, int Nfull)
{
    const int k = (rank * N + Nfull - 1) / Nfull;
    return k < 1 ? 1 : k;
}

// The k-th smallest P of the training set by the letter of the definition: the set's members gathered and sorted.  *N: the set's
// size; with N = 0 or k outside 1 .. N the value is 0.  (The CPU program's; the kernel counts instead: k_caf_cfar_os.)
inline double os_select(const float *src, int comps, int nd, int R, int guard, const Params &q, int d, int tau, int k, int *N)
{
    double x[(2 * MAX_HD + 1) * (2 * MAX_HR + 1)];
    int n = 0;
    for (int a = -(q.gd + q.td); a <= q.gd + q.td; ++a)
        for (int b = -(q.gr + q.tr); b <= q.gr + q.tr; ++b) {
            if (!trains(a, b, d, tau, nd, R, guard, q)) continue;
            const double v = cafp::power(src, comps, wrap(d + a, nd) * R + tau + b);
            int at = n++;
            for (; at > 0 && x[at - 1] > v; --at) x[at] = x[at - 1];
            x[at] = v;
        }
    *N = n;
    return k >= 1 && k <= n ? x[k - 1] : 0.0;
}

// one cell under OS, all of it: xk the k-th smallest of its N training cells, k = os_rank
CAFP_HD bool detect_os(const float *src, int comps, int nd, int R, int guard, const Params &q, int d, int tau, double p, double xk, int N, Cand *c)
{
    if (!cafp::in_set(d, nd, guard)) return false;
    c->i = d * R + tau;
    c->p = p;
    c->n = N;
    c->noise = xk;
    if (N < 1 || N < q.min_train || !(xk > 0.0)) return false;
    const double t = (double)q.alpha * xk;
    return p > t && local_max(src, comps, nd, R, guard, d, tau, p);
}

} // namespace cfar
} // namespace crsdr
