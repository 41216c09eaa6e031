// caf_clean_solve.hpp -- the fp64 arithmetic of crsdr_caf's second cancellation stage (include/crsdr.h, section (w), "Cleaning";
// crsdr_caf_set_clean): its limits, the walk over the array map's detection list that picks the targets, the table of the basis
// members that the picks add behind the canceller's, where an entry of the joint normal matrix sits, and its Cholesky factor.  The solve
// itself is cc::chol_solve on the longer factor.  Plain C++ that both the kernels of caf_clean.hpp and a CPU program compile
// (tools/caf_clean_cpu.cc; tests/test_host_caf_clean.py runs these very functions under the sanitizers; cl::phase alone has a host form
// of its own).
//
// Members.  The canceller's n1 = K (2 P + 1) members come first, their indices unchanged.  Behind them, per pick in pick order,
// q = -wq .. wq outer and j = -wl .. wl inner, member (lag l + j, Doppler g = f + q / 2); a lag outside 0 .. R - 1 is left out.  A target
// member's position within its pick, whether it is left out or not, is pos = (q + wq)(2 wl + 1) + (j + wl): tcoef's index.
// The joint matrix's rows behind the canceller's (the cross block and the target block, the lower triangle) are stored dense,
// A2 [n2max][nmax], row i - n1, column j <= i.
#pragma once
#include "caf_cancel_solve.hpp"

namespace crsdr {
namespace cl {

constexpr int MAX_TARGETS = 8, MAX_WL = 2, MAX_WQ = 2, MAX_MEMBERS = 64;
constexpr int MAX_SLOTS = MAX_TARGETS * (2 * MAX_WL + 1);            // distinct member lags of a line
constexpr int MAX_PAIRS = MAX_MEMBERS * (MAX_MEMBERS + 1) / 2;       // the packed lower triangle: 2080 entries, 32.5 KiB of fp64 pairs
constexpr long long MAX_SUMS = 1ll << 24, MAX_CELLS = 1ll << 24;
constexpr int STATUS_SINGULAR = 1, STATUS_TARGET = 2;
constexpr int LAUNCHES = 9;                                          // what a submit issues more with the stage on

struct Params {
    int max_targets;
    float min_snr;
    int wl, wq;
};

CC_HD int lags_of(const Params &p) { return 2 * p.wl + 1; }
CC_HD int per_pick(const Params &p) { return (2 * p.wl + 1) * (2 * p.wq + 1); }
CC_HD int max_target_members(const Params &p) { return p.max_targets * per_pick(p); }
CC_HD int max_slots(const Params &p) { return p.max_targets * lags_of(p); }
// the distinct member lags a line can have at R lags: what the sums' buffers are sized by
CC_HD int slots_of(const Params &p, int R) { return max_slots(p) < R ? max_slots(p) : R; }

// 0, or the number of the limit that fails (caf_engine.hpp words them).  taps, dopp: the canceller's
CC_HD int bad_limit(int nd, int R, long long lines, int nrows, int taps, int dopp, const Params &p)
{
    if (p.max_targets < 1 || p.max_targets > MAX_TARGETS) return 1;
    if (p.wl < 0 || p.wl > MAX_WL) return 2;
    if (p.wq < 0 || p.wq > MAX_WQ) return 3;
    if (cc::basis(taps, dopp) + max_target_members(p) > MAX_MEMBERS) return 4;
    if (!(p.min_snr > 0.f) || !(p.min_snr <= 3.402823466e38f)) return 5;
    if (lines * nd * (taps + max_slots(p)) * R > MAX_SUMS) return 6;
    if (2 * lines * nrows * nd * R > MAX_CELLS) return 7;
    return 0;
}

// |a| around the circle of nd bins
CC_HD double circular(double a, int nd)
{
    const double g = fabs(a);
    return g > 0.5 * (double)nd ? (double)nd - g : g;
}

// a record's (lag, Doppler) as the walk reads it: fp64 sums of the published fp32 figures, so exact
CC_HD int rec_lag(const float *rec) { return (int)rec[0]; }
CC_HD double rec_doppler(const float *rec) { return (double)rec[1] + (double)rec[6]; }

// The walk over det [Kdet][8], the array map's list of a line: the indices of the accepted records into picked [max_targets], in
// their order.  Returns how many.
CC_HD int pick_walk(const float *det, int count, int Kdet, int nd, int taps, int dopp, const Params &p, int *picked)
{
    const int n = count < Kdet ? count : Kdet;
    int nt = 0;
    for (int i = 0; i < n && nt < p.max_targets; ++i) {
        const float *rec = det + (size_t)i * 8;
        const int l = rec_lag(rec);
        const double f = rec_doppler(rec);
        if ((double)rec[3] < (double)p.min_snr) continue;
        if (l - p.wl <= taps - 1 && circular(f, nd) < (double)dopp + 1.0 + 0.5 * (double)p.wq) continue;     // touches the clutter basis
        bool touches = false;
        for (int t = 0; t < nt && !touches; ++t) {
            const float *o = det + (size_t)picked[t] * 8;
            const int dl = l - rec_lag(o);
            touches = (dl < 0 ? -dl : dl) <= 2 * p.wl && circular(f - rec_doppler(o), nd) < (double)p.wq + 1.0;
        }
        if (!touches) picked[nt++] = i;
    }
    return nt;
}

// a line's members behind the canceller's
struct Table {
    int ntgt, nmem, nslot, pad;
    int slot_lag[MAX_SLOTS];                         // the distinct member lags, in the order they are first met
    int lag[MAX_MEMBERS], slot[MAX_MEMBERS], owner[MAX_MEMBERS], pos[MAX_MEMBERS];
    double g[MAX_MEMBERS];
};

CC_HD void build_table(const float *det, const int *picked, int ntgt, int R, const Params &p, Table *t)
{
    t->ntgt = ntgt; t->nmem = 0; t->nslot = 0; t->pad = 0;
    for (int o = 0; o < ntgt; ++o) {
        const float *rec = det + (size_t)picked[o] * 8;
        const int l = rec_lag(rec);
        const double f = rec_doppler(rec);
        for (int q = -p.wq; q <= p.wq; ++q)
            for (int j = -p.wl; j <= p.wl; ++j) {
                const int m = l + j;
                if (m < 0 || m >= R) continue;       // left out, not wrapped
                int s = 0;
                while (s < t->nslot && t->slot_lag[s] != m) ++s;
                if (s == t->nslot) t->slot_lag[t->nslot++] = m;
                const int i = t->nmem++;
                t->lag[i] = m; t->slot[i] = s; t->owner[i] = o; t->pos[i] = (q + p.wq) * lags_of(p) + (j + p.wl);
                t->g[i] = f + 0.5 * (double)q;
            }
    }
}

// member i of the joint basis: its lag and its Doppler
CC_HD int member_lag(const Table &t, int taps, int n1, int i) { return i < n1 ? i % taps : t.lag[i - n1]; }
CC_HD double member_doppler(const Table &t, int taps, int dopp, int n1, int i) { return i < n1 ? (double)(i / taps - dopp) : t.g[i - n1]; }

// exp(2 pi i g k / nd), as the definition evaluates it: sincospi on the device.  The host build has no sincospi and takes cos and sin
// of the argument reduced to one turn -- the same value within a few ulps, not the same arithmetic: a CPU program that compiles this
// header runs the device's own code for everything but this function.
CC_HD cc::cd phase(double g, int k, int nd)
{
    cc::cd f;
#if defined(__HIP_DEVICE_COMPILE__)
    sincospi(2.0 * ((g * (double)k) / (double)nd), &f.im, &f.re);
#else
    const double x = 2.0 * ((g * (double)k) / (double)nd), r = x - 2.0 * floor(0.5 * x);      // (pi x reduced to one turn in exact arithmetic)
    f.re = cos(3.14159265358979323846 * r); f.im = sin(3.14159265358979323846 * r);
#endif
    return f;
}

// A_ij, j <= i: the canceller's S for the leading block, A2 behind it
CC_HD cc::cd joint_entry(const cc::cd *S, const cc::cd *A2, int taps, int dopp, int n1, int stride, int i, int j)
{
    return i < n1 ? cc::gram_entry(S, taps, dopp, i, j) : A2[(size_t)(i - n1) * stride + j];
}

// The joint factor by columns in member order, as cc::chol_factor.  0, STATUS_SINGULAR (a pivot of the canceller's block at or under
// the floor) or STATUS_TARGET (a target column's).  The leading block's columns see the arithmetic of cc::chol_factor alone.
CC_HD int joint_factor(const cc::cd *S, const cc::cd *A2, int taps, int dopp, int n, int stride, cc::cd *Lf)
{
    const int n1 = cc::basis(taps, dopp);
    const double floor_ = cc::pivot_floor(S, taps, dopp);
    for (int k = 0; k < n; ++k) {
        const double d = cc::chol_pivot(Lf, joint_entry(S, A2, taps, dopp, n1, stride, k, k).re, k);
        if (!(d > floor_)) return k < n1 ? STATUS_SINGULAR : STATUS_TARGET;
        const double lkk = sqrt(d), inv = 1.0 / lkk;
        Lf[cc::chol_index(k, k)] = cc::cd{lkk, inv};
        for (int i = k + 1; i < n; ++i) Lf[cc::chol_index(i, k)] = cc::chol_entry(Lf, joint_entry(S, A2, taps, dopp, n1, stride, i, k), i, k, inv);
    }
    return 0;
}

} // namespace cl
} // namespace crsdr
