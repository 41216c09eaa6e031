// caf_peak.hpp -- the fp64 arithmetic of the peak figures of crsdr_caf (include/crsdr.h, section (w)): where a range-Doppler map has its
// largest cell outside the zero-Doppler guard, how far that cell stands above the searched cells' mean, and the sub-cell offsets of
// the maximum.  Plain C++ that both the kernel of caf.hpp and a CPU program compile (tools/caf_peak_cpu.cc; tests/test_host_caf.py
// runs these very functions under the sanitizers).
//
// Definition (tests/caf_model.py is the fp64 statement).  A map has nd Doppler bins (FFT order) by R lags, cell i = d R + tau.
// P(i) = re^2 + im^2 of a row's published chi, evaluated in fp64, or the published array map itself.
//     s(d)    = d for d < nd / 2, else d - nd
//     S       = {(d, tau): |s(d)| >= guard}                         guard = 0: every cell; guard = g cuts 2 g - 1 bins around Doppler 0
//     (d*, tau*) = the first maximum of P over S in the order of i
//     ratio   = P* / mean of P over S                               0 if the mean is 0
//     dlag    = 0.5 (P- - P+) / (P- - 2 P* + P+) from (d*, tau* -+ 1)           0 at tau* = 0 or R - 1, 0 if the denominator is >= 0
//     ddop    = the same from (d* -+ 1 mod nd, tau*)                              0 if a neighbour is outside S, 0 if the denominator is >= 0
// both clamped to [-0.5, 0.5]; where P* = 0 (every searched cell zero) all six figures are 0.
// out[6] = (lag, doppler, power, ratio, dlag, ddop), each rounded once to fp32.
// The search is split into `step` interleaved parts (i = first, first + step, ...) that merge() joins: the kernel runs one part per
// thread, a CPU program any number.  The maximum is taken on (value, -index), so the joined result does not depend on the split or the
// order of the joins; the order of the fp64 additions of the mean is not pinned.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define CAFP_HD __host__ __device__ inline
#else
#define CAFP_HD inline
#endif

namespace crsdr {
namespace cafp {

struct Part { double best; int idx; double sum; };      // idx < 0: no cell seen

CAFP_HD int signed_bin(int d, int nd) { return d < nd / 2 ? d : d - nd; }
CAFP_HD bool in_set(int d, int nd, int guard)
{
    const int s = signed_bin(d, nd);
    return (s < 0 ? -s : s) >= guard;
}
// the number of Doppler bins in S
CAFP_HD int set_bins(int nd, int guard) { return guard <= 0 ? nd : nd - (2 * guard - 1); }

// comps = 2: src is chi [nd][R][2]; comps = 1: src is map [nd][R]
CAFP_HD double power(const float *src, int comps, int i)
{
    if (comps == 1) return (double)src[i];
    const double re = (double)src[2 * (size_t)i], im = (double)src[2 * (size_t)i + 1];
    return re * re + im * im;
}

CAFP_HD bool better(double v, int i, double bv, int bi) { return bi < 0 || v > bv || (v == bv && i < bi); }

CAFP_HD Part part(const float *src, int comps, int nd, int R, int guard, int first, int step)
{
    Part a{0.0, -1, 0.0};
    for (int i = first; i < nd * R; i += step) {
        if (!in_set(i / R, nd, guard)) continue;
        const double p = power(src, comps, i);
        a.sum += p;
        if (better(p, i, a.best, a.idx)) { a.best = p; a.idx = i; }
    }
    return a;
}

CAFP_HD void merge(Part &a, const Part &b)
{
    a.sum += b.sum;
    if (b.idx >= 0 && better(b.best, b.idx, a.best, a.idx)) { a.best = b.best; a.idx = b.idx; }
}

// the vertex of the parabola through (-1, pm), (0, p0), (1, pp)
CAFP_HD double vertex(double pm, double p0, double pp)
{
    const double den = pm - 2.0 * p0 + pp;
    if (!(den < 0.0)) return 0.0;
    const double x = 0.5 * (pm - pp) / den;
    return x < -0.5 ? -0.5 : (x > 0.5 ? 0.5 : x);
}

CAFP_HD void figures(const float *src, int comps, int nd, int R, int guard, const Part &t, float *out)
{
    if (t.idx < 0 || !(t.best > 0.0)) { for (int i = 0; i < 6; ++i) out[i] = 0.f; return; }      // nothing searched, or all of it zero
    const int d = t.idx / R, tau = t.idx - d * R;
    const double mean = t.sum / ((double)set_bins(nd, guard) * (double)R);
    double dlag = 0.0, ddop = 0.0;
    if (tau > 0 && tau < R - 1) dlag = vertex(power(src, comps, t.idx - 1), t.best, power(src, comps, t.idx + 1));
    const int dm = (d + nd - 1) & (nd - 1), dp = (d + 1) & (nd - 1);
    if (in_set(dm, nd, guard) && in_set(dp, nd, guard)) ddop = vertex(power(src, comps, dm * R + tau), t.best, power(src, comps, dp * R + tau));
    out[0] = (float)tau;
    out[1] = (float)signed_bin(d, nd);
    out[2] = (float)t.best;
    out[3] = mean > 0.0 ? (float)(t.best / mean) : 0.f;
    out[4] = (float)dlag;
    out[5] = (float)ddop;
}

} // namespace cafp
} // namespace crsdr
