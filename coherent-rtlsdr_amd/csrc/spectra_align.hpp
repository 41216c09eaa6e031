// spectra_align.hpp -- the fp64 arithmetic of the alignment figures of crsdr_spectra (include/crsdr.h, section (v)): residual delay,
// residual phase, gain and coherence of a row against row 0, from the published fp32 psd and cross.  Plain C++ that both the kernel of
// spectra.hpp and a CPU program compile (tools/spectra_align_cpu.cc; tests/test_host_spectra.py runs these very functions under the
// sanitizers).
//
// Definition (tests/spectra_model.py is the fp64 statement).  Band: signed bins s_i = lo + i, i < K, bin f_i = s_i mod N.
//     A         = sum_{i < K-1} S_c[f_{i+1}] conj(S_c[f_i])
//     delay     = -atan2(Im A, Re A) N / (2 pi)                    0 if A == 0
//     z         = sum_i S_c[f_i] exp(+2 pi i s_i delay / N)
//     phase     = atan2(Im z, Re z)
//     gain      = |z| / sum_i P_0[f_i]                             0 if the denominator is 0
//     coherence = min(1, sum_i |S_c[f_i]|^2 / sum_i P_0[f_i] P_c[f_i])     0 if the denominator is 0
// The sums are split into `step` interleaved parts (i = first, first + step, ...) that are added afterwards: the kernel runs one part
// per lane of a wave, a CPU program one part in all.  The order of the fp64 additions is not pinned.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SPA_HD __host__ __device__ inline
#else
#define SPA_HD inline
#endif

namespace crsdr {
namespace spa {

constexpr double kTwoPi = 6.283185307179586476925286766559;

// pass 1: A's part.  pass 2 (behind the delay): z's part, sum P_0, sum |S|^2, sum P_0 P_c
struct Lag { double re, im; };
struct Sums { double zre, zim, p0, ss, pp; };

SPA_HD int band_bin(int s, int N) { return s & (N - 1); }      // s mod N for a power of two, negative s included

// p0, pc [N] float, sc [N][2] float
SPA_HD Lag lag_part(const float *sc, int N, int lo, int K, int first, int step)
{
    Lag a{0.0, 0.0};
    for (int i = first; i + 1 < K; i += step) {
        const int f0 = band_bin(lo + i, N), f1 = band_bin(lo + i + 1, N);
        const double xr = (double)sc[2 * f1], xi = (double)sc[2 * f1 + 1], yr = (double)sc[2 * f0], yi = (double)sc[2 * f0 + 1];
        a.re += xr * yr + xi * yi;               // x conj(y)
        a.im += xi * yr - xr * yi;
    }
    return a;
}

SPA_HD double delay_of(Lag a, int N)
{
    if (a.re == 0.0 && a.im == 0.0) return 0.0;
    return -atan2(a.im, a.re) * (double)N / kTwoPi;
}

SPA_HD Sums sums_part(const float *p0, const float *pc, const float *sc, int N, int lo, int K, double delay, int first, int step)
{
    Sums t{0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = first; i < K; i += step) {
        const int s = lo + i, f = band_bin(s, N);
        const double xr = (double)sc[2 * f], xi = (double)sc[2 * f + 1], a = kTwoPi * (double)s * delay / (double)N;
        const double c = cos(a), sn = sin(a);
        t.zre += xr * c - xi * sn;
        t.zim += xr * sn + xi * c;
        t.p0 += (double)p0[f];
        t.ss += xr * xr + xi * xi;
        t.pp += (double)p0[f] * (double)pc[f];
    }
    return t;
}

// out = (delay, phase, gain, coherence), each rounded once
SPA_HD void figures(double delay, Sums t, float *out)
{
    const double phase = (t.zre == 0.0 && t.zim == 0.0) ? 0.0 : atan2(t.zim, t.zre);
    const double gain = t.p0 > 0.0 ? sqrt(t.zre * t.zre + t.zim * t.zim) / t.p0 : 0.0;
    double coh = t.pp > 0.0 ? t.ss / t.pp : 0.0;
    if (coh > 1.0) coh = 1.0;
    out[0] = (float)delay; out[1] = (float)phase; out[2] = (float)gain; out[3] = (float)coh;
}

} // namespace spa
} // namespace crsdr
