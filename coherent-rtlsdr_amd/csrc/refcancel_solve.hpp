// refcancel_solve.hpp -- the host arithmetic of the reference-noise canceller (include/crsdr.h, crsdr_plan_set_refcancel): where a Gram
// entry sits, the Cholesky factor of a block's Gram and the solve of one row's normal equations, all in fp64.  Plain C++ that both
// the kernels of refcancel.hpp and a CPU program compile (tests/test_host_refcancel.py runs these very functions under the sanitizers).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define RC_HD __host__ __device__ inline
#else
#define RC_HD inline
#endif

namespace crsdr {
namespace rc {

constexpr int MAX_TAPS = 9, MAX_K = 4;
constexpr int GRAM_PAIRS = MAX_TAPS * (MAX_TAPS + 1) / 2;      // 45 entries on and above the diagonal
constexpr int GRAM_INTS = 2 * GRAM_PAIRS;                      // (re, im) each
constexpr int STATUS_SINGULAR = 1, STATUS_IDLE = 2;            // status bit 0: the solve failed; 2: the pass did not run for this batch

struct cd { double re, im; };

// Entry (i, j), i <= j, of the 9 x 9 Gram of the taps -4 .. 4 (index = tap + 4): row-major over the upper triangle.
RC_HD int gram_index(int i, int j) { return i * MAX_TAPS - i * (i - 1) / 2 + (j - i); }

// G_ij = sum_n conj(r_i[n]) r_j[n] of the `taps` central taps (ti, tj in 0 .. taps - 1), from the packed integer sums
RC_HD cd gram_entry(const int32_t *gram, int taps, int ti, int tj)
{
    const int off = MAX_K - (taps - 1) / 2, i = ti + off, j = tj + off;
    if (i <= j) { const int32_t *g = gram + 2 * gram_index(i, j); return cd{(double)g[0], (double)g[1]}; }
    const int32_t *g = gram + 2 * gram_index(j, i);
    return cd{(double)g[0], -(double)g[1]};
}

// packed lower triangle of the factor: entry (i, k), k <= i.  The diagonal holds (L_kk, 1 / L_kk).
RC_HD int chol_index(int i, int k) { return i * (i + 1) / 2 + k; }

// G = L L^H.  false: a pivot <= 2^-40 G_00 (G_00 the centre entry, sum |r|^2) -- an all-zero or rank-deficient reference row.
RC_HD bool chol_factor(const int32_t *gram, int taps, cd *Lf)
{
    const double floor_ = ldexp((double)gram[2 * gram_index(MAX_K, MAX_K)], -40);
    for (int k = 0; k < taps; ++k) {
        double d = gram_entry(gram, taps, k, k).re;
        for (int m = 0; m < k; ++m) { const cd l = Lf[chol_index(k, m)]; d -= l.re * l.re + l.im * l.im; }
        if (!(d > floor_)) return false;
        const double lkk = sqrt(d), inv = 1.0 / lkk;
        Lf[chol_index(k, k)] = cd{lkk, inv};
        for (int i = k + 1; i < taps; ++i) {
            cd s = gram_entry(gram, taps, i, k);
            for (int m = 0; m < k; ++m) {          // s -= L_im conj(L_km)
                const cd a = Lf[chol_index(i, m)], b = Lf[chol_index(k, m)];
                s.re -= a.re * b.re + a.im * b.im;
                s.im -= a.im * b.re - a.re * b.im;
            }
            Lf[chol_index(i, k)] = cd{s.re * inv, s.im * inv};
        }
    }
    return true;
}

// g = G^-1 c from the factor (forward, then backward substitution); c is overwritten by the intermediate
RC_HD void chol_solve(const cd *Lf, int taps, cd *c, cd *g)
{
    for (int i = 0; i < taps; ++i) {
        cd s = c[i];
        for (int m = 0; m < i; ++m) {              // s -= L_im y_m
            const cd a = Lf[chol_index(i, m)], y = c[m];
            s.re -= a.re * y.re - a.im * y.im;
            s.im -= a.re * y.im + a.im * y.re;
        }
        const double inv = Lf[chol_index(i, i)].im;
        c[i] = cd{s.re * inv, s.im * inv};
    }
    for (int i = taps - 1; i >= 0; --i) {
        cd s = c[i];
        for (int m = i + 1; m < taps; ++m) {       // s -= conj(L_mi) g_m
            const cd a = Lf[chol_index(m, i)], x = g[m];
            s.re -= a.re * x.re + a.im * x.im;
            s.im -= a.re * x.im - a.im * x.re;
        }
        const double inv = Lf[chol_index(i, i)].im;
        g[i] = cd{s.re * inv, s.im * inv};
    }
}

// the share of the row's power that stays: clamp((E - Re sum conj(g_j) c_j) / E, 0, 1), 1 for E == 0
RC_HD double residual_share(double E, const cd *g, const cd *c, int taps)
{
    if (!(E > 0.0)) return 1.0;
    double s = 0.0;
    for (int j = 0; j < taps; ++j) s += g[j].re * c[j].re + g[j].im * c[j].im;
    const double r = (E - s) / E;
    return r < 0.0 ? 0.0 : (r > 1.0 ? 1.0 : r);
}

// One row from its integer sums: factor, solve, residual.  Returns the status (0 or STATUS_SINGULAR, then g = 0, residual from g = 0).
RC_HD int solve_row(const int32_t *gram, int taps, const cd *c, double E, cd *g, double *residual)
{
    cd Lf[GRAM_PAIRS], y[MAX_TAPS];
    for (int j = 0; j < taps; ++j) { y[j] = c[j]; g[j] = cd{0.0, 0.0}; }
    const bool ok = chol_factor(gram, taps, Lf);
    if (ok) chol_solve(Lf, taps, y, g);
    *residual = residual_share(E, g, c, taps);
    return ok ? 0 : STATUS_SINGULAR;
}

} // namespace rc
} // namespace crsdr
