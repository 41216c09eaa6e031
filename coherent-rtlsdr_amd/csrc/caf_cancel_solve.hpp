// caf_cancel_solve.hpp -- the fp64 arithmetic of crsdr_caf's direct-path and clutter canceller (include/crsdr.h, section (w),
// crsdr_caf_set_cancel): its limits, where a basis member and an entry of the normal matrix sit, the Cholesky factor of a line's matrix,
// the solve of one row's normal equations and the share of the row's power that stays.  Plain C++ that both the kernels of
// caf_cancel.hpp and a CPU program compile (tools/caf_cancel_cpu.cc; tests/test_host_caf_cancel.py runs these very functions under the
// sanitizers).
//
// Basis member (m, p), 0 <= m < K = taps, -P <= p <= P = dopp, has the index j = (p + P) K + m (m fastest within p), n = K (2 P + 1).
// The normal matrix depends on (m, m', p - p') alone: A_(m',p'),(m,p) = S[p - p'][m][m'], S[q][m][m'] = sum_k phi_q[k] G[k][m][m'],
// q = -2 P .. 2 P, stored S [4 P + 1][K][K].
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define CC_HD __host__ __device__ inline
#else
#define CC_HD inline
#endif

namespace crsdr {
namespace cc {

constexpr int MAX_TAPS = 32, MAX_DOPP = 2, MAX_BASIS = 48;
constexpr int MAX_PAIRS = MAX_BASIS * (MAX_BASIS + 1) / 2;     // the packed lower triangle: 1176 entries, 18.4 KiB of fp64 pairs
constexpr long long MAX_SUMS = 1ll << 24;                      // (max_batch / frames) * nd * K * R entries of G
constexpr int STATUS_SINGULAR = 1;

struct cd { double re, im; };

CC_HD int basis(int taps, int dopp) { return taps * (2 * dopp + 1); }

// 0, or the number of the limit that fails (caf_engine.hpp words them)
CC_HD int bad_limit(int nd, int R, long long lines, int taps, int dopp)
{
    if (dopp < 0 || dopp > MAX_DOPP) return 1;
    if (taps < 1 || taps > R || taps > MAX_TAPS) return 2;
    if (basis(taps, dopp) > MAX_BASIS) return 3;
    if (2 * dopp + 1 > nd) return 4;
    if (lines * nd * taps * R > MAX_SUMS) return 5;
    return 0;
}

// A_ij, i = (m', p') the row and j = (m, p) the column, from S
CC_HD cd gram_entry(const cd *S, int taps, int dopp, int i, int j)
{
    const int mi = i % taps, pi = i / taps, mj = j % taps, pj = j / taps;
    return S[((pj - pi + 2 * dopp) * taps + mj) * taps + mi];
}

// packed lower triangle of the factor: entry (i, k), k <= i.  The diagonal holds (L_kk, 1 / L_kk).
CC_HD int chol_index(int i, int k) { return i * (i + 1) / 2 + k; }

// A = L L^H by columns.  Column k from the columns in front of it: the pivot d = A_kk - sum_{m < k} |L_km|^2, then every entry below it
// on its own -- the kernel gives each to a thread, the sums in the same order as here.
CC_HD double chol_pivot(const cd *Lf, double akk, int k)
{
    double d = akk;
    for (int m = 0; m < k; ++m) { const cd l = Lf[chol_index(k, m)]; d -= l.re * l.re + l.im * l.im; }
    return d;
}

CC_HD cd chol_entry(const cd *Lf, cd aik, int i, int k, double inv)
{
    cd s = aik;
    for (int m = 0; m < k; ++m) {                  // s -= L_im conj(L_km)
        const cd a = Lf[chol_index(i, m)], b = Lf[chol_index(k, m)];
        s.re -= a.re * b.re + a.im * b.im;
        s.im -= a.im * b.re - a.re * b.im;
    }
    return cd{s.re * inv, s.im * inv};
}

// the pivot floor: 2^-40 A_(0,0),(0,0) = 2^-40 sum |X_r|^2 over the line
CC_HD double pivot_floor(const cd *S, int taps, int dopp) { return ldexp(gram_entry(S, taps, dopp, 0, 0).re, -40); }

// false: a pivot <= the floor -- an all-zero or rank-deficient reference
CC_HD bool chol_factor(const cd *S, int taps, int dopp, cd *Lf)
{
    const int n = basis(taps, dopp);
    const double floor_ = pivot_floor(S, taps, dopp);
    for (int k = 0; k < n; ++k) {
        const double d = chol_pivot(Lf, gram_entry(S, taps, dopp, k, k).re, k);
        if (!(d > floor_)) return false;
        const double lkk = sqrt(d), inv = 1.0 / lkk;
        Lf[chol_index(k, k)] = cd{lkk, inv};
        for (int i = k + 1; i < n; ++i) Lf[chol_index(i, k)] = chol_entry(Lf, gram_entry(S, taps, dopp, i, k), i, k, inv);
    }
    return true;
}

// h = A^-1 c from the factor (forward, then backward substitution); y [n] takes the intermediate
CC_HD void chol_solve(const cd *Lf, int n, const cd *c, cd *y, cd *h)
{
    for (int i = 0; i < n; ++i) {
        cd s = c[i];
        for (int m = 0; m < i; ++m) {              // s -= L_im y_m
            const cd a = Lf[chol_index(i, m)], v = y[m];
            s.re -= a.re * v.re - a.im * v.im;
            s.im -= a.re * v.im + a.im * v.re;
        }
        const double inv = Lf[chol_index(i, i)].im;
        y[i] = cd{s.re * inv, s.im * inv};
    }
    for (int i = n - 1; i >= 0; --i) {
        cd s = y[i];
        for (int m = i + 1; m < n; ++m) {          // s -= conj(L_mi) h_m
            const cd a = Lf[chol_index(m, i)], x = h[m];
            s.re -= a.re * x.re + a.im * x.im;
            s.im -= a.re * x.im - a.im * x.re;
        }
        const double inv = Lf[chol_index(i, i)].im;
        h[i] = cd{s.re * inv, s.im * inv};
    }
}

// the share of the row's power that stays: clamp((E - Re sum conj(h_j) c_j) / E, 0, 1), 1 for E == 0
CC_HD double residual_share(double E, const cd *h, const cd *c, int n)
{
    if (!(E > 0.0)) return 1.0;
    double s = 0.0;
    for (int j = 0; j < n; ++j) s += h[j].re * c[j].re + h[j].im * c[j].im;
    const double r = (E - s) / E;
    return r < 0.0 ? 0.0 : (r > 1.0 ? 1.0 : r);
}

} // namespace cc
} // namespace crsdr
