// caf_integrate_solve.hpp -- the host arithmetic of crsdr_caf's integration across lines (include/crsdr.h, section (w), "Integration
// across lines"; crsdr_caf_set_integrate, crsdr_map_integrate): the limits, the whole-cell offsets of the range walk, the forgetting
// factor, the clamped source cell and the three-operation update.  Plain C++ that both the kernel of caf_integrate.hpp and a CPU
// program compile (tools/caf_integrate_cpu.cc; tests/test_host_caf_integrate.py runs these very functions under the sanitizers).
// tests/caf_integrate_model.py is the fp64 statement, the header's four sentences taken literally.
//
// Every fp64 operation below is rounded on its own: the device goes through __dmul_rn / __dadd_rn, which the compiler never contracts,
// and the host is built with -ffp-contract=off; the numpy model, which cannot contract, gives the same bytes.
// The state buffer of `state_bytes` bytes is a 16-byte header (int64 m: lines since the last reset; int64 0) and nmaps nd R doubles;
// all zero is the empty state.
#pragma once
#include <math.h>
#include <stdint.h>

#include "caf_peak.hpp"

namespace crsdr {
namespace integ {

constexpr int ARRAY = 1, BEAMS = 2;
constexpr int HEADER_BYTES = 16;
constexpr double MAX_WALK = 1024.0;                            // |coupling| * (nd / 2): the most cells a line may walk

struct Params { double forget, coupling; };

CAFP_HD bool fin(double v) { return v >= -1.7976931348623157e308 && v <= 1.7976931348623157e308; }      // (NaN fails both)

CAFP_HD double mul(double a, double b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __dmul_rn(a, b);
#else
    return a * b;
#endif
}

CAFP_HD double add(double a, double b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __dadd_rn(a, b);
#else
    return a + b;
#endif
}

// 0, or the number of the limit of section (w) that fails (caf_engine.hpp words them)
CAFP_HD int bad_limit(int nd, const Params &q)
{
    if (!fin(q.forget) || !(q.forget > 0.0) || !(q.forget <= 1.0)) return 1;
    if (!fin(q.coupling)) return 2;
    if (!((q.coupling < 0.0 ? -q.coupling : q.coupling) * (double)(nd / 2) <= MAX_WALK)) return 3;
    return 0;
}

CAFP_HD size_t state_bytes(int nmaps, int nd, int R) { return (size_t)HEADER_BYTES + sizeof(double) * (size_t)nmaps * (size_t)nd * (size_t)R; }

// delta(d) = c * s(d): one multiplication
CAFP_HD double delta(double coupling, int s) { return mul(coupling, (double)s); }

// o(m, d) = floor(m * delta + 0.5): one multiplication, one addition
CAFP_HD int64_t offset(int64_t m, double dl) { return (int64_t)floor(add(mul((double)m, dl), 0.5)); }

// D(d) of line m: the cells the accumulated row moves before the line's update; 0 at m = 0
CAFP_HD int64_t step(int64_t m, double coupling, int s)
{
    if (m < 1) return 0;
    const double dl = delta(coupling, s);
    return offset(m, dl) - offset(m - 1, dl);
}

// the running mean until the window is full, exponential forgetting from then on
CAFP_HD double lambda(int64_t m, double forget)
{
    const double mean = 1.0 / (double)(m + 1);
    return forget > mean ? forget : mean;
}

// the cell of I that I'[tau] copies: whole cells, clamped at both ends of the lags
CAFP_HD int source(int tau, int64_t D, int R)
{
    const int64_t t = (int64_t)tau - D;
    return t < 0 ? 0 : t > (int64_t)(R - 1) ? R - 1 : (int)t;
}

// I = I' + lambda (P - I'): three operations, each rounded once
CAFP_HD double update(double shifted, float p, double lam) { return add(shifted, mul(lam, add((double)p, -shifted))); }

// One line of one map on the host, as the kernel does it: row [nd][R] in and out, tmp [R] scratch, imap [nd][R]
inline void line(double *I, double *tmp, int64_t m, const Params &q, const float *P, int nd, int R, float *imap)
{
    const double lam = lambda(m, q.forget);
    for (int d = 0; d < nd; ++d) {
        const int64_t D = step(m, q.coupling, cafp::signed_bin(d, nd));
        double *row = I + (size_t)d * R;
        for (int tau = 0; tau < R; ++tau) tmp[tau] = row[source(tau, D, R)];
        for (int tau = 0; tau < R; ++tau) {
            row[tau] = update(tmp[tau], P[(size_t)d * R + tau], lam);
            imap[(size_t)d * R + tau] = (float)row[tau];
        }
    }
}

} // namespace integ
} // namespace crsdr
