// caf_beams.hpp -- the decisions of crsdr_caf's coherent beam maps (include/crsdr.h, section (w), "Beams"; crsdr_caf_set_beams,
// crsdr_beam_maps, crsdr_beam_fuse, crsdr_caf_beam_steer): the limits, which row is which element, a beam sum and its power in the
// kernel's order, the steering weights, and the fusion of the beams' detection lists -- the candidate a record names, the order of the
// candidates, "within one cell", suppression and the survivor's record.  Plain C++ that both the kernels of caf_beams_kernels.hpp and
// a CPU program compile (tools/caf_beams_cpu.cc; tests/test_host_caf_beams.py runs these very functions under the sanitizers).
// tests/caf_beams_model.py is the fp64 statement.
//
// Elements e = 0 .. m - 1 are the rows c != ref_row in ascending order (brg::row_of: the bearings' rule), m = nrows - 1.
//     z_b[i] = sum_e w_b,e chi_c(e)[i]        fp32, e ascending, per element  re = fma(-wi, ci, fma(wr, cr, re)),
//                                                                             im = fma( wr, ci, fma(wi, cr, im))
//     bmap_b[i] = (float)((double)re z re z + (double)im z im z)
// which is what two v_mfma_f32_32x32x2_f32 per element leave in the accumulators: a k-ordered chain of fused multiply-adds.
// Fusion.  The candidates of a line are the slots q < min(bcount[b], K) of every beam's list; a slot whose lag or Doppler lies
// outside the map (hand-made lists only) is no candidate.  A before A'  <=>  P > P', or P == P' and b < b', or those equal and i < i'
// (i = d R + tau; a hand-made list that names one cell twice in one beam: the earlier slot, so that the order is total on any list).
// A candidate is suppressed iff another comes before it and lies within one cell of it (|tau - tau'| <= 1, no wrap;
// |d - d'| <= 1 modulo nd), whether or not that other is itself suppressed.  The survivors in that order are the fused list.
#pragma once
#include <math.h>
#include <stdint.h>

#include "caf_bearing_solve.hpp"

namespace crsdr {
namespace bm {

constexpr int MAX_M = 64, MAX_BEAMS = 64, GROUP = 32;          // GROUP: the beams of one MFMA tile
constexpr int MAX_CAND = MAX_BEAMS * cfar::MAX_DET;
constexpr long long MAX_CELLS = 1ll << 24;                     // (max_batch / frames) * nbeams * nd * R floats of bmap

// 0, or the number of the limit of section (w) that fails (caf_engine.hpp words them).  weights [nbeams][m][2] on the host.
CAFP_HD int bad_limit(int nrows, long long lines, int nd, int R, int nbeams, const float *weights, unsigned flags)
{
    const long long m = (long long)nrows - 1;
    if (m < 1 || m > MAX_M) return 1;
    if (nbeams < 1 || nbeams > MAX_BEAMS) return 2;
    if (!weights) return 3;
    for (long long k = 0; k < 2ll * nbeams * m; ++k)
        if (!(weights[k] >= -3.402823466e+38f && weights[k] <= 3.402823466e+38f)) return 4;      // (NaN fails both, an infinity one)
    if (flags) return 5;
    if (lines * nbeams * nd * R > MAX_CELLS) return 6;
    return 0;
}

// the kernel's chain for one beam at one cell: chi [nrows][cells][2] of a line, w [m][2] of the beam
CAFP_HD void beam_sum(const float *chi, size_t cells, int m, int ref_row, const float *w, size_t i, float *re, float *im)
{
    float zr = 0.f, zi = 0.f;
    for (int e = 0; e < m; ++e) {
        const float *c = chi + 2 * ((size_t)brg::row_of(e, ref_row) * cells + i);
        zr = fmaf(-w[2 * e + 1], c[1], fmaf(w[2 * e], c[0], zr));
        zi = fmaf(w[2 * e], c[1], fmaf(w[2 * e + 1], c[0], zi));
    }
    *re = zr; *im = zi;
}

CAFP_HD float power(float re, float im) { return (float)((double)re * (double)re + (double)im * (double)im); }

// w = a(x, y) / sqrt(m) of one direction, each part rounded once: the bearings' fp64 steering expression and element order
// (brg::stat), on the host only
inline void steer(float *w, int mx, int my, float d, int ncx, int ncy, double x, double y)
{
    const double pi = 3.14159265358979323846;
    const double alpha = x * pi / (double)ncx, beta = y * pi / (double)ncy;
    const double ca = cos(alpha), sb = sin(beta), cb = cos(beta), s = 1.0 / sqrt((double)(mx * my));
    for (int iy = 0; iy < my; ++iy)
        for (int ix = 0; ix < mx; ++ix) {
            const int e = iy * mx + ix;
            const double ph = 2.0 * pi * (double)d * ((double)ix * ca * sb + (double)iy * cb);
            w[2 * e] = (float)(cos(ph) * s);
            w[2 * e + 1] = (float)(sin(ph) * s);
        }
}

// ---- fusion ----
// a candidate: its power, its cell, and beam * MAX_DET + slot.  i < 0: none
struct Cand { float p; int i, key; };
CAFP_HD int beam_of(const Cand &c) { return c.key / cfar::MAX_DET; }
CAFP_HD int slot_of(const Cand &c) { return c.key % cfar::MAX_DET; }

// the candidate that slot q of beam b names (rec: its eight figures)
CAFP_HD Cand candidate(const float *rec, int b, int q, int nd, int R) { return Cand{rec[2], brg::cell_of(rec, nd, R), b * cfar::MAX_DET + q}; }

CAFP_HD int live_slots(int count, int K) { return count < 0 ? 0 : count < K ? count : K; }

CAFP_HD bool before(const Cand &x, const Cand &y)
{
    if (x.p != y.p) return x.p > y.p;
    const int bx = beam_of(x), by = beam_of(y);
    if (bx != by) return bx < by;
    if (x.i != y.i) return x.i < y.i;
    return x.key < y.key;                                          // (one cell twice in one beam, hand-made lists only: the earlier slot)
}

// within one cell: lag does not wrap, Doppler does (nd a power of two, at least 8)
CAFP_HD bool near(int i, int j, int nd, int R)
{
    const int di = i / R, dj = j / R, dt = (i - di * R) - (j - dj * R), dd = (di - dj) & (nd - 1);
    return dt >= -1 && dt <= 1 && (dd <= 1 || dd == nd - 1);
}

// is candidate x of list [n] suppressed?  (whether or not the one that suppresses it is itself suppressed; i < 0: no candidate)
CAFP_HD bool suppressed(const Cand *list, int n, int x, int nd, int R)
{
    const Cand c = list[x];
    for (int y = 0; y < n; ++y)
        if (y != x && list[y].i >= 0 && before(list[y], c) && near(list[y].i, c.i, nd, R)) return true;
    return false;
}

// a survivor's record: its bdet record bit for bit, the eighth figure the beam
CAFP_HD void record(const float *rec, int b, float *out)
{
    for (int k = 0; k < 7; ++k) out[k] = rec[k];
    out[7] = (float)b;
}

// a line, all of it, on the host: bdet [nbeams][K][8], bcount [nbeams] -> fused [K][8], the number of survivors.  list, alive: MAX_CAND
inline int fuse(const float *bdet, const int32_t *bcount, int nbeams, int K, int nd, int R, Cand *list, unsigned char *alive, float *fused)
{
    int n = 0, nf = 0;
    for (int b = 0; b < nbeams; ++b)
        for (int q = 0; q < live_slots(bcount[b], K); ++q) {
            const Cand c = candidate(bdet + ((size_t)b * K + q) * 8, b, q, nd, R);
            if (c.i >= 0) list[n++] = c;
        }
    for (int x = 0; x < n; ++x) { alive[x] = suppressed(list, n, x, nd, R) ? 0 : 1; nf += alive[x]; }
    for (int k = 0; k < K * 8; ++k) fused[k] = 0.f;
    for (int x = 0; x < n; ++x) {
        if (!alive[x]) continue;
        int rank = 0;
        for (int y = 0; y < n; ++y) rank += alive[y] && before(list[y], list[x]) ? 1 : 0;
        if (rank < K) record(bdet + ((size_t)beam_of(list[x]) * K + slot_of(list[x])) * 8, beam_of(list[x]), fused + (size_t)rank * 8);
    }
    return nf;
}

} // namespace bm
} // namespace crsdr
