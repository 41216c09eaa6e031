// caf_track.hpp -- the decisions and the fp64 arithmetic of crsdr_caf's tracker (include/crsdr.h, section (w), "Tracks";
// crsdr_caf_set_track, crsdr_track): the limits, what a measurement is, the wrap, predict, the gate's d2, update and coast, the status
// rules, the strict order of the assignment, lowest-free-slot initiation, the id counter and the output record.  Plain C++ that both the
// kernel of caf_track_kernels.hpp and a CPU program compile (tools/caf_track_cpu.cc; tests/test_host_caf_track.py runs these very
// functions under the sanitizers).  tests/caf_track_model.py is the fp64 statement, written as the header's sequential sentences.
//
// A track's state is x = (r, f, g) and the upper triangle of its covariance, P = (P00, P01, P02, P11, P12, P22).  The motion model is
//     r' = r + c (f + g / 2),  f' = wrap(f + g),  g' = g          F = [1 c c/2; 0 1 1; 0 0 1],  P' = F P F^T + diag(q_r, q_f, q_g)
// and the measurement is (r, f) with noise diag(sigma_r^2, sigma_f^2).  Every operation below is written out once, in one order, and the
// library is built without contraction: the kernel and the CPU program give the same bits.
// The state buffer of `state_bytes` bytes is a 16-byte header (the id counter: ids issued so far modulo 2^24 - 1) and max_tracks slots
// of 128 bytes; all zero is the empty table.
#pragma once
#include <math.h>
#include <stdint.h>

#include "caf_peak.hpp"

namespace crsdr {
namespace trk {

constexpr int MAX_TRACKS = 128, MAX_MEAS = 64, MAX_HIST = 32, REC = 16;
constexpr int SRC_ARRAY = 0, SRC_FUSED = 1;
constexpr int FREE = 0, TENTATIVE = 1, CONFIRMED = 2, ENDED = 3;
constexpr int ID_PERIOD = (1 << 24) - 1;                       // ids run 1 .. 2^24 - 1 and continue at 1
constexpr int HEADER_BYTES = 16;

struct Params {
    int max_tracks, source;
    double sigma_r, sigma_f, gate, p0_g, q_r, q_f, q_g, coupling;
    int m, n, tent_miss, conf_miss;
};

// a slot of the state buffer: 10 doubles, 4 floats and 8 words, 128 bytes
struct Slot {
    double x[3], P[6];
    double d2;                                                 // of the last assignment (the record's figure of this line only)
    float power, snr, aux0, aux1;                              // remembered from the last assigned measurement
    int32_t id, status, age, hits, misses;
    uint32_t hist;
    uint32_t reserved[2];
};
static_assert(sizeof(Slot) == 128, "a slot of the tracker's state is 128 bytes");

struct Meas { double zr, zf; float power, snr, aux0, aux1; };

CAFP_HD bool fin(double v) { return v >= -1.7976931348623157e308 && v <= 1.7976931348623157e308; }      // (NaN fails both)

// 0, or the number of the limit of section (w) that fails (caf_engine.hpp words them)
CAFP_HD int bad_limit(const Params &q)
{
    if (q.max_tracks < 1 || q.max_tracks > MAX_TRACKS) return 1;
    if (q.source != SRC_ARRAY && q.source != SRC_FUSED) return 2;
    if (!fin(q.sigma_r) || !(q.sigma_r > 0.0) || !fin(q.sigma_f) || !(q.sigma_f > 0.0)) return 3;
    if (!fin(q.gate) || !(q.gate > 0.0)) return 4;
    if (!fin(q.p0_g) || !(q.p0_g > 0.0)) return 5;
    if (!fin(q.q_r) || !(q.q_r >= 0.0) || !fin(q.q_f) || !(q.q_f >= 0.0) || !fin(q.q_g) || !(q.q_g >= 0.0)) return 6;
    if (!fin(q.coupling)) return 7;
    if (q.m < 1 || q.n < q.m || q.n > MAX_HIST) return 8;
    if (q.tent_miss < 1 || q.conf_miss < 1) return 9;
    return 0;
}

CAFP_HD size_t state_bytes(int max_tracks) { return (size_t)HEADER_BYTES + sizeof(Slot) * (size_t)max_tracks; }

CAFP_HD int live_slots(int count, int K) { return count < 0 ? 0 : count < K ? count : K; }

// the value of v in [-nd / 2, nd / 2) modulo nd
CAFP_HD double wrap(double v, int nd)
{
    const double n = (double)nd, h = (double)(nd / 2);
    return v - n * floor((v + h) / n);
}

// the measurement a record names (only lag, Doppler, power, snr, dlag and ddop are read); false: its lag or Doppler lies outside the map,
// or its dlag or ddop is not finite (hand-made lists only)
CAFP_HD bool measurement(const float *rec, int nd, int R, Meas *z)
{
    const float lag = rec[0], dop = rec[1];
    if (!(lag >= 0.f && lag < (float)R) || !(dop >= (float)(-nd / 2) && dop < (float)(nd / 2))) return false;
    z->zr = (double)lag + (double)rec[5];
    z->zf = (double)dop + (double)rec[6];
    z->power = rec[2]; z->snr = rec[3];
    return fin(z->zr) && fin(z->zf);
}

CAFP_HD bool live(int status) { return status == TENTATIVE || status == CONFIRMED; }

// step 1: x, P -> x', P'
CAFP_HD void predict(Slot &s, const Params &q, int nd)
{
    const double c = q.coupling, b = 0.5 * c;
    const double r = s.x[0], f = s.x[1], g = s.x[2];
    s.x[0] = r + c * (f + 0.5 * g);
    s.x[1] = wrap(f + g, nd);
    const double *P = s.P;
    // A = F P, row by row (P symmetric: P10 = P01, ...)
    const double a00 = P[0] + c * P[1] + b * P[2], a01 = P[1] + c * P[3] + b * P[4], a02 = P[2] + c * P[4] + b * P[5];
    const double a11 = P[3] + P[4], a12 = P[4] + P[5];
    // P' = A F^T, the upper triangle
    const double n00 = a00 + c * a01 + b * a02, n01 = a01 + a02, n02 = a02;
    const double n11 = a11 + a12, n12 = a12, n22 = P[5];
    s.P[0] = n00 + q.q_r; s.P[1] = n01; s.P[2] = n02;
    s.P[3] = n11 + q.q_f; s.P[4] = n12; s.P[5] = n22 + q.q_g;
}

// step 2
CAFP_HD bool exits(const Slot &s, int R) { return s.x[0] < -1.0 || s.x[0] > (double)R; }

// step 3: the innovation, S and d2 of a predicted track against a measurement
struct Gate { double nu0, nu1, s00, s01, s11, det, d2; };
CAFP_HD Gate gate(const Slot &s, const Params &q, int nd, double zr, double zf)
{
    Gate t;
    t.nu0 = zr - s.x[0];
    t.nu1 = wrap(zf - s.x[1], nd);
    t.s00 = s.P[0] + q.sigma_r * q.sigma_r; t.s01 = s.P[1]; t.s11 = s.P[3] + q.sigma_f * q.sigma_f;
    t.det = t.s00 * t.s11 - t.s01 * t.s01;
    t.d2 = (t.s11 * t.nu0 * t.nu0 - 2.0 * t.s01 * t.nu0 * t.nu1 + t.s00 * t.nu1 * t.nu1) / t.det;
    return t;
}
CAFP_HD bool candidate(double d2, const Params &q) { return d2 <= q.gate; }      // (a NaN is none)

// step 4: the strict total order of the candidates, (d2, i, j) ascending (the kernel's walks go through a row or a column in ascending
// index with a strict comparison of d2, which is this order within a row or a column)
CAFP_HD bool before(double d2a, int ia, int ja, double d2b, int ib, int jb)
{
    if (d2a != d2b) return d2a < d2b;
    if (ia != ib) return ia < ib;
    return ja < jb;
}

// step 5, an assigned track
CAFP_HD void update(Slot &s, const Params &q, int nd, const Meas &z)
{
    const Gate t = gate(s, q, nd, z.zr, z.zf);
    double k0[3], k1[3];
    const double b0[3] = {s.P[0], s.P[1], s.P[2]}, b1[3] = {s.P[1], s.P[3], s.P[4]};      // P' H^T: the first two columns
    for (int i = 0; i < 3; ++i) {
        k0[i] = (b0[i] * t.s11 - b1[i] * t.s01) / t.det;
        k1[i] = (b1[i] * t.s00 - b0[i] * t.s01) / t.det;
    }
    s.x[0] = s.x[0] + (k0[0] * t.nu0 + k1[0] * t.nu1);
    s.x[1] = wrap(s.x[1] + (k0[1] * t.nu0 + k1[1] * t.nu1), nd);
    s.x[2] = s.x[2] + (k0[2] * t.nu0 + k1[2] * t.nu1);
    // P = P' - K S K^T, the upper triangle (the lower is its copy)
    double ks0[3], ks1[3];
    for (int i = 0; i < 3; ++i) { ks0[i] = k0[i] * t.s00 + k1[i] * t.s01; ks1[i] = k0[i] * t.s01 + k1[i] * t.s11; }
    s.P[0] -= ks0[0] * k0[0] + ks1[0] * k1[0];
    s.P[1] -= ks0[0] * k0[1] + ks1[0] * k1[1];
    s.P[2] -= ks0[0] * k0[2] + ks1[0] * k1[2];
    s.P[3] -= ks0[1] * k0[1] + ks1[1] * k1[1];
    s.P[4] -= ks0[1] * k0[2] + ks1[1] * k1[2];
    s.P[5] -= ks0[2] * k0[2] + ks1[2] * k1[2];
    s.hits += 1; s.misses = 0; s.hist = (s.hist << 1) | 1u; s.age += 1;
    s.d2 = t.d2; s.power = z.power; s.snr = z.snr; s.aux0 = z.aux0; s.aux1 = z.aux1;
}

// step 5, every other live track: x = x', P = P' stand as predict left them
CAFP_HD void coast(Slot &s)
{
    s.misses += 1; s.hist = s.hist << 1; s.age += 1; s.d2 = 0.0;
}

CAFP_HD int popcount(uint32_t v)
{
    int n = 0;
    for (; v; v &= v - 1) ++n;
    return n;
}

// step 6: the status of a live track after its update or coast
CAFP_HD int next_status(const Slot &s, const Params &q)
{
    if (s.status == TENTATIVE) {
        const uint32_t mask = q.n >= 32 ? 0xffffffffu : ((1u << q.n) - 1u);
        if (popcount(s.hist & mask) >= q.m) return CONFIRMED;
        if (s.misses >= q.tent_miss || s.age >= q.n) return ENDED;
        return TENTATIVE;
    }
    return s.misses >= q.conf_miss ? ENDED : CONFIRMED;
}

// step 7: the id of the u-th track initiated behind `counter` ids, and the counter behind `n` more
CAFP_HD int id_of(int counter, int u) { return (int)(((long long)counter + u) % ID_PERIOD) + 1; }
CAFP_HD int counter_after(int counter, int n) { return (int)(((long long)counter + n) % ID_PERIOD); }

CAFP_HD void initiate(Slot &s, const Params &q, int nd, const Meas &z, int id)
{
    s.x[0] = z.zr; s.x[1] = wrap(z.zf, nd); s.x[2] = 0.0;
    s.P[0] = q.sigma_r * q.sigma_r; s.P[1] = 0.0; s.P[2] = 0.0; s.P[3] = q.sigma_f * q.sigma_f; s.P[4] = 0.0; s.P[5] = q.p0_g;
    s.d2 = 0.0; s.power = z.power; s.snr = z.snr; s.aux0 = z.aux0; s.aux1 = z.aux1;
    s.id = id; s.status = TENTATIVE; s.age = 0; s.hits = 1; s.misses = 0; s.hist = 1u;
}

// the record of a slot: status as reported (ENDED once), slot = this line's measurement slot or -1; a free slot is all zero
CAFP_HD void record(const Slot &s, int status, int slot, float *out)
{
    if (status == FREE) { for (int k = 0; k < REC; ++k) out[k] = 0.f; return; }
    out[0] = (float)s.id; out[1] = (float)status;
    out[2] = (float)s.x[0]; out[3] = (float)s.x[1]; out[4] = (float)s.x[2];
    out[5] = (float)sqrt(s.P[0]); out[6] = (float)sqrt(s.P[3]);
    out[7] = (float)s.age; out[8] = (float)s.hits; out[9] = (float)s.misses;
    out[10] = (float)slot; out[11] = (float)(slot >= 0 ? s.d2 : 0.0);
    out[12] = s.power; out[13] = s.snr; out[14] = s.aux0; out[15] = s.aux1;
}

// a line, all of it, on the host, by the header's sequential sentences with the assignment as mutual-first rounds (what the kernel
// does; tests/test_caf_track_model.py pins the rounds equal to the greedy walk).  slots [T] and *counter are the state, in and out;
// det [K][8], aux [K][2] or NULL; trk [T][16], ntrk [4].  d2, scratch: T K doubles and T + K ints of working space
inline void line(Slot *slots, int32_t *counter, const Params &q, const float *det, int count, const float *aux, int K, int nd, int R, double *d2, int *scratch,
                 float *trk, int32_t *ntrk)
{
    const int T = q.max_tracks, nm = live_slots(count, K);
    int *of_track = scratch, *of_meas = scratch + T;          // the measurement of a track, the track of a measurement; -1: none
    Meas z[MAX_MEAS];
    bool valid[MAX_MEAS], was_free[MAX_TRACKS], active[MAX_TRACKS];
    for (int j = 0; j < nm; ++j) {
        valid[j] = measurement(det + (size_t)j * 8, nd, R, &z[j]);
        z[j].aux0 = aux ? aux[2 * j] : -1.f; z[j].aux1 = aux ? aux[2 * j + 1] : -1.f;
        of_meas[j] = -1;
    }
    for (int i = 0; i < T; ++i) {
        Slot &s = slots[i];
        was_free[i] = s.status == FREE; of_track[i] = -1; active[i] = false;
        if (!live(s.status)) continue;
        predict(s, q, nd);
        if (exits(s, R)) { s.status = ENDED; s.d2 = 0.0; continue; }
        active[i] = true;
        for (int j = 0; j < nm; ++j) {
            const double d = valid[j] ? gate(s, q, nd, z[j].zr, z[j].zf).d2 : 0.0;
            d2[(size_t)i * K + j] = valid[j] && candidate(d, q) ? d : INFINITY;
        }
    }
    for (bool any = true; any;) {
        any = false;
        int rbest[MAX_TRACKS], cbest[MAX_MEAS];
        for (int i = 0; i < T; ++i) {
            rbest[i] = -1;
            if (!active[i] || of_track[i] >= 0) continue;
            for (int j = 0; j < nm; ++j)
                if (of_meas[j] < 0 && d2[(size_t)i * K + j] < INFINITY && (rbest[i] < 0 || before(d2[(size_t)i * K + j], i, j, d2[(size_t)i * K + rbest[i]], i, rbest[i])))
                    rbest[i] = j;
        }
        for (int j = 0; j < nm; ++j) {
            cbest[j] = -1;
            if (of_meas[j] >= 0) continue;
            for (int i = 0; i < T; ++i)
                if (active[i] && of_track[i] < 0 && d2[(size_t)i * K + j] < INFINITY &&
                    (cbest[j] < 0 || before(d2[(size_t)i * K + j], i, j, d2[(size_t)cbest[j] * K + j], cbest[j], j)))
                    cbest[j] = i;
        }
        for (int i = 0; i < T; ++i)
            if (rbest[i] >= 0 && cbest[rbest[i]] == i) { of_track[i] = rbest[i]; of_meas[rbest[i]] = i; any = true; }
    }
    int nlive = 0, nconf = 0, ninit = 0, ndrop = 0;
    int reported[MAX_TRACKS];
    for (int i = 0; i < T; ++i) {
        Slot &s = slots[i];
        reported[i] = s.status;
        if (!active[i]) continue;
        if (of_track[i] >= 0) update(s, q, nd, z[of_track[i]]); else coast(s);
        s.status = reported[i] = next_status(s, q);
    }
    int at = 0;
    for (int j = 0; j < nm; ++j) {
        if (!valid[j] || of_meas[j] >= 0) continue;
        while (at < T && !was_free[at]) ++at;
        if (at >= T) { ++ndrop; continue; }
        initiate(slots[at], q, nd, z[j], id_of(*counter, ninit));
        reported[at] = TENTATIVE; of_track[at] = j;
        ++ninit; ++at;
    }
    *counter = counter_after(*counter, ninit);
    for (int i = 0; i < T; ++i) {
        record(slots[i], reported[i], of_track[i], trk + (size_t)i * REC);
        nlive += live(reported[i]) ? 1 : 0; nconf += reported[i] == CONFIRMED ? 1 : 0;
        if (reported[i] == ENDED) { slots[i] = Slot{}; }
    }
    ntrk[0] = nlive; ntrk[1] = nconf; ntrk[2] = ninit; ntrk[3] = ndrop;
}

} // namespace trk
} // namespace crsdr
