// caf_track_kernels.hpp -- the tracker of crsdr_caf on the device (include/crsdr.h, section (w), "Tracks"; crsdr_caf_set_track,
// crsdr_track).  Part of crsdr.hip's translation unit through caf_engine.hpp.  Every decision and every fp64 operation is a function of
// caf_track.hpp, which tools/caf_track_cpu.cc compiles for the host; this file is who does what, and when.
//
// k_caf_track: ONE workgroup of 128 threads per engine, looping over the lines of the submit, so that the host is not needed between
// lines.  Thread i owns track slot i: its state lives in registers from the load in front of the first line to the store behind the
// last, and predict, the range exit, update, coast, the status rules and the record are its own.  Thread j < K also owns measurement
// slot j of the line.  The T x K matrix of d2 is fp64 in dynamic LDS, rows padded to an odd length (K | 1), so that the threads of a
// wave, each walking its own row, spread over the banks; a pair that is no candidate holds +inf.
// Assignment: rounds of "take every candidate that is the first of its row and of its column among the free ones".  Per round thread i
// walks the free columns of its row for the smallest (d2, j), thread j the free rows of its column for the smallest (d2, i) -- strict
// comparisons in ascending order, so that of equal d2 the lower index stays -- and row i takes its first where that column's first is
// i.  The first candidate of the strict order among the free ones is always mutual, so every round but the last takes at least one, and
// a mutual first is what the sequential walk takes: the same set (tests/test_caf_track_model.py pins it).  One thread per row and per
// column walks serially where a wave reduction per row would put the rows behind each other: all rows run at once here.
// Initiation: two wave ballots, one over the unassigned measurements and one over the slots that were free when the line began, give
// each its rank by a prefix count; the free slot of rank u takes the unassigned measurement of rank u and the id counter + u.
// Nothing depends on the order in which waves arrive: every shared word has one writer between two barriers.  All stores are plain
// vector stores.
#pragma once

#include "caf_track.hpp"

namespace crsdr {
namespace caf_track {

constexpr int THREADS = 128;
constexpr int AUX_NONE = 0, AUX_PAIRS = 1, AUX_DIR = 2, AUX_BEAM = 3;      // (-1, -1); aux [K][2]; dir [K][8]: cx + dx, cy + dy; (the record's beam, -1)
static_assert(THREADS >= trk::MAX_TRACKS && THREADS >= trk::MAX_MEAS && THREADS == 128, "one thread per track slot and per measurement slot, two waves");

CAFP_HD int row_len(int K) { return K | 1; }
inline size_t lds_bytes(int T, int K) { return sizeof(double) * (size_t)T * (size_t)row_len(K); }

// det + line det_stride: [K][8]; count + line count_stride; aux + line K (2 or 8) by aux_mode; state: trk::state_bytes, in and out;
// trk [nlines][T][16], ntrk [nlines][4]
__global__ __launch_bounds__(THREADS) void k_caf_track(const float *__restrict__ det, size_t det_stride, const int32_t *__restrict__ count, size_t count_stride,
                                                       const float *__restrict__ aux, int aux_mode, int nlines, int K, int nd, int R, trk::Params q,
                                                       unsigned char *__restrict__ state, float *__restrict__ out, int32_t *__restrict__ nout)
{
    extern __shared__ double d2m[];                         // [T][row_len(K)]
    __shared__ trk::Meas z[trk::MAX_MEAS];
    __shared__ int valid[trk::MAX_MEAS], of_meas[trk::MAX_MEAS], cbest[trk::MAX_MEAS], ulist[trk::MAX_MEAS];
    __shared__ int rowfree[trk::MAX_TRACKS];
    __shared__ int wfree[2], wlive[2], wconf[2], nun_s;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, T = q.max_tracks, LD = row_len(K);
    const unsigned long long below = (1ull << lane) - 1ull;
    const double inf = __builtin_huge_val();
    int32_t *header = (int32_t *)state;
    trk::Slot *slots = (trk::Slot *)(state + trk::HEADER_BYTES);
    trk::Slot s = trk::Slot{};
    if (tid < T) s = slots[tid];
    int counter = header[0];

    for (int line = 0; line < nlines; ++line) {
        const int nm = trk::live_slots(count[(size_t)line * count_stride], K);
        if (tid < trk::MAX_MEAS) {
            valid[tid] = 0; of_meas[tid] = -1;
            if (tid < nm) {
                const float *rec = det + (size_t)line * det_stride + (size_t)tid * 8;
                trk::Meas m;
                valid[tid] = trk::measurement(rec, nd, R, &m) ? 1 : 0;
                m.aux0 = -1.f; m.aux1 = -1.f;
                if (aux_mode == AUX_PAIRS) {
                    const float *a = aux + ((size_t)line * K + tid) * 2;
                    m.aux0 = a[0]; m.aux1 = a[1];
                } else if (aux_mode == AUX_DIR) {
                    const float *a = aux + ((size_t)line * K + tid) * 8;
                    m.aux0 = (float)((double)a[0] + (double)a[3]); m.aux1 = (float)((double)a[1] + (double)a[4]);
                } else if (aux_mode == AUX_BEAM) m.aux0 = rec[7];
                z[tid] = m;
            }
        }
        const bool was_free = tid < T && s.status == trk::FREE;
        int of_track = -1;
        bool act = false;
        if (trk::live(s.status)) {
            trk::predict(s, q, nd);
            if (trk::exits(s, R)) { s.status = trk::ENDED; s.d2 = 0.0; } else act = true;
        }
        rowfree[tid] = act ? 1 : 0;
        __syncthreads();
        if (act)
            for (int j = 0; j < nm; ++j) {
                const double d = valid[j] ? trk::gate(s, q, nd, z[j].zr, z[j].zf).d2 : 0.0;
                d2m[tid * LD + j] = valid[j] && trk::candidate(d, q) ? d : inf;
            }
        __syncthreads();

        for (;;) {
            int rb = -1;
            if (act && of_track < 0) {
                double best = inf;
                for (int j = 0; j < nm; ++j) {
                    if (of_meas[j] >= 0) continue;
                    const double d = d2m[tid * LD + j];
                    if (d < best) { best = d; rb = j; }
                }
            }
            if (tid < nm && of_meas[tid] < 0) {
                double best = inf;
                int cb = -1;
                for (int i = 0; i < T; ++i) {
                    if (!rowfree[i]) continue;
                    const double d = d2m[i * LD + tid];
                    if (d < best) { best = d; cb = i; }
                }
                cbest[tid] = cb;
            }
            __syncthreads();
            const bool take = rb >= 0 && cbest[rb] == tid;
            if (take) { of_track = rb; of_meas[rb] = tid; rowfree[tid] = 0; }
            if (!__syncthreads_or(take ? 1 : 0)) break;
        }

        int rep = s.status;
        if (act) {
            if (of_track >= 0) trk::update(s, q, nd, z[of_track]); else trk::coast(s);
            s.status = rep = trk::next_status(s, q);
        }

        // initiation: the unassigned measurements and the slots free at the start of the line, each ranked by a prefix count
        const bool um = tid < nm && valid[tid] && of_meas[tid] < 0;
        const unsigned long long mb = __ballot(um ? 1 : 0), fb = __ballot(was_free ? 1 : 0);
        if (um) ulist[__popcll(mb & below)] = tid;           // (measurement slots are threads 0 .. 63: the first wave alone)
        if (lane == 0) { wfree[wave] = __popcll(fb); if (wave == 0) nun_s = __popcll(mb); }
        __syncthreads();
        const int nun = nun_s, nfree = wfree[0] + wfree[1], frank = __popcll(fb & below) + (wave ? wfree[0] : 0);
        const int ninit = nun < nfree ? nun : nfree;
        if (was_free && frank < nun) {
            of_track = ulist[frank];
            trk::initiate(s, q, nd, z[of_track], trk::id_of(counter, frank));
            rep = trk::TENTATIVE;
        }
        counter = trk::counter_after(counter, ninit);

        if (tid < T) trk::record(s, rep, of_track, out + ((size_t)line * T + tid) * trk::REC);
        const unsigned long long lb = __ballot(trk::live(rep) ? 1 : 0), cb2 = __ballot(rep == trk::CONFIRMED ? 1 : 0);
        if (lane == 0) { wlive[wave] = __popcll(lb); wconf[wave] = __popcll(cb2); }
        if (rep == trk::ENDED) s = trk::Slot{};
        __syncthreads();                                    // (and the line's shared words are free for the next line)
        if (tid == 0) {
            int32_t *n = nout + (size_t)line * 4;
            n[0] = wlive[0] + wlive[1]; n[1] = wconf[0] + wconf[1]; n[2] = ninit; n[3] = nun - ninit;
        }
    }
    if (tid < T) slots[tid] = s;
    if (tid == 0) header[0] = counter;
}

} // namespace caf_track
} // namespace crsdr
