// caf_integrate.hpp -- crsdr_caf's integration across lines on the device (include/crsdr.h, section (w), "Integration across lines";
// crsdr_caf_set_integrate, crsdr_map_integrate).  Part of crsdr.hip's translation unit through caf_engine.hpp.  The offsets, lambda, the
// clamped source cell and the update are functions of caf_integrate_solve.hpp, which tools/caf_integrate_cpu.cc compiles for the host;
// this file is who does what, and when.
//
// k_caf_integrate: a workgroup of 256 threads owns `nb` whole Doppler bins of one map (nb = bins_of(nd, R): a power of two, several bins
// when R is small, one from R = 129 on).  Their state rows sit in dynamic LDS as fp64, twice (2 x nb x R x 8 bytes, 16 KiB at the
// most): a row enters once in front of the first line and leaves once behind the last, and the workgroup loops over the submit's lines
// with ONE barrier per line:
//     the P cells of the line, coalesced, already in registers (loaded PF = 8 lines ahead: a line then costs a barrier, not a trip
//     to memory);
//     the shifted read of I from the current half -- consecutive lanes read consecutive doubles, an 8-byte read per lane that no
//     offset takes off its alignment, and the lanes that clamp read one address, which broadcasts;
//     the three operations;
//     the new row into the other half, imap out, coalesced.
// D(d) and lambda do not depend on the lane: thread t < nb works out D of bin t for the NEXT line, thread 0 lambda, into a
// two-deep table in LDS that the line's barrier publishes; a cell reads its bin's entry.
// The counter m lives in the state's header.  Every workgroup reads it when it starts; nobody writes it until every workgroup has
// finished: the workgroups count themselves out through the header's second word, and the last one writes m + nlines and puts that
// word back to 0.  Which workgroup is last changes nothing that is written.  All stores are plain vector stores.
// Per map the traffic is nlines x cells x 8 bytes (P in, imap out) and cells x 16 (the state in and out).
#pragma once

#include "caf_integrate_solve.hpp"

namespace crsdr {
namespace caf_integrate {

constexpr int THREADS = 256;
constexpr int CPT = 4;                                         // cells per thread: nb R <= max(256, R) <= 1024
constexpr int PF = 8;                                          // lines of P in registers ahead of the one at work
static_assert(PF % 2 == 0, "a line's half of the double-buffered rows is its slot's parity");
static_assert(THREADS * CPT >= caf::CAF_MAX_LAGS, "a workgroup holds at least one whole row");

// the bins of a workgroup: the largest power of two with nb R <= 256, at least 1, at most nd (nd a power of two: nb divides it)
inline int bins_of(int nd, int R)
{
    int nb = 1;
    while (2 * nb * R <= THREADS && 2 * nb <= nd) nb *= 2;
    return nb;
}
inline size_t lds_bytes(int nb, int R) { return sizeof(double) * 2 * (size_t)nb * (size_t)R; }

// maps [nlines][nmaps][nd][R]; state: integ::state_bytes(nmaps, nd, R), in and out; imap [nlines][nmaps][nd][R].
// grid (nd / nb, nmaps)
__global__ __launch_bounds__(THREADS) void k_caf_integrate(const float *__restrict__ maps, int nlines, int nmaps, int nd, int R, int nb, integ::Params q,
                                                           unsigned char *__restrict__ state, float *__restrict__ imap)
{
    extern __shared__ double rows[];                            // [2][nb R]
    __shared__ int Dsh[2][THREADS];
    __shared__ double Lsh[2];
    const int tid = threadIdx.x, d0 = (int)blockIdx.x * nb, map = (int)blockIdx.y;
    const int bins = nd - d0 < nb ? nd - d0 : nb, wg_cells = nb * R, valid = bins * R;
    const size_t cells = (size_t)nd * (size_t)R, base = (size_t)map * cells + (size_t)d0 * (size_t)R;
    long long *header = (long long *)state;
    double *I = (double *)(state + integ::HEADER_BYTES) + base;
    const long long m0 = header[0];

    // what a thread's cells are does not change with the line: the bin of the workgroup, the lag, whether there is one
    int bin[CPT], tau[CPT];
    bool has[CPT];
#pragma unroll
    for (int j = 0; j < CPT; ++j) {
        const int k = tid + j * THREADS;
        has[j] = k < valid;
        bin[j] = has[j] ? k / R : 0;
        tau[j] = has[j] ? k - bin[j] * R : 0;
        if (has[j]) rows[k] = I[k];
    }
    if (tid < bins) Dsh[0][tid] = (int)integ::step(m0, q.coupling, cafp::signed_bin(d0 + tid, nd));
    if (tid == 0) Lsh[0] = integ::lambda(m0, q.forget);
    // the P cells of the first PF lines: PF loads in flight per cell, so that a line costs a barrier and not a trip to memory
    float p[PF][CPT];
#pragma unroll
    for (int u = 0; u < PF; ++u)
#pragma unroll
        for (int j = 0; j < CPT; ++j) p[u][j] = has[j] && u < nlines ? maps[(size_t)u * (size_t)nmaps * cells + base + (size_t)(tid + j * THREADS)] : 0.f;
    __syncthreads();

    for (int line0 = 0; line0 < nlines; line0 += PF) {
#pragma unroll
        for (int u = 0; u < PF; ++u) {
            const int line = line0 + u, h = u & 1;                // (PF is even: the half is the slot's parity)
            if (line >= nlines) break;                            // (the same for every thread: the barrier below stays whole)
            const double *cur = rows + (size_t)h * wg_cells;
            double *nxt = rows + (size_t)(h ^ 1) * wg_cells;
            const size_t at = (size_t)line * (size_t)nmaps * cells + base;
            const double lam = Lsh[h];
#pragma unroll
            for (int j = 0; j < CPT; ++j) {
                if (!has[j]) continue;
                const int k = tid + j * THREADS;
                const double v = integ::update(cur[bin[j] * R + integ::source(tau[j], (int64_t)Dsh[h][bin[j]], R)], p[u][j], lam);
                nxt[k] = v;
                imap[at + (size_t)k] = (float)v;
            }
            if (line + PF < nlines) {
#pragma unroll
                for (int j = 0; j < CPT; ++j)
                    if (has[j]) p[u][j] = maps[at + (size_t)PF * (size_t)nmaps * cells + (size_t)(tid + j * THREADS)];
            }
            if (line + 1 < nlines) {
                const long long m = m0 + line + 1;
                if (tid < bins) Dsh[h ^ 1][tid] = (int)integ::step(m, q.coupling, cafp::signed_bin(d0 + tid, nd));
                if (tid == 0) Lsh[h ^ 1] = integ::lambda(m, q.forget);
            }
            __syncthreads();
        }
    }

    const double *fin = rows + (size_t)(nlines & 1) * wg_cells;
#pragma unroll
    for (int j = 0; j < CPT; ++j)
        if (has[j]) I[tid + j * THREADS] = fin[tid + j * THREADS];
    // the counter: behind every workgroup's read of it, so by the one that counts itself out last.  The count is a relaxed atomic: a
    // thread's read of m has returned before the first barrier (lambda and D are made of it), and the last ticket is known only when
    // every workgroup has taken one; a release here would write the L2 back once per workgroup for nothing
    if (tid == 0) {
        const long long groups = (long long)gridDim.x * (long long)gridDim.y;
        const long long ticket = __hip_atomic_fetch_add(&header[1], 1ll, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (ticket == groups - 1) {
            header[0] = m0 + nlines;
            header[1] = 0;
        }
    }
}

} // namespace caf_integrate
} // namespace crsdr
