// beams.hpp -- beams toward the directions crsdr_doa found (crsdr_doa_set_beams): per estimate and beam slot a weight vector from the
// subspace the engine already holds, then the weighted sum of the packets' signal rows, one IQ stream per slot.
//
//   k_doa_beam_weights  grid (estimate, slot), one wave: steering vector a of the slot's direction (s_vecd2d's formula in fp64), then
//                         conventional  u = a / m                                   power = sum_r sv[r] |v_r^H a|^2 / m^2
//                         MVDR          z = sum_r v_r (v_r^H a) / (sv[r] + delta)   u = z / Re(a^H z)   power = 1 / Re(a^H z)
//                       with delta = loading * sv[0]; fp64 from the published fp32 vec / sv, rounded once.  sv[0] == 0: u = a / m, power 0.
//                       Slots from found[e] on: weights 0, power -1.
//   k_doa_beam_apply    grid (sample tile, block): y[t][b][n] = sum_c u[e][b][c-1] (I_c[n] + j Q_c[n]) / 127 over the signal rows
//                       c = 1 .. m, NO conjugate: the covariance is X^H X (the conjugate of E[x x^H]), so the steering vector at a MUSIC
//                       peak is conj(a_true) and w^H x becomes u^T x.
//
// The apply kernel's shape.  A thread owns two consecutive samples (one dword of every row) and all NB beam slots of them: a loaded
// sample is converted once and used 4 NB times, and the accumulators (4 NB floats) stay in registers.  The weights are the same for
// the whole workgroup: it copies them into LDS once (at most 8 KiB) and every wave reads them back as broadcasts.  (Left to the
// compiler as scalar loads they overflow the SGPR file at 8 and 16 slots -- 1500 v_writelane / v_readlane around the 1152 FMAs of
// eight rows -- and the 16-slot kernel ran at a third of this one's rate.)  Lane i of a wave reads dword i of a row's 256-byte
// segment and writes 16 bytes of every beam at 16 i: every load instruction is one contiguous 256 bytes and every store one
// contiguous 1 KiB.  (Eight samples per thread from one 16-byte load, as the covariance reads the rows, would put a lane's stores
// 64 bytes apart -- four partial writes per 64-byte request on the store side, which at four beams and more carries as many bytes as
// the loads -- or need 16 NB accumulators per thread; the row segments are contiguous either way.)  The rows are read once and the
// beams written once: the stores are non-temporal.  Plain fmaf, no packed math (the Makefile's note on v_pk_fma_f32's rate).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace crsdr {
namespace beams {

constexpr int MAX_M = 64, MAX_BEAMS = 16, BW_THREADS = 64, AP_THREADS = 256;
enum { MODE_OFF = 0, MODE_CONVENTIONAL = 1, MODE_MVDR = 2 };

// grid (nest, nbeams), BW_THREADS = 64 threads (m <= 64: thread i owns element i and column i).
//   vec [nest][m][m] (column r = v_r), sv [nest][m];  the slot's direction: fixed ? angles [nbeams][2] (alpha, beta)
//   : found ? peaks [nest][nbeams][2] with found [nest] : peak [nest][2] (one slot); refined: NULL, or offsets [nest][nbeams][2] in
//   grid cells added to the slot's grid point in fp64 (crsdr_doa_set_refine).  With NULL the arithmetic is what it was without it.
//   weights [nest][nbeams][m], power [nest][nbeams]
__global__ __launch_bounds__(BW_THREADS) void k_doa_beam_weights(const float2 *__restrict__ vec, const float *__restrict__ sv, int m, int mx, float d, int ncx,
                                                                  int ncy, int mode, float loading, const float *__restrict__ angles,
                                                                  const int32_t *__restrict__ found, const int32_t *__restrict__ peaks,
                                                                  const int32_t *__restrict__ peak, const float *__restrict__ refined, float2 *__restrict__ weights,
                                                                  float *__restrict__ power)
{
    __shared__ double2 sa[MAX_M], sg[MAX_M];
    __shared__ double sred[MAX_M];
    const int e = blockIdx.x, b = blockIdx.y, nb = gridDim.y, i = threadIdx.x;
    const size_t slot = (size_t)e * nb + b;
    float2 *u = weights + slot * m;
    double alpha, beta;
    if (angles) {
        alpha = (double)angles[2 * b]; beta = (double)angles[2 * b + 1];
    } else {
        const int32_t *p = found ? peaks + 2 * slot : peak + 2 * (size_t)e;
        if (found && b >= found[e]) {                              // an empty slot (workgroup-uniform)
            if (i < m) u[i] = make_float2(0.f, 0.f);
            if (i == 0) power[slot] = -1.0f;
            return;
        }
        const double pi = 3.14159265358979323846;
        if (refined) {
            alpha = ((double)p[0] + (double)refined[2 * slot]) * pi / (double)ncx; beta = ((double)p[1] + (double)refined[2 * slot + 1]) * pi / (double)ncy;
        } else {
            alpha = (double)p[0] * pi / (double)ncx; beta = (double)p[1] * pi / (double)ncy;
        }
    }
    const float2 *V = vec + (size_t)e * m * m;
    const float *s = sv + (size_t)e * m;
    double2 a = make_double2(0.0, 0.0);
    if (i < m) {
        const int ix = i % mx, iy = i / mx;
        const double ph = 2.0 * 3.14159265358979323846 * (double)d * ((double)ix * cos(alpha) * sin(beta) + (double)iy * cos(beta));
        a = make_double2(cos(ph), sin(ph));
        sa[i] = a;
    }
    __syncthreads();
    // thread r: g_r = v_r^H a, and its terms of the two sums over r
    const double s0 = (double)s[0], delta = (double)loading * s0;
    const bool mvdr = mode == MODE_MVDR && s0 != 0.0;
    double term = 0.0;
    if (i < m) {
        double gr = 0.0, gi = 0.0;
        for (int c = 0; c < m; ++c) {
            const float2 v = V[(size_t)c * m + i];
            const double2 ac = sa[c];
            gr += (double)v.x * ac.x + (double)v.y * ac.y;        // conj(v) a
            gi += (double)v.x * ac.y - (double)v.y * ac.x;
        }
        const double g2 = gr * gr + gi * gi, sr = (double)s[i];
        if (mvdr) { const double w = 1.0 / (sr + delta); sg[i] = make_double2(gr * w, gi * w); term = g2 * w; }
        else term = sr * g2;
    }
    sred[i] = term;
    __syncthreads();
    double sum = 0.0;
    for (int r = 0; r < m; ++r) sum += sred[r];                   // the same order in every thread
    if (mvdr) {
        // sum = Re(a^H z) = sum_r |g_r|^2 / (sv[r] + delta)
        if (i < m) {
            double zr = 0.0, zi = 0.0;
            for (int r = 0; r < m; ++r) {
                const float2 v = V[(size_t)i * m + r];
                const double2 g = sg[r];
                zr += (double)v.x * g.x - (double)v.y * g.y;
                zi += (double)v.x * g.y + (double)v.y * g.x;
            }
            u[i] = make_float2((float)(zr / sum), (float)(zi / sum));
        }
        if (i == 0) power[slot] = (float)(1.0 / sum);
    } else {
        if (i < m) u[i] = make_float2((float)(a.x / (double)m), (float)(a.y / (double)m));
        if (i == 0) power[slot] = (float)(sum / ((double)m * (double)m));
    }
}

// 4 bytes from a 4-byte aligned row (a packet's matrix starts at 16 + 4 N; rows are a multiple of 32 bytes)
__device__ __forceinline__ uint32_t row_dword(const int8_t *p) { return *reinterpret_cast<const uint32_t *>(p); }

// The arithmetic of a beam, shared by the batched kernel and crsdr_beamform (the same instruction sequence: the same bits).  Called by
// every thread of an AP_THREADS workgroup.
//   matrix [1 + m][B] int8, m <= MAX_M; u [nbeams][m], the same for the whole workgroup; out [nbeams][B / 2];
//   pair = which two samples of the block this thread owns.
// The workgroup first lays the weights out in LDS as [m][NB], a row's slots side by side: in the row loop they are 16-byte reads of one
// address per wave (a broadcast, two slots each).  Slots nbeams .. NB - 1 of the template repeat the last one's weights and store nothing.
template <int NB>
__device__ __forceinline__ void beam_pair(const int8_t *__restrict__ matrix, int m, int B, const float2 *__restrict__ u, int nbeams, float2 *__restrict__ out,
                                          int pair)
{
    __shared__ __attribute__((aligned(16))) float2 wl[MAX_M * NB];
    for (int i = threadIdx.x; i < m * NB; i += AP_THREADS) {
        const int c = i / NB, b = i - c * NB;
        wl[i] = u[(size_t)min(b, nbeams - 1) * m + c];
    }
    __syncthreads();
    const int pairs = B >> 2;
    if (pair >= pairs) return;
    const int8_t *row = matrix + (size_t)B + 4 * (size_t)pair;      // signal row 1
    float re0[NB], im0[NB], re1[NB], im1[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) re0[b] = im0[b] = re1[b] = im1[b] = 0.f;
    // ROWS rows are loaded before the first is used (a rolled loop, and the compiler's own unrolling of it, waits out one round trip
    // per row): as many as the accumulators leave room for.  The rows past the last are the last one again, loaded and not used.
    constexpr int ROWS = NB <= 4 ? 16 : 8;
    for (int c0 = 0; c0 < m; c0 += ROWS) {
        uint32_t w[ROWS];
#pragma unroll
        for (int k = 0; k < ROWS; ++k) w[k] = row_dword(row + (size_t)min(c0 + k, m - 1) * B);
#pragma unroll
        for (int k = 0; k < ROWS; ++k) {
            const int c = c0 + k;
            if (c < m) {
                const float i0 = (float)(int8_t)(w[k] & 0xFF), q0 = (float)(int8_t)((w[k] >> 8) & 0xFF);
                const float i1 = (float)(int8_t)((w[k] >> 16) & 0xFF), q1 = (float)(int8_t)(w[k] >> 24);
#pragma unroll
                for (int b = 0; b < NB; ++b) {
                    const float2 v = wl[c * NB + b];
                    re0[b] = fmaf(-v.y, q0, fmaf(v.x, i0, re0[b]));
                    im0[b] = fmaf(v.y, i0, fmaf(v.x, q0, im0[b]));
                    re1[b] = fmaf(-v.y, q1, fmaf(v.x, i1, re1[b]));
                    im1[b] = fmaf(v.y, i1, fmaf(v.x, q1, im1[b]));
                }
            }
        }
    }
    const float sc = 1.0f / 127.0f;
    typedef float f4 __attribute__((ext_vector_type(4)));
#pragma unroll
    for (int b = 0; b < NB; ++b)
        if (b < nbeams) {
            const f4 y = {re0[b] * sc, im0[b] * sc, re1[b] * sc, im1[b] * sc};
            __builtin_nontemporal_store(y, reinterpret_cast<f4 *>(out + (size_t)b * (B >> 1) + 2 * (size_t)pair));
        }
}

// grid (ceil(B / 4 / AP_THREADS), nblocks).  Packet t at packets + t * packet_stride, its matrix at + matrix_off (4-byte aligned);
// weights [nest][nbeams][m] of estimate t / frames; beams [nblocks][nbeams][B / 2].
template <int NB>
__global__ __launch_bounds__(AP_THREADS) void k_doa_beam_apply(const int8_t *__restrict__ packets, size_t packet_stride, size_t matrix_off, int nrows, int B,
                                                               int frames, const float2 *__restrict__ weights, int nbeams, float2 *__restrict__ beams)
{
    const int t = blockIdx.y, m = nrows - 1;
    beam_pair<NB>(packets + (size_t)t * packet_stride + matrix_off, m, B, weights + (size_t)(t / frames) * nbeams * m, nbeams,
                  beams + (size_t)t * nbeams * (B >> 1), (int)(blockIdx.x * AP_THREADS + threadIdx.x));
}

// crsdr_beamform: one matrix.  grid (ceil(B / 4 / AP_THREADS))
template <int NB>
__global__ __launch_bounds__(AP_THREADS) void k_beamform(const int8_t *__restrict__ matrix, int nrows, int B, const float2 *__restrict__ weights, int nbeams,
                                                         float2 *__restrict__ out)
{
    beam_pair<NB>(matrix, nrows - 1, B, weights, nbeams, out, (int)(blockIdx.x * AP_THREADS + threadIdx.x));
}

__host__ __device__ constexpr int slots_for(int nbeams) { return nbeams <= 1 ? 1 : nbeams <= 2 ? 2 : nbeams <= 4 ? 4 : nbeams <= 8 ? 8 : 16; }

} // namespace beams
} // namespace crsdr
