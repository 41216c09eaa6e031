// refine.hpp -- a direction off the scan grid (crsdr_doa_set_refine, crsdr_refine2d): an fp64 zoom search for the maximum of the map
// between the grid points, around a direction (cx, cy) the scan found.
//
// The search (include/crsdr.h has the same words).  Cell coordinates x, y (doubles), alpha = x pi / ncx, beta = y pi / ncy; the steering
// vector is k_doa_beam_weights' fp64 expression, ph_i = 2 pi (double)d (ix cos(alpha) sin(beta) + iy cos(beta)), a_i = (cos ph_i, sin ph_i);
// f(x, y) is the object's map in fp64 from the published fp32 vec / sv, y_r = v_r^H a:
//     MUSIC     (M / sum_{r >= k} |y_r|^2)^2
//     Bartlett  S,  Capon 1 / S,   S = sum_r w_r |y_r|^2 with spectrum.hpp's w_r in fp64, not rounded to fp32
//     sv[0] == 0: f = 0
//     x = cx, y = cy, s = 1/2
//     repeat `levels` times:
//         c = f(x, y); best = c; (bx, by) = (x, y)
//         for i in -3..3, for j in -3..3 (i major), (i, j) != (0, 0):
//             px = min(max(x + i s, 0), ncx); py = min(max(y + j s, 0), ncy); v = f(px, py)
//             if v > c and v > best: best = v; (bx, by) = (px, py)
//         (x, y) = (bx, by); s = s / 4
// The centre keeps ties, a NaN never wins, the lowest index wins equal values.  Every coordinate is a multiple of 2^-(2 levels - 1) and
// |x - cx| < 2: the offsets are exact in fp32.  49 points per level whatever the data.
//
// Shape.  grid (slot, matrix), RF_WAVES waves.  A lane is one of the 49 lattice points (lanes 49 .. 63 repeat the last and are not
// read).  Per level: the waves share the elements i of the lanes' steering vectors (one fp64 sincos per element and lane, i = wave,
// wave + RF_WAVES, ..) and write them to LDS as A[i][lane], 16 bytes per lane side by side: conflict-free like the scans'.  Then the
// waves share the columns of vec four at a time (block b = columns 4b .. 4b + 3 to wave b mod RF_WAVES): per element one 16-byte read
// of a[i] and four 8-byte broadcasts of vec[i][4b ..] (vec lies in LDS as it is published, fp32, staged once per workgroup) serve 16
// fp64 FMAs on eight accumulators.  Each wave adds its blocks' w_r |y_r|^2 in ascending r, the partial sums meet in LDS and are added
// in wave order: no atomics, the same bits wherever a matrix stands in a batch.  Wave 0 forms f of the 49 points; every thread then
// walks them in the definition's order, so all hold the same (x, y) for the next level without another exchange.
// Trip counts are workgroup-uniform (levels, ceil(M / 4) blocks less MUSIC's signal-only ones, M elements), the barriers plain __syncthreads().  An empty slot
// returns before any barrier, uniformly for the workgroup.
//   LDS: A [M][64] cf64 + w [M] f64 + vec [M][M] cf32 = 98 816 bytes at M = 64: above the 64 KiB default, the callers raise the limit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace crsdr {
namespace refine {

enum { KIND_MUSIC = 0, KIND_BARTLETT = 1, KIND_CAPON = 2 };
constexpr int MAX_M = 64, MAX_LEVELS = 8, RF_WAVES = 4, RF_THREADS = 64 * RF_WAVES, SIDE = 7, POINTS = SIDE * SIDE, COLS = 4;

__host__ __device__ constexpr size_t lds_bytes(int M)
{
    return sizeof(double2) * (size_t)M * 64 + sizeof(double) * (size_t)M + sizeof(float2) * (size_t)M * M;
}

// grid (nslots, nmat), 64 W threads (W = RF_WAVES; a template, so that the kernel is emitted where it is first launched), lds_bytes(M) of dynamic LDS.
//   vec [nmat][M][M] (column r = v_r), sv [nmat][M]; korder [nmat] or NULL: the matrix's source count in place of k (MUSIC)
//   dirs [nmat][nslots][2] (cx, cy), found [nmat] or NULL (every slot holds a direction); a slot from found on, or one whose
//   direction lies outside [0, Cx] x [0, Cy], is empty: offsets (0, 0), angles (-1, -1), value -1
//   offsets [nmat][nslots][2], angles [nmat][nslots][2], values [nmat][nslots]
template <int W>
__global__ __launch_bounds__(64 * W) void k_doa_refine(const float2 *__restrict__ vec, const float *__restrict__ sv, int M, int kind, int k,
                                                           const int32_t *__restrict__ korder, float loading, float d, int Mx, int Cx, int Cy,
                                                           const int32_t *__restrict__ dirs, const int32_t *__restrict__ found, int levels,
                                                           float *__restrict__ offsets, float *__restrict__ angles, float *__restrict__ values)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char rsm[];
    double2 *A = reinterpret_cast<double2 *>(rsm);                       // [M][64]
    double *w = reinterpret_cast<double *>(A + (size_t)M * 64);          // [M]
    float2 *U = reinterpret_cast<float2 *>(w + M);                       // [M][M], as published
    __shared__ double part[W][64];
    __shared__ double fval[64];
    const int b = blockIdx.x, nslots = gridDim.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t e = blockIdx.y, slot = e * nslots + b;
    const int32_t cx = dirs[2 * slot], cy = dirs[2 * slot + 1];
    if ((found && b >= found[e]) || cx < 0 || cy < 0 || cx > Cx || cy > Cy) {      // an empty slot (workgroup-uniform)
        if (tid < 2) { offsets[2 * slot + tid] = 0.f; angles[2 * slot + tid] = -1.f; }
        if (tid == 0) values[slot] = -1.f;
        return;
    }
    const double pi = 3.14159265358979323846;
    const float *s = sv + e * M;
    const double s0 = (double)s[0];
    double x = (double)cx, y = (double)cy, best = 0.0;
    if (s0 != 0.0) {                                                     // (workgroup-uniform; an all-zero estimate: f = 0, the centre keeps every tie)
        const float2 *V = vec + e * M * M;
        for (int i = tid; i < M * M; i += 64 * W) U[i] = V[i];
        const int ke = korder ? korder[e] : k;
        if (tid < M) {
            const double sr = (double)s[tid];
            w[tid] = kind == KIND_MUSIC ? (tid >= ke ? 1.0 : 0.0)
                   : kind == KIND_CAPON ? 1.0 / (sr + (double)loading * s0) : sr / ((double)M * (double)M);
        }
        const int p = min(lane, POINTS - 1), li = p / SIDE - SIDE / 2, lj = p % SIDE - SIDE / 2;
        // MUSIC: the blocks wholly below k_e hold signal columns alone (w = 0) and are passed over; a block stays with its wave
        const int nblk = (M + COLS - 1) / COLS, blk0 = kind == KIND_MUSIC ? max(ke, 0) / COLS : 0;
        double step = 0.5;
        for (int l = 0; l < levels; ++l) {
            const double px = fmin(fmax(x + (double)li * step, 0.0), (double)Cx), py = fmin(fmax(y + (double)lj * step, 0.0), (double)Cy);
            const double alpha = px * pi / (double)Cx, beta = py * pi / (double)Cy;
            const double ca = cos(alpha), sb = sin(beta), cb = cos(beta);
            for (int i = wave; i < M; i += W) {
                const int ix = i % Mx, iy = i / Mx;
                const double ph = 2.0 * pi * (double)d * ((double)ix * ca * sb + (double)iy * cb);
                double sn, cs;
                sincos(ph, &sn, &cs);
                A[(size_t)i * 64 + lane] = make_double2(cs, sn);
            }
            __syncthreads();                                             // A (and, at the first level, U and w) in place
            double S = 0.0;
            for (int blk = wave; blk < nblk; blk += W) {
                if (blk < blk0) continue;                                // (wave-uniform)
                const int r0 = COLS * blk;
                int col[COLS];
#pragma unroll
                for (int c = 0; c < COLS; ++c) col[c] = min(r0 + c, M - 1);          // (behind the last column: it again, not added)
                double yr[COLS], yi[COLS];
#pragma unroll
                for (int c = 0; c < COLS; ++c) yr[c] = yi[c] = 0.0;
#pragma unroll 2
                for (int i = 0; i < M; ++i) {
                    const double2 a = A[(size_t)i * 64 + lane];
#pragma unroll
                    for (int c = 0; c < COLS; ++c) {                    // y += conj(u) a
                        const float2 u = U[i * M + col[c]];
                        const double ur = (double)u.x, ui = (double)u.y;
                        yr[c] = fma(ui, a.y, fma(ur, a.x, yr[c]));
                        yi[c] = fma(-ui, a.x, fma(ur, a.y, yi[c]));
                    }
                }
#pragma unroll
                for (int c = 0; c < COLS; ++c)
                    if (r0 + c < M) S = fma(w[r0 + c], fma(yr[c], yr[c], yi[c] * yi[c]), S);
            }
            part[wave][lane] = S;
            __syncthreads();                                             // the waves' partial sums
            if (wave == 0) {
                double t = part[0][lane];
#pragma unroll
                for (int v = 1; v < W; ++v) t += part[v][lane];
                double f;
                if (kind == KIND_MUSIC) { const double q = (double)M / t; f = q * q; }
                else f = kind == KIND_CAPON ? 1.0 / t : t;
                fval[lane] = f;
            }
            __syncthreads();                                             // f of the 49 points
            // the definition's walk, the same in every thread
            const double c = fval[POINTS / 2];
            double bx = x, by = y;
            best = c;
            for (int q = 0; q < POINTS; ++q) {
                if (q == POINTS / 2) continue;
                const double v = fval[q];
                if (v > c && v > best) {
                    best = v;
                    bx = fmin(fmax(x + (double)(q / SIDE - SIDE / 2) * step, 0.0), (double)Cx);
                    by = fmin(fmax(y + (double)(q % SIDE - SIDE / 2) * step, 0.0), (double)Cy);
                }
            }
            x = bx; y = by; step *= 0.25;
        }
    }
    if (tid == 0) {
        offsets[2 * slot] = (float)(x - (double)cx); offsets[2 * slot + 1] = (float)(y - (double)cy);
        angles[2 * slot] = (float)(x * pi / (double)Cx); angles[2 * slot + 1] = (float)(y * pi / (double)Cy);
        values[slot] = (float)best;
    }
}

} // namespace refine
} // namespace crsdr
