// subband_beams.hpp -- a beam per frequency band toward each band's directions (crsdr_doa_set_subband_beams / crsdr_subband_beamform).
//
// Definition (tests/doa_subband_beams_model.py is the fp64 statement of it).  With subbands on, every (estimate e, band i) has its own
// subspace, so beams.hpp's k_doa_beam_weights, launched over nest * nbands matrices, leaves weights u [e][i][slot][m].  The beam is the
// weighted sum of the rows' band SPECTRA, not of their samples: with X_c[t][j][f] the segment spectrum of subband.hpp (window w,
// forward transform of (I + jQ) / 127) and c_w = 1 / sqrt(N sum_n w[n]^2),
//     Y[t][i][b][j][u] = c_w sum_c u_{e,i,b}[c - 1] X_c[t][j][(first + i width + u) mod N],       NO conjugate (beams.hpp says why)
// one narrowband IQ stream per (packet, band, slot): the band's channeliser output, `width` bins at J = L / N samples per packet.
// c_w is the normalisation behind R_f: mean_j |Y|^2 of one bin is u^H R_f u.
//
//   k_doa_subband_beam_apply  grid (K slice of segments, packet), 256 threads, dynamic LDS.  Per chunk of segments the workgroup loads
//                             ALL m rows (16-byte loads of the int8 packets), applies the window and runs the N-point transform in
//                             LDS with k_doa_subband_cov's own front end (subband.hpp's sb_fill_tables, sb_unpack_window, sb_pass1 and
//                             sb_pass2: one statement of the passes, so the same spectra) -- every row once per segment, where the covariance transforms a row
//                             once per unit group that touches it.  Then a thread owns one (band, segment, bin of the band) and
//                             runs over the m channels once per group of up to four slots, the spectra and the band's weights
//                             both from LDS, 4 fmaf per (channel, slot).
// LDS.  A segment of all rows is m N float2: 128 KiB at m = 64, N = 256, so the spectra are dynamic LDS, sized by the host to
// sbb_lds_points() = as many whole segments as fit in 40 KiB, at least one (131080 bytes at the largest shape; with the 19 KiB of
// static LDS under the CU's 160 KiB).  Segments are laid out at a stride of m N + 1 float2: the lanes of a wave are consecutive
// segments reading the same (row, bin), and m N is a multiple of 8, which would put all of them on one or two banks; at an odd
// stride 32 lanes of an 8-byte read fall on 32 different bank pairs.
// Weights.  The bands' weights are staged in LDS as [band][m][slots padded to the group], 16 KiB at most: as many bands at a time as
// fit (all 16 of the 21-row, 2-slot case; 2 at m = 64 with 16 slots).  The lanes of a wave mostly share a band: broadcast reads.
// Stores.  Consecutive lanes are consecutive (segment, bin) of one (band, slot): 8 bytes each, contiguous, non-temporal (written
// once, read by the next consumer or the host).
// Order.  A sample is a chain of 2 m fmaf over the channels in order and one multiplication by the scale, whatever the chunking and
// the grid: a packet has the same bits wherever it sits in a batch, and from crsdr_subband_beamform.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "covariance.hpp"
#include "fft_lds.hpp"
#include "subband.hpp"

namespace crsdr {
namespace sbbeams {

constexpr int SBB_THREADS = subband::SB_THREADS, SBB_MAX_ROWS = 64, SBB_MAX_BEAMS = 16;      // (the shared front end strides by SB_THREADS)
constexpr int SBB_LDS_POINTS = 5120;       // float2 of spectra per chunk (40 KiB) wherever a segment of all rows is smaller
constexpr int SBB_WEIGHT_POINTS = 2048;    // float2 of staged weights (16 KiB): at least one band (64 rows x 16 slots = 1024)

__host__ __device__ constexpr int sbb_seg_stride(int m, int N) { return m * N + 1; }
// K slices per packet: subband.hpp's split of the segments, from (B, N) alone
__host__ __device__ constexpr int sbb_spb(int B, int N) { return subband::subband_spb(B, N); }
// float2 of dynamic LDS: whole segments, as many as fit the budget or a slice needs, at least one
__host__ __device__ constexpr int sbb_lds_points(int m, int B, int N)
{
    const int stride = sbb_seg_stride(m, N), J = B / (2 * N), spb = sbb_spb(B, N), per_slice = (J + spb - 1) / spb;
    int sc = SBB_LDS_POINTS / stride;
    sc = sc < 1 ? 1 : sc;
    sc = sc > per_slice ? per_slice : sc;
    return sc * stride;
}
// the slot count of the staged weights: 1, 2, or padded to the groups of four a thread carries at once
__host__ __device__ constexpr int sbb_padded(int nbeams) { return nbeams <= 2 ? nbeams : (nbeams + 3) & ~3; }

typedef float sbb_f2 __attribute__((ext_vector_type(2)));

// The threads' share of bands g0 .. g0 + bg - 1 of a transformed chunk: SG slots at a time.
//   A   [sc][stride]: segment jj's row c at jj * stride + c * N, bin f in slot (f mod FA) FB + f / FA (subband.hpp)
//   wl  [bg][m][nbp]: the staged weights;  out: the packet's [nbands][nbeams][J][width]
template <int LOG2N, int SG>
__device__ __forceinline__ void sbb_items(const float2 *__restrict__ A, int stride, const float2 *__restrict__ wl, int m, int nbp, int g0, int bg, int sc, int s0,
                                          int first, int width, int nbeams, int J, float scale, float2 *__restrict__ out)
{
    constexpr int N = 1 << LOG2N, LA = subband::sb_fa_log2(LOG2N), FA = 1 << LA, LB = LOG2N - LA;
    const int per = sc * width, items = bg * per;
    const size_t slot_stride = (size_t)J * width;
    for (int it = threadIdx.x; it < items; it += SBB_THREADS) {
        const int bl = it / per, rem = it - bl * per, jj = rem / width, u = rem - jj * width;
        const int band = g0 + bl, f = (first + band * width + u) & (N - 1), bin_slot = ((f & (FA - 1)) << LB) + (f >> LA);
        const float2 *x = A + jj * stride + bin_slot;
        const float2 *w = wl + bl * m * nbp;
        float2 *o = out + ((size_t)band * nbeams * J + (size_t)(s0 + jj)) * width + u;
        for (int b0 = 0; b0 < nbeams; b0 += SG) {
            float re[SG], im[SG];
#pragma unroll
            for (int s = 0; s < SG; ++s) re[s] = im[s] = 0.f;
#pragma unroll 4
            for (int c = 0; c < m; ++c) {
                const float2 v = x[c * N];
#pragma unroll
                for (int s = 0; s < SG; ++s) {
                    const float2 k = w[c * nbp + b0 + s];
                    re[s] = fmaf(-k.y, v.y, fmaf(k.x, v.x, re[s]));
                    im[s] = fmaf(k.y, v.x, fmaf(k.x, v.y, im[s]));
                }
            }
#pragma unroll
            for (int s = 0; s < SG; ++s)
                if (b0 + s < nbeams) {
                    const sbb_f2 y = {re[s] * scale, im[s] * scale};
                    __builtin_nontemporal_store(y, reinterpret_cast<sbb_f2 *>(o + (size_t)(b0 + s) * slot_stride));
                }
        }
    }
}

// The arithmetic of the band beams, shared by the batched kernel and crsdr_subband_beamform (the same instruction sequence: the same
// bits).  Called by every thread of an SBB_THREADS workgroup with lds_points float2 of dynamic LDS (sbb_lds_points()).
//   matrix [1 + m][B] int8, m <= 64;  u [nbands][nbeams][m];  out [nbands][nbeams][J][width];  segments seg_lo .. seg_hi - 1 of the packet
template <int LOG2N>
__device__ __forceinline__ void subband_beam_slice(const int8_t *__restrict__ matrix, int m, int B, int first, int nbands, int width, int window,
                                                   const float2 *__restrict__ u, int nbeams, float2 *__restrict__ out, int seg_lo, int seg_hi, int lds_points)
{
    constexpr int N = 1 << LOG2N, LA = subband::sb_fa_log2(LOG2N), FA = 1 << LA, LB = LOG2N - LA, FB = 1 << LB;
    extern __shared__ __attribute__((aligned(16))) float sbb_lds[];                // float2 [segment of the chunk][stride]
    __shared__ __attribute__((aligned(16))) float2 wl[SBB_WEIGHT_POINTS];          // [band of the group][m][nbp]
    __shared__ float2 tw[N];                                                       // W_N^t
    __shared__ float win[N];
    float2 *A = reinterpret_cast<float2 *>(sbb_lds);
    const int tid = threadIdx.x, J = B / (2 * N), stride = sbb_seg_stride(m, N);
    const int SC = min(lds_points / stride, seg_hi - seg_lo);
    const int nbp = sbb_padded(nbeams), bg_max = min(nbands, SBB_WEIGHT_POINTS / (m * nbp));
    subband::sb_fill_tables<LOG2N>(tw, win, window);
    // c_w / 127: 1 / (127 sqrt(N sum w^2)), sum w^2 = N (rect), 3 N / 8 (periodic Hann)
    const float scale = (float)(1.0 / (127.0 * sqrt((double)N * (window == subband::WINDOW_HANN ? 0.375 * (double)N : (double)N))));
    // bands g0 .. g0 + bg - 1 -> wl, slots past nbeams zero
    auto stage = [&](int g0, int bg) {
        for (int i = tid; i < bg * m * nbp; i += SBB_THREADS) {
            const int bl = i / (m * nbp), r = i - bl * (m * nbp), c = r / nbp, b = r - c * nbp;
            wl[i] = b < nbeams ? u[((size_t)(g0 + bl) * nbeams + b) * m + c] : make_float2(0.f, 0.f);
        }
    };
    const bool one_group = bg_max >= nbands;
    if (one_group) stage(0, nbands);
    __syncthreads();
    for (int s0 = seg_lo; s0 < seg_hi; s0 += SC) {
        const int sc = min(SC, seg_hi - s0);
        // load: 16 bytes = 8 samples per item; a row's chunk is contiguous
        const int ppr = sc * N / 8;              // pieces per row
        for (int it = tid; it < m * ppr; it += SBB_THREADS) {
            const int r = it / ppr, piece = it - r * ppr;
            const uint4 wd = cov::cov_load16(matrix + (size_t)(1 + r) * B + (size_t)s0 * 2 * N + (size_t)piece * 16);
            const int jj = (piece * 8) >> LOG2N, n0 = (piece * 8) & (N - 1);
            subband::sb_unpack_window(wd, win, n0, A + jj * stride + r * N + n0);
        }
        __syncthreads();
        // pass 1: FA-point DFTs at stride FB, then W_N^(n2 k1)
        for (int it = tid; it < sc * m * FB; it += SBB_THREADS) {
            const int n2 = it & (FB - 1), sr = it >> LB, jj = sr / m;
            subband::sb_pass1<LOG2N>(A + jj * stride + (sr - jj * m) * N + n2, tw, n2);
        }
        __syncthreads();
        if constexpr (FB > 1) {
            // pass 2: FB-point DFTs of consecutive points
            for (int it = tid; it < sc * m * FA; it += SBB_THREADS) {
                const int k1 = it & (FA - 1), sr = it >> LA, jj = sr / m;
                subband::sb_pass2<LOG2N>(A + jj * stride + (sr - jj * m) * N + k1 * FB);
            }
            __syncthreads();
        }
        for (int g0 = 0; g0 < nbands; g0 += bg_max) {
            const int bg = min(bg_max, nbands - g0);
            if (!one_group) {
                stage(g0, bg);
                __syncthreads();
            }
            if (nbeams == 1) sbb_items<LOG2N, 1>(A, stride, wl, m, nbp, g0, bg, sc, s0, first, width, nbeams, J, scale, out);
            else if (nbeams == 2) sbb_items<LOG2N, 2>(A, stride, wl, m, nbp, g0, bg, sc, s0, first, width, nbeams, J, scale, out);
            else sbb_items<LOG2N, 4>(A, stride, wl, m, nbp, g0, bg, sc, s0, first, width, nbeams, J, scale, out);
            if (!one_group) __syncthreads();
        }
        __syncthreads();
    }
}

// grid (spb, nblocks).  Packet t at packets + t * packet_stride, its matrix at + matrix_off (4-byte aligned); weights
// [nest][nbands][nbeams][m] of estimate t / frames; beams [nblocks][nbands][nbeams][J][width].
template <int LOG2N>
__global__ __launch_bounds__(SBB_THREADS) void k_doa_subband_beam_apply(const int8_t *__restrict__ packets, size_t packet_stride, size_t matrix_off, int nrows, int B,
                                                                        int frames, int first, int nbands, int width, int window,
                                                                        const float2 *__restrict__ weights, int nbeams, int lds_points, float2 *__restrict__ beams)
{
    const int t = blockIdx.y, m = nrows - 1, J = B >> (LOG2N + 1), part = blockIdx.x, spb = gridDim.x;
    const int seg_lo = (int)(((long long)J * part) / spb), seg_hi = (int)(((long long)J * (part + 1)) / spb);
    subband_beam_slice<LOG2N>(packets + (size_t)t * packet_stride + matrix_off, m, B, first, nbands, width, window,
                              weights + (size_t)(t / frames) * nbands * nbeams * m, nbeams, beams + (size_t)t * nbands * nbeams * J * width, seg_lo, seg_hi,
                              lds_points);
}

// crsdr_subband_beamform: one matrix.  grid (spb)
template <int LOG2N>
__global__ __launch_bounds__(SBB_THREADS) void k_subband_beamform(const int8_t *__restrict__ matrix, int nrows, int B, int first, int nbands, int width, int window,
                                                                  const float2 *__restrict__ weights, int nbeams, int lds_points, float2 *__restrict__ out)
{
    const int J = B >> (LOG2N + 1), part = blockIdx.x, spb = gridDim.x;
    const int seg_lo = (int)(((long long)J * part) / spb), seg_hi = (int)(((long long)J * (part + 1)) / spb);
    subband_beam_slice<LOG2N>(matrix, nrows - 1, B, first, nbands, width, window, weights, nbeams, out, seg_lo, seg_hi, lds_points);
}

} // namespace sbbeams
} // namespace crsdr
