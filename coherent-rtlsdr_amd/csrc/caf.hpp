// caf.hpp -- range-Doppler maps (the cross-ambiguity function) of a packet's rows against one of them: crsdr_caf / crsdr_ambiguity.
//
// Definition (include/crsdr.h, section (w); tests/caf_model.py is the fp64 statement of it).  Row c of a packet's matrix [nrows][B] int8
// holds L = B / 2 samples, here the integers X_c[n] = I + jQ.  Ls = seg, a packet has J = L / Ls segments, a line is `frames` packets,
// slow time k = t J + j < nd = frames J, R = nlags, r = ref_row:
//     y_c[k][tau]   = sum_{n < Ls} X_c[t][j Ls + n] conj(X_r[t][j Ls + n - tau])         int32, exact; X_r[t][m] = 0 for m < 0
//     chi_c[d][tau] = 1 / (127^2 Ls sum w) * sum_k w[k] y_c[k][tau] exp(-2 pi i d k / nd)      chi [nest][nrows][nd][R] float2
//     map[d][tau]   = sum_{c != r} |chi_c[d][tau]|^2                                            map [nest][nd][R] float
// and the peak figures of every row's |chi|^2 and of map: caf_peak.hpp.
//
//   k_caf<LG>     grid (row * tiles + tile, line), 256 threads: ONE (line, row, tile of T = min(16, 4096 / nd) lags) per workgroup, both
//                 stages in it, nothing between workgroups.
//                 Range stage.  The line's row goes through LDS in chunks of 1024 words (a word = two samples, I0 Q0 I1 Q1): the row's
//                 words and, in front of the reference's, the `pre` words the tile's largest lag reaches back -- zeros in front of the
//                 packet's first sample, so a chunk never reads another packet.  Plain 4-byte loads: a matrix row is only 4-byte
//                 aligned.  An item is (piece of 8 words, an even lag and the odd lag behind it): both read the same row words and the same
//                 nine reference words.  Per word, with x = r[i + 1] for the even lag and w = v_alignbit(r[i + 1], r[i], 16) for the odd one
//                 (its reference straddles two words), for each of the two:
//                     re = sdot4(s, w)                                     I I + Q Q
//                     p  = sdot4(swap(s), w)                               Q_s I_r + I_s Q_r         swap: v_perm, bytes (Q0 I0 Q1 I1)
//                     e  = sdot4(swap(s), w & 0x00ff00ff)                  Q_s I_r                   the even-byte mask
//                 and Im = Q_s I_r - I_s Q_r = 2 e - p: the odd-byte product is p - e, so its mask and a fourth product are not needed.
//                 Ten instructions per word and pair, the swap and the realignment included: five per word and lag.  A wave's 64 items
//                 are 8 pieces by 8 pairs: the row's words are one broadcast address per piece and neighbouring pairs read neighbouring
//                 reference words.  The piece's four int32 sums go into ACC [nd][T][2] in LDS by ds_add (integers: any order gives the
//                 same bits), lag fastest, so that a wave's adds fall on consecutive words.  At nd = 4096 a tile is one lag of either
//                 parity: an item is then (piece, lag), the shift of v_alignbit 0 or 16.
//                 Doppler stage.  ACC is read into registers, converted with one rounding, multiplied by the window and written back over
//                 it as A [T][nd] float2 in spectra.hpp's padded layout; the twiddles take the place of the staged words; the T transforms
//                 run as one chunk of spectra.hpp's network (sp_pass); scale, digit reversal, and the store with tau fastest.
//                 LDS: A 34 KiB (32 KiB at nd = 4096, unpadded as in spectra.hpp) + max(twiddles, staged words) <= 64 KiB static.
//                 k_caf<LG, 1> and k_caf<LG, 2> are the canceller's two passes around the same range stage (CancelArgs below,
//                 caf_cancel.hpp): the sums of the first lags and the row's energy, and the rows with the reference's part taken out
//                 of ACC in fp64 before the Doppler stage.  k_caf<LG, 3> is the second stage's pass (CleanArgs, caf_clean.hpp): MODE 2
//                 with the line's target members behind the canceller's.  k_caf<LG> itself compiles to the instructions it had
//                 without them.
//   k_caf_map     grid (cells / 32, line): the fp64 sum of |chi|^2 over the rows but r, eight interleaved parts of the rows added in a
//                 fixed order, rounded once.
//   k_caf_peak    grid (entry, line), 256 threads: caf_peak.hpp's search, one part per thread, merged by a tree in LDS.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "caf_clean_solve.hpp"
#include "caf_peak.hpp"
#include "fft_lds.hpp"
#include "spectra.hpp"

namespace crsdr {
namespace caf {

constexpr int CAF_THREADS = 256, CAF_POINTS = 4096, CAF_TILE = 16;
constexpr int CAF_MIN_LOG2 = 3, CAF_MAX_LOG2 = 12;                     // log2 nd
constexpr int CAF_MIN_SEG_LOG2 = 4, CAF_MAX_SEG_LOG2 = 12, CAF_MAX_LAGS = 1024;
constexpr int CAF_CHUNK = 1024, CAF_PIECE = 8;                         // words
constexpr int CAF_PRE_MAX = CAF_MAX_LAGS / 2;                          // ((R - 1) >> 1) + 1 <= 512 words in front of a chunk
// the row's chunk, the reference's chunk with its prefix, and the word an even lag's last v_alignbit names without using it
constexpr int CAF_STAGE_WORDS = CAF_CHUNK + CAF_PRE_MAX + CAF_CHUNK + CAF_PIECE;

__host__ __device__ constexpr int caf_log2_tile(int lg) { return lg <= 8 ? 4 : 12 - lg; }
__host__ __device__ constexpr int caf_tile(int lg) { return 1 << caf_log2_tile(lg); }
__host__ __device__ constexpr int caf_tiles(int lg, int nlags) { return (nlags + caf_tile(lg) - 1) >> caf_log2_tile(lg); }
template <int LG>
constexpr int caf_u_words() { return 2 * (1 << LG) > CAF_STAGE_WORDS ? 2 * (1 << LG) : CAF_STAGE_WORDS; }

// Packet t of the batch at packets + t * packet_stride, its matrix [nrows][B] int8 at + matrix_off (4-byte aligned).
// tw_g, win: spectra::k_spectra_tables at N = nd.  scale = fp32(1 / (127^2 Ls sum w)).
// MODE 0 is crsdr_caf's kernel with the canceller off.  The canceller's two passes (caf_cancel.hpp) are the same code around the same
// range stage: MODE 1 stops behind it and leaves the sums of the lags < nlags (there: taps) and the row's energy; MODE 2 takes the
// reference's part out of ACC, in fp64 with one rounding, before the Doppler stage reads it.
struct CancelArgs {
    int taps = 0, dopp = 0, nlags = 0;             // nlags: G's (the map's), which MODE 1 does not get as its own
    const int2 *G = nullptr;                       // [nest][nd][taps][nlags]
    const double2 *h = nullptr, *ph = nullptr;     // [nest][nrows][n] fp64 coefficients; exp(2 pi i j / nd), j < nd
    const int *status = nullptr;                   // [nest]
    int2 *Y = nullptr;                             // [nest][nrows][nd][taps]
    long long *E = nullptr;                        // [nest][nrows]
};
// MODE 3 is MODE 2 on the joint coefficients of the second stage (caf_clean.hpp): the canceller's members as MODE 2 takes them, then the
// line's target members.  h [nest][nrows][hstride], the canceller's n1 first; status: the joint solve's (bit 0: nothing is taken out;
// bit 1: the canceller's members alone, whose h is then stage 1's).
struct CleanArgs : CancelArgs {
    int hstride = 0, slots = 0, members = 0;       // h's stride; G2's lags and ph2's members per line as allocated
    const cl::Table *tab = nullptr;                // [nest]: the lines' members
    const int2 *G2 = nullptr;                      // [nest][nd][slots][nlags]
    const double2 *ph2 = nullptr;                  // [nest][members][nd]
};

template <typename T>
__device__ __forceinline__ const T &caf_only(const T &t) { return t; }

// MODE 0 takes no further argument; MODE 1 and 2 one CancelArgs; MODE 3 one CleanArgs.
template <int LG, int MODE = 0, typename... CN>
__global__ __launch_bounds__(CAF_THREADS) void k_caf(const int8_t *__restrict__ packets, size_t packet_stride, size_t matrix_off, int nrows, int B, int frames,
                                                     int lgseg, int nlags, int ref_row, const float2 *__restrict__ tw_g, const float *__restrict__ win, float scale,
                                                     float2 *__restrict__ chi, const CN... cna)
{
    constexpr int ND = 1 << LG, LT = caf_log2_tile(LG), T = 1 << LT, CELLS = ND * T, PER = CELLS >= CAF_THREADS ? CELLS / CAF_THREADS : 1;
    __shared__ float2 A[spectra::sp_lds_points<LG>()];
    __shared__ uint32_t U[caf_u_words<LG>()];
    int *ACC = reinterpret_cast<int *>(A);
    uint32_t *SW = U, *RW = U + CAF_CHUNK;
    const int tid = threadIdx.x, tiles = caf_tiles(LG, nlags), row = blockIdx.x / tiles, tile = blockIdx.x - row * tiles, e = blockIdx.y;
    const int lag0 = tile << LT, tt = min(T, nlags - lag0), pre = ((lag0 + tt - 1) >> 1) + 1;
    const int words = B >> 2, J = (B >> 1) >> lgseg, nchunks = (words + CAF_CHUNK - 1) / CAF_CHUNK;

    if constexpr (MODE == 1) if (row == ref_row) return;            // (the whole workgroup: nothing of row r is solved for)
    [[maybe_unused]] long long energy = 0;
    for (int i = tid; i < 2 * CELLS; i += CAF_THREADS) ACC[i] = 0;
    for (int f = 0; f < frames; ++f) {
        const int8_t *m = packets + (size_t)(e * frames + f) * packet_stride + matrix_off;
        const uint32_t *srow = reinterpret_cast<const uint32_t *>(m + (size_t)row * B), *rrow = reinterpret_cast<const uint32_t *>(m + (size_t)ref_row * B);
        for (int c = 0; c < nchunks; ++c) {
            const int w0 = c * CAF_CHUNK, cw = min(CAF_CHUNK, words - w0);
            __syncthreads();                                         // (the chunk before is read; the first time: ACC is zero)
            for (int i = tid; i < cw; i += CAF_THREADS) SW[i] = srow[w0 + i];
            for (int i = tid; i < pre + cw; i += CAF_THREADS) {
                const int g = w0 - pre + i;
                RW[i] = g >= 0 ? rrow[g] : 0u;                       // X_r = 0 in front of the packet
            }
            __syncthreads();
            if constexpr (MODE == 1)
                if (tile == 0)
                    for (int i = tid; i < cw; i += CAF_THREADS) energy += __builtin_amdgcn_sdot4((int)SW[i], (int)SW[i], 0, false);
            if constexpr (T >= 2) {
                // an even lag and the odd one behind it per item: the same row words, swaps and reference words serve both
                for (int it = tid; it < (cw / CAF_PIECE) << (LT - 1); it += CAF_THREADS) {
                    const int l = (it & (T / 2 - 1)) * 2, p = it >> (LT - 1);
                    if (l >= tt) continue;
                    const uint32_t *r = RW + pre + p * CAF_PIECE - ((lag0 + l) >> 1) - 1, *s = SW + p * CAF_PIECE;      // (lag0 is even)
                    int re0 = 0, pp0 = 0, ee0 = 0, re1 = 0, pp1 = 0, ee1 = 0;
                    uint32_t x0 = r[0];
#pragma unroll
                    for (int i = 0; i < CAF_PIECE; ++i) {
                        const uint32_t x1 = r[i + 1], w = __builtin_amdgcn_alignbit(x1, x0, 16), sv = s[i], sx = __builtin_amdgcn_perm(sv, sv, 0x02030001u);
                        x0 = x1;
                        re0 = __builtin_amdgcn_sdot4((int)sv, (int)x1, re0, false);
                        pp0 = __builtin_amdgcn_sdot4((int)sx, (int)x1, pp0, false);
                        ee0 = __builtin_amdgcn_sdot4((int)sx, (int)(x1 & 0x00ff00ffu), ee0, false);
                        re1 = __builtin_amdgcn_sdot4((int)sv, (int)w, re1, false);
                        pp1 = __builtin_amdgcn_sdot4((int)sx, (int)w, pp1, false);
                        ee1 = __builtin_amdgcn_sdot4((int)sx, (int)(w & 0x00ff00ffu), ee1, false);
                    }
                    const int k = f * J + ((2 * (w0 + p * CAF_PIECE)) >> lgseg);
                    int *a = &ACC[((k << LT) + l) * 2];
                    atomicAdd(a, re0);
                    atomicAdd(a + 1, 2 * ee0 - pp0);
                    if (l + 1 < tt) {                                // (a tile's tail may end on the even lag)
                        atomicAdd(a + 2, re1);
                        atomicAdd(a + 3, 2 * ee1 - pp1);
                    }
                }
            } else {                                                 // nd = 4096: one lag a tile, of either parity
                for (int it = tid; it < (cw / CAF_PIECE) << LT; it += CAF_THREADS) {
                    const int l = it & (T - 1), p = it >> LT;
                    if (l >= tt) continue;
                    const int lag = lag0 + l, odd = lag & 1;
                    const uint32_t *r = RW + pre + p * CAF_PIECE - (lag >> 1) - odd, *s = SW + p * CAF_PIECE;
                    const uint32_t sh = (uint32_t)odd << 4;
                    int re = 0, pp = 0, ee = 0;
                    uint32_t x0 = r[0];
#pragma unroll
                    for (int i = 0; i < CAF_PIECE; ++i) {
                        const uint32_t x1 = r[i + 1], w = __builtin_amdgcn_alignbit(x1, x0, sh), sv = s[i], sx = __builtin_amdgcn_perm(sv, sv, 0x02030001u);
                        x0 = x1;
                        re = __builtin_amdgcn_sdot4((int)sv, (int)w, re, false);
                        pp = __builtin_amdgcn_sdot4((int)sx, (int)w, pp, false);
                        ee = __builtin_amdgcn_sdot4((int)sx, (int)(w & 0x00ff00ffu), ee, false);
                    }
                    const int k = f * J + ((2 * (w0 + p * CAF_PIECE)) >> lgseg);
                    atomicAdd(&ACC[((k << LT) + l) * 2], re);
                    atomicAdd(&ACC[((k << LT) + l) * 2 + 1], 2 * ee - pp);
                }
            }
        }
    }
    __syncthreads();

    if constexpr (MODE == 1) {
        const CancelArgs &cn = caf_only(cna...);
        // the sums of the lags < taps as they are, and E = sum |X_c|^2 over the line: integers, so any order gives the same bits
        int2 *Y = cn.Y + ((size_t)e * nrows + row) * ND * (size_t)nlags + lag0;
        for (int it = tid; it < CELLS; it += CAF_THREADS) {
            const int l = it & (T - 1), k = it >> LT;
            if (l < tt) Y[(size_t)k * nlags + l] = make_int2(ACC[2 * it], ACC[2 * it + 1]);
        }
        if (tile != 0) return;
        __syncthreads();                                             // (ACC is read: its place serves the tree, 8-byte aligned as U need not be)
        long long *red = reinterpret_cast<long long *>(A);
        red[tid] = energy;
        __syncthreads();
        for (int h = CAF_THREADS / 2; h >= 1; h >>= 1) {
            if (tid < h) red[tid] += red[tid + h];
            __syncthreads();
        }
        if (tid == 0) cn.E[(size_t)e * nrows + row] = red[0];
        return;
    }
    if constexpr (MODE >= 2) {
        // y' = y - sum_(m,p) h_(m,p) phi_p[k] G[k][m][tau]: fp64 from the integers, one rounding; its bits take y's place in ACC.
        // Row r and a singular line keep y: (float)(double)y is (float)y.
        // MODE 3: the same with the joint h, then y'' = y' - sum_i h_i phi_(g_i)[k] G2[k][slot_i][tau] over the line's target members
        // (none where the joint solve fell back: its h is then stage 1's, and these are MODE 2's bits).
        const auto &cn = caf_only(cna...);
        const int K = cn.taps, P = cn.dopp, Rg = cn.nlags;
        bool on = row != ref_row;
        size_t hstride = (size_t)(K * (2 * P + 1));
        [[maybe_unused]] int nm = 0;
        if constexpr (MODE == 3) {
            const int st = cn.status[e];
            on = on && (st & 1) == 0;
            nm = st == 0 ? cn.tab[e].nmem : 0;
            hstride = (size_t)cn.hstride;
        } else {
            on = on && cn.status[e] == 0;
        }
        const double2 *h = cn.h + ((size_t)e * nrows + row) * hstride;
        const int2 *G = cn.G + (size_t)e * ND * (size_t)K * Rg + lag0;
#pragma unroll 1
        for (int it = tid; it < CELLS; it += CAF_THREADS) {
            const int l = it & (T - 1), k = it >> LT;
            double re = (double)ACC[2 * it], im = (double)ACC[2 * it + 1];
            if (on && l < tt) {
                const int2 *g = G + (size_t)k * K * Rg + l;
                for (int p = -P; p <= P; ++p) {
                    double ar = 0.0, ai = 0.0;                        // sum_m h_(m,p) G[k][m][tau]
                    const double2 *hp = h + (p + P) * K;
                    for (int m = 0; m < K; ++m) {
                        const int2 gi = g[(size_t)m * Rg];
                        const double gr = (double)gi.x, gq = (double)gi.y;
                        ar = fma(hp[m].x, gr, ar); ar = fma(-hp[m].y, gq, ar);
                        ai = fma(hp[m].x, gq, ai); ai = fma(hp[m].y, gr, ai);
                    }
                    const double2 f = cn.ph[(p * k) & (ND - 1)];
                    re = fma(-f.x, ar, re); re = fma(f.y, ai, re);
                    im = fma(-f.x, ai, im); im = fma(-f.y, ar, im);
                }
                if constexpr (MODE == 3) {
                    const int2 *g2 = cn.G2 + ((size_t)e * ND + k) * (size_t)cn.slots * Rg + lag0 + l;
                    const int *slot = cn.tab[e].slot;
                    const double2 *ht = h + K * (2 * P + 1), *ph2 = cn.ph2 + (size_t)e * cn.members * ND + k;
                    for (int i = 0; i < nm; ++i) {
                        const int2 gi = g2[(size_t)slot[i] * Rg];
                        const double2 hi = ht[i], f = ph2[(size_t)i * ND];
                        const double gr = (double)gi.x, gq = (double)gi.y;
                        double ar = 0.0, ai = 0.0;
                        ar = fma(hi.x, gr, ar); ar = fma(-hi.y, gq, ar);
                        ai = fma(hi.x, gq, ai); ai = fma(hi.y, gr, ai);
                        re = fma(-f.x, ar, re); re = fma(f.y, ai, re);
                        im = fma(-f.x, ai, im); im = fma(-f.y, ar, im);
                    }
                }
            }
            ACC[2 * it] = __float_as_int((float)re);
            ACC[2 * it + 1] = __float_as_int((float)im);
        }
        __syncthreads();
    }

    int yr[PER], yi[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const int i = tid + j * CAF_THREADS;
        yr[j] = i < CELLS ? ACC[2 * i] : 0;
        yi[j] = i < CELLS ? ACC[2 * i + 1] : 0;
    }
    float2 *tw = reinterpret_cast<float2 *>(U);
    for (int t = tid; t < ND; t += CAF_THREADS) tw[t] = tw_g[t];
    __syncthreads();
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const int i = tid + j * CAF_THREADS, k = i >> LT, l = i & (T - 1);
        if (i < CELLS) {
            const float w = win[k];
            if constexpr (MODE >= 2) A[spectra::sp_pad<LG>(l * ND + k)] = make_float2(__int_as_float(yr[j]) * w, __int_as_float(yi[j]) * w);
            else A[spectra::sp_pad<LG>(l * ND + k)] = make_float2((float)yr[j] * w, (float)yi[j] * w);
        }
    }
    __syncthreads();
    spectra::sp_pass<LG, 0>(A, tw, tt, tid);                         // (a barrier ends it)

    float2 *out = chi + ((size_t)e * nrows + row) * ND * (size_t)nlags + lag0;
    for (int it = tid; it < CELLS; it += CAF_THREADS) {
        const int l = it & (T - 1), slot = it >> LT;
        if (l >= tt) continue;
        const float2 x = A[spectra::sp_pad<LG>(l * ND + slot)];
        out[(size_t)digit_reverse<LG>(slot) * nlags + l] = make_float2(x.x * scale, x.y * scale);
    }
}

// grid (ceil(nd R / 32), nest), 256 threads = 32 cells x 8 parts: part q adds rows q, q + 8, ... in fp64, the parts are added in part
// order.  (One thread per cell over all the rows left a line of 1025 rows to 63 workgroups of 1024 dependent loads each: 0.30 ms.)
constexpr int CAF_MAP_CELLS = 32, CAF_MAP_PARTS = CAF_THREADS / CAF_MAP_CELLS;
__global__ __launch_bounds__(CAF_THREADS) void k_caf_map(const float2 *__restrict__ chi, int nrows, int cells, int ref_row, float *__restrict__ map)
{
    __shared__ double part[CAF_MAP_PARTS][CAF_MAP_CELLS];
    const int l = threadIdx.x % CAF_MAP_CELLS, q = threadIdx.x / CAF_MAP_CELLS, i = blockIdx.x * CAF_MAP_CELLS + l, e = blockIdx.y;
    const float *c = reinterpret_cast<const float *>(chi + (size_t)e * nrows * cells);
    double s = 0.0;
    if (i < cells)
        for (int row = q; row < nrows; row += CAF_MAP_PARTS)
            if (row != ref_row) s += cafp::power(c + (size_t)row * cells * 2, 2, i);
    part[q][l] = s;
    __syncthreads();
    if (q != 0 || i >= cells) return;
    for (int k = 1; k < CAF_MAP_PARTS; ++k) s += part[k][l];
    map[(size_t)e * cells + i] = (float)s;
}

// grid (nrows + 1, nest).  peak [nest][nrows + 1][6]: the rows' |chi|^2, then map
__global__ __launch_bounds__(CAF_THREADS) void k_caf_peak(const float2 *__restrict__ chi, const float *__restrict__ map, int nrows, int nd, int R, int guard,
                                                          float *__restrict__ peak)
{
    __shared__ cafp::Part parts[CAF_THREADS];
    const int entry = blockIdx.x, e = blockIdx.y, tid = threadIdx.x, comps = entry < nrows ? 2 : 1;
    const size_t cells = (size_t)nd * R;
    const float *src = entry < nrows ? reinterpret_cast<const float *>(chi + ((size_t)e * nrows + entry) * cells) : map + (size_t)e * cells;
    parts[tid] = cafp::part(src, comps, nd, R, guard, tid, CAF_THREADS);
    __syncthreads();
    for (int h = CAF_THREADS / 2; h >= 1; h >>= 1) {
        if (tid < h) cafp::merge(parts[tid], parts[tid + h]);
        __syncthreads();
    }
    if (tid == 0) cafp::figures(src, comps, nd, R, guard, parts[0], peak + ((size_t)e * (nrows + 1) + entry) * 6);
}

} // namespace caf
} // namespace crsdr
