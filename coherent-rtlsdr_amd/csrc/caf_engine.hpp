// caf_engine.hpp -- the crsdr_caf object behind include/crsdr.h, and its per-op form crsdr_ambiguity.  Part of crsdr.hip's translation
// unit: included at its very end, behind spectra_engine.hpp, so that the existing kernels keep their places in the code object.
// (w) Range-Doppler maps (crsdr_caf): per line of `frames` packets every row's cross-ambiguity function against row ref_row, the array
//     map and the peak figures (caf.hpp, caf_peak.hpp).  Every buffer, the twiddle and window tables included, is made at create; a
//     submit is three launches on one stream whatever the batch size (rows, map, peaks), no lock, no allocation, no synchronisation.
//     With a detector set (crsdr_caf_set_cfar; caf_cfar.hpp, caf_cfar_kernels.hpp) two more: the tiles' candidates, and their merge into
//     the detection lists and the array map's snapshots.
//     With a canceller set (crsdr_caf_set_cancel; caf_cancel.hpp, caf_cancel_solve.hpp) five launches take the place of the rows' one:
//     the reference's sums, the rows' first lags, the normal equations' sums, factor and solves, and the rows with the subtraction.
//     With bearings set (crsdr_caf_set_bearing; caf_bearing.hpp, caf_bearing_solve.hpp) three more behind the detector's: the slots'
//     records, the scan's tiles, and the merge with the zoom search.
//     With beams set (crsdr_caf_set_beams; caf_beams.hpp, caf_beams_kernels.hpp) one more: every beam's map across the rows on the fp32
//     matrix pipe; with the detector on three more behind it: the detector's two on the beam maps, (line, beam) taking the place of
//     the line, and the fusion of the beams' lists into one per line.
//     With adaptation set (crsdr_caf_set_beam_adapt; caf_adapt.hpp, caf_adapt_kernels.hpp) two more ahead of the beam maps: the training
//     cells' covariance per line on the fp64 matrix pipe, and the line's solve, whose weights the beam kernel then reads.
//     With the tracker set (crsdr_caf_set_track; caf_track.hpp, caf_track_kernels.hpp) one more behind everything else: one workgroup
//     that walks the lines of the submit and carries the tracks from submit to submit.
//     With integration set (crsdr_caf_set_integrate; caf_integrate.hpp, caf_integrate_solve.hpp) one more behind the array map, whose
//     place the integrated map takes in front of the detector, and one more behind the beam maps, likewise.
//     With cleaning set (crsdr_caf_set_clean; caf_clean.hpp, caf_clean_solve.hpp) nine more behind the detector's: the picks, the
//     reference's and the rows' sums at the picks' lags, the joint sums, factor and solves, the rows with the joint subtraction, their
//     map, and the detector's two on them.
//
// Shape of the host code (doa_engine.hpp's).  A feature is a sub-struct of crsdr_caf: its parameters and its DevBufs.  Every launch
// goes through caf_run, which checks and counts it.  A submit is caf_launch's flat list of stages (maps, integration, detector,
// bearings, beams, their integration, the beams' lists, tracker), each of which returns at once with its feature off; what it left (CafLast) is written once at its end.
// A setter asks caf_rules, empties its feature behind caf_quiesce (caf_clear), builds the new one in a local, between submits, and
// moves it in when every allocation has succeeded.  A fetch reads its state from CafLast and copies through DevFetch.  The per-op
// calls share the *_enqueue functions with the stages (the same kernels on the same arguments, so the same bits) and caf_shape_ok.
#pragma once

#include "caf.hpp"
#include "caf_adapt_kernels.hpp"
#include "caf_beams_kernels.hpp"
#include "caf_bearing.hpp"
#include "caf_cancel.hpp"
#include "caf_cfar_kernels.hpp"
#include "caf_clean.hpp"
#include "caf_integrate.hpp"
#include "caf_track_kernels.hpp"

// `launch` with LG = log2 nd, 3 .. 12
#define CAF_DISPATCH(lg, launch)                                                    \
    switch (lg) {                                                                   \
    case 3: { constexpr int LG = 3; launch; } break;                                \
    case 4: { constexpr int LG = 4; launch; } break;                                \
    case 5: { constexpr int LG = 5; launch; } break;                                \
    case 6: { constexpr int LG = 6; launch; } break;                                \
    case 7: { constexpr int LG = 7; launch; } break;                                \
    case 8: { constexpr int LG = 8; launch; } break;                                \
    case 9: { constexpr int LG = 9; launch; } break;                                \
    case 10: { constexpr int LG = 10; launch; } break;                              \
    case 11: { constexpr int LG = 11; launch; } break;                              \
    default: { constexpr int LG = 12; launch; } break;                              \
    }

constexpr int kTrackMaxLines = 4096;
constexpr long long kCafMaxCells = 1ll << 24;           // (max_batch / frames) * nrows * nd * nlags

// the canceller's device memory for `lines` lines: the engine's own buffers, or parts of one per-op slot
struct CancelBufs {
    int taps = 0, dopp = 0;
    int2 *G = nullptr, *Y = nullptr;
    double2 *ph = nullptr, *S = nullptr, *C = nullptr, *W = nullptr, *h = nullptr;
    long long *E = nullptr;
    int *status = nullptr;
    float *coef = nullptr, *cinfo = nullptr;
};

// what the last submit left: where, how much, and which features ran (kCafRan*).  A setter clears its feature's bit: "nothing submitted
// since"; without kCafRanBase nothing is left at all
constexpr unsigned kCafRanBase = 1u, kCafRanCancel = 2u, kCafRanCfar = 4u, kCafRanBearing = 8u, kCafRanBeams = 16u, kCafRanTrack = 32u, kCafRanIntegrate = 64u, kCafRanAdapt = 128u, kCafRanClean = 256u;
struct CafLast {
    hipStream_t stream = nullptr;
    int nest = 0, launches = 0;
    unsigned ran = 0;
};

struct crsdr_caf {
    DoaStream own;
    int nrows = 0, B = 0, device = 0, max_batch = 1, frames = 1, seg = 0, nlags = 0, ref_row = 0, window = 0, guard = 0, nd = 0;
    DevBuf<float2> tw, chi;
    DevBuf<float> win, map, peak;
    // crsdr_caf_set_cfar: on (false = off), the tiles' candidates [lines][nrows + 1][tiles][keep] and counts, and the results
    struct Cfar {
        bool on = false;
        cfar::Params prm{};
        int keep = 0;
        DevBuf<cfar::Cand> slots;
        DevBuf<int32_t> tcount, count;
        DevBuf<float> det, snap;
    } cf;
    // crsdr_caf_set_cancel: on (false = off) and what CancelBufs names
    struct Cancel {
        bool on = false;
        int taps = 0, dopp = 0;
        DevBuf<int2> G, Y;
        DevBuf<double2> ph, S, C, W, h;
        DevBuf<long long> E;
        DevBuf<int> status;
        DevBuf<float> coef, cinfo;
        CancelBufs bufs() const { return CancelBufs{taps, dopp, G, Y, ph, S, C, W, h, E, status, coef, cinfo}; }
    } cn;
    // crsdr_caf_set_bearing: on (false = off), the slots' records [lines][K][brg::REC], the tiles' maxima and the results
    struct Bearing {
        bool on = false;
        brg::Params prm{};
        DevBuf<double> rec;
        DevBuf<bearing::Best> tbest;
        DevBuf<float> dir, spec;
    } bg;
    // crsdr_caf_set_beams: on (false = off), det: the detector was on when they were set; the weights [nb][m][2], the maps and, with
    // det, the detector's scratch for (line, beam) maps and the lists
    struct Beams {
        bool on = false, det = false;
        int nb = 0;
        DevBuf<float> w, bmap, bdet, fused;
        DevBuf<int32_t> bcount, nfused, tcount;
        DevBuf<cfar::Cand> slots;
    } bb;
    // crsdr_caf_set_beam_adapt: on (false = off), the tiles' sums [lines][tiles][m (m + 1) / 2], the lines' weights, figures and status
    struct Adapt {
        bool on = false;
        ad::Params prm{};
        DevBuf<double2> part;
        DevBuf<float> aw, ainfo;
        DevBuf<int32_t> astat;
    } ba;
    // crsdr_caf_set_track: on (false = off), the state that a submit hands to the next, and the results
    struct Track {
        bool on = false;
        trk::Params prm{};
        DevBuf<unsigned char> state;
        DevBuf<float> trk;
        DevBuf<int32_t> ntrk;
    } tk;
    // crsdr_caf_set_integrate: on (false = off), which maps, the state that a submit hands to the next -- the array map's block, then
    // the beam maps', each a header and its doubles; a block whose flag is off is not there -- and the integrated maps
    struct Integrate {
        bool on = false;
        int what = 0;
        integ::Params prm{};
        DevBuf<unsigned char> state;
        DevBuf<float> imap, ibmap;
        bool array() const { return on && (what & integ::ARRAY); }
        bool beams() const { return on && (what & integ::BEAMS); }
    } ig;
    // crsdr_caf_set_clean: on (false = off), the sizes its buffers have (n2max target members, nmax members, slots member lags a
    // line), the lines' member tables, the sums, the joint solve's scratch and coefficients, and the results
    struct Clean {
        bool on = false;
        cl::Params prm{};
        int n2max = 0, nmax = 0, slots = 0;
        DevBuf<cl::Table> tab;
        DevBuf<int2> G2, Y2;
        DevBuf<double2> ph2, A2, C2, Wj, hj;
        DevBuf<int> jstat;
        DevBuf<float> tgt, tcoef, tinfo, rmap, rdet, rsnap;
        DevBuf<int32_t> ntgt, rcount;
        DevBuf<float2> rchi;
    } cl_;
    CafLast last;
    size_t lines() const { return (size_t)(max_batch / frames); }      // the most a submit leaves: what every setter sizes its buffers by
};

// a submit's stream, lines and launches so far; a per-op call's stream, and a count that nobody reads
struct CafRun {
    hipStream_t S;
    int nest = 0, launches = 0;
};

// every launch: the kernel, its error, the count
template <typename Kernel, typename... Args>
static int caf_run(CafRun &r, Kernel kern, dim3 grid, dim3 block, size_t lds, const Args &...args)
{
    hipLaunchKernelGGL(kern, grid, block, lds, r.S, args...);
    HIP_TRY(hipGetLastError());
    ++r.launches;
    return CRSDR_OK;
}

// every limit of section (w), for crsdr_caf_create and crsdr_ambiguity (max_batch = frames = 1)
static int caf_args_ok(const char *who, int nrows, int blocksize, int max_batch, int frames, int seg, int nlags, int ref_row, int window, int guard)
{
    const int lgs = ilog2_exact(seg);
    if (lgs < caf::CAF_MIN_SEG_LOG2 || lgs > caf::CAF_MAX_SEG_LOG2) return fail(CRSDR_EINVAL, "%s: seg = %d (a power of two in [16, 4096])", who, seg);
    if (nrows < 2) return fail(CRSDR_EINVAL, "%s: nrows = %d (at least 2: the reference row and another)", who, nrows);
    if (blocksize < 2 * seg || blocksize % (2 * seg) || blocksize > (1 << kMaxLog2Plan))
        return fail(CRSDR_EINVAL, "%s: blocksize = %d (a multiple of 2 seg = %d, up to %d)", who, blocksize, 2 * seg, 1 << kMaxLog2Plan);
    if (ref_row < 0 || ref_row >= nrows) return fail(CRSDR_EINVAL, "%s: ref_row = %d (0..%d)", who, ref_row, nrows - 1);
    if (nlags < 1 || nlags > seg || nlags > caf::CAF_MAX_LAGS) return fail(CRSDR_EINVAL, "%s: nlags = %d (1..min(seg, %d))", who, nlags, caf::CAF_MAX_LAGS);
    if (max_batch < 1 || max_batch > kMaxBatch) return fail(CRSDR_EINVAL, "%s: max_batch = %d (1..%d)", who, max_batch, kMaxBatch);
    if (frames < 1 || frames > max_batch) return fail(CRSDR_EINVAL, "%s: frames = %d (1..max_batch = %d)", who, frames, max_batch);
    const long long nd = (long long)frames * (blocksize / (2 * seg));
    const int lgd = nd <= (1 << caf::CAF_MAX_LOG2) ? ilog2_exact((int)nd) : -1;
    if (lgd < caf::CAF_MIN_LOG2 || lgd > caf::CAF_MAX_LOG2)
        return fail(CRSDR_EINVAL, "%s: nd = frames * blocksize / (2 seg) = %lld (a power of two in [8, 4096])", who, nd);
    if ((long long)(max_batch / frames) * nrows * nd * nlags > kCafMaxCells)
        return fail(CRSDR_EINVAL, "%s: (max_batch / frames) * nrows * nd * nlags = %lld (at most 2^24)", who, (long long)(max_batch / frames) * nrows * nd * nlags);
    if (window != CRSDR_WINDOW_RECT && window != CRSDR_WINDOW_HANN) return fail(CRSDR_EINVAL, "%s: window = %d", who, window);
    if (guard < 0 || guard > nd / 2) return fail(CRSDR_EINVAL, "%s: guard = %d (0..nd / 2 = %lld)", who, guard, nd / 2);
    return CRSDR_OK;
}

// What the per-op calls ask of a line's shape, in the order they have always asked it: nd (a power of two; any size with pow2 off, for
// crsdr_beam_maps), R, nrows, ref_row, guard.  A call without rows or without a guard passes nrows 2, ref_row 0, guard 0: they hold.
static int caf_shape_ok(const char *who, int nd, int R, int guard, int ref_row, int nrows, bool pow2 = true)
{
    const bool in_range = nd >= 1 && nd <= (1 << caf::CAF_MAX_LOG2);
    if (pow2 && (!in_range || ilog2_exact(nd) < caf::CAF_MIN_LOG2)) return fail(CRSDR_EINVAL, "%s: nd = %d (a power of two in [8, 4096])", who, nd);
    if (!in_range) return fail(CRSDR_EINVAL, "%s: nd = %d (1..4096)", who, nd);
    if (R < 1 || R > caf::CAF_MAX_LAGS) return fail(CRSDR_EINVAL, "%s: R = %d (1..%d)", who, R, caf::CAF_MAX_LAGS);
    if (nrows < 2 || (long long)nrows * nd * R > kCafMaxCells) return fail(CRSDR_EINVAL, "%s: nrows = %d (at least 2, nrows * nd * R at most 2^24)", who, nrows);
    if (ref_row < 0 || ref_row >= nrows) return fail(CRSDR_EINVAL, "%s: ref_row = %d (0..%d)", who, ref_row, nrows - 1);
    if (guard < 0 || guard > nd / 2) return fail(CRSDR_EINVAL, "%s: guard = %d (0..nd / 2 = %d)", who, guard, nd / 2);
    return CRSDR_OK;
}

// every limit of the canceller of section (w), for crsdr_caf_set_cancel and crsdr_ambiguity_cancel
static int cancel_args_ok(const char *who, int nd, int nlags, long long lines, const crsdr_caf_cancel_desc *d)
{
    switch (cc::bad_limit(nd, nlags, lines, d->taps, d->dopp)) {
    case 0: return CRSDR_OK;
    case 1: return fail(CRSDR_EINVAL, "%s: dopp = %d (0..%d)", who, d->dopp, cc::MAX_DOPP);
    case 2: return fail(CRSDR_EINVAL, "%s: taps = %d (1..min(nlags = %d, %d))", who, d->taps, nlags, cc::MAX_TAPS);
    case 3: return fail(CRSDR_EINVAL, "%s: taps (2 dopp + 1) = %d (at most %d)", who, cc::basis(d->taps, d->dopp), cc::MAX_BASIS);
    case 4: return fail(CRSDR_EINVAL, "%s: 2 dopp + 1 = %d exceeds nd = %d", who, 2 * d->dopp + 1, nd);
    default: return fail(CRSDR_EINVAL, "%s: (max_batch / frames) * nd * taps * nlags = %lld (at most 2^24)", who, lines * nd * d->taps * nlags);
    }
}

// the phase table of the canceller, exp(2 pi i j / nd): at set_cancel, and per call for crsdr_ambiguity_cancel
static int cancel_table(CafRun &r, int nd, double2 *ph)
{
    return caf_run(r, cancel::k_cancel_phase, dim3((unsigned)((nd + cancel::THREADS - 1) / cancel::THREADS)), dim3(cancel::THREADS), 0, nd, ph);
}

// the rows with the canceller: five launches in the place of k_caf's one
static int cancel_enqueue(CafRun &r, const int8_t *packets, size_t packet_stride, size_t matrix_offset, int nest, int nrows, int B, int frames, int lg, int lgseg,
                          int nlags, int ref_row, const float2 *tw, const float *win, float scale, float2 *chi, const CancelBufs &c)
{
    const int nd = 1 << lg, K = c.taps, P = c.dopp, n = cc::basis(K, P), entries = (4 * P + 1) * K * K + nrows * n;
    int rc = caf_run(r, cancel::k_cancel_g, dim3((unsigned)((nd * (nlags + K - 1) + cancel::THREADS - 1) / cancel::THREADS), (unsigned)nest), dim3(cancel::THREADS), 0,
                     packets, packet_stride, matrix_offset, B, frames, lgseg, nd, nlags, K, ref_row, c.G);
    if (rc) return rc;
    caf::CancelArgs a1, a2;
    a1.Y = c.Y; a1.E = c.E;
    a2.taps = K; a2.dopp = P; a2.nlags = nlags; a2.G = c.G; a2.h = c.h; a2.ph = c.ph; a2.status = c.status;
    CAF_DISPATCH(lg, rc = caf_run(r, (caf::k_caf<LG, 1, caf::CancelArgs>), dim3((unsigned)(nrows * caf::caf_tiles(lg, K)), (unsigned)nest), dim3(caf::CAF_THREADS), 0, packets,
                                  packet_stride, matrix_offset, nrows, B, frames, lgseg, K, ref_row, tw, win, scale, chi, a1));
    if (rc || (rc = caf_run(r, cancel::k_cancel_sums, dim3((unsigned)((entries + cancel::SUM_ENTRIES - 1) / cancel::SUM_ENTRIES), (unsigned)nest), dim3(cancel::THREADS), 0,
                            (const int2 *)c.G, (const int2 *)c.Y, (const double2 *)c.ph, nrows, nd, nlags, K, P, ref_row, c.S, c.C)) ||
        (rc = caf_run(r, cancel::k_cancel_solve, dim3((unsigned)nest, (unsigned)((nrows + cancel::SOLVE_ROWS - 1) / cancel::SOLVE_ROWS)), dim3(cancel::THREADS), 0,
                      (const double2 *)c.S, (const double2 *)c.C, (const long long *)c.E, nrows, K, P, ref_row, c.W, c.h, c.status, c.coef, c.cinfo)))
        return rc;
    CAF_DISPATCH(lg, rc = caf_run(r, (caf::k_caf<LG, 2, caf::CancelArgs>), dim3((unsigned)(nrows * caf::caf_tiles(lg, nlags)), (unsigned)nest), dim3(caf::CAF_THREADS), 0,
                                  packets, packet_stride, matrix_offset, nrows, B, frames, lgseg, nlags, ref_row, tw, win, scale, chi, a2));
    return rc;
}

// the three launches, for the object and for crsdr_ambiguity: the same kernels on the same arguments, so the same bits.  cn: the
// canceller's buffers, or NULL with it off.
static int caf_enqueue(CafRun &r, const int8_t *packets, size_t packet_stride, size_t matrix_offset, int nblocks, int nrows, int B, int frames, int seg, int nlags,
                       int ref_row, int window, int guard, const float2 *tw, const float *win, float2 *chi, float *map, float *peak, const CancelBufs *cn = nullptr)
{
    const int nest = nblocks / frames, nd = frames * (B / (2 * seg)), lg = ilog2_exact(nd), lgseg = ilog2_exact(seg), cells = nd * nlags;
    // sum w: nd (rect), nd / 2 (periodic Hann)
    const float scale = (float)(1.0 / (127.0 * 127.0 * (double)seg * (window == CRSDR_WINDOW_HANN ? 0.5 * (double)nd : (double)nd)));
    const dim3 grow((unsigned)(nrows * caf::caf_tiles(lg, nlags)), (unsigned)nest);
    int rc = CRSDR_OK;
    if (cn) {
        rc = cancel_enqueue(r, packets, packet_stride, matrix_offset, nest, nrows, B, frames, lg, lgseg, nlags, ref_row, tw, win, scale, chi, *cn);
    } else {
        CAF_DISPATCH(lg, rc = caf_run(r, (caf::k_caf<LG, 0>), grow, dim3(caf::CAF_THREADS), 0, packets, packet_stride, matrix_offset, nrows, B, frames, lgseg, nlags, ref_row,
                                      tw, win, scale, chi));
    }
    if (rc || (rc = caf_run(r, caf::k_caf_map, dim3((unsigned)((cells + caf::CAF_MAP_CELLS - 1) / caf::CAF_MAP_CELLS), (unsigned)nest), dim3(caf::CAF_THREADS), 0,
                            (const float2 *)chi, nrows, cells, ref_row, map)))
        return rc;
    return caf_run(r, caf::k_caf_peak, dim3((unsigned)(nrows + 1), (unsigned)nest), dim3(caf::CAF_THREADS), 0, (const float2 *)chi, (const float *)map, nrows, nd, nlags, guard,
                   peak);
}

constexpr int kCfarAlphaMaxTrain = 65536;          // crsdr_cfar_alpha_est: the sums run over ntrain terms

// every limit of the detector of section (w), for crsdr_caf_set_cfar and crsdr_cfar
static int cfar_args_ok(const char *who, int nd, const crsdr_cfar_desc *d, cfar::Params *prm)
{
    *prm = cfar::Params{d->gd, d->gr, d->td, d->tr, d->alpha, d->min_train, d->max_det};
    switch (cfar::bad_limit(nd, *prm)) {
    case 0: return CRSDR_OK;
    case 1: return fail(CRSDR_EINVAL, "%s: gd, gr, td, tr = %d, %d, %d, %d (none negative)", who, d->gd, d->gr, d->td, d->tr);
    case 2: return fail(CRSDR_EINVAL, "%s: gd + td = %d + %d (at most %d)", who, d->gd, d->td, cfar::MAX_HD);
    case 3: return fail(CRSDR_EINVAL, "%s: gr + tr = %d + %d (at most %d)", who, d->gr, d->tr, cfar::MAX_HR);
    case 4: return fail(CRSDR_EINVAL, "%s: td + tr = 0 (no training cells)", who);
    case 5: return fail(CRSDR_EINVAL, "%s: 2 (gd + td) + 1 = %d exceeds nd = %d", who, 2 * (d->gd + d->td) + 1, nd);
    case 6: return fail(CRSDR_EINVAL, "%s: alpha = %g (finite and greater than 0)", who, (double)d->alpha);
    case 7: return fail(CRSDR_EINVAL, "%s: min_train = %d (at least 1)", who, d->min_train);
    default: return fail(CRSDR_EINVAL, "%s: max_det = %d (1..%d)", who, d->max_det, cfar::MAX_DET);
    }
}

// the estimator's limits, for crsdr_caf_set_cfar_estimator and crsdr_cfar_est; prm: the detector's, whose window gives Nfull.  NULL or
// cell averaging leaves prm as cfar_args_ok made it
static int cfar_est_ok(const char *who, const crsdr_cfar_est_desc *e, cfar::Params *prm)
{
    if (!e) return CRSDR_OK;
    cfar::Params t = *prm;
    t.est = e->estimator;
    t.axis = t.est == cfar::EST_GO || t.est == cfar::EST_SO ? e->axis : 0;
    t.rank = t.est == cfar::EST_OS ? e->rank : 0;
    switch (cfar::bad_estimator(t)) {
    case 0: *prm = t; return CRSDR_OK;
    case 1: return fail(CRSDR_EINVAL, "%s: estimator = %d (0 cell averaging, 1 greatest-of, 2 smallest-of, 3 ordered statistic)", who, e->estimator);
    case 2: return fail(CRSDR_EINVAL, "%s: axis = %d (0 lag, 1 Doppler)", who, e->axis);
    default: return fail(CRSDR_EINVAL, "%s: rank = %d (1..Nfull = %d)", who, e->rank, cfar::full_count(t));
    }
}

// the detector's two launches, for the object and for crsdr_cfar: the same kernels on the same arguments, so the same bits.  The
// estimator picks the tiles' kernel; the merge is the same behind each
static int cfar_enqueue(CafRun &r, const float2 *chi, const float *map, int nest, int nrows, int entries, int nd, int R, int guard, const cfar::Params &prm, int keep,
                        cfar::Cand *slots, int32_t *tcount, float *det, int32_t *count, float *snap)
{
    const int tiles = cfar::tiles_of(nd, R);
    const auto kern = prm.est == cfar::EST_OS ? cfar::k_caf_cfar_os : prm.est == cfar::EST_GO ? cfar::k_caf_cfar<cfar::EST_GO> :
                      prm.est == cfar::EST_SO ? cfar::k_caf_cfar<cfar::EST_SO> : cfar::k_caf_cfar<cfar::EST_CA>;
    const int rc = caf_run(r, kern, dim3((unsigned)(entries * tiles), (unsigned)nest), dim3(cfar::THREADS), 0, chi, map, nrows, entries, nd, R, guard, prm, keep,
                           slots, tcount);
    if (rc) return rc;
    return caf_run(r, cfar::k_caf_cfar_merge, dim3((unsigned)entries, (unsigned)nest), dim3(cfar::THREADS), 0, chi, map, nrows, entries, nd, R, guard, prm, keep,
                   (const cfar::Cand *)slots, (const int32_t *)tcount, det, count, snap);
}

// every limit of the bearings of section (w), for crsdr_caf_set_bearing and crsdr_bearing
static int bearing_args_ok(const char *who, int nrows, long long lines, int K, const crsdr_caf_bearing_desc *d, brg::Params *prm)
{
    *prm = brg::Params{d->mx, d->my, d->ncx, d->ncy, d->d, d->mode, d->loading, d->levels, d->flags};
    switch (brg::bad_limit(nrows, lines, K, *prm)) {
    case 0: return CRSDR_OK;
    case 1: return fail(CRSDR_EINVAL, "%s: mx, my = %d, %d (at least 1)", who, d->mx, d->my);
    case 2: return fail(CRSDR_EINVAL, "%s: mx my = %lld (nrows - 1 = %d, in 2..%d)", who, (long long)d->mx * d->my, nrows - 1, brg::MAX_M);
    case 3: return fail(CRSDR_EINVAL, "%s: ncx, ncy = %d, %d (%d..%d)", who, d->ncx, d->ncy, brg::MIN_NC, brg::MAX_NC);
    case 4: return fail(CRSDR_EINVAL, "%s: d = %g (finite and greater than 0)", who, (double)d->d);
    case 5: return fail(CRSDR_EINVAL, "%s: mode = %d", who, d->mode);
    case 6: return fail(CRSDR_EINVAL, "%s: loading = %g (1e-6..1)", who, (double)d->loading);
    case 7: return fail(CRSDR_EINVAL, "%s: levels = %d (0..%d)", who, d->levels, brg::MAX_LEVELS);
    case 8: return fail(CRSDR_EINVAL, "%s: flags = 0x%x", who, d->flags);
    default: return fail(CRSDR_EINVAL, "%s: (max_batch / frames) * max_det * ncx * ncy = %lld (at most 2^24 with the spectrum kept)", who, lines * K * d->ncx * d->ncy);
    }
}

// the bearings' three launches, for the object and for crsdr_bearing: the same kernels on the same arguments, so the same bits.
// det, count: the array map's entry of the first line.
static int bearing_enqueue(CafRun &r, const float2 *chi, const float *det, size_t det_stride, const int32_t *count, size_t count_stride, int nest, int nrows, int nd,
                           int R, int ref_row, int guard, const cfar::Params &cp, const brg::Params &bp, double *rec, bearing::Best *tbest, float *dir, float *spec)
{
    const int K = cp.max_det, tiles = bearing::tiles_of(bp.ncx, bp.ncy);
    int rc = caf_run(r, bearing::k_bearing_slot, dim3((unsigned)K, (unsigned)nest), dim3(bearing::THREADS), bearing::slot_lds_bytes(bp.mx * bp.my, cp.gr + cp.tr), chi, det,
                     det_stride, count, count_stride, nrows, nd, R, ref_row, guard, cp, bp, K, rec);
    if (rc || (rc = caf_run(r, bearing::k_bearing_scan, dim3((unsigned)tiles, (unsigned)K, (unsigned)nest), dim3(bearing::THREADS), 0, (const double *)rec, bp, K, spec, tbest))) return rc;
    return caf_run(r, bearing::k_bearing_finish, dim3((unsigned)K, (unsigned)nest), dim3(bearing::FIN_THREADS), 0, (const double *)rec, (const bearing::Best *)tbest, tiles, bp,
                   K, dir);
}

// every limit of the beams of section (w), for crsdr_caf_set_beams and crsdr_beam_maps.  weights: on the host
static int beams_args_ok(const char *who, int nrows, long long lines, int nd, int R, int nbeams, const float *weights, unsigned flags)
{
    switch (bm::bad_limit(nrows, lines, nd, R, nbeams, weights, flags)) {
    case 0: return CRSDR_OK;
    case 1: return fail(CRSDR_EINVAL, "%s: m = nrows - 1 = %d (1..%d)", who, nrows - 1, bm::MAX_M);
    case 2: return fail(CRSDR_EINVAL, "%s: nbeams = %d (1..%d)", who, nbeams, bm::MAX_BEAMS);
    case 3: return fail(CRSDR_EINVAL, "%s: NULL weights", who);
    case 4: return fail(CRSDR_EINVAL, "%s: a weight is not finite", who);
    case 5: return fail(CRSDR_EINVAL, "%s: flags = 0x%x (none yet)", who, flags);
    default: return fail(CRSDR_EINVAL, "%s: (max_batch / frames) * nbeams * nd * R = %lld (at most 2^24)", who, lines * nbeams * nd * R);
    }
}

// every limit of the adaptive beams of section (w), for crsdr_caf_set_beam_adapt and crsdr_beam_adapt
static int adapt_args_ok(const char *who, int nrows, int nd, int R, const crsdr_caf_beam_adapt_desc *d, ad::Params *prm)
{
    *prm = ad::Params{d->d_lo, d->d_n, d->r_lo, d->r_n, d->loading, d->flags};
    switch (ad::bad_limit(nrows, nd, R, *prm)) {
    case 0: return CRSDR_OK;
    case 1: return fail(CRSDR_EINVAL, "%s: m = nrows - 1 = %d (1..%d)", who, nrows - 1, ad::MAX_M);
    case 2: return fail(CRSDR_EINVAL, "%s: d_lo = %d (0..nd - 1 = %d)", who, d->d_lo, nd - 1);
    case 3: return fail(CRSDR_EINVAL, "%s: d_n = %d (1..nd = %d)", who, d->d_n, nd);
    case 4: return fail(CRSDR_EINVAL, "%s: r_lo = %d (not negative)", who, d->r_lo);
    case 5: return fail(CRSDR_EINVAL, "%s: r_n = %d (at least 1)", who, d->r_n);
    case 6: return fail(CRSDR_EINVAL, "%s: r_lo + r_n = %d + %d (at most R = %d)", who, d->r_lo, d->r_n, R);
    case 7: return fail(CRSDR_EINVAL, "%s: loading = %g (1e-6..1)", who, (double)d->loading);
    default: return fail(CRSDR_EINVAL, "%s: flags = 0x%x (none yet)", who, d->flags);
    }
}

// the adaptive weights' two launches, for the object and for crsdr_beam_adapt: the same kernels on the same arguments, so the same bits
static int beam_adapt_enqueue(CafRun &r, const float2 *chi, const float *w, int nest, int nrows, int nd, int R, int ref_row, int nb, const ad::Params &prm, double2 *part,
                              float *aw, float *ainfo, int32_t *astat)
{
    const int m = nrows - 1;
    const int rc = caf_run(r, caf_adapt::k_caf_beam_cov, dim3((unsigned)ad::tiles_of(ad::cells_of(prm)), (unsigned)nest), dim3(caf_adapt::THREADS), 0, chi, nrows, nd, R, ref_row,
                           prm, part);
    if (rc) return rc;
    return caf_run(r, caf_adapt::k_caf_beam_adapt, dim3((unsigned)nest), dim3(caf_adapt::THREADS), caf_adapt::adapt_lds_bytes(m), (const double2 *)part, w, m, nb, prm, aw, ainfo,
                   astat);
}

// the beam maps' one launch, for the object and for crsdr_beam_maps: the same kernel on the same arguments, so the same bits.
// wstride: 0 for one set of weights, nb m 2 for a set per line (the adaptive ones)
static int beam_maps_enqueue(CafRun &r, const float2 *chi, const float *w, size_t wstride, int nest, int nrows, int cells, int ref_row, int nb, float *bmap)
{
    const dim3 grid((unsigned)((cells + caf_beams::WG_CELLS - 1) / caf_beams::WG_CELLS), (unsigned)nest);
    return caf_run(r, caf_beams::groups_of(nb) == 1 ? caf_beams::k_caf_beams<1> : caf_beams::k_caf_beams<2>, grid, dim3(caf_beams::THREADS),
                   caf_beams::table_bytes(nrows - 1, nb), chi, w, wstride, nrows, cells, ref_row, nb, bmap);
}

// the fusion's one launch, for the object and for crsdr_beam_fuse
static int beam_fuse_enqueue(CafRun &r, const float *bdet, const int32_t *bcount, int nest, int nb, int K, int nd, int R, float *fused, int32_t *nfused)
{
    return caf_run(r, caf_beams::k_caf_beam_fuse, dim3((unsigned)nest), dim3(caf_beams::THREADS), 0, bdet, bcount, nb, K, nd, R, fused, nfused);
}

// every limit of the tracker of section (w), for crsdr_caf_set_track, crsdr_track and crsdr_track_state_bytes
static int track_args_ok(const char *who, const crsdr_caf_track_desc *d, trk::Params *prm)
{
    *prm = trk::Params{d->max_tracks, d->source, d->sigma_r, d->sigma_f, d->gate, d->p0_g, d->q_r, d->q_f, d->q_g, d->coupling, d->m, d->n, d->tent_miss, d->conf_miss};
    switch (trk::bad_limit(*prm)) {
    case 0: return CRSDR_OK;
    case 1: return fail(CRSDR_EINVAL, "%s: max_tracks = %d (1..%d)", who, d->max_tracks, trk::MAX_TRACKS);
    case 2: return fail(CRSDR_EINVAL, "%s: source = %d", who, d->source);
    case 3: return fail(CRSDR_EINVAL, "%s: sigma_r, sigma_f = %g, %g (finite and greater than 0)", who, d->sigma_r, d->sigma_f);
    case 4: return fail(CRSDR_EINVAL, "%s: gate = %g (finite and greater than 0)", who, d->gate);
    case 5: return fail(CRSDR_EINVAL, "%s: p0_g = %g (finite and greater than 0)", who, d->p0_g);
    case 6: return fail(CRSDR_EINVAL, "%s: q_r, q_f, q_g = %g, %g, %g (finite, none negative)", who, d->q_r, d->q_f, d->q_g);
    case 7: return fail(CRSDR_EINVAL, "%s: coupling = %g (finite)", who, d->coupling);
    case 8: return fail(CRSDR_EINVAL, "%s: m, n = %d, %d (1 <= m <= n <= %d)", who, d->m, d->n, trk::MAX_HIST);
    default: return fail(CRSDR_EINVAL, "%s: tent_miss, conf_miss = %d, %d (at least 1)", who, d->tent_miss, d->conf_miss);
    }
}

// the tracker's one launch, for the object and for crsdr_track: the same kernel on the same arguments, so the same bits
static int track_enqueue(CafRun &r, const float *det, size_t det_stride, const int32_t *count, size_t count_stride, const float *aux, int aux_mode, int nlines, int K,
                         int nd, int R, const trk::Params &prm, unsigned char *state, float *out, int32_t *nout)
{
    return caf_run(r, caf_track::k_caf_track, dim3(1), dim3(caf_track::THREADS), caf_track::lds_bytes(prm.max_tracks, K), det, det_stride, count, count_stride, aux, aux_mode,
                   nlines, K, nd, R, prm, state, out, nout);
}

// every limit of the integration of section (w), for crsdr_caf_set_integrate and crsdr_map_integrate (check_what false: `what` is not read)
static int integrate_args_ok(const char *who, int nd, const crsdr_caf_integrate_desc *d, bool check_what, integ::Params *prm)
{
    *prm = integ::Params{d->forget, d->coupling};
    switch (integ::bad_limit(nd, *prm)) {
    case 0: break;
    case 1: return fail(CRSDR_EINVAL, "%s: forget = %g (finite, in (0, 1])", who, d->forget);
    case 2: return fail(CRSDR_EINVAL, "%s: coupling = %g (finite)", who, d->coupling);
    default: return fail(CRSDR_EINVAL, "%s: |coupling| * (nd / 2) = %g (at most %g cells a line)", who, fabs(d->coupling) * (double)(nd / 2), integ::MAX_WALK);
    }
    if (check_what && (d->what < 1 || d->what > (integ::ARRAY | integ::BEAMS)))
        return fail(CRSDR_EINVAL, "%s: what = %d (CRSDR_INTEGRATE_ARRAY, CRSDR_INTEGRATE_BEAMS or both)", who, d->what);
    return CRSDR_OK;
}

// the integration's one launch, for the object and for crsdr_map_integrate: the same kernel on the same arguments, so the same bits
static int integrate_enqueue(CafRun &r, const float *maps, int nlines, int nmaps, int nd, int R, const integ::Params &prm, unsigned char *state, float *imap)
{
    const int nb = caf_integrate::bins_of(nd, R);
    return caf_run(r, caf_integrate::k_caf_integrate, dim3((unsigned)((nd + nb - 1) / nb), (unsigned)nmaps), dim3(caf_integrate::THREADS), caf_integrate::lds_bytes(nb, R), maps,
                   nlines, nmaps, nd, R, nb, prm, state, imap);
}

// The three dynamic LDS limits above the 64 KiB default, k_bearing_slot's, k_caf_track's and k_caf_beam_adapt's, are function attributes of the current
// device, shared by every live object: each create sets all three to the most any object can ask for, so that no call lowers a limit under
// another and no setter has to think of them.  crsdr_bearing, crsdr_track and crsdr_beam_adapt do the same for their calls.
static int caf_lds_limits()
{
    HIP_TRY(hipFuncSetAttribute((const void *)bearing::k_bearing_slot, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bearing::slot_lds_bytes(brg::MAX_M, cfar::MAX_HR)));
    HIP_TRY(hipFuncSetAttribute((const void *)caf_track::k_caf_track, hipFuncAttributeMaxDynamicSharedMemorySize, (int)caf_track::lds_bytes(trk::MAX_TRACKS, trk::MAX_MEAS)));
    HIP_TRY(hipFuncSetAttribute((const void *)caf_adapt::k_caf_beam_adapt, hipFuncAttributeMaxDynamicSharedMemorySize, (int)caf_adapt::adapt_lds_bytes(ad::MAX_M)));
    return CRSDR_OK;
}

// ---- the object: create, destroy, and what the setters share ----
// the object's device, and no kernel of the last submit still on the buffers: what every setter, track_reset and destroy do first
static int caf_quiesce(crsdr_caf *q)
{
    HIP_TRY(hipSetDevice(q->device));
    if (q->last.ran & kCafRanBase) HIP_TRY(hipDeviceSynchronize());      // (the last submit's stream may be the caller's, and gone)
    return CRSDR_OK;
}

static void caf_free(crsdr_caf *q)
{
    if (!q) return;
    (void)caf_quiesce(q);
    delete q;                                            // the buffers, then the stream
}

// a setter's first half, behind its checks: the last submit may still write the buffers let go here; then the feature is off, and
// nothing has been submitted since it was set.  The second half builds the new feature in a local and moves it in whole.
template <typename Feature>
static int caf_clear(crsdr_caf *q, Feature &f, unsigned ran_bit)
{
    const int rc = caf_quiesce(q);
    if (!rc) { f = Feature(); q->last.ran &= ~ran_bit; }
    return rc;
}

// Who must be off before whom, who must be on before whom: every rule of the setters, each feature's in the order they are asked.
// must_be_on false: `feature` is not changed, set or turned off, while `other` is on, which works on its buffers and parameters (asked
// ahead of the descriptor's limits).  true: `feature` is not set while `other` is off (asked behind them, and not to turn it off).
// (the first nine name a state that `other` can ask for; the rest only a setter's question)
enum { kCafCfar, kCafBearing, kCafBeams, kCafBeamLists, kCafTrack, kCafIntegrate, kCafClean, kCafCancel, kCafArrayIntegrated, kCafTrackFused, kCafCfarEst,
       kCafIntegrateBeams, kCafAdapt, kCafIntegrateArray };
static const struct CafRule { int feature; bool must_be_on; int other; const char *refusal; } kCafRules[] = {
    {kCafCfar, false, kCafTrack, "caf_set_cfar: the tracker is on (crsdr_caf_set_track): its measurements are this detector's lists; turn it off first"},
    {kCafCfar, false, kCafBeams, "caf_set_cfar: beams are on (crsdr_caf_set_beams): whether they are detected on, and the lists' sizes, are this detector's; turn them off first"},
    {kCafCfar, false, kCafBearing, "caf_set_cfar: bearings are on (crsdr_caf_set_bearing): their buffers and training set are this detector's; turn them off first"},
    {kCafCfar, false, kCafClean, "caf_set_cfar: cleaning is on (crsdr_caf_set_clean): its picks are this detector's list and its lists this detector's; turn it off first"},
    {kCafCfarEst, false, kCafTrack, "caf_set_cfar_estimator: the tracker is on (crsdr_caf_set_track): its measurements are this detector's lists; turn it off first"},
    {kCafCfarEst, false, kCafBeams, "caf_set_cfar_estimator: beams are on (crsdr_caf_set_beams): their lists are this detector's; turn them off first"},
    {kCafCfarEst, false, kCafBearing, "caf_set_cfar_estimator: bearings are on (crsdr_caf_set_bearing): they follow this detector's lists; turn them off first"},
    {kCafCfarEst, false, kCafClean, "caf_set_cfar_estimator: cleaning is on (crsdr_caf_set_clean): its picks follow this detector's list; turn it off first"},
    {kCafCfarEst, true, kCafCfar, "caf_set_cfar_estimator: no detector set (crsdr_caf_set_cfar): the estimator belongs to its descriptor"},
    {kCafBearing, false, kCafTrack, "caf_set_bearing: the tracker is on (crsdr_caf_set_track): its auxiliary pairs are these bearings; turn it off first"},
    {kCafBearing, true, kCafCfar, "caf_set_bearing: no detector set (crsdr_caf_set_cfar): there are no detections to take a bearing of"},
    {kCafBeams, false, kCafTrack, "caf_set_beams: the tracker is on (crsdr_caf_set_track): the fused list may be its source; turn it off first"},
    {kCafBeams, false, kCafIntegrate, "caf_set_beams: integration is on (crsdr_caf_set_integrate): the beam maps' state has their number and size; turn it off first"},
    {kCafAdapt, false, kCafTrack, "caf_set_beam_adapt: the tracker is on (crsdr_caf_set_track): its state belongs to the maps this changes; turn it off first"},
    {kCafAdapt, false, kCafIntegrate, "caf_set_beam_adapt: integration is on (crsdr_caf_set_integrate): its state belongs to the maps this changes; turn it off first"},
    {kCafAdapt, true, kCafBeams, "caf_set_beam_adapt: no beams set (crsdr_caf_set_beams): the adaptation belongs to their descriptor"},
    {kCafTrack, true, kCafCfar, "caf_set_track: no detector set (crsdr_caf_set_cfar): there are no detections to track"},
    {kCafTrackFused, true, kCafBeamLists, "caf_set_track: the fused source needs beams with detection (crsdr_caf_set_beams behind crsdr_caf_set_cfar)"},
    {kCafIntegrate, false, kCafTrack, "caf_set_integrate: the tracker is on (crsdr_caf_set_track): its measurements are the lists of the maps this changes; turn it off first"},
    {kCafIntegrate, false, kCafBearing, "caf_set_integrate: bearings are on (crsdr_caf_set_bearing): they follow the lists of the map this changes; turn them off first"},
    {kCafIntegrateBeams, true, kCafBeams, "caf_set_integrate: CRSDR_INTEGRATE_BEAMS needs beams (crsdr_caf_set_beams): there are no beam maps to integrate"},
    {kCafIntegrateArray, false, kCafClean, "caf_set_integrate: cleaning is on (crsdr_caf_set_clean): with CRSDR_INTEGRATE_ARRAY its picks would come from another line's energy; turn it off first"},
    {kCafCancel, false, kCafClean, "caf_set_cancel: cleaning is on (crsdr_caf_set_clean): its basis begins with this canceller's and its sums are this canceller's; turn it off first"},
    {kCafClean, false, kCafArrayIntegrated, "caf_set_clean: CRSDR_INTEGRATE_ARRAY is on (crsdr_caf_set_integrate): the picks would come from another line's energy; turn it off first"},
    {kCafClean, true, kCafCancel, "caf_set_clean: no canceller set (crsdr_caf_set_cancel): the joint basis begins with the canceller's"},
    {kCafClean, true, kCafCfar, "caf_set_clean: no detector set (crsdr_caf_set_cfar): there are no detections to pick from"},
};

static int caf_rules(const crsdr_caf *q, int feature, bool must_be_on)
{
    const bool on[] = {q->cf.on, q->bg.on, q->bb.on, q->bb.on && q->bb.det, q->tk.on, q->ig.on, q->cl_.on, q->cn.on, q->ig.array()};
    for (const CafRule &u : kCafRules)
        if (u.feature == feature && u.must_be_on == must_be_on && on[u.other] != must_be_on) return fail(CRSDR_ESTATE, "%s", u.refusal);
    return CRSDR_OK;
}

extern "C" int crsdr_caf_create(crsdr_caf **caf, const crsdr_caf_desc *desc)
{
    if (!caf || !desc) return fail(CRSDR_EINVAL, "caf_create: NULL argument");
    *caf = nullptr;
    const int mb = desc->max_batch ? desc->max_batch : 1, F = desc->frames ? desc->frames : 1;
    { const int rc_ = caf_args_ok("caf_create", desc->nrows, desc->blocksize, mb, F, desc->seg, desc->nlags, desc->ref_row, desc->window, desc->guard); if (rc_) return rc_; }
    { int rc = require_device(); if (rc) return rc; }
    int ndev = 0;
    (void)crsdr_device_count(&ndev);
    if (desc->device < 0 || desc->device >= ndev) return fail(CRSDR_ENODEV, "caf_create: device %d of %d", desc->device, ndev);

    crsdr_caf *q = new (std::nothrow) crsdr_caf();
    if (!q) return fail(CRSDR_ENOMEM, "caf_create: out of host memory");
    q->nrows = desc->nrows; q->B = desc->blocksize; q->device = desc->device; q->max_batch = mb; q->frames = F; q->seg = desc->seg; q->nlags = desc->nlags;
    q->ref_row = desc->ref_row; q->window = desc->window; q->guard = desc->guard; q->nd = F * (q->B / (2 * q->seg));
    const size_t lines = q->lines(), cells = (size_t)q->nd * (size_t)q->nlags;
    int rc = [&]() -> int {
        HIP_TRY(hipSetDevice(q->device));
        HIP_TRY(hipStreamCreateWithFlags(&q->own.s, hipStreamNonBlocking));
        int r = CRSDR_OK;
        if ((r = q->tw.alloc((size_t)q->nd)) || (r = q->win.alloc((size_t)q->nd)) || (r = q->chi.alloc(lines * (size_t)q->nrows * cells)) || (r = q->map.alloc(lines * cells)) ||
            (r = q->peak.alloc(lines * (size_t)(q->nrows + 1) * 6)) || (r = caf_lds_limits()))
            return r;
        if ((r = spectra_tables(q->own.s, q->nd, q->window, q->tw, q->win))) return r;
        HIP_TRY(hipStreamSynchronize(q->own.s));         // a submit may come on any stream
        return CRSDR_OK;
    }();
    if (rc) { caf_free(q); return rc; }
    *caf = q;
    return CRSDR_OK;
}

extern "C" int crsdr_caf_destroy(crsdr_caf *caf)
{
    if (!caf) return fail(CRSDR_EINVAL, "caf_destroy: NULL caf");
    caf_free(caf);
    return CRSDR_OK;
}

// ---- a submit: the stages in stream order, each of which returns at once with its feature off ----
// the rows (plain, or the canceller's five), the map, the peaks
static int caf_stage_maps(crsdr_caf *q, CafRun &r, const int8_t *packets, size_t packet_stride, size_t matrix_offset, int nblocks)
{
    const CancelBufs cb = q->cn.bufs();
    return caf_enqueue(r, packets, packet_stride, matrix_offset, nblocks, q->nrows, q->B, q->frames, q->seg, q->nlags, q->ref_row, q->window, q->guard, q->tw, q->win, q->chi,
                       q->map, q->peak, q->cn.on ? &cb : nullptr);
}

// the array map across the lines: one launch whatever the batch (the state's first block)
static int caf_stage_integrate(crsdr_caf *q, CafRun &r)
{
    crsdr_caf::Integrate &g = q->ig;
    if (!g.array()) return CRSDR_OK;
    return integrate_enqueue(r, q->map, r.nest, 1, q->nd, q->nlags, g.prm, g.state, g.imap);
}

// (the detector's array-map entry reads the integrated map where there is one; the rows' entries and the snapshots read chi as ever)
static int caf_stage_cfar(crsdr_caf *q, CafRun &r)
{
    crsdr_caf::Cfar &c = q->cf;
    if (!c.on) return CRSDR_OK;
    return cfar_enqueue(r, q->chi, q->ig.array() ? q->ig.imap : q->map, r.nest, q->nrows, q->nrows + 1, q->nd, q->nlags, q->guard, c.prm, c.keep, c.slots, c.tcount, c.det, c.count, c.snap);
}

// the second stage, behind the detector whose array-map list it picks from: nine launches whatever the batch and the picks.  It reads
// the canceller's and the detector's buffers and writes its own; the detector's tile scratch is free again by stream order
static int caf_stage_clean(crsdr_caf *q, CafRun &r, const int8_t *packets, size_t packet_stride, size_t matrix_offset)
{
    crsdr_caf::Clean &c = q->cl_;
    if (!c.on) return CRSDR_OK;
    const crsdr_caf::Cancel &cn = q->cn;
    const crsdr_caf::Cfar &cf = q->cf;
    const int nest = r.nest, nrows = q->nrows, nd = q->nd, R = q->nlags, lg = ilog2_exact(nd), lgseg = ilog2_exact(q->seg), K = cn.taps, P = cn.dopp, cells = nd * R;
    const size_t Kd = (size_t)cf.prm.max_det, entries = (size_t)(nrows + 1);
    const int sums = c.n2max * c.nmax + nrows * c.n2max;
    const float scale = (float)(1.0 / (127.0 * 127.0 * (double)q->seg * (q->window == CRSDR_WINDOW_HANN ? 0.5 * (double)nd : (double)nd)));
    int rc = caf_run(r, clean::k_clean_pick, dim3((unsigned)nest), dim3(64), 0, (const float *)(cf.det.p + (size_t)nrows * Kd * 8), entries * Kd * 8,
                     (const int32_t *)(cf.count.p + nrows), entries, (int)Kd, nd, R, K, P, c.prm, c.tab.p, c.tgt.p, c.ntgt.p);
    if (rc || (rc = caf_run(r, clean::k_clean_g, dim3((unsigned)nd, (unsigned)nest), dim3(clean::THREADS), 0, packets, packet_stride, matrix_offset, q->B, q->frames, lgseg, nd,
                            R, q->ref_row, (const cl::Table *)c.tab.p, c.slots, c.n2max, c.G2.p, c.ph2.p)) ||
        (rc = caf_run(r, clean::k_clean_y, dim3((unsigned)((nd * c.slots + clean::THREADS - 1) / clean::THREADS), (unsigned)nrows, (unsigned)nest), dim3(clean::THREADS), 0,
                      packets, packet_stride, matrix_offset, nrows, q->B, q->frames, lgseg, nd, q->ref_row, (const cl::Table *)c.tab.p, c.slots, c.Y2.p)) ||
        (rc = caf_run(r, clean::k_clean_sums, dim3((unsigned)((sums + clean::SUM_ENTRIES - 1) / clean::SUM_ENTRIES), (unsigned)nest), dim3(clean::THREADS), 0,
                      (const int2 *)cn.G.p, (const int2 *)c.G2.p, (const int2 *)c.Y2.p, (const double2 *)c.ph2.p, (const cl::Table *)c.tab.p, nrows, nd, R, K, P, q->ref_row,
                      c.slots, c.n2max, c.n2max, c.nmax, c.A2.p, c.C2.p)) ||
        (rc = caf_run(r, clean::k_clean_solve, dim3((unsigned)nest, (unsigned)((nrows + clean::SOLVE_ROWS - 1) / clean::SOLVE_ROWS)), dim3(clean::THREADS), 0,
                      (const double2 *)cn.S.p, (const double2 *)cn.C.p, (const long long *)cn.E.p, (const double2 *)cn.h.p, (const double2 *)c.A2.p, (const double2 *)c.C2.p,
                      (const cl::Table *)c.tab.p, nrows, K, P, q->ref_row, c.n2max, c.nmax, cl::per_pick(c.prm), c.Wj.p, c.hj.p, c.jstat.p, c.tcoef.p, c.tinfo.p)))
        return rc;
    caf::CleanArgs a;
    a.taps = K; a.dopp = P; a.nlags = R; a.G = cn.G; a.h = c.hj; a.ph = cn.ph; a.status = c.jstat;
    a.hstride = c.nmax; a.slots = c.slots; a.members = c.n2max; a.tab = c.tab; a.G2 = c.G2; a.ph2 = c.ph2;
    CAF_DISPATCH(lg, rc = caf_run(r, (caf::k_caf<LG, 3, caf::CleanArgs>), dim3((unsigned)(nrows * caf::caf_tiles(lg, R)), (unsigned)nest), dim3(caf::CAF_THREADS), 0, packets,
                                  packet_stride, matrix_offset, nrows, q->B, q->frames, lgseg, R, q->ref_row, (const float2 *)q->tw.p, (const float *)q->win.p, scale, c.rchi.p, a));
    if (rc || (rc = caf_run(r, caf::k_caf_map, dim3((unsigned)((cells + caf::CAF_MAP_CELLS - 1) / caf::CAF_MAP_CELLS), (unsigned)nest), dim3(caf::CAF_THREADS), 0,
                            (const float2 *)c.rchi.p, nrows, cells, q->ref_row, c.rmap.p)))
        return rc;
    return cfar_enqueue(r, c.rchi, c.rmap, nest, nrows, nrows + 1, nd, R, q->guard, cf.prm, cf.keep, cf.slots, cf.tcount, c.rdet, c.rcount, c.rsnap);
}

// (the bearings and the tracker read the array map's lists: entry nrows of the nrows + 1 of a line)
static int caf_stage_bearing(crsdr_caf *q, CafRun &r)
{
    crsdr_caf::Bearing &g = q->bg;
    if (!g.on) return CRSDR_OK;
    const size_t K = (size_t)q->cf.prm.max_det, entries = (size_t)(q->nrows + 1);
    return bearing_enqueue(r, q->chi, q->cf.det.p + (size_t)q->nrows * K * 8, entries * K * 8, q->cf.count.p + q->nrows, entries, r.nest, q->nrows, q->nd, q->nlags, q->ref_row,
                           q->guard, q->cf.prm, g.prm, g.rec, g.tbest, g.dir, g.spec);
}

static int caf_stage_beams(crsdr_caf *q, CafRun &r)
{
    crsdr_caf::Beams &g = q->bb;
    if (!g.on) return CRSDR_OK;
    crsdr_caf::Adapt &a = q->ba;
    if (!a.on) return beam_maps_enqueue(r, q->chi, g.w, 0, r.nest, q->nrows, q->nd * q->nlags, q->ref_row, g.nb, g.bmap);
    // the lines' own weights first: two launches whatever the batch, and the maps read aw line by line
    const int rc = beam_adapt_enqueue(r, q->chi, g.w, r.nest, q->nrows, q->nd, q->nlags, q->ref_row, g.nb, a.prm, a.part, a.aw, a.ainfo, a.astat);
    if (rc) return rc;
    return beam_maps_enqueue(r, q->chi, a.aw, (size_t)g.nb * (size_t)(q->nrows - 1) * 2, r.nest, q->nrows, q->nd * q->nlags, q->ref_row, g.nb, g.bmap);
}

// the beam maps across the lines, (line, beam) in bmap's order: one launch (the state's block behind the array map's, if that is there)
static int caf_stage_integrate_beams(crsdr_caf *q, CafRun &r)
{
    crsdr_caf::Integrate &g = q->ig;
    if (!g.beams()) return CRSDR_OK;
    unsigned char *state = g.state.p + (g.array() ? integ::state_bytes(1, q->nd, q->nlags) : 0);
    return integrate_enqueue(r, q->bb.bmap, r.nest, q->bb.nb, q->nd, q->nlags, g.prm, state, g.ibmap);
}

// the detector on the beams' maps and the fusion of their lists: (line, beam) is the line of a one-map call, as crsdr_cfar has it with comps = 1
static int caf_stage_beam_lists(crsdr_caf *q, CafRun &r)
{
    crsdr_caf::Beams &g = q->bb;
    if (!g.on || !g.det) return CRSDR_OK;
    const int rc = cfar_enqueue(r, nullptr, q->ig.beams() ? q->ig.ibmap : g.bmap, r.nest * g.nb, 0, 1, q->nd, q->nlags, q->guard, q->cf.prm, q->cf.keep, g.slots, g.tcount, g.bdet, g.bcount, nullptr);
    if (rc) return rc;
    return beam_fuse_enqueue(r, g.bdet, g.bcount, r.nest, g.nb, q->cf.prm.max_det, q->nd, q->nlags, g.fused, g.nfused);
}

static int caf_stage_track(crsdr_caf *q, CafRun &r)
{
    crsdr_caf::Track &t = q->tk;
    if (!t.on) return CRSDR_OK;
    const size_t K = (size_t)q->cf.prm.max_det, entries = (size_t)(q->nrows + 1);
    if (t.prm.source == trk::SRC_FUSED)
        return track_enqueue(r, q->bb.fused, K * 8, q->bb.nfused, 1, nullptr, caf_track::AUX_BEAM, r.nest, (int)K, q->nd, q->nlags, t.prm, t.state, t.trk, t.ntrk);
    return track_enqueue(r, q->cf.det.p + (size_t)q->nrows * K * 8, entries * K * 8, q->cf.count.p + q->nrows, entries, q->bg.on ? q->bg.dir.p : nullptr,
                         q->bg.on ? caf_track::AUX_DIR : caf_track::AUX_NONE, r.nest, (int)K, q->nd, q->nlags, t.prm, t.state, t.trk, t.ntrk);
}

static int caf_launch(crsdr_caf *q, const int8_t *packets, size_t packet_stride, size_t matrix_offset, int nblocks, hipStream_t S)
{
    CafRun r{S, nblocks / q->frames};
    int rc = caf_stage_maps(q, r, packets, packet_stride, matrix_offset, nblocks);
    if (!rc) rc = caf_stage_integrate(q, r);
    if (!rc) rc = caf_stage_cfar(q, r);
    if (!rc) rc = caf_stage_clean(q, r, packets, packet_stride, matrix_offset);
    if (!rc) rc = caf_stage_bearing(q, r);
    if (!rc) rc = caf_stage_beams(q, r);
    if (!rc) rc = caf_stage_integrate_beams(q, r);
    if (!rc) rc = caf_stage_beam_lists(q, r);
    if (!rc) rc = caf_stage_track(q, r);
    // Deliberately also behind a stage that failed to launch: the kernels ahead of it are on S and write the buffers, so the object
    // counts as submitted from the first launch on, and destroy and the setters wait for them (caf_quiesce).  The features' bits
    // stand for whole stages only.
    if (r.launches)
        q->last = CafLast{S, r.nest, r.launches, rc ? kCafRanBase : kCafRanBase | (q->cn.on ? kCafRanCancel : 0u) | (q->cf.on ? kCafRanCfar : 0u) | (q->bg.on ? kCafRanBearing : 0u) |
                                                                      (q->bb.on ? kCafRanBeams : 0u) | (q->tk.on ? kCafRanTrack : 0u) | (q->ig.on ? kCafRanIntegrate : 0u) | (q->ba.on ? kCafRanAdapt : 0u) | (q->cl_.on ? kCafRanClean : 0u)};
    return rc;
}

extern "C" int crsdr_caf_submit(crsdr_caf *q, const void *device_packets, size_t packet_stride, size_t matrix_offset, int nblocks, void *hip_stream)
{
    if (!q || !device_packets) return fail(CRSDR_EINVAL, "caf_submit: NULL caf or packets");
    if (nblocks < 1 || nblocks > q->max_batch || nblocks % q->frames)
        return fail(CRSDR_EINVAL, "caf_submit: nblocks = %d (1..max_batch = %d, a multiple of frames = %d)", nblocks, q->max_batch, q->frames);
    if (((uintptr_t)device_packets + matrix_offset) % 4 || packet_stride % 4)
        return fail(CRSDR_EINVAL, "caf_submit: matrix start and packet stride must be 4-byte aligned");
    if (nblocks > 1 && packet_stride < (size_t)q->nrows * (size_t)q->B)
        return fail(CRSDR_EINVAL, "caf_submit: packet_stride = %zu is smaller than a matrix of %d x %d", packet_stride, q->nrows, q->B);
    HIP_TRY(hipSetDevice(q->device));
    return caf_launch(q, (const int8_t *)device_packets, packet_stride, matrix_offset, nblocks, hip_stream ? (hipStream_t)hip_stream : q->own.s);
}

extern "C" int crsdr_caf_submit_plan(crsdr_caf *q, crsdr_plan *p)
{
    if (!q || !p) return fail(CRSDR_EINVAL, "caf_submit_plan: NULL argument");
    if (p->nrows != q->nrows || p->B != q->B || p->device != q->device)
        return fail(CRSDR_EINVAL, "caf_submit_plan: plan is %d x %d on device %d, caf %d x %d on device %d", p->nrows, p->B, p->device, q->nrows, q->B, q->device);
    if (p->d_slab) return fail(CRSDR_ESTATE, "caf_submit_plan: the plan writes slabs (crsdr_plan_bind_slab): its packets hold no matrix");
    if (!p->submitted || p->last_nblocks < 1) return fail(CRSDR_ESTATE, "caf_submit_plan: the plan has no submitted batch");
    if (p->last_nblocks > q->max_batch || p->last_nblocks % q->frames)
        return fail(CRSDR_EINVAL, "caf_submit_plan: the plan's batch of %d blocks (caf: at most %d, a multiple of frames = %d)", p->last_nblocks, q->max_batch, q->frames);
    HIP_TRY(hipSetDevice(q->device));
    // the batch's last kernel is on p->stream: stream order alone puts the maps behind it
    return caf_launch(q, p->d_packet, p->packet_stride, p->matrix_off, p->last_nblocks, p->stream);
}

extern "C" int crsdr_caf_last_submit(crsdr_caf *q, int *nest, int *launches)
{
    if (!q) return fail(CRSDR_EINVAL, "caf_last_submit: NULL caf");
    if (!(q->last.ran & kCafRanBase)) return fail(CRSDR_ESTATE, "caf_last_submit: nothing submitted");
    if (nest) *nest = q->last.nest;
    if (launches) *launches = q->last.launches;
    return CRSDR_OK;
}

// ---- the maps ----
extern "C" int crsdr_caf_fetch(crsdr_caf *q, float *chi, float *map, float *peak)
{
    if (!q) return fail(CRSDR_EINVAL, "caf_fetch: NULL caf");
    if (!(q->last.ran & kCafRanBase)) return fail(CRSDR_ESTATE, "caf_fetch: nothing submitted");
    const size_t lines = (size_t)q->last.nest, cells = (size_t)q->nd * (size_t)q->nlags;
    return DevFetch(q->device, q->last.stream).copy(chi, q->chi.p, lines * (size_t)q->nrows * cells).copy(map, q->map.p, lines * cells)
        .copy(peak, q->peak.p, lines * (size_t)(q->nrows + 1) * 6).wait();
}

extern "C" int crsdr_caf_device_buffers(crsdr_caf *q, void **chi, void **map, void **peak)
{
    if (!q) return fail(CRSDR_EINVAL, "caf_device_buffers: NULL caf");
    if (chi) *chi = q->chi;
    if (map) *map = q->map;
    if (peak) *peak = q->peak;
    return CRSDR_OK;
}

// ---- the detector ----
extern "C" int crsdr_caf_set_cfar(crsdr_caf *q, const crsdr_cfar_desc *desc)
{
    if (!q) return fail(CRSDR_EINVAL, "caf_set_cfar: NULL caf");
    { const int rc = caf_rules(q, kCafCfar, false); if (rc) return rc; }
    cfar::Params prm{};
    if (desc) { const int rc_ = cfar_args_ok("caf_set_cfar", q->nd, desc, &prm); if (rc_) return rc_; }
    { const int rc = caf_clear(q, q->cf, kCafRanCfar); if (rc || !desc) return rc; }
    const size_t lines = q->lines(), maps = lines * (size_t)(q->nrows + 1), K = (size_t)prm.max_det, tiles = (size_t)cfar::tiles_of(q->nd, q->nlags);
    crsdr_caf::Cfar f;
    f.prm = prm; f.keep = cfar::tile_keep(prm.max_det, q->nd, q->nlags); f.on = true;
    int r = CRSDR_OK;
    if ((r = f.slots.alloc(maps * tiles * (size_t)f.keep)) || (r = f.tcount.alloc(maps * tiles)) || (r = f.count.alloc(maps)) || (r = f.det.alloc(maps * K * 8)) ||
        (r = f.snap.alloc(lines * K * (size_t)q->nrows * 2)))
        return r;
    q->cf = std::move(f);
    return CRSDR_OK;
}

// The estimator of the descriptor last set.  Nothing is allocated: the lists' sizes are the descriptor's.
extern "C" int crsdr_caf_set_cfar_estimator(crsdr_caf *q, const crsdr_cfar_est_desc *desc)
{
    if (!q) return fail(CRSDR_EINVAL, "caf_set_cfar_estimator: NULL caf");
    { const int rc = caf_rules(q, kCafCfarEst, false); if (rc) return rc; }
    // (the estimator and the axis need no detector to be judged; the rank needs its window, so the state is asked between them)
    if (desc && (desc->estimator < cfar::EST_CA || desc->estimator > cfar::EST_OS))
        return fail(CRSDR_EINVAL, "caf_set_cfar_estimator: estimator = %d (0 cell averaging, 1 greatest-of, 2 smallest-of, 3 ordered statistic)", desc->estimator);
    if (desc && (desc->estimator == cfar::EST_GO || desc->estimator == cfar::EST_SO) && (desc->axis < 0 || desc->axis > 1))
        return fail(CRSDR_EINVAL, "caf_set_cfar_estimator: axis = %d (0 lag, 1 Doppler)", desc->axis);
    { const int rc = caf_rules(q, kCafCfarEst, true); if (rc) return rc; }
    cfar::Params prm = q->cf.prm;
    prm.est = cfar::EST_CA; prm.axis = 0; prm.rank = 0;
    { const int rc = cfar_est_ok("caf_set_cfar_estimator", desc, &prm); if (rc) return rc; }
    { const int rc = caf_quiesce(q); if (rc) return rc; }
    q->cf.prm = prm;
    q->last.ran &= ~kCafRanCfar;
    return CRSDR_OK;
}

extern "C" int crsdr_caf_fetch_cfar(crsdr_caf *q, float *det, int32_t *count, float *snap)
{
    if (!q) return fail(CRSDR_EINVAL, "caf_fetch_cfar: NULL caf");
    if (!q->cf.on) return fail(CRSDR_ESTATE, "caf_fetch_cfar: no detector set (crsdr_caf_set_cfar)");
    if (!(q->last.ran & kCafRanCfar)) return fail(CRSDR_ESTATE, "caf_fetch_cfar: nothing submitted since the detector was set");
    const size_t lines = (size_t)q->last.nest, maps = lines * (size_t)(q->nrows + 1), K = (size_t)q->cf.prm.max_det;
    return DevFetch(q->device, q->last.stream).copy(det, q->cf.det.p, maps * K * 8).copy(count, q->cf.count.p, maps).copy(snap, q->cf.snap.p, lines * K * (size_t)q->nrows * 2)
        .wait();
}

extern "C" int crsdr_caf_cfar_device_buffers(crsdr_caf *q, void **det, void **count, void **snap)
{
    if (!q) return fail(CRSDR_EINVAL, "caf_cfar_device_buffers: NULL caf");
    if (!q->cf.on) return fail(CRSDR_ESTATE, "caf_cfar_device_buffers: no detector set (crsdr_caf_set_cfar)");
    if (det) *det = q->cf.det;
    if (count) *count = q->cf.count;
    if (snap) *snap = q->cf.snap;
    return CRSDR_OK;
}

extern "C" int crsdr_cfar_alpha(double pfa, int ntrain, float *alpha)
{
    if (!alpha) return fail(CRSDR_EINVAL, "cfar_alpha: NULL alpha");
    if (!(pfa > 0.0 && pfa < 1.0)) return fail(CRSDR_EINVAL, "cfar_alpha: pfa = %g (inside (0, 1))", pfa);
    if (ntrain < 1) return fail(CRSDR_EINVAL, "cfar_alpha: ntrain = %d (at least 1)", ntrain);
    *alpha = (float)((double)ntrain * (pow(pfa, -1.0 / (double)ntrain) - 1.0));
    return CRSDR_OK;
}

// The false-alarm probability of a cell under exponential noise of mean 1 in every cell, at threshold factor alpha (section (w)):
//   SO   2 (2 + T)^-n sum_{i < n} C(n - 1 + i, i) (2 + T)^-i,  T = alpha / n, n the cells of a half; the terms through their logarithms
//   GO   2 (1 + T)^-n - P_SO
//   OS   prod_{i < rank} (N - i) / (N - i + alpha)
static double cfar_pfa(int est, int n, int rank, double alpha)
{
    if (est == cfar::EST_OS) {
        double p = 1.0;
        for (int i = 0; i < rank; ++i) p *= (double)(n - i) / ((double)(n - i) + alpha);
        return p;
    }
    const double T = alpha / (double)n, lx = -log(2.0 + T);
    double so = 0.0, lc = 0.0;
    for (int i = 0; i < n; ++i) {
        if (i) lc += log((double)(n - 1 + i) / (double)i);
        so += exp(lc + (double)(n + i) * lx);
    }
    so *= 2.0;
    return est == cfar::EST_SO ? so : 2.0 * exp(-(double)n * log(1.0 + T)) - so;
}

extern "C" int crsdr_cfar_alpha_est(double pfa, int ntrain, const crsdr_cfar_est_desc *est, float *alpha)
{
    if (!est || est->estimator == cfar::EST_CA) return crsdr_cfar_alpha(pfa, ntrain, alpha);
    if (!alpha) return fail(CRSDR_EINVAL, "cfar_alpha_est: NULL alpha");
    if (!(pfa > 0.0 && pfa < 1.0)) return fail(CRSDR_EINVAL, "cfar_alpha_est: pfa = %g (inside (0, 1))", pfa);
    if (est->estimator < cfar::EST_CA || est->estimator > cfar::EST_OS) return fail(CRSDR_EINVAL, "cfar_alpha_est: estimator = %d (0..3)", est->estimator);
    if (ntrain < 1 || ntrain > kCfarAlphaMaxTrain) return fail(CRSDR_EINVAL, "cfar_alpha_est: ntrain = %d (1..%d)", ntrain, kCfarAlphaMaxTrain);
    if (est->estimator == cfar::EST_OS && (est->rank < 1 || est->rank > ntrain)) return fail(CRSDR_EINVAL, "cfar_alpha_est: rank = %d (1..ntrain = %d)", est->rank, ntrain);
    // the probability falls as alpha grows, from 1 at alpha = 0: a bracket by doubling, then bisection down to neighbouring doubles
    double lo = 0.0, hi = 1.0;
    while (cfar_pfa(est->estimator, ntrain, est->rank, hi) > pfa && hi < 1e300) hi *= 2.0;
    for (int it = 0; it < 2200; ++it) {
        const double mid = 0.5 * (lo + hi);
        if (!(mid > lo && mid < hi)) break;
        if (cfar_pfa(est->estimator, ntrain, est->rank, mid) > pfa) lo = mid; else hi = mid;
    }
    *alpha = (float)hi;
    return CRSDR_OK;
}

// crsdr_cfar and crsdr_cfar_est: est NULL is cell averaging
static int cfar_op(const char *who, float *det, int32_t *count, const float *src, int comps, int nd, int R, int guard, const crsdr_cfar_desc *desc,
                   const crsdr_cfar_est_desc *est, int mem_kind)
{
    if (!src || !desc || (!det && !count)) return fail(CRSDR_EINVAL, "%s: need src, a descriptor and at least one of det, count", who);
    if (comps != 1 && comps != 2) return fail(CRSDR_EINVAL, "%s: comps = %d (1: a map, 2: a chi)", who, comps);
    { const int rc_ = caf_shape_ok(who, nd, R, guard, 0, 2); if (rc_) return rc_; }
    cfar::Params prm{};
    { const int rc_ = cfar_args_ok(who, nd, desc, &prm); if (rc_) return rc_; }
    { const int rc_ = cfar_est_ok(who, est, &prm); if (rc_) return rc_; }
    if (mem_kind != CRSDR_MEM_HOST && mem_kind != CRSDR_MEM_DEVICE) return fail(CRSDR_EINVAL, "%s: mem_kind = %d", who, mem_kind);
    OP_PROLOGUE_MEM("cfar", mem_kind);
    const size_t cells = (size_t)nd * (size_t)R, K = (size_t)prm.max_det, tiles = (size_t)cfar::tiles_of(nd, R);
    const size_t sb = sizeof(float) * cells * (size_t)comps, db = sizeof(float) * K * 8, nb = sizeof(int32_t);
    const int keep = cfar::tile_keep(prm.max_det, nd, R);
    OpStage st(mem_kind);
    const float *d_s = (const float *)st.in(0, src, sb, comps == 2 ? 8 : 4);
    float *d_d = (float *)st.out(1, det, db, 4);
    int32_t *d_n = (int32_t *)st.out(2, count, nb, 4);
    if (st.rc) return st.rc;
    if (st.misaligned) return fail(CRSDR_EINVAL, "%s: device det, count and a map 4-byte, a chi 8-byte aligned", who);
    if (st.spare(1, d_d, db) || st.spare(2, d_n, nb)) return st.rc;
    OP_RESERVE(3, sizeof(cfar::Cand) * tiles * (size_t)keep);
    OP_RESERVE(4, sizeof(int32_t) * tiles);
    CafRun r{nullptr};
    { const int rc_ = cfar_enqueue(r, comps == 2 ? (const float2 *)d_s : nullptr, comps == 1 ? d_s : nullptr, 1, comps == 2 ? 1 : 0, 1, nd, R, guard, prm, keep,
                                   (cfar::Cand *)g_op.buf[3], (int32_t *)g_op.buf[4], d_d, d_n, nullptr); if (rc_) return rc_; }
    st.back(det, d_d, db);
    st.back(count, d_n, nb);
    return st.finish();
}

extern "C" int crsdr_cfar(float *det, int32_t *count, const float *src, int comps, int nd, int R, int guard, const crsdr_cfar_desc *desc, int mem_kind)
{
    return cfar_op("cfar", det, count, src, comps, nd, R, guard, desc, nullptr, mem_kind);
}

extern "C" int crsdr_cfar_est(float *det, int32_t *count, const float *src, int comps, int nd, int R, int guard, const crsdr_cfar_desc *desc,
                              const crsdr_cfar_est_desc *est, int mem_kind)
{
    return cfar_op("cfar_est", det, count, src, comps, nd, R, guard, desc, est, mem_kind);
}

// ---- the bearings ----
extern "C" int crsdr_caf_set_bearing(crsdr_caf *q, const crsdr_caf_bearing_desc *desc)
{
    if (!q) return fail(CRSDR_EINVAL, "caf_set_bearing: NULL caf");
    { const int rc = caf_rules(q, kCafBearing, false); if (rc) return rc; }
    const size_t lines = q->lines();
    brg::Params prm{};
    if (desc) {
        // (the detector off: the limits that need its K are checked with K = 1, and the call is refused for the state below)
        const int rc_ = bearing_args_ok("caf_set_bearing", q->nrows, (long long)lines, q->cf.on ? q->cf.prm.max_det : 1, desc, &prm);
        if (rc_) return rc_;
        { const int rc = caf_rules(q, kCafBearing, true); if (rc) return rc; }
    }
    { const int rc = caf_clear(q, q->bg, kCafRanBearing); if (rc || !desc) return rc; }
    const size_t K = (size_t)q->cf.prm.max_det, npts = (size_t)prm.ncx * (size_t)prm.ncy, tiles = (size_t)bearing::tiles_of(prm.ncx, prm.ncy);
    crsdr_caf::Bearing f;
    f.prm = prm; f.on = true;
    int r = CRSDR_OK;
    if ((r = f.rec.alloc(lines * K * brg::REC)) || (r = f.tbest.alloc(lines * K * tiles)) || (r = f.dir.alloc(lines * K * 8)) ||
        ((prm.flags & brg::KEEP_SPECTRUM) && (r = f.spec.alloc(lines * K * npts))))
        return r;
    q->bg = std::move(f);
    return CRSDR_OK;
}

extern "C" int crsdr_caf_fetch_bearing(crsdr_caf *q, float *dir, float *spec)
{
    if (!q) return fail(CRSDR_EINVAL, "caf_fetch_bearing: NULL caf");
    if (!q->bg.on) return fail(CRSDR_ESTATE, "caf_fetch_bearing: no bearings set (crsdr_caf_set_bearing)");
    if (!(q->last.ran & kCafRanBearing)) return fail(CRSDR_ESTATE, "caf_fetch_bearing: nothing submitted since the bearings were set");
    if (spec && !q->bg.spec.p) return fail(CRSDR_ESTATE, "caf_fetch_bearing: the spectrum is not kept (CRSDR_BEARING_KEEP_SPECTRUM)");
    const size_t slots = (size_t)q->last.nest * (size_t)q->cf.prm.max_det, npts = (size_t)q->bg.prm.ncx * (size_t)q->bg.prm.ncy;
    return DevFetch(q->device, q->last.stream).copy(dir, q->bg.dir.p, slots * 8).copy(spec, q->bg.spec.p, slots * npts).wait();
}

extern "C" int crsdr_caf_bearing_device_buffers(crsdr_caf *q, void **dir, void **spec)
{
    if (!q) return fail(CRSDR_EINVAL, "caf_bearing_device_buffers: NULL caf");
    if (!q->bg.on) return fail(CRSDR_ESTATE, "caf_bearing_device_buffers: no bearings set (crsdr_caf_set_bearing)");
    if (dir) *dir = q->bg.dir;
    if (spec) *spec = q->bg.spec;
    return CRSDR_OK;
}

extern "C" int crsdr_bearing(float *dir, float *spec, const float *chi, int nrows, int nd, int R, int ref_row, int guard, const float *det, const int32_t *count,
                             const crsdr_cfar_desc *cdesc, const crsdr_caf_bearing_desc *bdesc, int mem_kind)
{
    if (!chi || !det || !count || !cdesc || !bdesc || (!dir && !spec)) return fail(CRSDR_EINVAL, "bearing: need chi, det, count, both descriptors and at least one of dir, spec");
    { const int rc_ = caf_shape_ok("bearing", nd, R, guard, ref_row, nrows); if (rc_) return rc_; }
    cfar::Params cp{};
    brg::Params bp{};
    { const int rc_ = cfar_args_ok("bearing", nd, cdesc, &cp); if (rc_) return rc_; }
    { const int rc_ = bearing_args_ok("bearing", nrows, 1, cp.max_det, bdesc, &bp); if (rc_) return rc_; }
    if (spec && !(bp.flags & brg::KEEP_SPECTRUM)) return fail(CRSDR_EINVAL, "bearing: spec asked for without CRSDR_BEARING_KEEP_SPECTRUM");
    OP_PROLOGUE_MEM("bearing", mem_kind);
    const size_t cells = (size_t)nd * (size_t)R, K = (size_t)cp.max_det, npts = (size_t)bp.ncx * (size_t)bp.ncy, tiles = (size_t)bearing::tiles_of(bp.ncx, bp.ncy);
    const size_t cb = sizeof(float2) * (size_t)nrows * cells, tb = sizeof(float) * K * 8, nb = sizeof(int32_t), db = sizeof(float) * K * 8, sb = sizeof(float) * K * npts;
    const bool keep = (bp.flags & brg::KEEP_SPECTRUM) != 0;
    OpStage st(mem_kind);
    const float2 *d_c = (const float2 *)st.in(0, chi, cb, 8);
    const float *d_t = (const float *)st.in(1, det, tb, 4);
    const int32_t *d_n = (const int32_t *)st.in(2, count, nb, 4);
    float *d_d = (float *)st.out(3, dir, db, 4);
    float *d_s = keep ? (float *)st.out(4, spec, sb, 4) : nullptr;
    if (st.rc) return st.rc;
    if (st.misaligned) return fail(CRSDR_EINVAL, "bearing: device det, count, dir and spec 4-byte, chi 8-byte aligned");
    if (st.spare(3, d_d, db) || (keep && st.spare(4, d_s, sb))) return st.rc;
    OP_RESERVE(5, sizeof(double) * K * brg::REC);
    OP_RESERVE(6, sizeof(bearing::Best) * K * tiles);
    { const int rc_ = caf_lds_limits(); if (rc_) return rc_; }
    CafRun r{nullptr};
    { const int rc_ = bearing_enqueue(r, d_c, d_t, 0, d_n, 0, 1, nrows, nd, R, ref_row, guard, cp, bp, (double *)g_op.buf[5], (bearing::Best *)g_op.buf[6], d_d, d_s); if (rc_) return rc_; }
    st.back(dir, d_d, db);
    if (keep) st.back(spec, d_s, sb);
    return st.finish();
}

// ---- the beams ----
extern "C" int crsdr_caf_set_beams(crsdr_caf *q, const crsdr_caf_beams_desc *desc)
{
    if (!q) return fail(CRSDR_EINVAL, "caf_set_beams: NULL caf");
    { const int rc = caf_rules(q, kCafBeams, false); if (rc) return rc; }
    const size_t lines = q->lines(), cells = (size_t)q->nd * (size_t)q->nlags, m = (size_t)(q->nrows - 1);
    if (desc) { const int rc_ = beams_args_ok("caf_set_beams", q->nrows, (long long)lines, q->nd, q->nlags, desc->nbeams, desc->weights, desc->flags); if (rc_) return rc_; }
    { const int rc = caf_clear(q, q->ba, kCafRanAdapt); if (rc) return rc; }       // the adaptation belongs to the descriptor that goes
    { const int rc = caf_clear(q, q->bb, kCafRanBeams); if (rc || !desc) return rc; }
    const size_t nb = (size_t)desc->nbeams, maps = lines * nb;
    crsdr_caf::Beams f;
    f.nb = desc->nbeams; f.det = q->cf.on; f.on = true;
    int r = CRSDR_OK;
    if ((r = f.w.alloc(nb * m * 2)) || (r = f.bmap.alloc(maps * cells)) || (r = HIP_RC(hipMemcpy(f.w.p, desc->weights, sizeof(float) * nb * m * 2, hipMemcpyHostToDevice)))) return r;
    if (f.det) {
        const size_t K = (size_t)q->cf.prm.max_det, tiles = (size_t)cfar::tiles_of(q->nd, q->nlags);
        if ((r = f.slots.alloc(maps * tiles * (size_t)q->cf.keep)) || (r = f.tcount.alloc(maps * tiles)) || (r = f.bcount.alloc(maps)) || (r = f.bdet.alloc(maps * K * 8)) ||
            (r = f.fused.alloc(lines * K * 8)) || (r = f.nfused.alloc(lines)))
            return r;
    }
    q->bb = std::move(f);
    return CRSDR_OK;
}

extern "C" int crsdr_caf_fetch_beams(crsdr_caf *q, float *bmap, float *bdet, int32_t *bcount, float *fused, int32_t *nfused)
{
    if (!q) return fail(CRSDR_EINVAL, "caf_fetch_beams: NULL caf");
    if (!q->bb.on) return fail(CRSDR_ESTATE, "caf_fetch_beams: no beams set (crsdr_caf_set_beams)");
    if (!(q->last.ran & kCafRanBeams)) return fail(CRSDR_ESTATE, "caf_fetch_beams: nothing submitted since the beams were set");
    if ((bdet || bcount || fused || nfused) && !q->bb.det) return fail(CRSDR_ESTATE, "caf_fetch_beams: the detector was off when the beams were set: there are no lists");
    const size_t lines = (size_t)q->last.nest, maps = lines * (size_t)q->bb.nb, cells = (size_t)q->nd * (size_t)q->nlags, K = (size_t)q->cf.prm.max_det;
    return DevFetch(q->device, q->last.stream).copy(bmap, q->bb.bmap.p, maps * cells).copy(bdet, q->bb.bdet.p, maps * K * 8).copy(bcount, q->bb.bcount.p, maps)
        .copy(fused, q->bb.fused.p, lines * K * 8).copy(nfused, q->bb.nfused.p, lines).wait();
}

extern "C" int crsdr_caf_beams_device_buffers(crsdr_caf *q, void **bmap, void **bdet, void **bcount, void **fused, void **nfused)
{
    if (!q) return fail(CRSDR_EINVAL, "caf_beams_device_buffers: NULL caf");
    if (!q->bb.on) return fail(CRSDR_ESTATE, "caf_beams_device_buffers: no beams set (crsdr_caf_set_beams)");
    if (bmap) *bmap = q->bb.bmap;
    if (bdet) *bdet = q->bb.bdet;
    if (bcount) *bcount = q->bb.bcount;
    if (fused) *fused = q->bb.fused;
    if (nfused) *nfused = q->bb.nfused;
    return CRSDR_OK;
}

extern "C" int crsdr_beam_maps(float *bmap, const float *chi, int nrows, int nd, int R, int ref_row, const float *weights, int nbeams, int mem_kind)
{
    if (!bmap || !chi) return fail(CRSDR_EINVAL, "beam_maps: need bmap and chi");
    // (the maps do not depend on the shape of a line, only on its nd R cells: nd need not be a power of two here)
    { const int rc_ = caf_shape_ok("beam_maps", nd, R, 0, ref_row, nrows, false); if (rc_) return rc_; }
    { const int rc_ = beams_args_ok("beam_maps", nrows, 1, nd, R, nbeams, weights, 0u); if (rc_) return rc_; }
    OP_PROLOGUE_MEM("beam_maps", mem_kind);
    const size_t cells = (size_t)nd * (size_t)R, cb = sizeof(float2) * (size_t)nrows * cells, mb = sizeof(float) * (size_t)nbeams * cells;
    const size_t wb = sizeof(float) * 2 * (size_t)nbeams * (size_t)(nrows - 1);
    OpStage st(mem_kind);
    const float2 *d_c = (const float2 *)st.in(0, chi, cb, 8);
    float *d_m = (float *)st.out(1, bmap, mb, 4);
    if (st.rc) return st.rc;
    if (st.misaligned) return fail(CRSDR_EINVAL, "beam_maps: device bmap 4-byte, chi 8-byte aligned");
    OP_RESERVE(2, wb);                                      // (the weights are the host's in either kind)
    HIP_TRY(hipMemcpy(g_op.buf[2], weights, wb, hipMemcpyHostToDevice));
    CafRun r{nullptr};
    { const int rc_ = beam_maps_enqueue(r, d_c, (const float *)g_op.buf[2], 0, 1, nrows, (int)cells, ref_row, nbeams, d_m); if (rc_) return rc_; }
    st.back(bmap, d_m, mb);
    return st.finish();
}

// ---- the adaptive beams ----
extern "C" int crsdr_caf_set_beam_adapt(crsdr_caf *q, const crsdr_caf_beam_adapt_desc *desc)
{
    if (!q) return fail(CRSDR_EINVAL, "caf_set_beam_adapt: NULL caf");
    { const int rc = caf_rules(q, kCafAdapt, false); if (rc) return rc; }
    ad::Params prm{};
    if (desc) {
        { const int rc_ = adapt_args_ok("caf_set_beam_adapt", q->nrows, q->nd, q->nlags, desc, &prm); if (rc_) return rc_; }
        { const int rc = caf_rules(q, kCafAdapt, true); if (rc) return rc; }
    }
    { const int rc = caf_clear(q, q->ba, kCafRanAdapt); if (rc || !desc) return rc; }
    const size_t lines = q->lines(), m = (size_t)(q->nrows - 1), nb = (size_t)q->bb.nb;
    crsdr_caf::Adapt f;
    f.prm = prm; f.on = true;
    int r = CRSDR_OK;
    if ((r = f.part.alloc(lines * (size_t)ad::tiles_of(ad::cells_of(prm)) * (size_t)ad::pairs_of((int)m))) || (r = f.aw.alloc(lines * nb * m * 2)) ||
        (r = f.ainfo.alloc(lines * nb * 2)) || (r = f.astat.alloc(lines)))
        return r;
    q->ba = std::move(f);
    return CRSDR_OK;
}

extern "C" int crsdr_caf_fetch_beam_adapt(crsdr_caf *q, float *aw, float *ainfo, int32_t *astat)
{
    if (!q) return fail(CRSDR_EINVAL, "caf_fetch_beam_adapt: NULL caf");
    if (!q->ba.on) return fail(CRSDR_ESTATE, "caf_fetch_beam_adapt: no adaptation set (crsdr_caf_set_beam_adapt)");
    if (!(q->last.ran & kCafRanAdapt)) return fail(CRSDR_ESTATE, "caf_fetch_beam_adapt: nothing submitted since the adaptation was set");
    const size_t lines = (size_t)q->last.nest, nb = (size_t)q->bb.nb, m = (size_t)(q->nrows - 1);
    return DevFetch(q->device, q->last.stream).copy(aw, q->ba.aw.p, lines * nb * m * 2).copy(ainfo, q->ba.ainfo.p, lines * nb * 2).copy(astat, q->ba.astat.p, lines).wait();
}

extern "C" int crsdr_caf_beam_adapt_device_buffers(crsdr_caf *q, void **aw, void **ainfo, void **astat)
{
    if (!q) return fail(CRSDR_EINVAL, "caf_beam_adapt_device_buffers: NULL caf");
    if (!q->ba.on) return fail(CRSDR_ESTATE, "caf_beam_adapt_device_buffers: no adaptation set (crsdr_caf_set_beam_adapt)");
    if (aw) *aw = q->ba.aw;
    if (ainfo) *ainfo = q->ba.ainfo;
    if (astat) *astat = q->ba.astat;
    return CRSDR_OK;
}

extern "C" int crsdr_beam_adapt(float *aw, float *ainfo, int32_t *astat, const float *chi, int nrows, int nd, int R, int ref_row, const float *weights, int nbeams,
                                const crsdr_caf_beam_adapt_desc *desc, int mem_kind)
{
    if (!chi || !desc || (!aw && !ainfo && !astat)) return fail(CRSDR_EINVAL, "beam_adapt: need chi, a descriptor and at least one of aw, ainfo, astat");
    { const int rc_ = caf_shape_ok("beam_adapt", nd, R, 0, ref_row, nrows, false); if (rc_) return rc_; }
    { const int rc_ = beams_args_ok("beam_adapt", nrows, 1, nd, R, nbeams, weights, 0u); if (rc_) return rc_; }
    ad::Params prm{};
    { const int rc_ = adapt_args_ok("beam_adapt", nrows, nd, R, desc, &prm); if (rc_) return rc_; }
    OP_PROLOGUE_MEM("beam_adapt", mem_kind);
    const size_t cells = (size_t)nd * (size_t)R, m = (size_t)(nrows - 1), nb = (size_t)nbeams, cb = sizeof(float2) * (size_t)nrows * cells;
    const size_t wb = sizeof(float) * 2 * nb * m, ib = sizeof(float) * 2 * nb, sb = sizeof(int32_t);
    OpStage st(mem_kind);
    const float2 *d_c = (const float2 *)st.in(0, chi, cb, 8);
    float *d_w = (float *)st.out(1, aw, wb, 4);
    float *d_i = (float *)st.out(2, ainfo, ib, 4);
    int32_t *d_s = (int32_t *)st.out(3, astat, sb, 4);
    if (st.rc) return st.rc;
    if (st.misaligned) return fail(CRSDR_EINVAL, "beam_adapt: device aw, ainfo and astat 4-byte, chi 8-byte aligned");
    if (st.spare(1, d_w, wb) || st.spare(2, d_i, ib) || st.spare(3, d_s, sb)) return st.rc;
    OP_RESERVE(4, wb);                                      // (the weights are the host's in either kind)
    HIP_TRY(hipMemcpy(g_op.buf[4], weights, wb, hipMemcpyHostToDevice));
    OP_RESERVE(5, sizeof(double2) * (size_t)ad::tiles_of(ad::cells_of(prm)) * (size_t)ad::pairs_of((int)m));
    { const int rc_ = caf_lds_limits(); if (rc_) return rc_; }
    CafRun r{nullptr};
    { const int rc_ = beam_adapt_enqueue(r, d_c, (const float *)g_op.buf[4], 1, nrows, nd, R, ref_row, nbeams, prm, (double2 *)g_op.buf[5], d_w, d_i, d_s); if (rc_) return rc_; }
    st.back(aw, d_w, wb);
    st.back(ainfo, d_i, ib);
    st.back(astat, d_s, sb);
    return st.finish();
}

extern "C" int crsdr_beam_fuse(float *fused, int32_t *nfused, const float *bdet, const int32_t *bcount, int nbeams, int K, int nd, int R, int mem_kind)
{
    if (!bdet || !bcount || (!fused && !nfused)) return fail(CRSDR_EINVAL, "beam_fuse: need bdet, bcount and at least one of fused, nfused");
    { const int rc_ = caf_shape_ok("beam_fuse", nd, R, 0, 0, 2); if (rc_) return rc_; }
    if (nbeams < 1 || nbeams > bm::MAX_BEAMS) return fail(CRSDR_EINVAL, "beam_fuse: nbeams = %d (1..%d)", nbeams, bm::MAX_BEAMS);
    if (K < 1 || K > cfar::MAX_DET) return fail(CRSDR_EINVAL, "beam_fuse: K = %d (1..%d)", K, cfar::MAX_DET);
    OP_PROLOGUE_MEM("beam_fuse", mem_kind);
    const size_t tb = sizeof(float) * (size_t)nbeams * (size_t)K * 8, nb = sizeof(int32_t) * (size_t)nbeams, fb = sizeof(float) * (size_t)K * 8;
    OpStage st(mem_kind);
    const float *d_t = (const float *)st.in(0, bdet, tb, 4);
    const int32_t *d_n = (const int32_t *)st.in(1, bcount, nb, 4);
    float *d_f = (float *)st.out(2, fused, fb, 4);
    int32_t *d_k = (int32_t *)st.out(3, nfused, sizeof(int32_t), 4);
    if (st.rc) return st.rc;
    if (st.misaligned) return fail(CRSDR_EINVAL, "beam_fuse: device bdet, bcount, fused and nfused 4-byte aligned");
    if (st.spare(2, d_f, fb) || st.spare(3, d_k, sizeof(int32_t))) return st.rc;
    CafRun r{nullptr};
    { const int rc_ = beam_fuse_enqueue(r, d_t, d_n, 1, nbeams, K, nd, R, d_f, d_k); if (rc_) return rc_; }
    st.back(fused, d_f, fb);
    st.back(nfused, d_k, sizeof(int32_t));
    return st.finish();
}

extern "C" int crsdr_caf_beam_steer(float *weights, int mx, int my, float d, int ncx, int ncy, const double *xy, int nbeams)
{
    if (!weights || !xy) return fail(CRSDR_EINVAL, "caf_beam_steer: NULL argument");
    if (mx < 1 || my < 1 || (long long)mx * my > bm::MAX_M) return fail(CRSDR_EINVAL, "caf_beam_steer: mx, my = %d, %d (at least 1, mx my at most %d)", mx, my, bm::MAX_M);
    if (nbeams < 1 || nbeams > bm::MAX_BEAMS) return fail(CRSDR_EINVAL, "caf_beam_steer: nbeams = %d (1..%d)", nbeams, bm::MAX_BEAMS);
    if (ncx < brg::MIN_NC || ncx > brg::MAX_NC || ncy < brg::MIN_NC || ncy > brg::MAX_NC)
        return fail(CRSDR_EINVAL, "caf_beam_steer: ncx, ncy = %d, %d (%d..%d)", ncx, ncy, brg::MIN_NC, brg::MAX_NC);
    if (!(d > 0.f) || !(d <= 3.402823466e+38f)) return fail(CRSDR_EINVAL, "caf_beam_steer: d = %g (finite and greater than 0)", (double)d);
    for (int k = 0; k < 2 * nbeams; ++k)
        if (!(xy[k] >= -1.7976931348623157e308 && xy[k] <= 1.7976931348623157e308)) return fail(CRSDR_EINVAL, "caf_beam_steer: a direction is not finite");
    for (int b = 0; b < nbeams; ++b) bm::steer(weights + 2 * (size_t)b * mx * my, mx, my, d, ncx, ncy, xy[2 * b], xy[2 * b + 1]);
    return CRSDR_OK;
}

// ---- the tracker ----
extern "C" int crsdr_caf_set_track(crsdr_caf *q, const crsdr_caf_track_desc *desc)
{
    if (!q) return fail(CRSDR_EINVAL, "caf_set_track: NULL caf");
    trk::Params prm{};
    if (desc) {
        { const int rc_ = track_args_ok("caf_set_track", desc, &prm); if (rc_) return rc_; }
        { const int rc = caf_rules(q, kCafTrack, true); if (rc) return rc; }
        if (prm.source == trk::SRC_FUSED) { const int rc = caf_rules(q, kCafTrackFused, true); if (rc) return rc; }
    }
    { const int rc = caf_clear(q, q->tk, kCafRanTrack); if (rc || !desc) return rc; }
    const size_t T = (size_t)prm.max_tracks, sb = trk::state_bytes(prm.max_tracks);
    crsdr_caf::Track f;
    f.prm = prm; f.on = true;
    int r = CRSDR_OK;
    if ((r = f.state.alloc(sb)) || (r = f.trk.alloc(q->lines() * T * trk::REC)) || (r = f.ntrk.alloc(q->lines() * 4)) || (r = HIP_RC(hipMemset(f.state.p, 0, sb)))) return r;
    q->tk = std::move(f);
    return CRSDR_OK;
}

extern "C" int crsdr_caf_track_reset(crsdr_caf *q)
{
    if (!q) return fail(CRSDR_EINVAL, "caf_track_reset: NULL caf");
    if (!q->tk.on) return fail(CRSDR_ESTATE, "caf_track_reset: no tracker set (crsdr_caf_set_track)");
    { const int rc = caf_quiesce(q); if (rc) return rc; }     // the last submit may still write the state
    HIP_TRY(hipMemset(q->tk.state.p, 0, trk::state_bytes(q->tk.prm.max_tracks)));
    return CRSDR_OK;
}

extern "C" int crsdr_caf_fetch_track(crsdr_caf *q, float *out, int32_t *nout)
{
    if (!q) return fail(CRSDR_EINVAL, "caf_fetch_track: NULL caf");
    if (!q->tk.on) return fail(CRSDR_ESTATE, "caf_fetch_track: no tracker set (crsdr_caf_set_track)");
    if (!(q->last.ran & kCafRanTrack)) return fail(CRSDR_ESTATE, "caf_fetch_track: nothing submitted since the tracker was set");
    const size_t lines = (size_t)q->last.nest, T = (size_t)q->tk.prm.max_tracks;
    return DevFetch(q->device, q->last.stream).copy(out, q->tk.trk.p, lines * T * trk::REC).copy(nout, q->tk.ntrk.p, lines * 4).wait();
}

extern "C" int crsdr_caf_track_device_buffers(crsdr_caf *q, void **out, void **nout)
{
    if (!q) return fail(CRSDR_EINVAL, "caf_track_device_buffers: NULL caf");
    if (!q->tk.on) return fail(CRSDR_ESTATE, "caf_track_device_buffers: no tracker set (crsdr_caf_set_track)");
    if (out) *out = q->tk.trk;
    if (nout) *nout = q->tk.ntrk;
    return CRSDR_OK;
}

extern "C" int crsdr_track_state_bytes(const crsdr_caf_track_desc *desc, size_t *bytes)
{
    if (!desc || !bytes) return fail(CRSDR_EINVAL, "track_state_bytes: NULL argument");
    trk::Params prm{};
    { const int rc_ = track_args_ok("track_state_bytes", desc, &prm); if (rc_) return rc_; }
    *bytes = trk::state_bytes(prm.max_tracks);
    return CRSDR_OK;
}

extern "C" int crsdr_track(float *out, int32_t *nout, void *state, const float *det, const int32_t *count, const float *aux, int nlines, int K, int nd, int R,
                           const crsdr_caf_track_desc *desc, int mem_kind)
{
    if (!state || !det || !count || !desc || (!out && !nout)) return fail(CRSDR_EINVAL, "track: need state, det, count, a descriptor and at least one of trk, ntrk");
    if (nlines < 1 || nlines > kTrackMaxLines) return fail(CRSDR_EINVAL, "track: nlines = %d (1..%d)", nlines, kTrackMaxLines);
    if (K < 1 || K > trk::MAX_MEAS) return fail(CRSDR_EINVAL, "track: K = %d (1..%d)", K, trk::MAX_MEAS);
    { const int rc_ = caf_shape_ok("track", nd, R, 0, 0, 2); if (rc_) return rc_; }
    trk::Params prm{};
    { const int rc_ = track_args_ok("track", desc, &prm); if (rc_) return rc_; }
    OP_PROLOGUE_MEM("track", mem_kind);
    const size_t L = (size_t)nlines, T = (size_t)prm.max_tracks, db = sizeof(float) * L * (size_t)K * 8, cb = sizeof(int32_t) * L, ab = sizeof(float) * L * (size_t)K * 2;
    const size_t sb = trk::state_bytes(prm.max_tracks), tb = sizeof(float) * L * T * trk::REC, nb = sizeof(int32_t) * L * 4;
    OpStage st(mem_kind);
    const float *d_d = (const float *)st.in(0, det, db, 4);
    const int32_t *d_c = (const int32_t *)st.in(1, count, cb, 4);
    const float *d_a = aux ? (const float *)st.in(2, aux, ab, 4) : nullptr;
    unsigned char *d_s = (unsigned char *)st.in(3, state, sb, 8);
    float *d_t = (float *)st.out(4, out, tb, 4);
    int32_t *d_n = (int32_t *)st.out(5, nout, nb, 4);
    if (st.rc) return st.rc;
    if (st.misaligned) return fail(CRSDR_EINVAL, "track: device det, count, aux, trk and ntrk 4-byte, state 8-byte aligned");
    if (st.spare(4, d_t, tb) || st.spare(5, d_n, nb)) return st.rc;
    { const int rc_ = caf_lds_limits(); if (rc_) return rc_; }
    CafRun r{nullptr};
    { const int rc_ = track_enqueue(r, d_d, (size_t)K * 8, d_c, 1, d_a, d_a ? caf_track::AUX_PAIRS : caf_track::AUX_NONE, nlines, K, nd, R, prm, d_s, d_t, d_n); if (rc_) return rc_; }
    st.back(out, d_t, tb);
    st.back(nout, d_n, nb);
    st.back(state, d_s, sb);
    return st.finish();
}

// ---- the integration across lines ----
static size_t integrate_state_bytes(const crsdr_caf *q, int what, int nbeams)
{
    return (what & integ::ARRAY ? integ::state_bytes(1, q->nd, q->nlags) : 0) + (what & integ::BEAMS ? integ::state_bytes(nbeams, q->nd, q->nlags) : 0);
}

extern "C" int crsdr_caf_set_integrate(crsdr_caf *q, const crsdr_caf_integrate_desc *desc)
{
    if (!q) return fail(CRSDR_EINVAL, "caf_set_integrate: NULL caf");
    { const int rc = caf_rules(q, kCafIntegrate, false); if (rc) return rc; }
    integ::Params prm{};
    if (desc) {
        { const int rc_ = integrate_args_ok("caf_set_integrate", q->nd, desc, true, &prm); if (rc_) return rc_; }
        if (desc->what & integ::BEAMS) { const int rc = caf_rules(q, kCafIntegrateBeams, true); if (rc) return rc; }
        if (desc->what & integ::ARRAY) { const int rc = caf_rules(q, kCafIntegrateArray, false); if (rc) return rc; }
    }
    { const int rc = caf_clear(q, q->ig, kCafRanIntegrate); if (rc || !desc) return rc; }
    const size_t lines = q->lines(), cells = (size_t)q->nd * (size_t)q->nlags, sb = integrate_state_bytes(q, desc->what, q->bb.nb);
    crsdr_caf::Integrate f;
    f.what = desc->what; f.prm = prm; f.on = true;
    int r = CRSDR_OK;
    if ((r = f.state.alloc(sb)) || ((f.what & integ::ARRAY) && (r = f.imap.alloc(lines * cells))) ||
        ((f.what & integ::BEAMS) && (r = f.ibmap.alloc(lines * (size_t)q->bb.nb * cells))) || (r = HIP_RC(hipMemset(f.state.p, 0, sb))))
        return r;
    q->ig = std::move(f);
    return CRSDR_OK;
}

extern "C" int crsdr_caf_integrate_reset(crsdr_caf *q)
{
    if (!q) return fail(CRSDR_EINVAL, "caf_integrate_reset: NULL caf");
    if (!q->ig.on) return fail(CRSDR_ESTATE, "caf_integrate_reset: no integration set (crsdr_caf_set_integrate)");
    { const int rc = caf_quiesce(q); if (rc) return rc; }     // the last submit may still write the state
    HIP_TRY(hipMemset(q->ig.state.p, 0, integrate_state_bytes(q, q->ig.what, q->bb.nb)));
    return CRSDR_OK;
}

extern "C" int crsdr_caf_fetch_integrate(crsdr_caf *q, float *imap, float *ibmap)
{
    if (!q) return fail(CRSDR_EINVAL, "caf_fetch_integrate: NULL caf");
    if (!q->ig.on) return fail(CRSDR_ESTATE, "caf_fetch_integrate: no integration set (crsdr_caf_set_integrate)");
    if (!(q->last.ran & kCafRanIntegrate)) return fail(CRSDR_ESTATE, "caf_fetch_integrate: nothing submitted since the integration was set");
    if (imap && !q->ig.array()) return fail(CRSDR_ESTATE, "caf_fetch_integrate: the array map is not integrated (CRSDR_INTEGRATE_ARRAY)");
    if (ibmap && !q->ig.beams()) return fail(CRSDR_ESTATE, "caf_fetch_integrate: the beam maps are not integrated (CRSDR_INTEGRATE_BEAMS)");
    const size_t lines = (size_t)q->last.nest, cells = (size_t)q->nd * (size_t)q->nlags;
    return DevFetch(q->device, q->last.stream).copy(imap, q->ig.imap.p, lines * cells).copy(ibmap, q->ig.ibmap.p, lines * (size_t)q->bb.nb * cells).wait();
}

extern "C" int crsdr_caf_integrate_device_buffers(crsdr_caf *q, void **imap, void **ibmap, void **state)
{
    if (!q) return fail(CRSDR_EINVAL, "caf_integrate_device_buffers: NULL caf");
    if (!q->ig.on) return fail(CRSDR_ESTATE, "caf_integrate_device_buffers: no integration set (crsdr_caf_set_integrate)");
    if (imap) *imap = q->ig.imap;
    if (ibmap) *ibmap = q->ig.ibmap;
    if (state) *state = q->ig.state;
    return CRSDR_OK;
}

constexpr long long kIntegrateMaxCells = 1ll << 26;     // crsdr_map_integrate: nlines * nmaps * nd * R

static int map_integrate_shape_ok(const char *who, int nmaps, int nd, int R)
{
    { const int rc_ = caf_shape_ok(who, nd, R, 0, 0, 2); if (rc_) return rc_; }
    if (nmaps < 1 || (long long)nmaps * nd * R > kCafMaxCells) return fail(CRSDR_EINVAL, "%s: nmaps = %d (at least 1, nmaps * nd * R at most 2^24)", who, nmaps);
    return CRSDR_OK;
}

extern "C" int crsdr_map_integrate_state_bytes(int nmaps, int nd, int R, size_t *bytes)
{
    if (!bytes) return fail(CRSDR_EINVAL, "map_integrate_state_bytes: NULL bytes");
    { const int rc_ = map_integrate_shape_ok("map_integrate_state_bytes", nmaps, nd, R); if (rc_) return rc_; }
    *bytes = integ::state_bytes(nmaps, nd, R);
    return CRSDR_OK;
}

extern "C" int crsdr_map_integrate(float *imap, void *state, const float *maps, int nlines, int nmaps, int nd, int R, const crsdr_caf_integrate_desc *desc, int mem_kind)
{
    if (!imap || !state || !maps || !desc) return fail(CRSDR_EINVAL, "map_integrate: need imap, state, maps and a descriptor");
    if (nlines < 1 || nlines > kTrackMaxLines) return fail(CRSDR_EINVAL, "map_integrate: nlines = %d (1..%d)", nlines, kTrackMaxLines);
    { const int rc_ = map_integrate_shape_ok("map_integrate", nmaps, nd, R); if (rc_) return rc_; }
    if ((long long)nlines * nmaps * nd * R > kIntegrateMaxCells) return fail(CRSDR_EINVAL, "map_integrate: nlines * nmaps * nd * R = %lld (at most 2^26)", (long long)nlines * nmaps * nd * R);
    integ::Params prm{};
    { const int rc_ = integrate_args_ok("map_integrate", nd, desc, false, &prm); if (rc_) return rc_; }
    OP_PROLOGUE_MEM("map_integrate", mem_kind);
    const size_t mb = sizeof(float) * (size_t)nlines * (size_t)nmaps * (size_t)nd * (size_t)R, sb = integ::state_bytes(nmaps, nd, R);
    OpStage st(mem_kind);
    const float *d_m = (const float *)st.in(0, maps, mb, 4);
    unsigned char *d_s = (unsigned char *)st.in(1, state, sb, 8);
    float *d_i = (float *)st.out(2, imap, mb, 4);
    if (st.rc) return st.rc;
    if (st.misaligned) return fail(CRSDR_EINVAL, "map_integrate: device maps and imap 4-byte, state 8-byte aligned");
    CafRun r{nullptr};
    { const int rc_ = integrate_enqueue(r, d_m, nlines, nmaps, nd, R, prm, d_s, d_i); if (rc_) return rc_; }
    st.back(imap, d_i, mb);
    st.back(state, d_s, sb);
    return st.finish();
}

// ---- the canceller ----
extern "C" int crsdr_caf_set_cancel(crsdr_caf *q, const crsdr_caf_cancel_desc *desc)
{
    if (!q) return fail(CRSDR_EINVAL, "caf_set_cancel: NULL caf");
    { const int rc = caf_rules(q, kCafCancel, false); if (rc) return rc; }
    const size_t lines = q->lines();
    if (desc) { const int rc_ = cancel_args_ok("caf_set_cancel", q->nd, q->nlags, (long long)lines, desc); if (rc_) return rc_; }
    { const int rc = caf_clear(q, q->cn, kCafRanCancel); if (rc || !desc) return rc; }
    const size_t K = (size_t)desc->taps, P = (size_t)desc->dopp, n = K * (2 * P + 1), rows = lines * (size_t)q->nrows, nd = (size_t)q->nd;
    crsdr_caf::Cancel f;
    f.taps = desc->taps; f.dopp = desc->dopp; f.on = true;
    CafRun table{q->own.s};
    int r = CRSDR_OK;
    if ((r = f.G.alloc(lines * nd * K * (size_t)q->nlags)) || (r = f.Y.alloc(rows * nd * K)) || (r = f.ph.alloc(nd)) || (r = f.S.alloc(lines * (4 * P + 1) * K * K)) ||
        (r = f.C.alloc(rows * n)) || (r = f.W.alloc(rows * n)) || (r = f.h.alloc(rows * n)) || (r = f.E.alloc(rows)) || (r = f.status.alloc(lines)) ||
        (r = f.coef.alloc(rows * n * 2)) || (r = f.cinfo.alloc(rows * 2)) || (r = cancel_table(table, q->nd, f.ph)) || (r = HIP_RC(hipStreamSynchronize(q->own.s))))
        return r;
    q->cn = std::move(f);
    return CRSDR_OK;
}

extern "C" int crsdr_caf_fetch_cancel(crsdr_caf *q, float *coef, float *cinfo)
{
    if (!q) return fail(CRSDR_EINVAL, "caf_fetch_cancel: NULL caf");
    if (!q->cn.on) return fail(CRSDR_ESTATE, "caf_fetch_cancel: no canceller set (crsdr_caf_set_cancel)");
    if (!(q->last.ran & kCafRanCancel)) return fail(CRSDR_ESTATE, "caf_fetch_cancel: nothing submitted since the canceller was set");
    const size_t rows = (size_t)q->last.nest * (size_t)q->nrows, n = (size_t)cc::basis(q->cn.taps, q->cn.dopp);
    return DevFetch(q->device, q->last.stream).copy(coef, q->cn.coef.p, rows * n * 2).copy(cinfo, q->cn.cinfo.p, rows * 2).wait();
}

extern "C" int crsdr_caf_cancel_device_buffers(crsdr_caf *q, void **coef, void **cinfo)
{
    if (!q) return fail(CRSDR_EINVAL, "caf_cancel_device_buffers: NULL caf");
    if (!q->cn.on) return fail(CRSDR_ESTATE, "caf_cancel_device_buffers: no canceller set (crsdr_caf_set_cancel)");
    if (coef) *coef = q->cn.coef;
    if (cinfo) *cinfo = q->cn.cinfo;
    return CRSDR_OK;
}

// crsdr_ambiguity (cd = NULL) and crsdr_ambiguity_cancel
static int ambiguity(float *chi, float *map, float *peak, const int8_t *matrix, int nrows, int blocksize, int seg, int nlags, int ref_row, int window, int guard, int mem_kind,
                     const crsdr_caf_cancel_desc *cd, float *coef, float *cinfo)
{
    if (!matrix || (!chi && !map && !peak && !coef && !cinfo)) return fail(CRSDR_EINVAL, "ambiguity: need matrix and at least one output");
    { const int rc_ = caf_args_ok("ambiguity", nrows, blocksize, 1, 1, seg, nlags, ref_row, window, guard); if (rc_) return rc_; }
    if (cd) { const int rc_ = cancel_args_ok("ambiguity_cancel", blocksize / (2 * seg), nlags, 1, cd); if (rc_) return rc_; }
    OP_PROLOGUE_MEM("ambiguity", mem_kind);
    const size_t nd = (size_t)(blocksize / (2 * seg)), cells = nd * (size_t)nlags, mb = (size_t)nrows * (size_t)blocksize;
    const size_t cb = sizeof(float2) * (size_t)nrows * cells, pb = sizeof(float) * cells, kb = sizeof(float) * 6 * (size_t)(nrows + 1);
    OpStage st(mem_kind);
    const int8_t *d_m = (const int8_t *)st.in(0, matrix, mb, 4);
    float2 *d_c = (float2 *)st.out(1, chi, cb, 8);
    float *d_p = (float *)st.out(2, map, pb, 4);
    float *d_k = (float *)st.out(3, peak, kb, 4);
    const size_t K = cd ? (size_t)cd->taps : 0, P = cd ? (size_t)cd->dopp : 0, n = K * (2 * P + 1), fb = sizeof(float) * 2 * (size_t)nrows * n, ib = sizeof(float) * 2 * (size_t)nrows;
    float *d_f = cd ? (float *)st.out(5, coef, fb, 4) : nullptr, *d_i = cd ? (float *)st.out(6, cinfo, ib, 4) : nullptr;
    if (st.rc) return st.rc;
    if (st.misaligned) return fail(CRSDR_EINVAL, "ambiguity: device matrix, map, peak, coef and cinfo 4-byte, chi 8-byte aligned");
    if (st.spare(1, d_c, cb) || st.spare(2, d_p, pb) || st.spare(3, d_k, kb)) return st.rc;
    OP_RESERVE(4, sizeof(float2) * nd + sizeof(float) * nd);
    float2 *tw = (float2 *)g_op.buf[4];
    float *win = (float *)(tw + nd);
    { const int rc_ = spectra_tables(0, (int)nd, window, tw, win); if (rc_) return rc_; }
    CafRun r{nullptr};
    CancelBufs c;
    if (cd) {
        if (st.spare(5, d_f, fb) || st.spare(6, d_i, ib)) return st.rc;
        // one slot for the rest, the 16-byte types first
        const size_t nph = nd, nS = (4 * P + 1) * K * K, nC = (size_t)nrows * n, nG = nd * K * (size_t)nlags, nY = (size_t)nrows * nd * K;
        OP_RESERVE(7, sizeof(double2) * (nph + nS + 3 * nC) + sizeof(long long) * (size_t)nrows + sizeof(int2) * (nG + nY) + sizeof(int));
        c.taps = cd->taps; c.dopp = cd->dopp;
        c.ph = (double2 *)g_op.buf[7]; c.S = c.ph + nph; c.C = c.S + nS; c.W = c.C + nC; c.h = c.W + nC;
        c.E = (long long *)(c.h + nC); c.G = (int2 *)(c.E + nrows); c.Y = c.G + nG; c.status = (int *)(c.Y + nY);
        c.coef = d_f; c.cinfo = d_i;
        { const int rc_ = cancel_table(r, (int)nd, c.ph); if (rc_) return rc_; }
    }
    { const int rc_ = caf_enqueue(r, d_m, mb, 0, 1, nrows, blocksize, 1, seg, nlags, ref_row, window, guard, tw, win, d_c, d_p, d_k, cd ? &c : nullptr); if (rc_) return rc_; }
    st.back(coef, d_f, fb);
    st.back(cinfo, d_i, ib);
    st.back(chi, d_c, cb);
    st.back(map, d_p, pb);
    st.back(peak, d_k, kb);
    return st.finish();
}

extern "C" int crsdr_ambiguity(float *chi, float *map, float *peak, const int8_t *matrix, int nrows, int blocksize, int seg, int nlags, int ref_row, int window, int guard,
                               int mem_kind)
{
    return ambiguity(chi, map, peak, matrix, nrows, blocksize, seg, nlags, ref_row, window, guard, mem_kind, nullptr, nullptr, nullptr);
}

extern "C" int crsdr_ambiguity_cancel(float *chi, float *map, float *peak, const int8_t *matrix, int nrows, int blocksize, int seg, int nlags, int ref_row, int window,
                                      int guard, int mem_kind, int taps, int dopp, float *coef, float *cinfo)
{
    const crsdr_caf_cancel_desc cd{taps, dopp};
    return ambiguity(chi, map, peak, matrix, nrows, blocksize, seg, nlags, ref_row, window, guard, mem_kind, &cd, coef, cinfo);
}

// ---- the second stage ----
// every limit of the cleaning of section (w), for crsdr_caf_set_clean and crsdr_ambiguity_clean.  taps, dopp: the canceller's
static int clean_args_ok(const char *who, int nd, int nlags, long long lines, int nrows, int taps, int dopp, const crsdr_caf_clean_desc *d, cl::Params *prm)
{
    *prm = cl::Params{d->max_targets, d->min_snr, d->wl, d->wq};
    switch (cl::bad_limit(nd, nlags, lines, nrows, taps, dopp, *prm)) {
    case 0: return CRSDR_OK;
    case 1: return fail(CRSDR_EINVAL, "%s: max_targets = %d (1..%d)", who, d->max_targets, cl::MAX_TARGETS);
    case 2: return fail(CRSDR_EINVAL, "%s: wl = %d (0..%d)", who, d->wl, cl::MAX_WL);
    case 3: return fail(CRSDR_EINVAL, "%s: wq = %d (0..%d)", who, d->wq, cl::MAX_WQ);
    case 4: return fail(CRSDR_EINVAL, "%s: taps (2 dopp + 1) + max_targets (2 wl + 1)(2 wq + 1) = %d (at most %d)", who, cc::basis(taps, dopp) + cl::max_target_members(*prm),
                        cl::MAX_MEMBERS);
    case 5: return fail(CRSDR_EINVAL, "%s: min_snr = %g (finite and greater than 0)", who, (double)d->min_snr);
    case 6: return fail(CRSDR_EINVAL, "%s: (max_batch / frames) * nd * (taps + max_targets (2 wl + 1)) * nlags = %lld (at most 2^24)", who,
                        lines * nd * (taps + cl::max_slots(*prm)) * nlags);
    default: return fail(CRSDR_EINVAL, "%s: 2 * (max_batch / frames) * nrows * nd * nlags = %lld (at most 2^24: chi and the residual's)", who, 2 * lines * nrows * nd * nlags);
    }
}

extern "C" int crsdr_caf_set_clean(crsdr_caf *q, const crsdr_caf_clean_desc *desc)
{
    if (!q) return fail(CRSDR_EINVAL, "caf_set_clean: NULL caf");
    const size_t lines = q->lines();
    cl::Params prm{};
    if (desc) {
        { const int rc = caf_rules(q, kCafClean, false); if (rc) return rc; }         // (turning it off is never refused)
        // (the canceller off: the limits that need its basis are checked with one member, and the call is refused for the state below)
        const int rc_ = clean_args_ok("caf_set_clean", q->nd, q->nlags, (long long)lines, q->nrows, q->cn.on ? q->cn.taps : 1, q->cn.on ? q->cn.dopp : 0, desc, &prm);
        if (rc_) return rc_;
        { const int rc = caf_rules(q, kCafClean, true); if (rc) return rc; }
    }
    { const int rc = caf_clear(q, q->cl_, kCafRanClean); if (rc || !desc) return rc; }
    const size_t rows = lines * (size_t)q->nrows, nd = (size_t)q->nd, R = (size_t)q->nlags, cells = nd * R, Kd = (size_t)q->cf.prm.max_det, T = (size_t)prm.max_targets;
    crsdr_caf::Clean f;
    f.prm = prm; f.n2max = cl::max_target_members(prm); f.nmax = cc::basis(q->cn.taps, q->cn.dopp) + f.n2max; f.slots = cl::slots_of(prm, q->nlags); f.on = true;
    const size_t n2 = (size_t)f.n2max, nm = (size_t)f.nmax, sl = (size_t)f.slots, maps = lines * (size_t)(q->nrows + 1);
    int r = CRSDR_OK;
    if ((r = f.tab.alloc(lines)) || (r = f.G2.alloc(lines * nd * sl * R)) || (r = f.Y2.alloc(rows * nd * sl)) || (r = f.ph2.alloc(lines * n2 * nd)) ||
        (r = f.A2.alloc(lines * n2 * nm)) || (r = f.C2.alloc(rows * n2)) || (r = f.Wj.alloc(rows * 2 * nm)) || (r = f.hj.alloc(rows * nm)) || (r = f.jstat.alloc(lines)) ||
        (r = f.tgt.alloc(lines * T * 8)) || (r = f.ntgt.alloc(lines)) || (r = f.tcoef.alloc(rows * n2 * 2)) || (r = f.tinfo.alloc(rows * 2)) ||
        (r = f.rchi.alloc(rows * cells)) || (r = f.rmap.alloc(lines * cells)) || (r = f.rdet.alloc(maps * Kd * 8)) || (r = f.rcount.alloc(maps)) ||
        (r = f.rsnap.alloc(lines * Kd * (size_t)q->nrows * 2)))
        return r;
    q->cl_ = std::move(f);
    return CRSDR_OK;
}

extern "C" int crsdr_caf_fetch_clean(crsdr_caf *q, float *tgt, int32_t *ntgt, float *tcoef, float *tinfo, float *rchi, float *rmap, float *rdet, int32_t *rcount,
                                     float *rsnap)
{
    if (!q) return fail(CRSDR_EINVAL, "caf_fetch_clean: NULL caf");
    const crsdr_caf::Clean &c = q->cl_;
    if (!c.on) return fail(CRSDR_ESTATE, "caf_fetch_clean: no cleaning set (crsdr_caf_set_clean)");
    if (!(q->last.ran & kCafRanClean)) return fail(CRSDR_ESTATE, "caf_fetch_clean: nothing submitted since the cleaning was set");
    const size_t lines = (size_t)q->last.nest, rows = lines * (size_t)q->nrows, cells = (size_t)q->nd * (size_t)q->nlags, maps = lines * (size_t)(q->nrows + 1);
    const size_t Kd = (size_t)q->cf.prm.max_det;
    return DevFetch(q->device, q->last.stream).copy(tgt, c.tgt.p, lines * (size_t)c.prm.max_targets * 8).copy(ntgt, c.ntgt.p, lines)
        .copy(tcoef, c.tcoef.p, rows * (size_t)c.n2max * 2).copy(tinfo, c.tinfo.p, rows * 2).copy(rchi, c.rchi.p, rows * cells).copy(rmap, c.rmap.p, lines * cells)
        .copy(rdet, c.rdet.p, maps * Kd * 8).copy(rcount, c.rcount.p, maps).copy(rsnap, c.rsnap.p, lines * Kd * (size_t)q->nrows * 2).wait();
}

extern "C" int crsdr_caf_clean_device_buffers(crsdr_caf *q, void **tgt, void **ntgt, void **tcoef, void **tinfo, void **rchi, void **rmap, void **rdet, void **rcount,
                                              void **rsnap)
{
    if (!q) return fail(CRSDR_EINVAL, "caf_clean_device_buffers: NULL caf");
    const crsdr_caf::Clean &c = q->cl_;
    if (!c.on) return fail(CRSDR_ESTATE, "caf_clean_device_buffers: no cleaning set (crsdr_caf_set_clean)");
    if (tgt) *tgt = c.tgt;
    if (ntgt) *ntgt = c.ntgt;
    if (tcoef) *tcoef = c.tcoef;
    if (tinfo) *tinfo = c.tinfo;
    if (rchi) *rchi = c.rchi;
    if (rmap) *rmap = c.rmap;
    if (rdet) *rdet = c.rdet;
    if (rcount) *rcount = c.rcount;
    if (rsnap) *rsnap = c.rsnap;
    return CRSDR_OK;
}

// The per-op form: a one-line engine made for the call, on the current device -- the engine's stages, so the same kernels on the same
// arguments.  Every check of the four descriptors comes before a device is touched.
extern "C" int crsdr_ambiguity_clean(const crsdr_clean_out *out, const int8_t *matrix, int nrows, int blocksize, int seg, int nlags, int ref_row, int window, int guard,
                                     int mem_kind, const crsdr_caf_cancel_desc *cancel, const crsdr_cfar_desc *cfar, const crsdr_cfar_est_desc *est,
                                     const crsdr_caf_clean_desc *clean)
{
    if (!out || !matrix || !cancel || !cfar || !clean) return fail(CRSDR_EINVAL, "ambiguity_clean: need out, matrix, and the canceller's, the detector's and the cleaning's descriptors");
    { const int rc_ = caf_args_ok("ambiguity_clean", nrows, blocksize, 1, 1, seg, nlags, ref_row, window, guard); if (rc_) return rc_; }
    const int nd = blocksize / (2 * seg);
    cfar::Params cp{};
    cl::Params lp{};
    { const int rc_ = cancel_args_ok("ambiguity_clean", nd, nlags, 1, cancel); if (rc_) return rc_; }
    { const int rc_ = cfar_args_ok("ambiguity_clean", nd, cfar, &cp); if (rc_) return rc_; }
    { const int rc_ = cfar_est_ok("ambiguity_clean", est, &cp); if (rc_) return rc_; }
    { const int rc_ = clean_args_ok("ambiguity_clean", nd, nlags, 1, nrows, cancel->taps, cancel->dopp, clean, &lp); if (rc_) return rc_; }
    if (mem_kind != CRSDR_MEM_HOST && mem_kind != CRSDR_MEM_DEVICE) return fail(CRSDR_EINVAL, "ambiguity_clean: mem_kind = %d", mem_kind);
    const bool host = mem_kind == CRSDR_MEM_HOST;
    if (!host) {
        const void *p4[] = {matrix, out->map, out->peak, out->coef, out->cinfo, out->det, out->count, out->snap, out->tgt, out->ntgt, out->tcoef, out->tinfo, out->rmap,
                            out->rdet, out->rcount, out->rsnap};
        bool mis = (uintptr_t)out->chi % 8 != 0 || (uintptr_t)out->rchi % 8 != 0;
        for (const void *p : p4) mis |= (uintptr_t)p % 4 != 0;
        if (mis) return fail(CRSDR_EINVAL, "ambiguity_clean: device pointers 4-byte, chi and rchi 8-byte aligned");
    }
    { const int rc_ = require_device(); if (rc_) return rc_; }
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    const crsdr_caf_desc cd{nrows, blocksize, dev, 1, 1, seg, nlags, ref_row, window, guard};
    crsdr_caf *q = nullptr;
    int rc = crsdr_caf_create(&q, &cd);
    if (rc) return rc;
    DevBuf<int8_t> staged;
    const size_t mb = (size_t)nrows * (size_t)blocksize;
    if (!(rc = crsdr_caf_set_cancel(q, cancel)) && !(rc = crsdr_caf_set_cfar(q, cfar)) && !(rc = est ? crsdr_caf_set_cfar_estimator(q, est) : CRSDR_OK) &&
        !(rc = crsdr_caf_set_clean(q, clean)) && !(rc = host ? staged.alloc(mb) : CRSDR_OK) &&
        !(rc = host ? HIP_RC(hipMemcpy(staged.p, matrix, mb, hipMemcpyHostToDevice)) : CRSDR_OK) &&
        !(rc = crsdr_caf_submit(q, host ? staged.p : matrix, mb, 0, 1, nullptr)) && !(rc = HIP_RC(hipStreamSynchronize(q->own.s)))) {
        const size_t cells = (size_t)nd * (size_t)nlags, n1 = (size_t)cc::basis(cancel->taps, cancel->dopp), Kd = (size_t)cp.max_det, r = (size_t)nrows;
        const crsdr_caf::Clean &c = q->cl_;
        const struct { void *dst; const void *src; size_t bytes; } copies[] = {
            {out->chi, q->chi.p, 8 * r * cells}, {out->map, q->map.p, 4 * cells}, {out->peak, q->peak.p, 4 * (r + 1) * 6}, {out->coef, q->cn.coef.p, 8 * r * n1},
            {out->cinfo, q->cn.cinfo.p, 8 * r}, {out->det, q->cf.det.p, 4 * (r + 1) * Kd * 8}, {out->count, q->cf.count.p, 4 * (r + 1)}, {out->snap, q->cf.snap.p, 8 * Kd * r},
            {out->tgt, c.tgt.p, 4 * (size_t)lp.max_targets * 8}, {out->ntgt, c.ntgt.p, 4}, {out->tcoef, c.tcoef.p, 8 * r * (size_t)c.n2max}, {out->tinfo, c.tinfo.p, 8 * r},
            {out->rchi, c.rchi.p, 8 * r * cells}, {out->rmap, c.rmap.p, 4 * cells}, {out->rdet, c.rdet.p, 4 * (r + 1) * Kd * 8}, {out->rcount, c.rcount.p, 4 * (r + 1)},
            {out->rsnap, c.rsnap.p, 8 * Kd * r}};
        for (const auto &cp_ : copies)
            if (cp_.dst && !rc) rc = HIP_RC(hipMemcpy(cp_.dst, cp_.src, cp_.bytes, host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice));
    }
    caf_free(q);
    return rc;
}
