// doa_engine.hpp -- the crsdr_doa object behind include/crsdr.h.  Part of crsdr.hip's translation unit: included there behind the plan
// (crsdr_doa_submit_plan reads one) and ahead of the per-op calls on the same kernels.
// (iv) batched direction-of-arrival engine (crsdr_doa): covariance -> noise subspace -> 2-D MUSIC scan + peak, one estimate per
//      `frames` packets, for a whole batch of packets where a plan left them.  Every buffer is allocated at create; a submit is five
//      launches on one stream whatever the batch size (covariance partials, their reducer, subspace, scan, peak), no lock, no
//      allocation, no synchronisation.  crsdr_doa_set_peaks allocates what the local-peak pass needs and adds its two launches,
//      crsdr_doa_set_beams what the beams need and theirs (beams.hpp), crsdr_doa_set_smoothing and crsdr_doa_set_order theirs and one
//      launch each (smooth.hpp): behind the reducer, and between the subspace and the scan.  crsdr_doa_set_subbands replaces the two
//      covariance launches by subband.hpp's (one covariance per estimate and frequency band) and reallocates every per-matrix buffer
//      for (max_batch / frames) * nbands matrices: the launches behind it then run over that many.  crsdr_doa_set_subband_beams on top of
//      it: the beam weights per (estimate, band) and subband_beams.hpp's apply kernel on the rows' band spectra.  crsdr_doa_set_spectrum
//      replaces the scan's kernel by spectrum.hpp's (the Bartlett or the Capon map): the same launches, nothing allocated.
//      crsdr_doa_set_refine adds refine.hpp's launch behind the directions and ahead of the beams, which then steer off the grid.
//      crsdr_doa_set_esprit adds esprit.hpp's launch between the source count and the scan (BESIDE), or puts it in the place of the
//      scan, the peak, the local peaks and the refinement (ONLY).  crsdr_doa_set_augment puts augment.hpp's launch where smoothing's
//      would be: the covariance of a filled virtual array from the receivers that are present.
//
// Shape of the host code.  A feature is a sub-struct of crsdr_doa: its parameters and its device buffers, each buffer owned by a
// DevBuf, so that "off" is an assignment of {} and nothing is freed by a list kept by hand.  What the last submit left (DoaLast) is
// written once by doa_launch; every fetch reads its state from there and copies through DevFetch.  A submit is doa_launch's stages.
#pragma once

// `launch` with NB = the apply kernel's slot count for nbeams (1, 2, 4, 8 or 16)
#define BEAMS_DISPATCH(nbeams, launch)                                              \
    switch (beams::slots_for(nbeams)) {                                             \
    case 1: { constexpr int NB = 1; launch; } break;                                \
    case 2: { constexpr int NB = 2; launch; } break;                                \
    case 4: { constexpr int NB = 4; launch; } break;                                \
    case 8: { constexpr int NB = 8; launch; } break;                                \
    default: { constexpr int NB = 16; launch; } break;                              \
    }

// `launch` with LG = log2 nfft
#define SUBBAND_DISPATCH(lg, launch)                                                \
    switch (lg) {                                                                   \
    case 3: { constexpr int LG = 3; launch; } break;                                \
    case 4: { constexpr int LG = 4; launch; } break;                                \
    case 5: { constexpr int LG = 5; launch; } break;                                \
    case 6: { constexpr int LG = 6; launch; } break;                                \
    case 7: { constexpr int LG = 7; launch; } break;                                \
    default: { constexpr int LG = 8; launch; } break;                               \
    }

// owning device buffer: freed on reset(), on assignment and with its owner
template <typename T>
struct DevBuf {
    T *p = nullptr;
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept : p(o.p) { o.p = nullptr; }
    DevBuf &operator=(DevBuf &&o) noexcept { if (this != &o) { reset(); p = o.p; o.p = nullptr; } return *this; }
    ~DevBuf() { reset(); }
    int alloc(size_t count) { reset(); HIP_TRY(hipMalloc((void **)&p, sizeof(T) * count)); return CRSDR_OK; }
    void reset() { if (p) (void)hipFree(p); p = nullptr; }
    operator T *() const { return p; }
};
// the object's own stream.  crsdr_doa's first member, so destroyed after every buffer
struct DoaStream {
    hipStream_t s = nullptr;
    ~DoaStream() { if (s) (void)hipStreamDestroy(s); }
};
// The frame of every engine's fetch, behind its own state checks: the object's device, copies on the last submit's stream for the host
// pointers that are not NULL, one wait.  The first failure is the answer; the calls behind it do nothing.
struct DevFetch {
    hipStream_t S;
    int rc;
    DevFetch(int device, hipStream_t stream) : S(stream), rc(HIP_RC(hipSetDevice(device))) {}
    template <typename T>
    DevFetch &copy(void *host, const T *dev, size_t count)
    {
        if (host && !rc) rc = HIP_RC(hipMemcpyAsync(host, dev, sizeof(T) * count, hipMemcpyDeviceToHost, S));
        return *this;
    }
    int wait() { return rc ? rc : HIP_RC(hipStreamSynchronize(S)); }
};

// the buffers with one entry per matrix (estimate, or estimate and band)
struct DoaMatrices {
    DevBuf<int> info;
    DevBuf<float2> rxx, vec;
    DevBuf<float> sv, peakv, pm;                 // pm: only with CRSDR_DOA_KEEP_SPECTRUM
    DevBuf<int32_t> peak;
    DevBuf<unsigned long long> wgbest;
};
// crsdr_doa_set_subbands: nfft (0 = off), the bands (first, nbands, width; nbands = 1 while off: every buffer behind the covariance
// holds (max_batch / frames) * nbands matrices either way), the window, K slices per packet, unit groups, the slices' partials
// [nest][frames * spb][subband_partial] and the bands' power [nest][nbands]
struct DoaSubbands {
    int nfft = 0, log2 = 0, first = 0, nbands = 1, width = 0, window = 0, spb = 1, groups = 1;
    DevBuf<float2> partial;
    DevBuf<float> power;
};
// crsdr_doa_set_peaks: `count` directions per estimate (0 = off), window radius, the spectrum workspace (without
// CRSDR_DOA_KEEP_SPECTRUM), the tiles' candidates [nest][tiles][count] and the results
struct DoaPeaks {
    int count = 0, radius = 0, tiles = 0;
    DevBuf<float> pmws, values;
    DevBuf<unsigned long long> cand;
    DevBuf<int32_t> found, dirs;
};
// crsdr_doa_set_beams: mode (0 = off), `nbeams` slots per estimate (nfixed of them at the caller's angles, else the estimate's own
// directions), weights [nest][nbeams][m], power [nest][nbeams], beams [max_batch][nbeams][B / 2].
// crsdr_doa_set_subband_beams: the same fields and buffers (the two kinds of beams exclude each other: one needs subbands off, the
// other on) with `band` set: weights [nest * nbands][nbeams][m], power [nest * nbands][nbeams], beams
// [max_batch][nbands][nbeams][J][width]; lds_points: float2 of dynamic LDS of the apply kernel
struct DoaBeams {
    int mode = 0, nbeams = 0, nfixed = 0, lds_points = 0;
    float loading = 0.f;
    bool band = false;
    DevBuf<float2> weights, beams;
    DevBuf<float> power, angles;
};
// crsdr_doa_set_smoothing: sub-arrays of sx x sy elements, the smoothed covariances [nest][sx sy][sx sy]
struct DoaSmooth {
    bool on = false;
    int sx = 0, sy = 0;
    uint32_t flags = 0;
    DevBuf<float2> rs;
};
// crsdr_doa_set_augment: a virtual array of vx x vy elements from the elements of `mask` (0 = all), the augmented covariances
// [nmat][vx vy][vx vy]
struct DoaAugment {
    bool on = false;
    int vx = 0, vy = 0;
    uint64_t mask = 0;
    DevBuf<float2> ra;
};
// crsdr_doa_set_order: criterion (0 = off), the candidates kmin .. kmax, whether the directions are capped by the count;
// k [nest], criterion values [nest][kmax - kmin + 1]
struct DoaOrder {
    int crit = 0, kmin = 0, kmax = 0, limit_dirs = 0;
    DevBuf<int32_t> k;
    DevBuf<float> values;
};
// crsdr_doa_set_refine: levels of the zoom search (0 = off); offsets and angles [nmat][slots][2], values [nmat][slots], slots = the
// directions of set_peaks or the one peak.  Allocated for the most matrices and slots there can be: no other setter resizes them
struct DoaRefine {
    int levels = 0;
    DevBuf<float> offsets, angles, values;
};
// crsdr_doa_set_esprit: mode (0 = off); found, status [nmat]; phases, angles, modulus [nmat][slots][2]; power, flags [nmat][slots],
// slots = k, or kmax with the source count on.  Allocated for the most matrices and slots there can be: no other setter resizes them
struct DoaEsprit {
    int mode = 0;
    DevBuf<int32_t> found, status, flags;
    DevBuf<double> phases;
    DevBuf<float> angles, modulus, power;
};
// what the last submit left: where, how much, and which features ran (kRan*).  A setter clears its feature's bit: "nothing submitted
// since"; without kRanBase nothing is left at all
constexpr unsigned kRanBase = 1u, kRanPeaks = 2u, kRanBeams = 4u, kRanSmooth = 8u, kRanOrder = 16u, kRanRefine = 32u, kRanEsprit = 64u, kRanScan = 128u, kRanAugment = 256u;
struct DoaLast {
    hipStream_t stream = nullptr;
    int nest = 0, nblocks = 0, ms = 0, launches = 0;
    unsigned ran = 0;
    int slots = 0;               // refined directions per matrix (the layout of that submit, whatever set_peaks says since)
    int eslots = 0;              // ESPRIT slots per matrix, likewise
};

struct crsdr_doa {
    DoaStream own;
    int nrows = 0, B = 0, m = 0, device = 0, max_batch = 1, frames = 1, k = 1, mx = 0, my = 0, ncx = 0, ncy = 0;
    float d = 0.f;
    uint32_t flags = 0;
    int nt = 1, ntri = 1, spb = 1, nwg = 0;        // operand blocks, tiles, K slices per packet, scan workgroups per estimate
    DevBuf<int> partial;                           // the plain covariance's partial sums and row sums
    DevBuf<int2> psum;
    DoaMatrices mat;
    DoaSubbands sub;
    DoaPeaks peaks;
    DoaBeams beams;
    DoaSmooth smooth;
    DoaAugment augment;
    DoaOrder order;
    DoaRefine refine;
    DoaEsprit esprit;
    int spectrum = CRSDR_SPECTRUM_MUSIC;           // crsdr_doa_set_spectrum: the map the scan computes, and CAPON's loading
    float spectrum_loading = 0.f;
    DoaLast last;
    // what the subspace, the order, the scan and the peaks work on: the virtual array while augmentation is on, the sub-arrays while
    // smoothing is (the two exclude each other), the array otherwise
    int sx() const { return augment.on ? augment.vx : smooth.on ? smooth.sx : mx; }
    int sy() const { return augment.on ? augment.vy : smooth.on ? smooth.sy : my; }
    int ms() const { return sx() * sy(); }
};
constexpr int kMaxDoaMatrices = 4096;      // (max_batch / frames) * nbands

static int doa_lds_limits();               // (behind the stages, which name the kernels it covers)
// refine.hpp's kernel is reached through these two, defined at the end of the translation unit: its first use lies behind every other
// kernel's, so the kernels ahead of it keep their order in the code object (see below)
static const void *doa_refine_kernel();
static void doa_refine_enqueue(dim3 grid, hipStream_t S, const float2 *vec, const float *sv, int M, int kind, int k, const int32_t *korder, float loading, float d, int Mx,
                               int Cx, int Cy, const int32_t *dirs, const int32_t *found, int levels, float *offsets, float *angles, float *values);
// esprit.hpp's kernel likewise
static void doa_esprit_enqueue(unsigned nmat, hipStream_t S, const float2 *vec, const float *sv, int M, int k, const int32_t *korder, float d, int SX, int SY, int slots,
                               int32_t *found, int32_t *status, double *phases, float *angles, float *modulus, float *power, int32_t *flags);
// the most sources ESPRIT can place on an mx x my array: the rows left when a column or a row of elements is dropped, and the kernel's 16
// augment.hpp's kernel likewise
static void doa_augment_enqueue(unsigned nmat, hipStream_t S, const float2 *rxx, int mx, int my, int vx, int vy, uint64_t mask, float2 *ra);
static int esprit_rank_limit(int mx, int my) { return std::min(std::min((mx - 1) * my, mx * (my - 1)), (int)esprit::MAX_K); }
// k_doa_scan<false> is named here, ahead of the stages, to keep the code object's kernels in the order they have always had: a
// device-only assembly of the translation unit then compares line by line with an earlier build's
static const void *const kDoaPlainScan = (const void *)doa::k_doa_scan<false>;

static void doa_free(crsdr_doa *q)
{
    if (!q) return;
    (void)hipSetDevice(q->device);
    if (q->last.ran & kRanBase) (void)hipDeviceSynchronize();      // (the last submit's stream may be the caller's, and gone)
    delete q;                                                      // the buffers, then the stream
}

// what every setter does first: the object's device, and no kernel of the last submit still on the buffers
static int doa_quiesce(crsdr_doa *q)
{
    HIP_TRY(hipSetDevice(q->device));
    if (q->last.ran & kRanBase) HIP_TRY(hipDeviceSynchronize());   // (the last submit's stream may be the caller's, and gone)
    return CRSDR_OK;
}

// the most matrices a submit leaves: what every setter sizes its buffers by
static size_t doa_capacity(const crsdr_doa *q) { return (size_t)(q->max_batch / q->frames) * (size_t)q->sub.nbands; }

static int doa_alloc_matrices(crsdr_doa *q)
{
    const size_t nest = doa_capacity(q), m = (size_t)q->m, grid = (size_t)q->ncx * q->ncy;
    DoaMatrices &t = q->mat;
    int rc = CRSDR_OK;
    if (q->sub.nfft) {
        const size_t slices = (size_t)q->max_batch * q->sub.spb;
        if ((rc = q->sub.partial.alloc(slices * subband::subband_partial(q->m, q->sub.nfft))) || (rc = q->sub.power.alloc(nest))) return rc;
    }
    if ((rc = t.rxx.alloc(nest * m * m)) || (rc = t.vec.alloc(nest * m * m)) || (rc = t.sv.alloc(nest * m)) || (rc = t.info.alloc(nest * 2)) ||
        (rc = t.wgbest.alloc(nest * q->nwg)) || (rc = t.peak.alloc(nest * 2)) || (rc = t.peakv.alloc(nest)))
        return rc;
    if (q->flags & CRSDR_DOA_KEEP_SPECTRUM) rc = t.pm.alloc(nest * grid);
    return rc;
}

static int doa_alloc(crsdr_doa *q)
{
    HIP_TRY(hipSetDevice(q->device));
    HIP_TRY(hipStreamCreateWithFlags(&q->own.s, hipStreamNonBlocking));
    const size_t T = (size_t)q->max_batch;
    int rc = CRSDR_OK;
    if ((rc = q->partial.alloc(T * q->spb * q->ntri * 2 * doa::TILE_ELEMS)) || (rc = q->psum.alloc(T * q->spb * doa::MAX_ROWS))) return rc;
    if ((rc = doa_alloc_matrices(q))) return rc;
    return doa_lds_limits();
}

extern "C" int crsdr_doa_create(crsdr_doa **doa, const crsdr_doa_desc *desc)
{
    if (!doa || !desc) return fail(CRSDR_EINVAL, "doa_create: NULL argument");
    *doa = nullptr;
    const int m = desc->nrows - 1, mb = desc->max_batch ? desc->max_batch : 1, F = desc->frames ? desc->frames : 1;
    if (m < 2 || m > music::MAX_M || desc->mx < 1 || desc->my < 1 || (long long)desc->mx * desc->my != m)
        return fail(CRSDR_EINVAL, "doa_create: nrows - 1 = %d signal rows must be mx * my (%d x %d) in [2, %d]", m, desc->mx, desc->my, music::MAX_M);
    if (desc->blocksize < 32 || desc->blocksize % 32 || desc->blocksize > (1 << kMaxLog2Plan))
        return fail(CRSDR_EINVAL, "doa_create: blocksize = %d (a multiple of 32 up to %d)", desc->blocksize, 1 << kMaxLog2Plan);
    if (mb < 1 || mb > kMaxBatch) return fail(CRSDR_EINVAL, "doa_create: max_batch = %d (1..%d)", mb, kMaxBatch);
    if (F < 1 || F > mb) return fail(CRSDR_EINVAL, "doa_create: frames = %d (1..max_batch = %d)", desc->frames, mb);
    if (desc->k < 1 || desc->k >= m) return fail(CRSDR_EINVAL, "doa_create: k = %d sources (1 <= k < %d)", desc->k, m);
    if (desc->ncx < 1 || desc->ncy < 1 || (long long)desc->ncx * desc->ncy > (1 << 24))
        return fail(CRSDR_EINVAL, "doa_create: scan grid %d x %d (at least 1 x 1, at most 2^24 points)", desc->ncx, desc->ncy);
    if (desc->flags & ~(uint32_t)(CRSDR_DOA_KEEP_SPECTRUM | CRSDR_DOA_KEEP_RXX)) return fail(CRSDR_EINVAL, "doa_create: flags = 0x%x", desc->flags);
    { int rc = require_device(); if (rc) return rc; }
    int ndev = 0;
    (void)crsdr_device_count(&ndev);
    if (desc->device < 0 || desc->device >= ndev) return fail(CRSDR_ENODEV, "doa_create: device %d of %d", desc->device, ndev);

    crsdr_doa *q = new (std::nothrow) crsdr_doa();
    if (!q) return fail(CRSDR_ENOMEM, "doa_create: out of host memory");
    q->nrows = desc->nrows; q->B = desc->blocksize; q->m = m; q->device = desc->device; q->max_batch = mb; q->frames = F; q->k = desc->k;
    q->mx = desc->mx; q->my = desc->my; q->ncx = desc->ncx; q->ncy = desc->ncy; q->d = desc->d; q->flags = desc->flags;
    q->nt = (m + doa::TILE - 1) / doa::TILE; q->ntri = doa::cov_tiles(q->nt);
    // K slices per packet: about 1024 workgroups for a full batch (four per CU, so that the loads of one cover the MFMAs of another), no
    // slice beyond 65536 bytes (the int32 partials stay exact), none below 512 (four MFMA steps per wave) unless the bound asks for it
    const int spb_min = (q->B + 65535) / 65536, spb_max = std::max(spb_min, std::min(64, q->B / 512));
    q->spb = std::min(std::max((1024 + mb - 1) / mb, spb_min), spb_max);
    q->nwg = (int)(((size_t)q->ncx * q->ncy + music::PT - 1) / music::PT);
    int rc = doa_alloc(q);                               // (with every dynamic LDS limit: doa_lds_limits)
    if (rc) { doa_free(q); return rc; }
    *doa = q;
    return CRSDR_OK;
}

extern "C" int crsdr_doa_destroy(crsdr_doa *doa)
{
    if (!doa) return fail(CRSDR_EINVAL, "doa_destroy: NULL doa");
    doa_free(doa);
    return CRSDR_OK;
}

// ---- a submit: five stages of launches on one stream ----
// snapshots behind a matrix, for the source count: every sample, or a band's J' * width spectra
static double doa_snapshots(const crsdr_doa *q)
{
    if (q->sub.nfft) return (double)q->frames * (double)(q->B / (2 * q->sub.nfft)) * (double)q->sub.width;
    return (double)q->frames * (double)(q->B / 2);
}

struct DoaRun {
    const int8_t *packets;
    size_t packet_stride, matrix_offset;
    int nblocks;
    hipStream_t S;
    unsigned nest;               // matrices behind the covariance: estimates, or estimates * nbands
    int M, launches = 0;         // the subspace's size; launches so far
    float *pm = nullptr;         // the scan's spectrum, if it leaves one
};

// every launch of a submit: the kernel, its error, the count
template <typename Kernel, typename... Args>
static int doa_run(DoaRun &r, Kernel kern, dim3 grid, dim3 block, size_t lds, const Args &...args)
{
    hipLaunchKernelGGL(kern, grid, block, lds, r.S, args...);
    HIP_TRY(hipGetLastError());
    ++r.launches;
    return CRSDR_OK;
}

// covariance, plain or per band: partials, then their reducer into mat.rxx
static int doa_stage_covariance(crsdr_doa *q, DoaRun &r)
{
    int rc = CRSDR_OK;
    if (q->sub.nfft) {
        // one covariance per (estimate, band); everything behind it runs over nest * nbands matrices, estimate e's band i at e * nbands + i
        const DoaSubbands &sb = q->sub;
        const dim3 grid((unsigned)(q->frames * sb.spb), (unsigned)sb.groups, r.nest);
        SUBBAND_DISPATCH(sb.log2, rc = doa_run(r, subband::k_doa_subband_cov<LG>, grid, dim3(subband::SB_THREADS), 0, r.packets, r.packet_stride, r.matrix_offset,
                                               q->nrows, q->B, q->frames, sb.spb, sb.window, sb.partial.p));
        if (rc) return rc;
        rc = doa_run(r, subband::k_doa_subband_reduce, dim3((unsigned)sb.nbands, r.nest), dim3(256), 0, (const float2 *)sb.partial, (int)grid.x, q->nrows, q->B, q->frames,
                     sb.log2, sb.first, sb.width, sb.window, q->mat.rxx.p, sb.power.p);
        r.nest *= (unsigned)sb.nbands;
        return rc;
    }
    const unsigned slices = (unsigned)(q->frames * q->spb);
    if ((rc = doa_run(r, q->nt == 1 ? doa::k_doa_cov<1> : doa::k_doa_cov<2>, dim3(slices, r.nest), dim3(doa::COV_THREADS), 0, r.packets, r.packet_stride,
                      r.matrix_offset, q->nrows, q->B, q->frames, q->spb, q->partial.p, q->psum.p)))
        return rc;
    return doa_run(r, doa::k_doa_cov_reduce, dim3((unsigned)q->ntri, r.nest), dim3(256), 0, (const int *)q->partial, (const int2 *)q->psum, (int)slices, q->ntri,
                   q->nrows, q->B, q->frames, q->mat.rxx.p);
}

// smoothing on: subspace, order, scan and peaks work on rs, an sx x sy array of M = ms elements (off: sx = mx, sy = my, M = m);
// augmentation on: on ra, a vx x vy array of M = mv elements
static int doa_stage_subspace(crsdr_doa *q, DoaRun &r)
{
    const float2 *cov = q->mat.rxx;
    if (q->smooth.on) {
        const int rc = doa_run(r, smooth::k_doa_smooth, dim3(r.nest), dim3(smooth::SM_THREADS), 0, (const float2 *)q->mat.rxx, q->mx, q->my, q->smooth.sx, q->smooth.sy,
                               q->smooth.flags, q->smooth.rs.p);
        if (rc) return rc;
        cov = q->smooth.rs;
    } else if (q->augment.on) {
        doa_augment_enqueue(r.nest, r.S, (const float2 *)q->mat.rxx, q->mx, q->my, q->augment.vx, q->augment.vy, q->augment.mask, q->augment.ra.p);
        HIP_TRY(hipGetLastError());
        ++r.launches;
        cov = q->augment.ra;
    }
    return doa_run(r, doa::k_doa_subspace, dim3(r.nest), dim3(music::JT), 2 * sizeof(double2) * (size_t)r.M * r.M, cov, r.M, q->mat.sv.p, q->mat.vec.p, q->mat.info.p);
}

// ESPRIT's slots per matrix: k, or the most the source count can say
static int doa_esprit_slots(const crsdr_doa *q) { return q->order.crit ? q->order.kmax : q->k; }

// what a submit with ESPRIT on needs, known on the host: checked before any launch
static int doa_esprit_ready(const crsdr_doa *q)
{
    const DoaEsprit &es = q->esprit;
    if (!es.mode) return CRSDR_OK;
    const int slots = doa_esprit_slots(q);
    if (q->sx() < 2 || q->sy() < 2 || slots > esprit_rank_limit(q->sx(), q->sy()))
        return fail(CRSDR_ESTATE, "doa_submit: ESPRIT is on (crsdr_doa_set_esprit): it needs an array of at least 2 x 2 (%d x %d) and at most %d sources (%d)", q->sx(), q->sy(),
                    q->sx() >= 2 && q->sy() >= 2 ? esprit_rank_limit(q->sx(), q->sy()) : 0, slots);
    if (es.mode == CRSDR_ESPRIT_ONLY && (q->peaks.count || q->refine.levels || (q->beams.mode && !q->beams.nfixed)))
        return fail(CRSDR_ESTATE, "doa_submit: CRSDR_ESPRIT_ONLY runs no scan: peaks, the refinement and beams that follow the directions need one, turn them off first");
    return CRSDR_OK;
}

// the source count (if on), ESPRIT (if on), the scan with k or with the counts, the peak
static int doa_stage_scan(crsdr_doa *q, DoaRun &r)
{
    const int M = r.M;
    const dim3 grid((unsigned)q->nwg, r.nest);
    // with peaks on, the scan always leaves its spectrum: the kept one, or the workspace
    r.pm = q->peaks.count && !q->mat.pm ? q->peaks.pmws.p : q->mat.pm.p;
    if (q->order.crit) {
        const int rc = doa_run(r, smooth::k_doa_order, dim3(r.nest), dim3(64), 0, (const float *)q->mat.sv, M, doa_snapshots(q), q->order.crit, q->order.kmin,
                               q->order.kmax, q->order.k.p, q->order.values.p);
        if (rc) return rc;
    }
    if (q->esprit.mode) {
        // the gridless directions: one wave per matrix on the subspace and the counts the scan would use
        DoaEsprit &es = q->esprit;
        doa_esprit_enqueue(r.nest, r.S, (const float2 *)q->mat.vec, (const float *)q->mat.sv, M, q->k, (const int32_t *)q->order.k, q->d, q->sx(), q->sy(),
                           doa_esprit_slots(q), es.found.p, es.status.p, es.phases.p, es.angles.p, es.modulus.p, es.power.p, es.flags.p);
        HIP_TRY(hipGetLastError());
        ++r.launches;
        if (es.mode == CRSDR_ESPRIT_ONLY) return CRSDR_OK;               // no scan, no peak
    }
    int rc;
    if (q->spectrum != CRSDR_SPECTRUM_MUSIC) {
        // a power map in the scan's place: every column of vec weighted by sv, whatever k or the counts say
        rc = doa_run(r, spectrum::k_doa_spectrum, grid, dim3(spectrum::PT), spectrum::lds_bytes(M), (const float2 *)q->mat.vec, (const float *)q->mat.sv, M, q->spectrum,
                     q->spectrum_loading, q->d, q->sx(), q->sy(), q->ncx, q->ncy, r.pm, q->mat.wgbest.p);
    } else {
        // the counts in place of k: the LDS of the most noise vectors an estimate can have, M - kmin
        const auto scan = q->order.crit ? doa::k_doa_scan<true> : doa::k_doa_scan<false>;
        rc = doa_run(r, scan, grid, dim3(music::PT), sizeof(float2) * ((size_t)M * (M - (q->order.crit ? q->order.kmin : q->k)) + (size_t)M * music::PT),
                     (const float2 *)q->mat.vec, M, q->k, q->d, q->sx(), q->sy(), q->ncx, q->ncy, r.pm, q->mat.wgbest.p, (const int32_t *)q->order.k);
    }
    if (rc) return rc;
    return doa_run(r, doa::k_doa_peak, dim3(r.nest), dim3(256), 0, (const unsigned long long *)q->mat.wgbest, q->nwg, q->ncy, q->mat.peak.p, q->mat.peakv.p);
}

static int doa_stage_local_peaks(crsdr_doa *q, DoaRun &r)
{
    const DoaPeaks &pk = q->peaks;
    if (!pk.count) return CRSDR_OK;
    const int rc = doa_run(r, doa::k_doa_local_peaks, dim3((unsigned)pk.tiles, r.nest), dim3(doa::LP_THREADS), doa::lp_lds(pk.radius), (const float *)r.pm, q->ncx,
                           q->ncy, pk.radius, pk.count, pk.cand.p);
    if (rc) return rc;
    return doa_run(r, doa::k_doa_peaks_merge, dim3(r.nest), dim3(doa::LP_THREADS), 0, (const unsigned long long *)pk.cand, pk.tiles * pk.count, q->ncy, pk.count,
                   pk.found.p, pk.dirs.p, pk.values.p, (const int32_t *)(q->order.crit && q->order.limit_dirs ? q->order.k.p : nullptr));
}

// the directions off the grid: one workgroup per (slot, matrix) on the subspace the scan used
static int doa_stage_refine(crsdr_doa *q, DoaRun &r)
{
    const DoaRefine &rf = q->refine;
    if (!rf.levels) return CRSDR_OK;
    const bool pk = q->peaks.count != 0;
    doa_refine_enqueue(dim3((unsigned)(pk ? q->peaks.count : 1), r.nest), r.S, (const float2 *)q->mat.vec, (const float *)q->mat.sv, r.M, q->spectrum, q->k,
                       (const int32_t *)q->order.k, q->spectrum_loading, q->d, q->sx(), q->ncx, q->ncy, (const int32_t *)(pk ? q->peaks.dirs.p : q->mat.peak.p),
                       (const int32_t *)(pk ? q->peaks.found.p : nullptr), rf.levels, rf.offsets.p, rf.angles.p, rf.values.p);
    HIP_TRY(hipGetLastError());
    ++r.launches;
    return CRSDR_OK;
}

// the weights per matrix, then the apply kernel over the packets: on their samples, or on their band spectra
static int doa_stage_beams(crsdr_doa *q, DoaRun &r)
{
    const DoaBeams &bm = q->beams;
    if (!bm.mode) return CRSDR_OK;
    int rc = doa_run(r, beams::k_doa_beam_weights, dim3(r.nest, (unsigned)bm.nbeams), dim3(beams::BW_THREADS), 0, (const float2 *)q->mat.vec, (const float *)q->mat.sv,
                     q->m, q->mx, q->d, q->ncx, q->ncy, bm.mode, bm.loading, (const float *)(bm.nfixed ? bm.angles.p : nullptr),
                     (const int32_t *)(q->peaks.count ? q->peaks.found.p : nullptr), (const int32_t *)q->peaks.dirs, (const int32_t *)q->mat.peak,
                     (const float *)(q->refine.levels && !bm.nfixed ? q->refine.offsets.p : nullptr), bm.weights.p, bm.power.p);
    if (rc) return rc;
    if (bm.band) {
        // the weights above are per (estimate, band): applied to the rows' band spectra
        const dim3 grid((unsigned)sbbeams::sbb_spb(q->B, q->sub.nfft), (unsigned)r.nblocks);
        SUBBAND_DISPATCH(q->sub.log2, rc = doa_run(r, sbbeams::k_doa_subband_beam_apply<LG>, grid, dim3(sbbeams::SBB_THREADS), sizeof(float2) * (size_t)bm.lds_points,
                                                   r.packets, r.packet_stride, r.matrix_offset, q->nrows, q->B, q->frames, q->sub.first, q->sub.nbands, q->sub.width,
                                                   q->sub.window, (const float2 *)bm.weights, bm.nbeams, bm.lds_points, bm.beams.p));
    } else {
        const dim3 grid((unsigned)((q->B / 4 + beams::AP_THREADS - 1) / beams::AP_THREADS), (unsigned)r.nblocks);
        BEAMS_DISPATCH(bm.nbeams, rc = doa_run(r, beams::k_doa_beam_apply<NB>, grid, dim3(beams::AP_THREADS), 0, r.packets, r.packet_stride, r.matrix_offset, q->nrows,
                                               q->B, q->frames, (const float2 *)bm.weights, bm.nbeams, bm.beams.p));
    }
    return rc;
}

static int doa_launch(crsdr_doa *q, const int8_t *packets, size_t packet_stride, size_t matrix_offset, int nblocks, hipStream_t S)
{
    DoaRun r{packets, packet_stride, matrix_offset, nblocks, S, (unsigned)(nblocks / q->frames), q->ms()};
    int rc = doa_esprit_ready(q);
    if (rc) return rc;
    // (CRSDR_ESPRIT_ONLY: the scan stage ends behind ESPRIT; peaks and the refinement are off, doa_esprit_ready saw to it)
    if ((rc = doa_stage_covariance(q, r)) || (rc = doa_stage_subspace(q, r)) || (rc = doa_stage_scan(q, r)) || (rc = doa_stage_local_peaks(q, r)) ||
        (rc = doa_stage_refine(q, r)) || (rc = doa_stage_beams(q, r)))
        return rc;
    q->last = DoaLast{S, (int)r.nest, nblocks, r.M, r.launches,
                      kRanBase | (q->peaks.count ? kRanPeaks : 0u) | (q->beams.mode ? kRanBeams : 0u) | (q->smooth.on ? kRanSmooth : 0u) | (q->augment.on ? kRanAugment : 0u) | (q->order.crit ? kRanOrder : 0u) |
                          (q->refine.levels ? kRanRefine : 0u) | (q->esprit.mode ? kRanEsprit : 0u) | (q->esprit.mode == CRSDR_ESPRIT_ONLY ? 0u : kRanScan),
                      q->refine.levels ? (q->peaks.count ? q->peaks.count : 1) : 0, q->esprit.mode ? doa_esprit_slots(q) : 0};
    return CRSDR_OK;
}

// The kernels' dynamic LDS limits are function attributes, shared by every live object: each create sets every limit the engine's
// kernels can need to the most any object can ask for (subspace and scan: m = 64, one signal vector; power maps: m = 64; local peaks: the largest radius;
// band beams: 64 rows of 256 points; the refinement: m = 64), so that a small object created after a large one cannot lower a limit under it, and no setter
// has to think of them.  (The per-op calls set their own kernels' limits.)
static int doa_lds_limits()
{
    constexpr size_t sub = 2 * sizeof(double2) * music::MAX_M * music::MAX_M;            // 128 KiB
    constexpr size_t scan = sizeof(float2) * (music::MAX_M * (music::MAX_M - 1) + music::MAX_M * music::PT);
    constexpr size_t sbb = sizeof(float2) * sbbeams::sbb_seg_stride(sbbeams::SBB_MAX_ROWS, 1 << subband::SB_MAX_LOG2);
    auto limit = [](const void *kern, size_t bytes) { return hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes); };
    HIP_TRY(limit((const void *)doa::k_doa_subspace, sub));
    HIP_TRY(limit(kDoaPlainScan, scan));
    HIP_TRY(limit((const void *)doa::k_doa_scan<true>, scan));
    HIP_TRY(limit((const void *)spectrum::k_doa_spectrum, spectrum::lds_bytes(music::MAX_M)));
    HIP_TRY(limit((const void *)doa::k_doa_local_peaks, doa::lp_lds(doa::MAX_RADIUS)));
    HIP_TRY(limit(doa_refine_kernel(), refine::lds_bytes(refine::MAX_M)));
    for (int lg = subband::SB_MIN_LOG2; lg <= subband::SB_MAX_LOG2; ++lg) SUBBAND_DISPATCH(lg, HIP_TRY(limit((const void *)sbbeams::k_doa_subband_beam_apply<LG>, sbb)));
    return CRSDR_OK;
}

extern "C" int crsdr_doa_submit(crsdr_doa *q, const void *device_packets, size_t packet_stride, size_t matrix_offset, int nblocks, void *hip_stream)
{
    if (!q || !device_packets) return fail(CRSDR_EINVAL, "doa_submit: NULL doa or packets");
    if (nblocks < 1 || nblocks > q->max_batch || nblocks % q->frames)
        return fail(CRSDR_EINVAL, "doa_submit: nblocks = %d (1..max_batch = %d, a multiple of frames = %d)", nblocks, q->max_batch, q->frames);
    if (((uintptr_t)device_packets + matrix_offset) % 4 || packet_stride % 4)
        return fail(CRSDR_EINVAL, "doa_submit: matrix start and packet stride must be 4-byte aligned");
    HIP_TRY(hipSetDevice(q->device));
    return doa_launch(q, (const int8_t *)device_packets, packet_stride, matrix_offset, nblocks, hip_stream ? (hipStream_t)hip_stream : q->own.s);
}

extern "C" int crsdr_doa_submit_plan(crsdr_doa *q, crsdr_plan *p)
{
    if (!q || !p) return fail(CRSDR_EINVAL, "doa_submit_plan: NULL argument");
    if (p->nrows != q->nrows || p->B != q->B || p->device != q->device)
        return fail(CRSDR_EINVAL, "doa_submit_plan: plan is %d x %d on device %d, doa %d x %d on device %d", p->nrows, p->B, p->device, q->nrows, q->B, q->device);
    if (p->d_slab) return fail(CRSDR_ESTATE, "doa_submit_plan: the plan writes slabs (crsdr_plan_bind_slab): its packets hold no matrix");
    if (!p->submitted || p->last_nblocks < 1) return fail(CRSDR_ESTATE, "doa_submit_plan: the plan has no submitted batch");
    if (p->last_nblocks > q->max_batch || p->last_nblocks % q->frames)
        return fail(CRSDR_EINVAL, "doa_submit_plan: the plan's batch of %d blocks (doa: at most %d, a multiple of frames = %d)", p->last_nblocks, q->max_batch, q->frames);
    HIP_TRY(hipSetDevice(q->device));
    // the batch's last kernel is on p->stream: stream order alone puts the covariance behind it
    return doa_launch(q, p->d_packet, p->packet_stride, p->matrix_off, p->last_nblocks, p->stream);
}

extern "C" int crsdr_doa_last_submit(crsdr_doa *q, int *nest, int *launches)
{
    if (!q) return fail(CRSDR_EINVAL, "doa_last_submit: NULL doa");
    if (!(q->last.ran & kRanBase)) return fail(CRSDR_ESTATE, "doa_last_submit: nothing submitted");
    if (nest) *nest = q->last.nest;
    if (launches) *launches = q->last.launches;
    return CRSDR_OK;
}

// ---- fetches ----
// Every fetch, behind its own state checks, copies through DevFetch on the last submit's stream.

extern "C" int crsdr_doa_fetch(crsdr_doa *q, int32_t *peak, float *peak_value, float *sv, int32_t *status, float *pm, float *rxx)
{
    if (!q) return fail(CRSDR_EINVAL, "doa_fetch: NULL doa");
    if (pm && !(q->flags & CRSDR_DOA_KEEP_SPECTRUM)) return fail(CRSDR_EINVAL, "doa_fetch: pm asked of a doa created without CRSDR_DOA_KEEP_SPECTRUM");
    if (rxx && !(q->flags & CRSDR_DOA_KEEP_RXX)) return fail(CRSDR_EINVAL, "doa_fetch: rxx asked of a doa created without CRSDR_DOA_KEEP_RXX");
    if (!(q->last.ran & kRanBase)) return fail(CRSDR_ESTATE, "doa_fetch: nothing submitted");
    if ((peak || peak_value || pm) && !(q->last.ran & kRanScan))
        return fail(CRSDR_ESTATE, "doa_fetch: the last submit ran no scan (CRSDR_ESPRIT_ONLY): no peak, peak_value or pm");
    const size_t nest = (size_t)q->last.nest, m = (size_t)q->m, ms = (size_t)q->last.ms;
    static_assert(kMaxDoaMatrices >= kMaxBatch, "status of every matrix of a submit");
    int info[2 * kMaxDoaMatrices];
    const int rc = DevFetch(q->device, q->last.stream).copy(peak, q->mat.peak.p, nest * 2).copy(peak_value, q->mat.peakv.p, nest).copy(sv, q->mat.sv.p, nest * ms)
                       .copy(status ? info : nullptr, q->mat.info.p, nest * 2).copy(pm, q->mat.pm.p, nest * (size_t)q->ncx * q->ncy)
                       .copy(rxx, q->mat.rxx.p, nest * m * m).wait();
    if (rc) return rc;
    if (status)
        for (size_t e = 0; e < nest; ++e) status[e] = info[2 * e + 1] ? 0 : 1;      // Jacobi sweeps ran out: data, not a failed call
    return CRSDR_OK;
}

extern "C" int crsdr_doa_device_buffers(crsdr_doa *q, void **peak, void **peak_value, void **sv, void **vec, void **pm)
{
    if (!q) return fail(CRSDR_EINVAL, "doa_device_buffers: NULL doa");
    if (peak) *peak = q->mat.peak;
    if (peak_value) *peak_value = q->mat.peakv;
    if (sv) *sv = q->mat.sv;
    if (vec) *vec = q->mat.vec;
    if (pm) *pm = q->mat.pm;
    return CRSDR_OK;
}

extern "C" int crsdr_doa_fetch_subspace(crsdr_doa *q, float *vec)
{
    if (!q || !vec) return fail(CRSDR_EINVAL, "doa_fetch_subspace: NULL doa or vec");
    if (!(q->last.ran & kRanBase)) return fail(CRSDR_ESTATE, "doa_fetch_subspace: nothing submitted");
    return DevFetch(q->device, q->last.stream).copy(vec, q->mat.vec.p, (size_t)q->last.nest * (size_t)q->last.ms * q->last.ms).wait();
}

// ---- the strongest local maxima of each spectrum (doa.hpp) ----
static int doa_alloc_peaks(crsdr_doa *q, int count)
{
    const size_t nest = doa_capacity(q), grid = (size_t)q->ncx * q->ncy;
    DoaPeaks &pk = q->peaks;
    pk.tiles = doa::lp_tiles(q->ncx, q->ncy);
    int rc = CRSDR_OK;
    if (!q->mat.pm && (rc = pk.pmws.alloc(nest * grid))) return rc;
    if ((rc = pk.cand.alloc(nest * pk.tiles * count)) || (rc = pk.found.alloc(nest)) || (rc = pk.dirs.alloc(nest * count * 2))) return rc;
    return pk.values.alloc(nest * count);
}

extern "C" int crsdr_doa_set_peaks(crsdr_doa *q, int count, int radius)
{
    if (!q) return fail(CRSDR_EINVAL, "doa_set_peaks: NULL doa");
    if (count < 0 || count > doa::MAX_PEAKS) return fail(CRSDR_EINVAL, "doa_set_peaks: count = %d (0..%d)", count, doa::MAX_PEAKS);
    if (count > 0 && (radius < 1 || radius > doa::MAX_RADIUS)) return fail(CRSDR_EINVAL, "doa_set_peaks: radius = %d (1..%d)", radius, doa::MAX_RADIUS);
    if (q->beams.mode && !q->beams.nfixed)
        return fail(CRSDR_ESTATE, "doa_set_peaks: beams follow the directions (crsdr_doa_set_beams or _set_subband_beams with nfixed = 0) and are sized by them: turn the beams off first");
    { const int rc = doa_quiesce(q); if (rc) return rc; }
    q->peaks = {}; q->last.ran &= ~kRanPeaks;
    if (count == 0) return CRSDR_OK;
    const int rc = doa_alloc_peaks(q, count);
    if (rc) { q->peaks = {}; return rc; }
    q->peaks.count = count; q->peaks.radius = radius;
    return CRSDR_OK;
}

extern "C" int crsdr_doa_fetch_directions(crsdr_doa *q, int32_t *found, int32_t *peaks, float *values)
{
    if (!q) return fail(CRSDR_EINVAL, "doa_fetch_directions: NULL doa");
    if (!q->peaks.count) return fail(CRSDR_ESTATE, "doa_fetch_directions: no crsdr_doa_set_peaks");
    if (!(q->last.ran & kRanPeaks)) return fail(CRSDR_ESTATE, "doa_fetch_directions: nothing submitted since crsdr_doa_set_peaks");
    if (!(q->last.ran & kRanScan)) return fail(CRSDR_ESTATE, "doa_fetch_directions: the last submit ran no scan (CRSDR_ESPRIT_ONLY)");
    const size_t nest = (size_t)q->last.nest, c = (size_t)q->peaks.count;
    return DevFetch(q->device, q->last.stream).copy(found, q->peaks.found.p, nest).copy(peaks, q->peaks.dirs.p, nest * c * 2).copy(values, q->peaks.values.p, nest * c).wait();
}

extern "C" int crsdr_doa_direction_buffers(crsdr_doa *q, void **found, void **peaks, void **values)
{
    if (!q) return fail(CRSDR_EINVAL, "doa_direction_buffers: NULL doa");
    if (found) *found = q->peaks.found;
    if (peaks) *peaks = q->peaks.dirs;
    if (values) *values = q->peaks.values;
    return CRSDR_OK;
}

// ---- beams toward the directions: on the samples (beams.hpp) or, `band`, on the band spectra (subband_beams.hpp) ----
// One implementation behind the two families of entry points; `who` is the caller's name in every message.
// complex points of one slot's beam in a packet: every sample, or nbands * width bins of J segments each (never more than B / 2)
static size_t doa_beam_points(const crsdr_doa *q, bool band)
{
    return band ? (size_t)q->sub.nbands * (size_t)(q->B / (2 * q->sub.nfft)) * (size_t)q->sub.width : (size_t)(q->B / 2);
}

static int doa_set_beams(crsdr_doa *q, const char *who, bool band, int mode, float loading, int nfixed, const float *fixed_angles)
{
    if (!q) return fail(CRSDR_EINVAL, "%s: NULL doa", who);
    if (mode != CRSDR_BEAM_OFF && mode != CRSDR_BEAM_CONVENTIONAL && mode != CRSDR_BEAM_MVDR) return fail(CRSDR_EINVAL, "%s: mode = %d", who, mode);
    if (mode == CRSDR_BEAM_MVDR && !(loading >= 1e-6f && loading <= 1.0f)) return fail(CRSDR_EINVAL, "%s: loading = %g (1e-6..1)", who, (double)loading);
    if (mode != CRSDR_BEAM_OFF && (nfixed < 0 || nfixed > beams::MAX_BEAMS)) return fail(CRSDR_EINVAL, "%s: nfixed = %d (0..%d)", who, nfixed, beams::MAX_BEAMS);
    if (mode != CRSDR_BEAM_OFF && nfixed > 0 && !fixed_angles) return fail(CRSDR_EINVAL, "%s: %d fixed directions and no angles", who, nfixed);
    if (mode != CRSDR_BEAM_OFF && !band && q->sub.nfft)
        return fail(CRSDR_ESTATE, "%s: subbands are on (crsdr_doa_set_subbands): a band's weights applied to the wideband samples mean nothing", who);
    if (mode != CRSDR_BEAM_OFF && band && !q->sub.nfft)
        return fail(CRSDR_ESTATE, "%s: subbands are off (crsdr_doa_set_subbands): the wideband beams are crsdr_doa_set_beams", who);
    if (mode != CRSDR_BEAM_OFF && q->augment.on)
        return fail(CRSDR_ESTATE, "%s: augmentation is on (crsdr_doa_set_augment): the subspace is the %d x %d virtual array's, and weights from it are not the physical rows'", who,
                    q->sx(), q->sy());
    if (mode != CRSDR_BEAM_OFF && q->ms() < q->m)
        return fail(CRSDR_ESTATE, "%s: smoothing over %d x %d sub-arrays is on (crsdr_doa_set_smoothing): the weights are %d-vectors and there is no %d x %d subspace", who,
                    q->sx(), q->sy(), q->m, q->m, q->m);
    if (q->beams.mode && q->beams.band != band) return CRSDR_OK;     // (off: the other kind of beams is its own call's to turn off)
    { const int rc = doa_quiesce(q); if (rc) return rc; }
    q->beams = {}; q->last.ran &= ~kRanBeams;
    if (mode == CRSDR_BEAM_OFF) return CRSDR_OK;
    // weights and power per matrix (wideband: subbands are off, one matrix per estimate), the beams per packet
    const size_t nmat = doa_capacity(q), nb = (size_t)(nfixed ? nfixed : q->peaks.count ? q->peaks.count : 1);
    DoaBeams &bm = q->beams;
    int rc = CRSDR_OK;
    auto alloc = [&](auto &buf, size_t count) {
        if (!rc && buf.alloc(count)) rc = fail(CRSDR_ENOMEM, "%s: %zu bytes of device memory", who, sizeof(*buf.p) * count);
    };
    alloc(bm.weights, nmat * nb * (size_t)q->m);
    alloc(bm.power, nmat * nb);
    alloc(bm.beams, (size_t)q->max_batch * nb * doa_beam_points(q, band));
    if (nfixed) {
        alloc(bm.angles, 2 * nb);
        if (!rc && hipMemcpy(bm.angles, fixed_angles, sizeof(float) * 2 * nb, hipMemcpyHostToDevice) != hipSuccess) rc = fail(CRSDR_EHIP, "%s: copy of the angles", who);
    }
    if (rc) { q->beams = {}; return rc; }
    bm.mode = mode; bm.nbeams = (int)nb; bm.nfixed = nfixed; bm.loading = mode == CRSDR_BEAM_MVDR ? loading : 0.f;
    bm.band = band; bm.lds_points = band ? sbbeams::sbb_lds_points(q->m, q->B, q->sub.nfft) : 0;
    return CRSDR_OK;
}

static int doa_fetch_beams(crsdr_doa *q, const char *who, bool band, float *weights, float *power, float *beams)
{
    const char *kind = band ? "subband_" : "";
    if (!q) return fail(CRSDR_EINVAL, "%s: NULL doa", who);
    if (!q->beams.mode || q->beams.band != band) return fail(CRSDR_ESTATE, "%s: no crsdr_doa_set_%sbeams", who, kind);
    if (!(q->last.ran & kRanBeams)) return fail(CRSDR_ESTATE, "%s: nothing submitted since crsdr_doa_set_%sbeams", who, kind);
    const size_t nmat = (size_t)q->last.nest, nb = (size_t)q->beams.nbeams;
    return DevFetch(q->device, q->last.stream).copy(weights, q->beams.weights.p, nmat * nb * (size_t)q->m).copy(power, q->beams.power.p, nmat * nb)
                      .copy(beams, q->beams.beams.p, (size_t)q->last.nblocks * nb * doa_beam_points(q, band)).wait();
}

static int doa_beam_buffers(crsdr_doa *q, const char *who, bool band, void **weights, void **power, void **beams, int *nbeams)
{
    if (!q) return fail(CRSDR_EINVAL, "%s: NULL doa", who);
    const bool on = q->beams.band == band;               // (both kinds off: the wideband call's NULLs and 0)
    if (weights) *weights = on ? q->beams.weights.p : nullptr;
    if (power) *power = on ? q->beams.power.p : nullptr;
    if (beams) *beams = on ? q->beams.beams.p : nullptr;
    if (nbeams) *nbeams = on ? q->beams.nbeams : 0;
    return CRSDR_OK;
}

extern "C" int crsdr_doa_set_beams(crsdr_doa *q, int mode, float loading, int nfixed, const float *fixed_angles)
{ return doa_set_beams(q, "doa_set_beams", false, mode, loading, nfixed, fixed_angles); }
extern "C" int crsdr_doa_fetch_beams(crsdr_doa *q, float *weights, float *power, float *beams)
{ return doa_fetch_beams(q, "doa_fetch_beams", false, weights, power, beams); }
extern "C" int crsdr_doa_beam_buffers(crsdr_doa *q, void **weights, void **power, void **beams, int *nbeams)
{ return doa_beam_buffers(q, "doa_beam_buffers", false, weights, power, beams, nbeams); }
extern "C" int crsdr_doa_set_subband_beams(crsdr_doa *q, int mode, float loading, int nfixed, const float *fixed_angles)
{ return doa_set_beams(q, "doa_set_subband_beams", true, mode, loading, nfixed, fixed_angles); }
extern "C" int crsdr_doa_fetch_subband_beams(crsdr_doa *q, float *weights, float *power, float *beams)
{ return doa_fetch_beams(q, "doa_fetch_subband_beams", true, weights, power, beams); }
extern "C" int crsdr_doa_subband_beam_buffers(crsdr_doa *q, void **weights, void **power, void **beams, int *nbeams)
{ return doa_beam_buffers(q, "doa_subband_beam_buffers", true, weights, power, beams, nbeams); }

// ---- the map the scan computes (spectrum.hpp) ----
extern "C" int crsdr_doa_set_spectrum(crsdr_doa *q, int kind, float loading)
{
    if (!q) return fail(CRSDR_EINVAL, "doa_set_spectrum: NULL doa");
    { const int rc = spectrum_args_ok("doa_set_spectrum", kind, loading, true); if (rc) return rc; }
    { const int rc = doa_quiesce(q); if (rc) return rc; }
    // pm, the peak, the directions and the beams toward them all change their meaning: nothing the last submit left stays
    q->last.ran = 0;
    q->spectrum = kind; q->spectrum_loading = kind == CRSDR_SPECTRUM_CAPON ? loading : 0.f;
    return CRSDR_OK;
}

// ---- the directions off the scan grid (refine.hpp) ----
extern "C" int crsdr_doa_set_refine(crsdr_doa *q, int levels)
{
    if (!q) return fail(CRSDR_EINVAL, "doa_set_refine: NULL doa");
    if (levels < 0 || levels > refine::MAX_LEVELS) return fail(CRSDR_EINVAL, "doa_set_refine: levels = %d (0..%d)", levels, refine::MAX_LEVELS);
    { const int rc = doa_quiesce(q); if (rc) return rc; }
    q->refine = {}; q->last.ran &= ~kRanRefine;
    if (levels == 0) return CRSDR_OK;
    // the most matrices and slots any later setter can ask for
    const size_t slots = (size_t)kMaxDoaMatrices * doa::MAX_PEAKS;
    DoaRefine &rf = q->refine;
    if (rf.offsets.alloc(2 * slots) || rf.angles.alloc(2 * slots) || rf.values.alloc(slots)) {
        q->refine = {};
        return fail(CRSDR_ENOMEM, "doa_set_refine: %zu bytes of device memory", sizeof(float) * 5 * slots);
    }
    rf.levels = levels;
    return CRSDR_OK;
}

extern "C" int crsdr_doa_fetch_refined(crsdr_doa *q, float *offsets, float *angles, float *values)
{
    if (!q) return fail(CRSDR_EINVAL, "doa_fetch_refined: NULL doa");
    if (!q->refine.levels) return fail(CRSDR_ESTATE, "doa_fetch_refined: no crsdr_doa_set_refine");
    if (!(q->last.ran & kRanRefine)) return fail(CRSDR_ESTATE, "doa_fetch_refined: nothing submitted since crsdr_doa_set_refine");
    if (!(q->last.ran & kRanScan)) return fail(CRSDR_ESTATE, "doa_fetch_refined: the last submit ran no scan (CRSDR_ESPRIT_ONLY)");
    const size_t n = (size_t)q->last.nest * (size_t)q->last.slots;
    return DevFetch(q->device, q->last.stream).copy(offsets, q->refine.offsets.p, 2 * n).copy(angles, q->refine.angles.p, 2 * n).copy(values, q->refine.values.p, n).wait();
}

extern "C" int crsdr_doa_refined_buffers(crsdr_doa *q, void **offsets, void **angles, void **values, int *slots)
{
    if (!q) return fail(CRSDR_EINVAL, "doa_refined_buffers: NULL doa");
    if (offsets) *offsets = q->refine.offsets;
    if (angles) *angles = q->refine.angles;
    if (values) *values = q->refine.values;
    if (slots) *slots = q->refine.levels ? (q->last.ran & kRanRefine ? q->last.slots : q->peaks.count ? q->peaks.count : 1) : 0;
    return CRSDR_OK;
}

// ---- the gridless directions (esprit.hpp) ----
extern "C" int crsdr_doa_set_esprit(crsdr_doa *q, int mode)
{
    if (!q) return fail(CRSDR_EINVAL, "doa_set_esprit: NULL doa");
    if (mode != CRSDR_ESPRIT_OFF && mode != CRSDR_ESPRIT_BESIDE && mode != CRSDR_ESPRIT_ONLY) return fail(CRSDR_EINVAL, "doa_set_esprit: mode = %d", mode);
    { const int rc = doa_quiesce(q); if (rc) return rc; }
    q->esprit = {}; q->last.ran &= ~kRanEsprit;
    if (mode == CRSDR_ESPRIT_OFF) return CRSDR_OK;
    // the most matrices and slots any later setter can ask for
    const size_t nmat = kMaxDoaMatrices, slots = nmat * esprit::MAX_K;
    DoaEsprit &es = q->esprit;
    if (es.found.alloc(nmat) || es.status.alloc(nmat) || es.flags.alloc(slots) || es.phases.alloc(2 * slots) || es.angles.alloc(2 * slots) || es.modulus.alloc(2 * slots) ||
        es.power.alloc(slots)) {
        q->esprit = {};
        return fail(CRSDR_ENOMEM, "doa_set_esprit: %zu bytes of device memory", 8 * nmat + 40 * slots);
    }
    es.mode = mode;
    return CRSDR_OK;
}

extern "C" int crsdr_doa_fetch_esprit(crsdr_doa *q, int32_t *found, int32_t *status, double *phases, float *angles, float *modulus, float *power, int32_t *flags)
{
    if (!q) return fail(CRSDR_EINVAL, "doa_fetch_esprit: NULL doa");
    if (!q->esprit.mode) return fail(CRSDR_ESTATE, "doa_fetch_esprit: no crsdr_doa_set_esprit");
    if (!(q->last.ran & kRanBase) || !(q->last.ran & kRanEsprit)) return fail(CRSDR_ESTATE, "doa_fetch_esprit: nothing submitted since crsdr_doa_set_esprit");
    const DoaEsprit &es = q->esprit;
    const size_t nmat = (size_t)q->last.nest, n = nmat * (size_t)q->last.eslots;
    return DevFetch(q->device, q->last.stream).copy(found, es.found.p, nmat).copy(status, es.status.p, nmat).copy(phases, es.phases.p, 2 * n).copy(angles, es.angles.p, 2 * n)
                      .copy(modulus, es.modulus.p, 2 * n).copy(power, es.power.p, n).copy(flags, es.flags.p, n).wait();
}

extern "C" int crsdr_doa_esprit_buffers(crsdr_doa *q, void **found, void **status, void **phases, void **angles, void **modulus, void **power, void **flags, int *slots)
{
    if (!q) return fail(CRSDR_EINVAL, "doa_esprit_buffers: NULL doa");
    const DoaEsprit &es = q->esprit;
    if (found) *found = es.found;
    if (status) *status = es.status;
    if (phases) *phases = es.phases;
    if (angles) *angles = es.angles;
    if (modulus) *modulus = es.modulus;
    if (power) *power = es.power;
    if (flags) *flags = es.flags;
    if (slots) *slots = es.mode ? (q->last.ran & kRanEsprit ? q->last.eslots : doa_esprit_slots(q)) : 0;
    return CRSDR_OK;
}

// ---- spatial smoothing and the source count (smooth.hpp) ----
extern "C" int crsdr_doa_set_smoothing(crsdr_doa *q, int sx, int sy, uint32_t flags)
{
    if (!q) return fail(CRSDR_EINVAL, "doa_set_smoothing: NULL doa");
    if (!smooth_shape_ok(q->mx, q->my, sx, sy, flags))
        return fail(CRSDR_EINVAL, "doa_set_smoothing: sub-arrays of %d x %d in an array of %d x %d, flags = 0x%x (1 <= sx <= mx, 1 <= sy <= my, sx * sy >= 2, CRSDR_SMOOTH_FB)", sx,
                    sy, q->mx, q->my, flags);
    const int ms = sx * sy;
    if (q->augment.on && (ms < q->m || flags))
        return fail(CRSDR_ESTATE, "doa_set_smoothing: augmentation is on (crsdr_doa_set_augment): its matrix is Hermitian block-Toeplitz, all its sub-array blocks are equal and it is "
                                  "persymmetric already, so smoothing it changes nothing: turn augmentation off first");
    if (q->k >= ms) return fail(CRSDR_EINVAL, "doa_set_smoothing: k = %d sources need sub-arrays of more than %d elements (%d x %d)", q->k, q->k, sx, sy);
    if (q->order.crit && q->order.kmax >= ms)
        return fail(CRSDR_EINVAL, "doa_set_smoothing: the order range ends at kmax = %d, sub-arrays of %d x %d have %d elements", q->order.kmax, sx, sy, ms);
    if (ms < q->m && q->beams.mode)
        return fail(CRSDR_ESTATE, "doa_set_smoothing: beams are on (crsdr_doa_set_beams or _set_subband_beams): their weights are %d-vectors from the %d x %d subspace: turn them off first", q->m,
                    q->m, q->m);
    { const int rc = doa_quiesce(q); if (rc) return rc; }
    // sv and vec change their shape: what the last submit left of the estimates is gone.  (Peaks, beams and the order keep their
    // own "submitted since": their fetches go on answering with that submit's values until the next one.)
    q->smooth = {}; q->last.ran &= ~(kRanBase | kRanSmooth);
    if (ms == q->m && !flags) return CRSDR_OK;
    const size_t nest = doa_capacity(q);
    if (q->smooth.rs.alloc(nest * ms * ms)) return fail(CRSDR_ENOMEM, "doa_set_smoothing: %zu bytes of device memory", sizeof(float2) * nest * ms * ms);
    q->smooth.on = true; q->smooth.sx = sx; q->smooth.sy = sy; q->smooth.flags = flags;
    return CRSDR_OK;
}

extern "C" int crsdr_doa_fetch_smoothed(crsdr_doa *q, float *rs)
{
    if (!q || !rs) return fail(CRSDR_EINVAL, "doa_fetch_smoothed: NULL doa or rs");
    if (!q->smooth.on) return fail(CRSDR_ESTATE, "doa_fetch_smoothed: no crsdr_doa_set_smoothing");
    if (!(q->last.ran & kRanSmooth)) return fail(CRSDR_ESTATE, "doa_fetch_smoothed: nothing submitted since crsdr_doa_set_smoothing");
    return DevFetch(q->device, q->last.stream).copy(rs, q->smooth.rs.p, (size_t)q->last.nest * (size_t)q->ms() * q->ms()).wait();
}

// ---- co-array augmentation (augment.hpp) ----
extern "C" int crsdr_doa_set_augment(crsdr_doa *q, int vx, int vy, uint64_t mask)
{
    if (!q) return fail(CRSDR_EINVAL, "doa_set_augment: NULL doa");
    if (vx != 0) {
        const int rc = augment_args_ok("doa_set_augment", q->mx, q->my, vx, vy, mask);
        if (rc) return rc;
        const int mv = vx * vy;
        if (q->k >= mv) return fail(CRSDR_EINVAL, "doa_set_augment: k = %d sources need a virtual array of more than %d elements (%d x %d)", q->k, q->k, vx, vy);
        if (q->order.crit && q->order.kmax >= mv)
            return fail(CRSDR_EINVAL, "doa_set_augment: the order range ends at kmax = %d, the virtual array of %d x %d has %d elements", q->order.kmax, vx, vy, mv);
        if (q->smooth.on)
            return fail(CRSDR_ESTATE, "doa_set_augment: smoothing is on (crsdr_doa_set_smoothing): the augmented matrix is block-Toeplitz and persymmetric already, smoothing it "
                                      "changes nothing: turn smoothing off first");
        if (q->beams.mode)
            return fail(CRSDR_ESTATE, "doa_set_augment: beams are on (crsdr_doa_set_beams or _set_subband_beams): the subspace would be the virtual array's, and weights from it are not "
                                      "the physical rows': turn them off first");
    }
    { const int rc = doa_quiesce(q); if (rc) return rc; }
    // sv and vec change their shape and every direction its array: nothing the last submit left stays
    q->augment = {}; q->last.ran = 0;
    if (vx == 0) return CRSDR_OK;
    const size_t nmat = doa_capacity(q), mv = (size_t)vx * vy;
    if (q->augment.ra.alloc(nmat * mv * mv)) return fail(CRSDR_ENOMEM, "doa_set_augment: %zu bytes of device memory", sizeof(float2) * nmat * mv * mv);
    q->augment.on = true; q->augment.vx = vx; q->augment.vy = vy; q->augment.mask = mask;
    return CRSDR_OK;
}

extern "C" int crsdr_doa_fetch_augmented(crsdr_doa *q, float *ra)
{
    if (!q || !ra) return fail(CRSDR_EINVAL, "doa_fetch_augmented: NULL doa or ra");
    if (!q->augment.on) return fail(CRSDR_ESTATE, "doa_fetch_augmented: no crsdr_doa_set_augment");
    if (!(q->last.ran & kRanAugment)) return fail(CRSDR_ESTATE, "doa_fetch_augmented: nothing submitted since crsdr_doa_set_augment");
    return DevFetch(q->device, q->last.stream).copy(ra, q->augment.ra.p, (size_t)q->last.nest * (size_t)q->ms() * q->ms()).wait();
}

extern "C" int crsdr_doa_augment_buffers(crsdr_doa *q, void **ra, int *vx, int *vy)
{
    if (!q) return fail(CRSDR_EINVAL, "doa_augment_buffers: NULL doa");
    if (ra) *ra = q->augment.ra;
    if (vx) *vx = q->augment.vx;
    if (vy) *vy = q->augment.vy;
    return CRSDR_OK;
}

extern "C" int crsdr_doa_set_order(crsdr_doa *q, int criterion, int kmin, int kmax, int limit_directions)
{
    if (!q) return fail(CRSDR_EINVAL, "doa_set_order: NULL doa");
    if (criterion != CRSDR_ORDER_OFF && criterion != CRSDR_ORDER_MDL && criterion != CRSDR_ORDER_AIC) return fail(CRSDR_EINVAL, "doa_set_order: criterion = %d", criterion);
    if (criterion != CRSDR_ORDER_OFF && (kmin < 1 || kmin > kmax || kmax >= q->ms()))
        return fail(CRSDR_EINVAL, "doa_set_order: k in %d .. %d (1 <= kmin <= kmax < %d, the subspace's size)", kmin, kmax, q->ms());
    { const int rc = doa_quiesce(q); if (rc) return rc; }
    q->order = {}; q->last.ran &= ~kRanOrder;
    if (criterion == CRSDR_ORDER_OFF) return CRSDR_OK;
    const size_t nest = doa_capacity(q), nc = (size_t)(kmax - kmin + 1);
    if (q->order.k.alloc(nest) || q->order.values.alloc(nest * nc)) {
        q->order = {};
        return fail(CRSDR_ENOMEM, "doa_set_order: device memory for %zu estimates of %zu candidates", nest, nc);
    }
    q->order.crit = criterion; q->order.kmin = kmin; q->order.kmax = kmax; q->order.limit_dirs = limit_directions != 0;
    return CRSDR_OK;
}

extern "C" int crsdr_doa_fetch_order(crsdr_doa *q, int32_t *k, float *criterion_values)
{
    if (!q) return fail(CRSDR_EINVAL, "doa_fetch_order: NULL doa");
    if (!q->order.crit) return fail(CRSDR_ESTATE, "doa_fetch_order: no crsdr_doa_set_order");
    if (!(q->last.ran & kRanOrder)) return fail(CRSDR_ESTATE, "doa_fetch_order: nothing submitted since crsdr_doa_set_order");
    const size_t nest = (size_t)q->last.nest, nc = (size_t)(q->order.kmax - q->order.kmin + 1);
    return DevFetch(q->device, q->last.stream).copy(k, q->order.k.p, nest).copy(criterion_values, q->order.values.p, nest * nc).wait();
}

extern "C" int crsdr_doa_order_buffers(crsdr_doa *q, void **k, void **criterion_values)
{
    if (!q) return fail(CRSDR_EINVAL, "doa_order_buffers: NULL doa");
    if (k) *k = q->order.k;
    if (criterion_values) *criterion_values = q->order.values;
    return CRSDR_OK;
}

// ---- one covariance per frequency band (subband.hpp) ----
// the bands' parameters (nfft = 0: off), nothing allocated yet
static void doa_subband_params(crsdr_doa *q, int nfft, int first, int nbands, int width, int window)
{
    q->sub = {};
    if (!nfft) return;
    DoaSubbands &sb = q->sub;
    sb.nfft = nfft; sb.log2 = ilog2_exact(nfft); sb.first = first; sb.nbands = nbands; sb.width = width; sb.window = window;
    sb.spb = subband::subband_spb(q->B, nfft); sb.groups = subband::subband_groups(q->m, nfft);
}

extern "C" int crsdr_doa_set_subbands(crsdr_doa *q, int nfft, int first, int nbands, int width, int window)
{
    if (!q) return fail(CRSDR_EINVAL, "doa_set_subbands: NULL doa");
    if (nfft != 0) {
        const int rc = subband_args_ok("doa_set_subbands", q->B, nfft, first, nbands, width, window);
        if (rc) return rc;
        if ((long long)(q->max_batch / q->frames) * nbands > kMaxDoaMatrices)
            return fail(CRSDR_EINVAL, "doa_set_subbands: %d estimates of %d bands (at most %d matrices per submit)", q->max_batch / q->frames, nbands, kMaxDoaMatrices);
    }
    if (q->peaks.count || q->beams.mode || q->smooth.on || q->order.crit)
        return fail(CRSDR_ESTATE, "doa_set_subbands: peaks, beams, smoothing or the source count are on: their buffers are sized by the bands, turn them off first");
    if (q->augment.on)
        return fail(CRSDR_ESTATE, "doa_set_subbands: augmentation is on (crsdr_doa_set_augment): its buffer is sized by the bands, turn it off first");
    { const int rc = doa_quiesce(q); if (rc) return rc; }
    q->last = {};                                        // the matrices change their number: what the last submit left is gone
    q->mat = {};
    doa_subband_params(q, nfft, first, nbands, width, window);
    int rc = doa_alloc_matrices(q);
    if (rc && nfft) {                                    // back to the plain engine, which fitted before
        q->mat = {};
        doa_subband_params(q, 0, 0, 1, 0, 0);
        (void)doa_alloc_matrices(q);
    }
    return rc;
}

extern "C" int crsdr_doa_fetch_subbands(crsdr_doa *q, float *power)
{
    if (!q || !power) return fail(CRSDR_EINVAL, "doa_fetch_subbands: NULL doa or power");
    if (!q->sub.nfft) return fail(CRSDR_ESTATE, "doa_fetch_subbands: no crsdr_doa_set_subbands");
    if (!(q->last.ran & kRanBase)) return fail(CRSDR_ESTATE, "doa_fetch_subbands: nothing submitted since crsdr_doa_set_subbands");
    return DevFetch(q->device, q->last.stream).copy(power, q->sub.power.p, (size_t)q->last.nest).wait();
}

extern "C" int crsdr_doa_subband_buffers(crsdr_doa *q, void **power)
{
    if (!q) return fail(CRSDR_EINVAL, "doa_subband_buffers: NULL doa");
    if (power) *power = q->sub.power;
    return CRSDR_OK;
}
