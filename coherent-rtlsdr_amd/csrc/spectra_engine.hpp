// spectra_engine.hpp -- the crsdr_spectra object behind include/crsdr.h, and its per-op form crsdr_welch.  Part of crsdr.hip's
// translation unit: included at its end, behind the plan (crsdr_spectra_submit_plan reads one) and behind every other kernel's first
// use, so that the existing kernels keep their places in the code object.
// (v) Welch spectra and reference cross-spectra (crsdr_spectra): per line of `frames` packets the auto-spectrum of every row, every
//     row's cross-spectrum against row 0 and four alignment figures per row (spectra.hpp, spectra_align.hpp).  Every buffer, the
//     twiddle and window tables included, is made at create; a submit is three launches on one stream whatever the batch size
//     (reference spectra, rows, alignment figures), no lock, no allocation, no synchronisation.
#pragma once

#include "spectra.hpp"

// `launch` with LG = log2 nfft, 4 .. 12
#define SPECTRA_DISPATCH(lg, launch)                                                \
    switch (lg) {                                                                   \
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

constexpr int kSpectraLaunches = 3;
constexpr long long kSpectraMaxPoints = 1ll << 24;      // (max_batch / frames) * nrows * nfft

struct crsdr_spectra {
    DoaStream own;
    int nrows = 0, B = 0, device = 0, max_batch = 1, frames = 1, nfft = 0, lg = 0, overlap = 0, window = 0, lo = 0, hi = 0;
    DevBuf<float2> tw, ref, cross;
    DevBuf<float> win, psd, align;
    hipStream_t last_stream = nullptr;
    int last_nest = 0;
    bool submitted = false;
};

// what crsdr_spectra_create and crsdr_welch ask of the transform and the band
static int spectra_args_ok(const char *who, int nrows, int blocksize, int nfft, int overlap, int window, int lo, int hi)
{
    const int lg = ilog2_exact(nfft);
    if (lg < spectra::SP_MIN_LOG2 || lg > spectra::SP_MAX_LOG2) return fail(CRSDR_EINVAL, "%s: nfft = %d (a power of two in [16, 4096])", who, nfft);
    if (nrows < 2) return fail(CRSDR_EINVAL, "%s: nrows = %d (at least 2: row 0 and a signal row)", who, nrows);
    if (blocksize < 2 * nfft || blocksize % (2 * nfft) || blocksize > (1 << kMaxLog2Plan))
        return fail(CRSDR_EINVAL, "%s: blocksize = %d (a multiple of 2 nfft = %d, up to %d)", who, blocksize, 2 * nfft, 1 << kMaxLog2Plan);
    if (overlap != 0 && overlap != 1) return fail(CRSDR_EINVAL, "%s: overlap = %d (0: hop nfft, 1: hop nfft / 2)", who, overlap);
    if (window != CRSDR_WINDOW_RECT && window != CRSDR_WINDOW_HANN) return fail(CRSDR_EINVAL, "%s: window = %d", who, window);
    if (lo < -nfft / 2 || hi > nfft / 2 - 1 || lo >= hi)
        return fail(CRSDR_EINVAL, "%s: band %d .. %d (signed bins, -nfft/2 <= lo < hi <= nfft/2 - 1)", who, lo, hi);
    return CRSDR_OK;
}

static int spectra_tables(hipStream_t S, int nfft, int window, float2 *tw, float *win)
{
    hipLaunchKernelGGL(spectra::k_spectra_tables, dim3((unsigned)((nfft + spectra::SP_THREADS - 1) / spectra::SP_THREADS)), dim3(spectra::SP_THREADS), 0, S, nfft, window,
                       tw, win);
    HIP_TRY(hipGetLastError());
    return CRSDR_OK;
}

// the three launches, for the object and for crsdr_welch: the same kernels on the same arguments, so the same bits
static int spectra_enqueue(hipStream_t S, const int8_t *packets, size_t packet_stride, size_t matrix_offset, int nblocks, int nrows, int B, int frames, int lg, int overlap,
                           int window, int lo, int hi, const float2 *tw, const float *win, float2 *ref, float *psd, float2 *cross, float *align)
{
    const int N = 1 << lg, J = spectra::sp_segments(B, N, overlap), nest = nblocks / frames, spc = spectra::sp_spc(N);
    const dim3 gref((unsigned)((J + spc - 1) / spc), (unsigned)nblocks), grow((unsigned)nrows, (unsigned)nest);
    SPECTRA_DISPATCH(lg, hipLaunchKernelGGL((spectra::k_spectra<LG, true>), gref, dim3(spectra::SP_THREADS), 0, S, packets, packet_stride, matrix_offset, nrows, B, frames,
                                            overlap, window, tw, win, ref, psd, cross));
    HIP_TRY(hipGetLastError());
    SPECTRA_DISPATCH(lg, hipLaunchKernelGGL((spectra::k_spectra<LG, false>), grow, dim3(spectra::SP_THREADS), 0, S, packets, packet_stride, matrix_offset, nrows, B, frames,
                                            overlap, window, tw, win, ref, psd, cross));
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(spectra::k_spectra_align, grow, dim3(64), 0, S, (const float *)psd, (const float2 *)cross, nrows, N, lo, hi - lo + 1, align);
    HIP_TRY(hipGetLastError());
    return CRSDR_OK;
}

static void spectra_free(crsdr_spectra *q)
{
    if (!q) return;
    (void)hipSetDevice(q->device);
    if (q->submitted) (void)hipDeviceSynchronize();      // (the last submit's stream may be the caller's, and gone)
    delete q;                                            // the buffers, then the stream
}

extern "C" int crsdr_spectra_create(crsdr_spectra **spectra, const crsdr_spectra_desc *desc)
{
    if (!spectra || !desc) return fail(CRSDR_EINVAL, "spectra_create: NULL argument");
    *spectra = nullptr;
    const int mb = desc->max_batch ? desc->max_batch : 1, F = desc->frames ? desc->frames : 1;
    { const int rc_ = spectra_args_ok("spectra_create", desc->nrows, desc->blocksize, desc->nfft, desc->overlap, desc->window, desc->band_lo, desc->band_hi); if (rc_) return rc_; }
    if (mb < 1 || mb > kMaxBatch) return fail(CRSDR_EINVAL, "spectra_create: max_batch = %d (1..%d)", mb, kMaxBatch);
    if (F < 1 || F > mb) return fail(CRSDR_EINVAL, "spectra_create: frames = %d (1..max_batch = %d)", desc->frames, mb);
    if ((long long)(mb / F) * desc->nrows * desc->nfft > kSpectraMaxPoints)
        return fail(CRSDR_EINVAL, "spectra_create: (max_batch / frames) * nrows * nfft = %lld (at most 2^24)", (long long)(mb / F) * desc->nrows * desc->nfft);
    { int rc = require_device(); if (rc) return rc; }
    int ndev = 0;
    (void)crsdr_device_count(&ndev);
    if (desc->device < 0 || desc->device >= ndev) return fail(CRSDR_ENODEV, "spectra_create: device %d of %d", desc->device, ndev);

    crsdr_spectra *q = new (std::nothrow) crsdr_spectra();
    if (!q) return fail(CRSDR_ENOMEM, "spectra_create: out of host memory");
    q->nrows = desc->nrows; q->B = desc->blocksize; q->device = desc->device; q->max_batch = mb; q->frames = F; q->nfft = desc->nfft; q->lg = ilog2_exact(desc->nfft);
    q->overlap = desc->overlap; q->window = desc->window; q->lo = desc->band_lo; q->hi = desc->band_hi;
    const size_t N = (size_t)q->nfft, J = (size_t)spectra::sp_segments(q->B, q->nfft, q->overlap), lines = (size_t)(mb / F) * (size_t)q->nrows;
    int rc = [&]() -> int {
        HIP_TRY(hipSetDevice(q->device));
        HIP_TRY(hipStreamCreateWithFlags(&q->own.s, hipStreamNonBlocking));
        int r = CRSDR_OK;
        if ((r = q->tw.alloc(N)) || (r = q->win.alloc(N)) || (r = q->ref.alloc((size_t)mb * J * N)) || (r = q->psd.alloc(lines * N)) || (r = q->cross.alloc(lines * N)) ||
            (r = q->align.alloc(lines * 4)))
            return r;
        if ((r = spectra_tables(q->own.s, q->nfft, q->window, q->tw, q->win))) return r;
        HIP_TRY(hipStreamSynchronize(q->own.s));         // a submit may come on any stream
        return CRSDR_OK;
    }();
    if (rc) { spectra_free(q); return rc; }
    *spectra = q;
    return CRSDR_OK;
}

extern "C" int crsdr_spectra_destroy(crsdr_spectra *spectra)
{
    if (!spectra) return fail(CRSDR_EINVAL, "spectra_destroy: NULL spectra");
    spectra_free(spectra);
    return CRSDR_OK;
}

static int spectra_launch(crsdr_spectra *q, const int8_t *packets, size_t packet_stride, size_t matrix_offset, int nblocks, hipStream_t S)
{
    const int rc = spectra_enqueue(S, packets, packet_stride, matrix_offset, nblocks, q->nrows, q->B, q->frames, q->lg, q->overlap, q->window, q->lo, q->hi, q->tw, q->win,
                                   q->ref, q->psd, q->cross, q->align);
    if (rc) return rc;
    q->last_stream = S; q->last_nest = nblocks / q->frames; q->submitted = true;
    return CRSDR_OK;
}

extern "C" int crsdr_spectra_submit(crsdr_spectra *q, const void *device_packets, size_t packet_stride, size_t matrix_offset, int nblocks, void *hip_stream)
{
    if (!q || !device_packets) return fail(CRSDR_EINVAL, "spectra_submit: NULL spectra or packets");
    if (nblocks < 1 || nblocks > q->max_batch || nblocks % q->frames)
        return fail(CRSDR_EINVAL, "spectra_submit: nblocks = %d (1..max_batch = %d, a multiple of frames = %d)", nblocks, q->max_batch, q->frames);
    if (((uintptr_t)device_packets + matrix_offset) % 4 || packet_stride % 4)
        return fail(CRSDR_EINVAL, "spectra_submit: matrix start and packet stride must be 4-byte aligned");
    if (nblocks > 1 && packet_stride < (size_t)q->nrows * (size_t)q->B)
        return fail(CRSDR_EINVAL, "spectra_submit: packet_stride = %zu is smaller than a matrix of %d x %d", packet_stride, q->nrows, q->B);
    HIP_TRY(hipSetDevice(q->device));
    return spectra_launch(q, (const int8_t *)device_packets, packet_stride, matrix_offset, nblocks, hip_stream ? (hipStream_t)hip_stream : q->own.s);
}

extern "C" int crsdr_spectra_submit_plan(crsdr_spectra *q, crsdr_plan *p)
{
    if (!q || !p) return fail(CRSDR_EINVAL, "spectra_submit_plan: NULL argument");
    if (p->nrows != q->nrows || p->B != q->B || p->device != q->device)
        return fail(CRSDR_EINVAL, "spectra_submit_plan: plan is %d x %d on device %d, spectra %d x %d on device %d", p->nrows, p->B, p->device, q->nrows, q->B, q->device);
    if (p->d_slab) return fail(CRSDR_ESTATE, "spectra_submit_plan: the plan writes slabs (crsdr_plan_bind_slab): its packets hold no matrix");
    if (!p->submitted || p->last_nblocks < 1) return fail(CRSDR_ESTATE, "spectra_submit_plan: the plan has no submitted batch");
    if (p->last_nblocks > q->max_batch || p->last_nblocks % q->frames)
        return fail(CRSDR_EINVAL, "spectra_submit_plan: the plan's batch of %d blocks (spectra: at most %d, a multiple of frames = %d)", p->last_nblocks, q->max_batch,
                    q->frames);
    HIP_TRY(hipSetDevice(q->device));
    // the batch's last kernel is on p->stream: stream order alone puts the spectra behind it
    return spectra_launch(q, p->d_packet, p->packet_stride, p->matrix_off, p->last_nblocks, p->stream);
}

extern "C" int crsdr_spectra_last_submit(crsdr_spectra *q, int *nest, int *launches)
{
    if (!q) return fail(CRSDR_EINVAL, "spectra_last_submit: NULL spectra");
    if (!q->submitted) return fail(CRSDR_ESTATE, "spectra_last_submit: nothing submitted");
    if (nest) *nest = q->last_nest;
    if (launches) *launches = kSpectraLaunches;
    return CRSDR_OK;
}

extern "C" int crsdr_spectra_fetch(crsdr_spectra *q, float *psd, float *cross, float *align)
{
    if (!q) return fail(CRSDR_EINVAL, "spectra_fetch: NULL spectra");
    if (!q->submitted) return fail(CRSDR_ESTATE, "spectra_fetch: nothing submitted");
    const size_t lines = (size_t)q->last_nest * (size_t)q->nrows, N = (size_t)q->nfft;
    return DevFetch(q->device, q->last_stream).copy(psd, q->psd.p, lines * N).copy(cross, q->cross.p, lines * N).copy(align, q->align.p, lines * 4).wait();
}

extern "C" int crsdr_spectra_device_buffers(crsdr_spectra *q, void **psd, void **cross, void **align)
{
    if (!q) return fail(CRSDR_EINVAL, "spectra_device_buffers: NULL spectra");
    if (psd) *psd = q->psd;
    if (cross) *cross = q->cross;
    if (align) *align = q->align;
    return CRSDR_OK;
}

extern "C" int crsdr_welch(float *psd, float *cross, float *align, const int8_t *matrix, int nrows, int blocksize, int nfft, int overlap, int window, int band_lo,
                           int band_hi, int mem_kind)
{
    if (!matrix || (!psd && !cross && !align)) return fail(CRSDR_EINVAL, "welch: need matrix and at least one of psd, cross, align");
    { const int rc_ = spectra_args_ok("welch", nrows, blocksize, nfft, overlap, window, band_lo, band_hi); if (rc_) return rc_; }
    if ((long long)nrows * nfft > kSpectraMaxPoints) return fail(CRSDR_EINVAL, "welch: nrows * nfft = %lld (at most 2^24)", (long long)nrows * nfft);
    OP_PROLOGUE_MEM("welch", mem_kind);
    const int lg = ilog2_exact(nfft);
    const size_t N = (size_t)nfft, J = (size_t)spectra::sp_segments(blocksize, nfft, overlap), mb = (size_t)nrows * (size_t)blocksize;
    const size_t pb = sizeof(float) * (size_t)nrows * N, cb = 2 * pb, ab = sizeof(float) * 4 * (size_t)nrows;
    OpStage st(mem_kind);
    const int8_t *d_m = (const int8_t *)st.in(0, matrix, mb, 4);
    float *d_p = (float *)st.out(1, psd, pb, 4);
    float2 *d_c = (float2 *)st.out(2, cross, cb, 8);
    float *d_a = (float *)st.out(3, align, ab, 4);
    if (st.rc) return st.rc;
    if (st.misaligned) return fail(CRSDR_EINVAL, "welch: device matrix, psd and align 4-byte, cross 8-byte aligned");
    if (st.spare(1, d_p, pb) || st.spare(2, d_c, cb) || st.spare(3, d_a, ab)) return st.rc;
    OP_RESERVE(4, sizeof(float2) * N + sizeof(float) * N);
    OP_RESERVE(5, sizeof(float2) * J * N);
    float2 *tw = (float2 *)g_op.buf[4];
    float *win = (float *)(tw + N);
    { const int rc_ = spectra_tables(0, nfft, window, tw, win); if (rc_) return rc_; }
    { const int rc_ = spectra_enqueue(0, d_m, mb, 0, 1, nrows, blocksize, 1, lg, overlap, window, band_lo, band_hi, tw, win, (float2 *)g_op.buf[5], d_p, d_c, d_a); if (rc_) return rc_; }
    st.back(psd, d_p, pb);
    st.back(cross, d_c, cb);
    st.back(align, d_a, ab);
    return st.finish();
}
