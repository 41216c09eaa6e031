#include "ccaf.h"

#include <cmath>
#include <cstdio>

namespace ccaf {

static_assert(sizeof(peak_t) == 6 * sizeof(float), "peak_t is crsdr_caf's six floats");

static_assert(sizeof(det_t) == 8 * sizeof(float), "det_t is the detector's eight floats");

static_assert(sizeof(dir_t) == 8 * sizeof(float), "dir_t is the bearings' eight floats");

static_assert(sizeof(fused_t) == 8 * sizeof(float), "fused_t is the fusion's eight floats");

static_assert(sizeof(track_t) == 16 * sizeof(float), "track_t is the tracker's sixteen floats");

double fused_t::snr_db() const { return snr > 0.f ? 10.0 * std::log10((double)snr) : -INFINITY; }
double det_t::snr_db() const { return snr > 0.f ? 10.0 * std::log10((double)snr) : -INFINITY; }
double peak_t::power_db() const { return power > 0.f ? 10.0 * std::log10((double)power) : -INFINITY; }
double peak_t::ratio_db() const { return ratio > 0.f ? 10.0 * std::log10((double)ratio) : -INFINITY; }

batch::batch(int nrows, int blocksize, int max_batch, int seg, int nlags, int ref_row, int window, int guard, int frames, int device)
    : rows(nrows), bins(seg > 0 ? (frames > 0 ? frames : 1) * (blocksize / (2 * seg)) : 0), lags(nlags)
{
    crsdr_caf_desc desc = {};
    desc.nrows = nrows; desc.blocksize = blocksize; desc.device = device; desc.max_batch = max_batch; desc.frames = frames; desc.seg = seg; desc.nlags = nlags;
    desc.ref_row = ref_row; desc.window = window; desc.guard = guard;
    if (crsdr_caf_create(&cf, &desc)) { std::fprintf(stderr, "ccaf::batch: %s\n", crsdr_last_error()); cf = nullptr; }
}

batch::~batch()
{
    if (cf) crsdr_caf_destroy(cf);
}

int batch::submit(crsdr_plan *plan)
{
    int rc = cf ? crsdr_caf_submit_plan(cf, plan) : CRSDR_ESTATE;
    if (rc && cf) std::fprintf(stderr, "ccaf::batch: %s\n", crsdr_last_error());
    return rc;
}

int batch::submit(const void *device_packets, size_t packet_stride, size_t matrix_offset, int nblocks, void *hip_stream)
{
    int rc = cf ? crsdr_caf_submit(cf, device_packets, packet_stride, matrix_offset, nblocks, hip_stream) : CRSDR_ESTATE;
    if (rc && cf) std::fprintf(stderr, "ccaf::batch: %s\n", crsdr_last_error());
    return rc;
}

int batch::set_cfar(const crsdr_cfar_desc *desc)
{
    int rc = cf ? crsdr_caf_set_cfar(cf, desc) : CRSDR_ESTATE;
    if (!rc) { kdet = desc ? desc->max_det : 0; det.clear(); count.clear(); snap.clear(); }
    if (rc && cf) std::fprintf(stderr, "ccaf::batch: %s\n", crsdr_last_error());
    return rc;
}

int batch::set_cfar_estimator(const crsdr_cfar_est_desc *est)
{
    int rc = cf ? crsdr_caf_set_cfar_estimator(cf, est) : CRSDR_ESTATE;
    if (rc && cf) std::fprintf(stderr, "ccaf::batch: %s\n", crsdr_last_error());
    return rc;
}

int batch::fetch_cfar(bool want_snap)
{
    int nest = 0;
    int rc = !cf || !kdet ? CRSDR_ESTATE : crsdr_caf_last_submit(cf, &nest, nullptr);
    if (!rc) {
        const size_t maps = (size_t)nest * (rows + 1);
        det.assign(maps * kdet, det_t{}); count.assign(maps, 0); snap.assign(want_snap ? (size_t)nest * kdet * rows * 2 : 0, 0.f);
        rc = crsdr_caf_fetch_cfar(cf, &det[0].lag, count.data(), want_snap ? snap.data() : nullptr);
    }
    if (!rc) nlines = nest;
    if (rc && cf && kdet) std::fprintf(stderr, "ccaf::batch: %s\n", crsdr_last_error());
    return rc;
}

int batch::set_bearing(const crsdr_caf_bearing_desc *desc)
{
    int rc = cf ? crsdr_caf_set_bearing(cf, desc) : CRSDR_ESTATE;
    if (!rc) { bearings = desc != nullptr; npts = desc && (desc->flags & CRSDR_BEARING_KEEP_SPECTRUM) ? desc->ncx * desc->ncy : 0; dir.clear(); spec.clear(); }
    if (rc && cf) std::fprintf(stderr, "ccaf::batch: %s\n", crsdr_last_error());
    return rc;
}

int batch::fetch_bearing(bool want_spec)
{
    int nest = 0;
    int rc = !cf || !bearings ? CRSDR_ESTATE : crsdr_caf_last_submit(cf, &nest, nullptr);
    if (!rc) {
        want_spec = want_spec && npts > 0;
        dir.assign((size_t)nest * kdet, dir_t{}); spec.assign(want_spec ? (size_t)nest * kdet * npts : 0, 0.f);
        rc = crsdr_caf_fetch_bearing(cf, &dir[0].cx, want_spec ? spec.data() : nullptr);
    }
    if (!rc) nlines = nest;
    if (rc && cf && bearings) std::fprintf(stderr, "ccaf::batch: %s\n", crsdr_last_error());
    return rc;
}

int batch::set_beams(const crsdr_caf_beams_desc *desc)
{
    int rc = cf ? crsdr_caf_set_beams(cf, desc) : CRSDR_ESTATE;
    if (!rc) { nb = desc ? desc->nbeams : 0; beam_lists = desc && kdet > 0; adapt = false; aw.clear(); ainfo.clear(); astat.clear(); bmap.clear(); bdet.clear(); bcount.clear(); fused.clear(); nfused.clear(); }
    if (rc && cf) std::fprintf(stderr, "ccaf::batch: %s\n", crsdr_last_error());
    return rc;
}

int batch::fetch_beams(bool want_bmap, bool want_lists)
{
    int nest = 0;
    int rc = !cf || !nb ? CRSDR_ESTATE : crsdr_caf_last_submit(cf, &nest, nullptr);
    if (!rc) {
        want_lists = want_lists && beam_lists;
        const size_t maps = (size_t)nest * nb;
        bmap.assign(want_bmap ? maps * bins * lags : 0, 0.f);
        bdet.assign(want_lists ? maps * kdet : 0, det_t{}); bcount.assign(want_lists ? maps : 0, 0);
        fused.assign(beam_lists ? (size_t)nest * kdet : 0, fused_t{}); nfused.assign(beam_lists ? (size_t)nest : 0, 0);
        rc = crsdr_caf_fetch_beams(cf, want_bmap ? bmap.data() : nullptr, want_lists ? &bdet[0].lag : nullptr, want_lists ? bcount.data() : nullptr,
                                   beam_lists ? &fused[0].lag : nullptr, beam_lists ? nfused.data() : nullptr);
    }
    if (!rc) nlines = nest;
    if (rc && cf && nb) std::fprintf(stderr, "ccaf::batch: %s\n", crsdr_last_error());
    return rc;
}

int batch::set_beam_adapt(const crsdr_caf_beam_adapt_desc *desc)
{
    int rc = cf ? crsdr_caf_set_beam_adapt(cf, desc) : CRSDR_ESTATE;
    if (!rc) { adapt = desc != nullptr; aw.clear(); ainfo.clear(); astat.clear(); }
    if (rc && cf) std::fprintf(stderr, "ccaf::batch: %s\n", crsdr_last_error());
    return rc;
}

int batch::fetch_beam_adapt(bool want_aw)
{
    int nest = 0;
    int rc = !cf || !adapt ? CRSDR_ESTATE : crsdr_caf_last_submit(cf, &nest, nullptr);
    if (!rc) {
        const size_t beams = (size_t)nest * nb;
        aw.assign(want_aw ? beams * (rows - 1) * 2 : 0, 0.f);
        ainfo.assign(beams * 2, 0.f); astat.assign((size_t)nest, 0);
        rc = crsdr_caf_fetch_beam_adapt(cf, want_aw ? aw.data() : nullptr, ainfo.data(), astat.data());
    }
    if (!rc) nlines = nest;
    if (rc && cf && adapt) std::fprintf(stderr, "ccaf::batch: %s\n", crsdr_last_error());
    return rc;
}

int batch::set_track(const crsdr_caf_track_desc *desc)
{
    int rc = cf ? crsdr_caf_set_track(cf, desc) : CRSDR_ESTATE;
    if (!rc) { ntracks = desc ? desc->max_tracks : 0; trk.clear(); ntrk.clear(); }
    if (rc && cf) std::fprintf(stderr, "ccaf::batch: %s\n", crsdr_last_error());
    return rc;
}

int batch::reset_track()
{
    int rc = cf ? crsdr_caf_track_reset(cf) : CRSDR_ESTATE;
    if (rc && cf) std::fprintf(stderr, "ccaf::batch: %s\n", crsdr_last_error());
    return rc;
}

int batch::fetch_track()
{
    int nest = 0;
    int rc = !cf || !ntracks ? CRSDR_ESTATE : crsdr_caf_last_submit(cf, &nest, nullptr);
    if (!rc) {
        trk.assign((size_t)nest * ntracks, track_t{}); ntrk.assign((size_t)nest * 4, 0);
        rc = crsdr_caf_fetch_track(cf, &trk[0].id, ntrk.data());
    }
    if (!rc) nlines = nest;
    if (rc && cf && ntracks) std::fprintf(stderr, "ccaf::batch: %s\n", crsdr_last_error());
    return rc;
}

int batch::set_integrate(const crsdr_caf_integrate_desc *desc)
{
    int rc = cf ? crsdr_caf_set_integrate(cf, desc) : CRSDR_ESTATE;
    if (!rc) { iwhat = desc ? desc->what : 0; imap.clear(); ibmap.clear(); }
    if (rc && cf) std::fprintf(stderr, "ccaf::batch: %s\n", crsdr_last_error());
    return rc;
}

int batch::reset_integrate()
{
    int rc = cf ? crsdr_caf_integrate_reset(cf) : CRSDR_ESTATE;
    if (rc && cf) std::fprintf(stderr, "ccaf::batch: %s\n", crsdr_last_error());
    return rc;
}

int batch::fetch_integrate()
{
    int nest = 0;
    int rc = !cf || !iwhat ? CRSDR_ESTATE : crsdr_caf_last_submit(cf, &nest, nullptr);
    if (!rc) {
        const bool a = (iwhat & CRSDR_INTEGRATE_ARRAY) != 0, b = (iwhat & CRSDR_INTEGRATE_BEAMS) != 0;
        const size_t cells = (size_t)nest * bins * lags;
        imap.assign(a ? cells : 0, 0.f); ibmap.assign(b ? cells * nb : 0, 0.f);
        rc = crsdr_caf_fetch_integrate(cf, a ? imap.data() : nullptr, b ? ibmap.data() : nullptr);
    }
    if (!rc) nlines = nest;
    if (rc && cf && iwhat) std::fprintf(stderr, "ccaf::batch: %s\n", crsdr_last_error());
    return rc;
}

int batch::set_cancel(const crsdr_caf_cancel_desc *desc)
{
    int rc = cf ? crsdr_caf_set_cancel(cf, desc) : CRSDR_ESTATE;
    if (!rc) { nbasis = desc ? desc->taps * (2 * desc->dopp + 1) : 0; coef.clear(); cinfo.clear(); }
    if (rc && cf) std::fprintf(stderr, "ccaf::batch: %s\n", crsdr_last_error());
    return rc;
}

int batch::fetch_cancel(bool want_coef)
{
    int nest = 0;
    int rc = !cf || !nbasis ? CRSDR_ESTATE : crsdr_caf_last_submit(cf, &nest, nullptr);
    if (!rc) {
        coef.assign(want_coef ? (size_t)nest * rows * nbasis * 2 : 0, 0.f); cinfo.assign((size_t)nest * rows * 2, 0.f);
        rc = crsdr_caf_fetch_cancel(cf, want_coef ? coef.data() : nullptr, cinfo.data());
    }
    if (!rc) nlines = nest;
    if (rc && cf && nbasis) std::fprintf(stderr, "ccaf::batch: %s\n", crsdr_last_error());
    return rc;
}

int batch::set_clean(const crsdr_caf_clean_desc *desc)
{
    int rc = cf ? crsdr_caf_set_clean(cf, desc) : CRSDR_ESTATE;
    if (!rc) {
        ntargets = desc ? desc->max_targets : 0; nper = desc ? (2 * desc->wl + 1) * (2 * desc->wq + 1) : 0;
        tgt.clear(); ntgt.clear(); tcoef.clear(); tinfo.clear(); rdet.clear(); rcount.clear();
    }
    if (rc && cf) std::fprintf(stderr, "ccaf::batch: %s\n", crsdr_last_error());
    return rc;
}

int batch::fetch_clean(bool want_tcoef)
{
    int nest = 0;
    int rc = !cf || !ntargets ? CRSDR_ESTATE : crsdr_caf_last_submit(cf, &nest, nullptr);
    if (!rc) {
        const size_t maps = (size_t)nest * (rows + 1);
        tgt.assign((size_t)nest * ntargets, det_t{}); ntgt.assign((size_t)nest, 0); tinfo.assign((size_t)nest * rows * 2, 0.f);
        tcoef.assign(want_tcoef ? (size_t)nest * rows * ntargets * nper * 2 : 0, 0.f); rdet.assign(maps * kdet, det_t{}); rcount.assign(maps, 0);
        rc = crsdr_caf_fetch_clean(cf, &tgt[0].lag, ntgt.data(), want_tcoef ? tcoef.data() : nullptr, tinfo.data(), nullptr, nullptr, &rdet[0].lag, rcount.data(), nullptr);
    }
    if (!rc) nlines = nest;
    if (rc && cf && ntargets) std::fprintf(stderr, "ccaf::batch: %s\n", crsdr_last_error());
    return rc;
}

int batch::fetch(bool want_chi, bool want_map)
{
    int nest = 0;
    int rc = cf ? crsdr_caf_last_submit(cf, &nest, nullptr) : CRSDR_ESTATE;
    if (!rc) {
        const size_t cells = (size_t)nest * bins * lags;
        chi.assign(want_chi ? 2 * cells * rows : 0, 0.f); map.assign(want_map ? cells : 0, 0.f); peak.assign((size_t)nest * (rows + 1), peak_t{});
        rc = crsdr_caf_fetch(cf, want_chi ? chi.data() : nullptr, want_map ? map.data() : nullptr, &peak[0].lag);
    }
    if (!rc) nlines = nest;
    if (rc && cf) std::fprintf(stderr, "ccaf::batch: %s\n", crsdr_last_error());
    return rc;
}
}
