#include "cspectra.h"

#include <cmath>
#include <cstdio>

namespace cspectra {

batch::batch(int nrows, int blocksize, int max_batch, int nfft, bool half_overlap, int window, int band_lo, int band_hi, int frames, int device) : rows(nrows), n(nfft)
{
    crsdr_spectra_desc desc = {};
    desc.nrows = nrows; desc.blocksize = blocksize; desc.device = device; desc.max_batch = max_batch; desc.frames = frames; desc.nfft = nfft;
    desc.overlap = half_overlap ? 1 : 0; desc.window = window;
    desc.band_lo = band_lo == band_hi ? -(nfft / 4) : band_lo;
    desc.band_hi = band_lo == band_hi ? nfft / 4 : band_hi;
    if (crsdr_spectra_create(&sp, &desc)) { std::fprintf(stderr, "cspectra::batch: %s\n", crsdr_last_error()); sp = nullptr; }
}

batch::~batch()
{
    if (sp) crsdr_spectra_destroy(sp);
}

int batch::submit(crsdr_plan *plan)
{
    int rc = sp ? crsdr_spectra_submit_plan(sp, plan) : CRSDR_ESTATE;
    if (rc && sp) std::fprintf(stderr, "cspectra::batch: %s\n", crsdr_last_error());
    return rc;
}

int batch::submit(const void *device_packets, size_t packet_stride, size_t matrix_offset, int nblocks, void *hip_stream)
{
    int rc = sp ? crsdr_spectra_submit(sp, device_packets, packet_stride, matrix_offset, nblocks, hip_stream) : CRSDR_ESTATE;
    if (rc && sp) std::fprintf(stderr, "cspectra::batch: %s\n", crsdr_last_error());
    return rc;
}

int batch::fetch(bool want_psd, bool want_cross)
{
    int nest = 0;
    int rc = sp ? crsdr_spectra_last_submit(sp, &nest, nullptr) : CRSDR_ESTATE;
    if (!rc) {
        const size_t lr = (size_t)nest * rows;
        psd.assign(want_psd ? lr * n : 0, 0.f); cross.assign(want_cross ? 2 * lr * n : 0, 0.f); align.assign(4 * lr, 0.f);
        rc = crsdr_spectra_fetch(sp, want_psd ? psd.data() : nullptr, want_cross ? cross.data() : nullptr, align.data());
    }
    if (!rc) nlines = nest;
    if (rc && sp) std::fprintf(stderr, "cspectra::batch: %s\n", crsdr_last_error());
    return rc;
}

int batch::strongest_bin(int e, int c, double *db) const
{
    const size_t o = ((size_t)e * rows + c) * n;
    if (psd.size() < o + n) return -1;
    int best = 0;
    for (int f = 1; f < n; ++f)
        if (psd[o + f] > psd[o + best]) best = f;
    if (db) *db = psd[o + best] > 0.f ? 10.0 * std::log10((double)psd[o + best]) : -INFINITY;
    return best;
}
}
