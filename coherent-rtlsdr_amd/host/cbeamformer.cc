#include "cbeamformer.h"

#include <cstdio>
#include <cstring>

namespace cbeamformer {

int covariance(const int8_t *packet, cmatrix &Rxx, int &M)
{
    uint32_t cols, rows;
    std::memcpy(&cols, packet + 4, 4);
    std::memcpy(&rows, packet + 8, 4);
    if (cols < 2 || rows < 16) return CRSDR_EINVAL;
    M = (int)cols - 1;
    Rxx.assign((size_t)M * M, {0.f, 0.f});
    int rc = crsdr_covariance(reinterpret_cast<float *>(Rxx.data()), packet + 16 + 4 * (size_t)cols, (int)cols, 2 * (int)rows, CRSDR_MEM_HOST);
    if (rc) std::fprintf(stderr, "covariance: %s\n", crsdr_last_error());
    return rc;
}

int noisesubspace(const cmatrix &Rxx, int M, cmatrix &U, std::vector<float> *S)
{
    U.assign((size_t)M * M, {0.f, 0.f});
    if (S) S->assign(M, 0.f);
    int rc = crsdr_noisesubspace(reinterpret_cast<float *>(U.data()), S ? S->data() : nullptr,
                                 reinterpret_cast<const float *>(Rxx.data()), M, CRSDR_MEM_HOST);
    if (rc) std::fprintf(stderr, "noisesubspace: %s\n", crsdr_last_error());
    return rc;
}

int pmusic2dvec(const cmatrix &U, int M, int K, float d, int Mx, int My, int Cx, int Cy, std::vector<float> &pm)
{
    pm.assign((size_t)Cx * Cy, 0.f);
    int rc = crsdr_pmusic2d(pm.data(), reinterpret_cast<const float *>(U.data()), M, K, d, Mx, My, Cx, Cy, CRSDR_MEM_HOST);
    if (rc) std::fprintf(stderr, "pmusic2dvec: %s\n", crsdr_last_error());
    return rc;
}

int pspectrum2dvec(const cmatrix &U, const std::vector<float> &S, int M, int kind, float loading, float d, int Mx, int My, int Cx, int Cy,
                   std::vector<float> &pm)
{
    // (the sizes that decide the allocation below are checked here, ahead of it; the rest by crsdr_spectrum2d)
    if (M < 0 || U.size() != (size_t)M * M || S.size() != (size_t)M || Cx < 1 || Cy < 1 || (long long)Cx * Cy > (1 << 24)) return CRSDR_EINVAL;
    pm.assign((size_t)Cx * Cy, 0.f);
    int rc = crsdr_spectrum2d(pm.data(), reinterpret_cast<const float *>(U.data()), S.data(), M, kind, loading, d, Mx, My, Cx, Cy, CRSDR_MEM_HOST);
    if (rc) std::fprintf(stderr, "pspectrum2dvec: %s\n", crsdr_last_error());
    return rc;
}

batch::batch(int nrows, int blocksize, int max_batch, int K, int frames, bool keep_spectrum, float d, int Mx, int My, int Cx, int Cy, int device)
    : m(nrows - 1), ms(nrows - 1), cx(Cx), cy(Cy), half(blocksize / 2), nframes(frames > 0 ? frames : 1), keep(keep_spectrum)
{
    crsdr_doa_desc desc = {};
    desc.nrows = nrows; desc.blocksize = blocksize; desc.device = device; desc.max_batch = max_batch; desc.frames = frames; desc.k = K;
    desc.mx = Mx; desc.my = My; desc.ncx = Cx; desc.ncy = Cy; desc.d = d;
    desc.flags = keep_spectrum ? CRSDR_DOA_KEEP_SPECTRUM : 0u;
    if (crsdr_doa_create(&doa, &desc)) { std::fprintf(stderr, "cbeamformer::batch: %s\n", crsdr_last_error()); doa = nullptr; }
}

batch::~batch()
{
    if (doa) crsdr_doa_destroy(doa);
}

int batch::submit(crsdr_plan *plan)
{
    int rc = doa ? crsdr_doa_submit_plan(doa, plan) : CRSDR_ESTATE;
    if (rc && doa) std::fprintf(stderr, "cbeamformer::batch: %s\n", crsdr_last_error());
    return rc;
}

int batch::submit(const void *device_packets, size_t packet_stride, size_t matrix_offset, int nblocks, void *hip_stream)
{
    int rc = doa ? crsdr_doa_submit(doa, device_packets, packet_stride, matrix_offset, nblocks, hip_stream) : CRSDR_ESTATE;
    if (rc && doa) std::fprintf(stderr, "cbeamformer::batch: %s\n", crsdr_last_error());
    return rc;
}

int batch::set_peaks(int count, int radius)
{
    int rc = doa ? crsdr_doa_set_peaks(doa, count, radius) : CRSDR_ESTATE;
    if (!rc) npeaks = count;
    if (rc && doa) std::fprintf(stderr, "cbeamformer::batch: %s\n", crsdr_last_error());
    return rc;
}

int batch::set_beams(int mode, float loading, int nfixed, const float *fixed_angles)
{
    int rc = doa ? crsdr_doa_set_beams(doa, mode, loading, nfixed, fixed_angles) : CRSDR_ESTATE;
    if (!rc) rc = crsdr_doa_beam_buffers(doa, nullptr, nullptr, nullptr, &nbeams);
    if (rc && doa) std::fprintf(stderr, "cbeamformer::batch: %s\n", crsdr_last_error());
    return rc;
}

int batch::set_smoothing(int sx, int sy, bool fb)
{
    int rc = doa ? crsdr_doa_set_smoothing(doa, sx, sy, fb ? CRSDR_SMOOTH_FB : 0u) : CRSDR_ESTATE;
    if (!rc) ms = sx * sy;
    if (rc && doa) std::fprintf(stderr, "cbeamformer::batch: %s\n", crsdr_last_error());
    return rc;
}

int batch::set_augment(int vx, int vy, uint64_t mask)
{
    int rc = doa ? crsdr_doa_set_augment(doa, vx, vy, mask) : CRSDR_ESTATE;
    if (!rc) {
        ms = vx ? vx * vy : m;
        aug_x = vx; aug_y = vx ? vy : 0;
        aug_receivers = 0;
        for (int i = 0; vx && i < m; ++i) aug_receivers += mask ? (int)((mask >> i) & 1u) : 1;
    }
    if (rc && doa) std::fprintf(stderr, "cbeamformer::batch: %s\n", crsdr_last_error());
    return rc;
}

int batch::set_order(int criterion, int kmin, int kmax, bool limit_directions)
{
    int rc = doa ? crsdr_doa_set_order(doa, criterion, kmin, kmax > 0 ? kmax : ms - 1, limit_directions ? 1 : 0) : CRSDR_ESTATE;
    if (!rc) counted = criterion != CRSDR_ORDER_OFF;
    if (rc && doa) std::fprintf(stderr, "cbeamformer::batch: %s\n", crsdr_last_error());
    return rc;
}

int batch::set_subbands(int nfft, int first, int count, int width, int window)
{
    int rc = doa ? crsdr_doa_set_subbands(doa, nfft, first, count, width, window) : CRSDR_ESTATE;
    if (!rc) { nbands = nfft ? count : 0; band_j = nfft ? half / nfft : 0; band_width = nfft ? width : 0; }
    if (rc && doa) std::fprintf(stderr, "cbeamformer::batch: %s\n", crsdr_last_error());
    return rc;
}

int batch::set_spectrum(int kind, float loading)
{
    int rc = doa ? crsdr_doa_set_spectrum(doa, kind, loading) : CRSDR_ESTATE;
    if (rc && doa) std::fprintf(stderr, "cbeamformer::batch: %s\n", crsdr_last_error());
    return rc;
}

int batch::set_refine(int levels)
{
    int rc = doa ? crsdr_doa_set_refine(doa, levels) : CRSDR_ESTATE;
    if (!rc) refining = levels;
    if (rc && doa) std::fprintf(stderr, "cbeamformer::batch: %s\n", crsdr_last_error());
    return rc;
}

int batch::set_esprit(int mode)
{
    int rc = doa ? crsdr_doa_set_esprit(doa, mode) : CRSDR_ESTATE;
    if (!rc) esprit_mode = mode;
    if (rc && doa) std::fprintf(stderr, "cbeamformer::batch: %s\n", crsdr_last_error());
    return rc;
}

int batch::set_subband_beams(int mode, float loading, int nfixed, const float *fixed_angles)
{
    int rc = doa ? crsdr_doa_set_subband_beams(doa, mode, loading, nfixed, fixed_angles) : CRSDR_ESTATE;
    if (!rc) rc = crsdr_doa_subband_beam_buffers(doa, nullptr, nullptr, nullptr, &nbandbeams);
    if (rc && doa) std::fprintf(stderr, "cbeamformer::batch: %s\n", crsdr_last_error());
    return rc;
}

int batch::fetch(bool want_beams)
{
    int nest = 0;
    int rc = doa ? crsdr_doa_last_submit(doa, &nest, nullptr) : CRSDR_ESTATE;
    if (!rc) {
        peak.assign(2 * (size_t)nest, 0); peak_value.assign(nest, 0.f); sv.assign((size_t)nest * ms, 0.f); status.assign(nest, 0);
        if (keep) pm.assign((size_t)nest * cx * cy, 0.f);
        // CRSDR_ESPRIT_ONLY: no scan ran, peak and peak_value keep their zeros and pm is not asked for
        const bool scan = esprit_mode != CRSDR_ESPRIT_ONLY;
        rc = crsdr_doa_fetch(doa, scan ? peak.data() : nullptr, scan ? peak_value.data() : nullptr, sv.data(), status.data(), keep && scan ? pm.data() : nullptr, nullptr);
    }
    if (!rc && esprit_mode) {
        rc = crsdr_doa_esprit_buffers(doa, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &nesprit);
        const size_t n = (size_t)nest * nesprit;
        esprit_found.assign(nest, 0); esprit_status.assign(nest, 0); esprit_phases.assign(2 * n, 0.0); esprit_angles.assign(2 * n, -1.f);
        esprit_modulus.assign(2 * n, -1.f); esprit_power.assign(n, -1.f); esprit_flags.assign(n, 0);
        if (!rc)
            rc = crsdr_doa_fetch_esprit(doa, esprit_found.data(), esprit_status.data(), esprit_phases.data(), esprit_angles.data(), esprit_modulus.data(),
                                        esprit_power.data(), esprit_flags.data());
    }
    if (!rc && nbands) {
        band_power.assign(nest, 0.f);
        rc = crsdr_doa_fetch_subbands(doa, band_power.data());
    }
    if (!rc && counted) {
        order.assign(nest, 0);
        rc = crsdr_doa_fetch_order(doa, order.data(), nullptr);
    }
    if (!rc && npeaks) {
        found.assign(nest, 0); directions.assign((size_t)nest * npeaks * 2, -1); direction_values.assign((size_t)nest * npeaks, -1.f);
        rc = crsdr_doa_fetch_directions(doa, found.data(), directions.data(), direction_values.data());
    }
    if (!rc && refining) {
        rc = crsdr_doa_refined_buffers(doa, nullptr, nullptr, nullptr, &nrefined);
        const size_t n = (size_t)nest * nrefined;
        refined_offsets.assign(2 * n, 0.f); refined_angles.assign(2 * n, -1.f); refined_values.assign(n, -1.f);
        if (!rc) rc = crsdr_doa_fetch_refined(doa, refined_offsets.data(), refined_angles.data(), refined_values.data());
    }
    if (!rc && nbeams) {
        weights.assign((size_t)nest * nbeams * m, {0.f, 0.f}); beam_power.assign((size_t)nest * nbeams, -1.f);
        if (want_beams) beams.assign((size_t)nest * nframes * nbeams * half, {0.f, 0.f});
        rc = crsdr_doa_fetch_beams(doa, reinterpret_cast<float *>(weights.data()), beam_power.data(),
                                   want_beams ? reinterpret_cast<float *>(beams.data()) : nullptr);
    }
    if (!rc && nbandbeams) {
        // nest counts (estimate, band) pairs: nest / nbands estimates of nframes blocks each
        band_weights.assign((size_t)nest * nbandbeams * m, {0.f, 0.f}); band_beam_power.assign((size_t)nest * nbandbeams, -1.f);
        if (want_beams) band_beams.assign((size_t)nest * nframes * nbandbeams * band_j * band_width, {0.f, 0.f});
        rc = crsdr_doa_fetch_subband_beams(doa, reinterpret_cast<float *>(band_weights.data()), band_beam_power.data(),
                                           want_beams ? reinterpret_cast<float *>(band_beams.data()) : nullptr);
    }
    if (rc && doa) std::fprintf(stderr, "cbeamformer::batch: %s\n", crsdr_last_error());
    return rc;
}

} // namespace cbeamformer
