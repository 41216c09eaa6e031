// cspectra -- the packets' spectra: a small class over crsdr_spectra (include/crsdr.h, section (v)), as cbeamformer::batch is over
// crsdr_doa.  What the reference's clients compute on the host from fetched packets (matlabclient/testchannels.m: a power spectrum per
// channel; matlabclient/seqnum_and_correlation.m: every column against column 1), on the device and on the packets as published.
#ifndef CSPECTRA_H
#define CSPECTRA_H
#include <cstddef>
#include <vector>

#include "../../include/crsdr.h"

namespace cspectra {

// One line per `frames` consecutive packets of a submit: the Welch auto-spectrum of every row (row 0 included), every row's
// cross-spectrum against row 0 and (delay, phase, gain, coherence) per row over the signed bins band_lo .. band_hi.
class batch {
    crsdr_spectra *sp = nullptr;
    int rows, n;

public:
    // band_lo == band_hi: the default band, +-nfft / 4
    batch(int nrows, int blocksize, int max_batch, int nfft, bool half_overlap = true, int window = CRSDR_WINDOW_HANN, int band_lo = 0, int band_hi = 0, int frames = 1,
          int device = 0);
    ~batch();
    batch(const batch &) = delete;
    batch &operator=(const batch &) = delete;
    bool ok() const { return sp != nullptr; }
    // the plan's last batch, behind it on the plan's stream; or packets anywhere on the device.  Asynchronous.
    int submit(crsdr_plan *plan);
    int submit(const void *device_packets, size_t packet_stride, size_t matrix_offset, int nblocks, void *hip_stream = nullptr);
    // waits, and fills what is asked for
    int fetch(bool want_psd = true, bool want_cross = false);
    int lines() const { return nlines; }
    int nrows() const { return rows; }
    int nfft() const { return n; }
    std::vector<float> psd;                          // [lines][nrows][nfft]
    std::vector<float> cross;                        // [lines][nrows][nfft][2]
    std::vector<float> align;                        // [lines][nrows][4]: delay (samples), phase (rad), gain, coherence
    // of line e, row c: the strongest bin (FFT order) of psd and its power in dB of full scale (needs want_psd)
    int strongest_bin(int e, int c, double *db = nullptr) const;

private:
    int nlines = 0;
};
}
#endif
