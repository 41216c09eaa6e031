// cbeamformer.h -- the first consumer of a published packet, with the function surface of the reference's
// beamformer client (beamformclient/heatmap2d2.cpp): packet -> covariance (:185-197) -> noisesubspace(Rxx, K)
// (:69-79) -> pmusic2dvec(Un, d, Mx, My, Cx, Cy) (:137-147).  Eigen types become plain row-major vectors;
// the arithmetic runs in libcrsdr.so (crsdr_covariance / crsdr_noisesubspace / crsdr_pmusic2d).
#ifndef CBEAMFORMERH
#define CBEAMFORMERH
#include <complex>
#include <cstdint>
#include <vector>

#include "../../include/crsdr.h"

typedef std::vector<std::complex<float>> cmatrix;   // row-major, dimensions carried by the caller

namespace cbeamformer {
// reference defaults: #define MX 7, MY 3 (:41-42), d = (1.225*1.24)/3 wavelengths (:198), 100 x 100 scan (:199)
constexpr int MX = 7, MY = 3, CX = 100, CY = 100;
constexpr float D = (1.225f * 1.24f) / 3.0f;

// Parses the packet header like main() (:296-300: cols = N at word 1, rows = L at word 2, data at 16 + 4*cols)
// and returns Rxx [(N-1)][(N-1)] of the signal channels (the first column is dropped, :190).
int covariance(const int8_t *packet, cmatrix &Rxx, int &M);
// U of the SVD ordered by singular value; Un = columns K .. M-1 (U.rightCols(M - K)).  S optional.
int noisesubspace(const cmatrix &Rxx, int M, cmatrix &U, std::vector<float> *S = nullptr);
// pm [Cx][Cy] row-major, not normalised
int pmusic2dvec(const cmatrix &U, int M, int K, float d, int Mx, int My, int Cx, int Cy, std::vector<float> &pm);
// the same grid as a power map in units of ((I + jQ) / 127)^2 (crsdr_spectrum2d): kind CRSDR_SPECTRUM_BARTLETT, a^H R a / M^2, or
// CRSDR_SPECTRUM_CAPON, 1 / a^H (R + loading S[0] I)^-1 a, from all of U and S as noisesubspace returns them.  No source count.
int pspectrum2dvec(const cmatrix &U, const std::vector<float> &S, int M, int kind, float loading, float d, int Mx, int My, int Cx, int Cy,
                   std::vector<float> &pm);

// The three steps above for a whole batch of packets where the engine's plan left them on the device (crsdr_doa): one submit, no
// host work per packet, a direction per `frames` consecutive blocks.  submit() only enqueues (on the plan's stream, behind the batch
// it reads); fetch() waits and fills the vectors below.  One submit at a time: fetch before the next.
class batch {
    crsdr_doa *doa = nullptr;
    int m = 0, ms = 0, cx = 0, cy = 0, npeaks = 0, nbeams = 0, half = 0, nframes = 1;      // ms: the subspace's size (m, or a sub-array's)
    bool counted = false;
    int refining = 0, nrefined = 0;                  // set_refine: levels; slots per estimate of the last fetch
    int esprit_mode = 0, nesprit = 0;                // set_esprit: the mode; slots per estimate of the last fetch
    bool keep = false;
    int nbands = 0;                                  // set_subbands: bands per estimate (0: off)
    int nbandbeams = 0, band_j = 0, band_width = 0;  // set_subband_beams: slots; set_subbands: segments per block, bins per band
    int aug_x = 0, aug_y = 0, aug_receivers = 0;     // set_augment: the virtual array (0: off), the receivers it is built from
public:
    // nrows x blocksize: the packets' geometry (1 + Mx * My rows); keep_spectrum: fetch() also fills pm
    batch(int nrows, int blocksize, int max_batch, int K = 1, int frames = 1, bool keep_spectrum = false, float d = D, int Mx = MX, int My = MY,
          int Cx = CX, int Cy = CY, int device = 0);
    ~batch();
    batch(const batch &) = delete;
    batch &operator=(const batch &) = delete;
    bool ok() const { return doa != nullptr; }
    int submit(crsdr_plan *plan);                    // the plan's last submitted batch
    int submit(const void *device_packets, size_t packet_stride, size_t matrix_offset, int nblocks, void *hip_stream = nullptr);
    // from the next submit on, the `count` strongest local maxima of each spectrum within a (2 radius + 1)^2 window as well
    // (crsdr_doa_set_peaks; count = 0: off).  Waits for the device if a submit was made.
    int set_peaks(int count, int radius = 1);
    // from the next submit on, a beam toward every direction of an estimate (crsdr_doa_set_beams: mode CRSDR_BEAM_*, the MVDR diagonal
    // loading as a fraction of the largest singular value) -- the count of set_peaks, or the one peak -- or toward nfixed (alpha, beta)
    // pairs in radians.  CRSDR_BEAM_OFF: off.  With following beams on, set_peaks is refused: turn them off first.
    int set_beams(int mode, float loading = 1e-2f, int nfixed = 0, const float *fixed_angles = nullptr);
    // from the next submit on, the covariance averaged over its sx x sy sub-arrays (fb: and with its backward image) feeds the subspace
    // (crsdr_doa_set_smoothing: coherent arrivals); sv then has sx * sy entries per estimate.  (Mx, My) without fb: off.  Discards the
    // last submit's results.  Refused while true sub-arrays and beams would be on together.
    int set_smoothing(int sx, int sy, bool fb = true);
    // from the next submit on, every estimate's source count (crsdr_doa_set_order: CRSDR_ORDER_MDL / CRSDR_ORDER_AIC over kmin .. kmax)
    // replaces K in its scan; limit_directions: set_peaks reports at most that many.  CRSDR_ORDER_OFF: off.
    int set_order(int criterion, int kmin = 1, int kmax = 0, bool limit_directions = false);      // kmax = 0: the largest, size - 1
    // from the next submit on, the covariance of a filled vx x vy virtual array, rebuilt from the per-lag averages over the receivers
    // of `mask` (bit i: element i is present; 0: all), feeds the subspace (crsdr_doa_set_augment: thinned arrays, dead receivers); sv then
    // has vx * vy entries per estimate and every direction is the virtual array's.  vx = 0: off.  Discards the last submit's results.
    // Refused while smoothing or beams are on, and for a mask that leaves a lag of the virtual array without a pair of receivers.
    int set_augment(int vx, int vy, uint64_t mask = 0);
    int virtual_x() const { return aug_x; }
    int virtual_y() const { return aug_y; }
    int receivers() const { return aug_receivers; }  // with set_augment: the receivers used
    // from the next submit on, one covariance per (estimate, band) in place of the time-domain one (crsdr_doa_set_subbands): band i is
    // `width` bins of an nfft-point transform from bin first + i * width on (FFT order, wrapping), window CRSDR_WINDOW_*.  Every vector
    // below then holds estimates() = blocks / frames * bands() entries, estimate e's band i at e * bands() + i, and band_power is
    // filled.  nfft = 0: off.  Before set_peaks, set_smoothing and set_order (refused while one of them or beams are on; the beams of
    // the bands are set_subband_beams).
    int set_subbands(int nfft, int first = 0, int count = 1, int width = 1, int window = CRSDR_WINDOW_RECT);
    // from the next submit on, the scan computes the Bartlett or the Capon power map (crsdr_doa_set_spectrum: kind CRSDR_SPECTRUM_*,
    // loading: Capon's diagonal loading as a fraction of the largest singular value) in place of the MUSIC pseudo-spectrum: pm, peak,
    // peak_value, the directions and the beams that follow them are then that map's, K and the source counts are not used.
    // CRSDR_SPECTRUM_MUSIC: back.  Any time; discards the last submit's results.
    int set_spectrum(int kind, float loading = 1e-2f);
    // from the next submit on, every direction (the slots of set_peaks, or the one peak) refined off the scan grid by `levels` levels
    // (1 .. 8) of the fp64 zoom search (crsdr_doa_set_refine); following beams then steer at the refined direction.  0: off.  Any time.
    int set_refine(int levels = 5);
    // with set_refine: per estimate and slot the offset from the grid point in cells [estimates][slots][2], (alpha, beta) in radians
    // [estimates][slots][2] and the map's value there [estimates][slots]; empty slots hold (0, 0), (-1, -1) and -1
    int refined_slots() const { return nrefined; }
    std::vector<float> refined_offsets, refined_angles, refined_values;
    // from the next submit on, the K directions of every estimate (its count's, with set_order) by 2-D ESPRIT on the signal subspace
    // (crsdr_doa_set_esprit): no grid, no search.  CRSDR_ESPRIT_BESIDE: beside the scan; CRSDR_ESPRIT_ONLY: in its place (no peak, no
    // spectrum; peaks, the refinement and beams that follow the directions must be off; the fetched angles can be the fixed_angles of
    // set_beams).  CRSDR_ESPRIT_OFF: off.  Any time.
    int set_esprit(int mode = CRSDR_ESPRIT_BESIDE);
    // with set_esprit: per estimate the directions found and the status; per estimate and slot the phases (mu, nu) [estimates][slots][2],
    // (alpha, beta) in radians [estimates][slots][2], (|lambda_x|, |lambda_y|) [estimates][slots][2] (about 1 for a plane wave), the
    // conventional power and the flags [estimates][slots]; slots by descending power, empty ones hold (0, 0), (-1, -1), (-1, -1), -1, 0
    int esprit_slots() const { return nesprit; }
    std::vector<int32_t> esprit_found, esprit_status, esprit_flags;
    std::vector<double> esprit_phases;
    std::vector<float> esprit_angles, esprit_modulus, esprit_power;
    int bands() const { return nbands; }
    std::vector<float> band_power;                   // with set_subbands: [estimates]: Re trace(R_band) / M, the squelch of a band's direction
    // with set_subbands on: from the next submit on, a beam per band toward every direction of that band (crsdr_doa_set_subband_beams;
    // the arguments of set_beams): the band's weights applied to the rows' band spectra, one narrowband IQ stream per (block, band, slot).
    // CRSDR_BEAM_OFF: off.  While on, set_subbands is refused, and set_peaks while the beams follow the directions.
    int set_subband_beams(int mode, float loading = 1e-2f, int nfixed = 0, const float *fixed_angles = nullptr);
    // with set_subband_beams: band_weights [estimates][slots][M] and band_beam_power [estimates][slots] (-1 in an empty slot), estimates
    // counting the bands as above, and, on request (fetch's want_beams), band_beams [blocks][bands][slots][segments][width]
    int band_beam_slots() const { return nbandbeams; }
    cmatrix band_weights, band_beams;
    std::vector<float> band_beam_power;
    // want_beams: also copy the beams' samples out (blocks x slots x blocksize / 2 complex floats)
    int fetch(bool want_beams = false);
    int estimates() const { return (int)status.size(); }
    std::vector<int32_t> peak;                       // [estimates][2]: (cx, cy) of the largest pm
    std::vector<float> peak_value, sv, pm;           // [estimates], [estimates][M or sx * sy], [estimates][Cx][Cy] (keep_spectrum)
    std::vector<int32_t> status;                     // 0 = converged
    int subspace_size() const { return ms; }
    std::vector<int32_t> order;                      // with set_order: [estimates], the source counts
    // with set_peaks: local peaks found per estimate (<= count), their (cx, cy) [estimates][count][2] in descending order and their pm
    // [estimates][count]; slots from found on hold (-1, -1) and -1
    std::vector<int32_t> found, directions;
    std::vector<float> direction_values;
    // with set_beams: weights [estimates][slots][M], beam_power [estimates][slots] (-1 in an empty slot) and, on request, the beams
    // [blocks][slots][blocksize / 2]
    int beam_slots() const { return nbeams; }
    cmatrix weights, beams;
    std::vector<float> beam_power;
};
}
#endif
