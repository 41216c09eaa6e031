// ccaf -- range-Doppler maps of the packets: a small class over crsdr_caf (include/crsdr.h, section (w)), as cspectra::batch is over
// crsdr_spectra.  Passive radar's front end, on the device and on the packets as published: every row against a reference row over
// delay and Doppler, the array map, and where each map peaks.
#ifndef CCAF_H
#define CCAF_H
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/crsdr.h"

namespace ccaf {

// (lag, doppler, power, ratio, dlag, ddop) of one map, as crsdr_caf lays them out
struct peak_t {
    float lag, doppler, power, ratio, dlag, ddop;
    double power_db() const;                         // of full scale, ((I + jQ) / 127)^2 = 1 against itself; -inf for 0
    double ratio_db() const;                         // the peak above the mean of the searched cells; -inf for 0
};

// (lag, doppler, power, snr, noise, dlag, ddop, ntrain) of one detection, as crsdr_caf's detector lays them out
struct det_t {
    float lag, doppler, power, snr, noise, dlag, ddop, ntrain;
    double snr_db() const;                           // the cell above its training cells' mean; -inf for 0
};

// (cx, cy, fit = T at the grid peak, dx, dy, alpha, beta, status) of one detection's bearing, as crsdr_caf's bearings lay them out
struct dir_t {
    float cx, cy, fit, dx, dy, alpha, beta, status;
    double alpha_deg() const { return (double)alpha * (180.0 / 3.14159265358979323846); }
    double beta_deg() const { return (double)beta * (180.0 / 3.14159265358979323846); }
};

// (lag, doppler, power, snr, noise, dlag, ddop, beam) of one fused detection of the beam maps, as crsdr_caf's beams lay them out
struct fused_t {
    float lag, doppler, power, snr, noise, dlag, ddop, beam;
    double snr_db() const;                           // the cell above its training cells' mean in its beam's map; -inf for 0
};

// (id, status, r, f, g, sigma_r, sigma_f, age, hits, misses, slot, d2, power, snr, aux0, aux1) of one track slot of one line, as crsdr_caf's
// tracker lays them out: status 0 free, 1 tentative, 2 confirmed, 3 ended in this line; r in lag cells, f in Doppler bins, g in bins per line
struct track_t {
    float id, status, r, f, g, sigma_r, sigma_f, age, hits, misses, slot, d2, power, snr, aux0, aux1;
    bool confirmed() const { return status == 2.f; }
};

// One line per `frames` consecutive packets of a submit: chi [nrows][nd][nlags] of every row against row ref_row over seg-sample
// segments, the array map [nd][nlags], and nrows + 1 peaks (the rows', then the map's) searched outside |Doppler| < guard.
class batch {
    crsdr_caf *cf = nullptr;
    int rows, bins, lags, kdet = 0, nbasis = 0, npts = 0;
    bool bearings = false, beam_lists = false, adapt = false;
    int nb = 0, ntracks = 0, iwhat = 0, ntargets = 0, nper = 0;

public:
    batch(int nrows, int blocksize, int max_batch, int seg, int nlags, int ref_row = 0, int window = CRSDR_WINDOW_RECT, int guard = 0, int frames = 1, int device = 0);
    ~batch();
    batch(const batch &) = delete;
    batch &operator=(const batch &) = delete;
    bool ok() const { return cf != nullptr; }
    // the plan's last batch, behind it on the plan's stream; or packets anywhere on the device.  Asynchronous.
    int submit(crsdr_plan *plan);
    int submit(const void *device_packets, size_t packet_stride, size_t matrix_offset, int nblocks, void *hip_stream = nullptr);
    // waits, and fills the peaks and what else is asked for
    int fetch(bool want_chi = false, bool want_map = false);
    // the CFAR detector behind every later submit (crsdr_caf_set_cfar; NULL: off).  Between submits: it waits for the last one.
    int set_cfar(const crsdr_cfar_desc *desc);
    // the noise estimate of the detector that is on (crsdr_caf_set_cfar_estimator; NULL: cell averaging).  Between submits, with the
    // bearings, beams and tracker off; every set_cfar puts it back to cell averaging.
    int set_cfar_estimator(const crsdr_cfar_est_desc *est);
    // waits, and fills count and det, and snap if asked for; CRSDR_ESTATE with the detector off
    int fetch_cfar(bool want_snap = true);
    int max_det() const { return kdet; }
    // the canceller in front of every later submit's Doppler stage (crsdr_caf_set_cancel; NULL: off).  Between submits, as set_cfar.
    int set_cancel(const crsdr_caf_cancel_desc *desc);
    // waits, and fills cinfo, and coef if asked for; CRSDR_ESTATE with the canceller off
    int fetch_cancel(bool want_coef = true);
    // a direction per detection of the array map behind every later submit (crsdr_caf_set_bearing; NULL: off).  Between submits, with
    // the detector on; while it is on set_cfar is refused.
    int set_bearing(const crsdr_caf_bearing_desc *desc);
    // waits, and fills dir beside det, and spec if asked for and kept; CRSDR_ESTATE with the bearings off
    int fetch_bearing(bool want_spec = false);
    // coherent beam maps across the rows behind every later submit (crsdr_caf_set_beams; NULL: off), weights [nbeams][nrows - 1][2].
    // Between submits; with the detector on at this call every beam map is detected on and the lists are fused into one per line;
    // while beams are on set_cfar is refused.
    int set_beams(const crsdr_caf_beams_desc *desc);
    // waits, and fills fused and nfused (with the detector), and bmap, bdet and bcount if asked for; CRSDR_ESTATE with the beams off
    int fetch_beams(bool want_bmap = false, bool want_lists = false);
    int nbeams() const { return nb; }
    // per line MVDR weights from the covariance of the line's own training cells in place of the beams' weights
    // (crsdr_caf_set_beam_adapt; NULL: off).  Between submits, with beams on and the integration and the tracker off; every
    // set_beams turns it off again.
    int set_beam_adapt(const crsdr_caf_beam_adapt_desc *desc);
    // waits, and fills ainfo and astat, and aw if asked for; CRSDR_ESTATE with the adaptation off
    int fetch_beam_adapt(bool want_aw = false);
    bool adaptive() const { return adapt; }
    // the tracker behind every later submit's lists (crsdr_caf_set_track; NULL: off), its table empty.  Between submits, with the
    // detector on (the fused source: with beams detected on); while it is on set_cfar, set_bearing and set_beams are refused.
    int set_track(const crsdr_caf_track_desc *desc);
    // the empty table again, ids from 1
    int reset_track();
    // waits, and fills trk and ntrk: the tracks of every line of the last submit; CRSDR_ESTATE with the tracker off
    int fetch_track();
    int max_tracks() const { return ntracks; }
    // the maps integrated across lines along the range walk, ahead of the detector (crsdr_caf_set_integrate; NULL: off), the state
    // empty.  Between submits, with bearings and the tracker off (CRSDR_INTEGRATE_BEAMS: with beams on); while it is on set_beams is
    // refused.  With it on det's entry nrows, and the beams' lists, are the integrated maps'.
    int set_integrate(const crsdr_caf_integrate_desc *desc);
    // the empty state again, m = 0
    int reset_integrate();
    // waits, and fills imap and ibmap, those whose flag is on; CRSDR_ESTATE with integration off
    int fetch_integrate();
    int integrated() const { return iwhat; }
    // the second cancellation stage behind every later submit's detector (crsdr_caf_set_clean; NULL: off): the strong detections of
    // the array map's list join the canceller's basis, and the maps and the list are formed again on the residual.  Between submits,
    // with the canceller and the detector on and the array map not integrated; while it is on set_cancel, set_cfar and
    // set_cfar_estimator are refused.
    int set_clean(const crsdr_caf_clean_desc *desc);
    // waits, and fills tgt, ntgt, tinfo, rdet and rcount, and tcoef if asked for; CRSDR_ESTATE with the stage off
    int fetch_clean(bool want_tcoef = false);
    int max_targets() const { return ntargets; }
    int basis() const { return nbasis; }             // taps (2 dopp + 1), 0 with the canceller off
    int lines() const { return nlines; }
    int nrows() const { return rows; }
    int nd() const { return bins; }
    int nlags() const { return lags; }
    std::vector<float> chi;                          // [lines][nrows][nd][nlags][2]
    std::vector<float> map;                          // [lines][nd][nlags]
    std::vector<peak_t> peak;                        // [lines][nrows + 1]
    // of line e: entry c < nrows is row c's peak, entry nrows the array map's
    const peak_t &at(int e, int c) const { return peak[(size_t)e * (rows + 1) + c]; }
    std::vector<det_t> det;                          // [lines][nrows + 1][max_det]: the strongest first, zeros behind the last
    std::vector<int32_t> count;                      // [lines][nrows + 1]: detected cells, which may be more than max_det
    std::vector<float> snap;                         // [lines][max_det][nrows][2]: chi of every row at the array map's detections
    std::vector<dir_t> dir;                          // [lines][max_det]: the bearing of the array map's detection k, zeros behind the last
    std::vector<float> spec;                         // [lines][max_det][ncx][ncy]: T on the grid, where kept and asked for
    const dir_t &bearing(int e, int k) const { return dir[(size_t)e * kdet + k]; }
    std::vector<float> bmap;                         // [lines][nbeams][nd][nlags]: every beam's map
    std::vector<det_t> bdet;                         // [lines][nbeams][max_det]: every beam map's detections
    std::vector<int32_t> bcount;                     // [lines][nbeams]
    std::vector<fused_t> fused;                      // [lines][max_det]: the beams' detections fused, the strongest first, zeros behind the last
    std::vector<int32_t> nfused;                     // [lines]: the survivors of the fusion, which may be more than max_det
    int fused_held(int e) const { return beam_lists ? (nfused[(size_t)e] < kdet ? nfused[(size_t)e] : kdet) : 0; }
    const fused_t &fused_at(int e, int k) const { return fused[(size_t)e * kdet + k]; }
    std::vector<float> aw;                           // [lines][nbeams][nrows - 1][2]: the adaptive weights, where asked for
    std::vector<float> ainfo;                        // [lines][nbeams][2]: the training cells' mean power through the adaptive beam and the caller's
    std::vector<int32_t> astat;                      // [lines]: 0, or the fallback's bits
    std::vector<track_t> trk;                        // [lines][max_tracks]: every slot of every line; free slots zero
    std::vector<int32_t> ntrk;                       // [lines][4]: live tracks after the line, confirmed, initiated, dropped
    const track_t &track_at(int e, int i) const { return trk[(size_t)e * ntracks + i]; }
    std::vector<float> imap;                         // [lines][nd][nlags]: the array map integrated across lines
    std::vector<float> ibmap;                        // [lines][nbeams][nd][nlags]: every beam's map, likewise
    std::vector<float> coef;                         // [lines][nrows][basis][2]: the canceller's filter of every row
    std::vector<float> cinfo;                        // [lines][nrows][2]: the share of the row's power that stays, and the status
    std::vector<det_t> tgt;                          // [lines][max_targets]: the records the second stage picked, zeros behind the last
    std::vector<int32_t> ntgt;                       // [lines]
    std::vector<float> tcoef;                        // [lines][nrows][max_targets][(2 wq + 1)(2 wl + 1)][2]: the target members' filter of every row
    std::vector<float> tinfo;                        // [lines][nrows][2]: the share that stays under the joint solve, and the status (0, 1, 2)
    std::vector<det_t> rdet;                         // [lines][nrows + 1][max_det]: the residual's detections, laid out as det
    std::vector<int32_t> rcount;                     // [lines][nrows + 1]
    const det_t &picked(int e, int t) const { return tgt[(size_t)e * ntargets + t]; }
    int residual_held(int e, int c) const { const int n = rcount[(size_t)e * (rows + 1) + c]; return n < kdet ? n : kdet; }
    const det_t &residual_detection(int e, int c, int k) const { return rdet[((size_t)e * (rows + 1) + c) * kdet + k]; }
    float residual(int e, int c) const { return cinfo[2 * ((size_t)e * rows + c)]; }
    bool singular(int e, int c) const { return cinfo[2 * ((size_t)e * rows + c) + 1] != 0.f; }
    // of line e and entry c: the number of detections held (at most max_det), and detection k of them
    int held(int e, int c) const { const int n = count[(size_t)e * (rows + 1) + c]; return n < kdet ? n : kdet; }
    const det_t &detection(int e, int c, int k) const { return det[((size_t)e * (rows + 1) + c) * kdet + k]; }
    // of line e: row c's chi (re, im) at the array map's detection k
    const float *snapshot(int e, int k, int c) const { return &snap[2 * (((size_t)e * kdet + k) * rows + c)]; }

private:
    int nlines = 0;
};
}
#endif
