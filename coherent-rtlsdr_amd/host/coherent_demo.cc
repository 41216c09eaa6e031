// coherent_demo.cc -- BASELINE config 1 plumbing on the reference's class surface: 1 ref + nsig
// synthetic channels (four.cfg shape by default) -> ccoherent::step() -> cpacketize sink.
// Exit code 0 iff every lag equals its injected delay and, in digital mode, the EMA phasors
// converge to exp(-j phi_k).  --dump writes the first generated block for the csynth/synth.py
// bit-exactness test; --cdsp runs a few class-cdsp identities through the per-op ABI.
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <thread>
#include <unistd.h>

#include "cbeamformer.h"
#include "ccoherent.h"
#include "ccontrol.h"
#include "ccaf.h"
#include "cspectra.h"

static int cdsp_selftest()
{
    const int n = 1024;
    std::vector<int8_t> i8(2 * n);
    for (int i = 0; i < 2 * n; ++i) i8[i] = (int8_t)((i * 37) % 251 - 125);
    std::vector<std::complex<float>> x(n), y(n);
    cdsp::convtofloat(x.data(), i8.data(), 2 * n);
    int bad = 0;
    for (int i = 0; i < n; ++i) bad += (x[i].real() != (float)i8[2 * i] * (1.0f / 127.0f));
    cdsp::scalarmul(y.data(), x.data(), std::complex<float>(1.0f, 0.0f), n);          // identity rotation
    std::vector<std::complex<int8_t>> q(n);
    cdsp::convto8bit(q.data(), y.data(), n);
    for (int i = 0; i < 2 * n; ++i) bad += (reinterpret_cast<int8_t *>(q.data())[i] != i8[i]); // int8 -> float -> int8 round trip
    std::complex<float> e = cdsp::conj_dotproduct(x.data(), x.data(), n);
    float ref = 0; for (int i = 0; i < n; ++i) ref += std::norm(x[i]);
    bad += (std::fabs(e.real() - ref) > 1e-3f * ref) + (std::fabs(e.imag()) > 1e-3f * ref);
    crsdr_fft_scheme sch = {n, 1, -1, nullptr, nullptr}, isch = {n, 1, +1, nullptr, nullptr};
    fft_scheme f = &sch, fi = &isch;
    std::vector<std::complex<float>> X(n), xb(n);
    cdsp::fft(X.data(), x.data(), &f);
    cdsp::fft(xb.data(), X.data(), &fi);
    float err = 0, nrm = 0;
    for (int i = 0; i < n; ++i) { err += std::norm(xb[i] / (float)n - x[i]); nrm += std::norm(x[i]); }
    bad += (std::sqrt(err / nrm) > 1e-6f);
    std::vector<float> m(n);
    uint32_t idx = cdsp::indexofmax(m.data(), X.data(), n);
    uint32_t idx_ref = 0; for (int i = 1; i < n; ++i) if (std::norm(X[i]) > std::norm(X[idx_ref])) idx_ref = i;
    bad += (idx != idx_ref);
    std::printf("cdsp selftest: %s\n", bad ? "FAIL" : "ok");
    return bad;
}

int main(int argc, char **argv)
{
    int nsig = 3, L = 8192, blocks = 12, mode = CRSDR_MODE_DIGITAL, dmax = -1;
    std::string dump, zmqaddr;
    bool run_cdsp = false, servo = false, threads = false, music = false, servo_table = false, bench = false, batch_parity = false, batched = false;
    int batch = 16, engine_delay_ms = 0, pace_us_arg = -1, peaks = 0, peak_radius = 1, beam_mode = CRSDR_BEAM_OFF, band_beam_mode = CRSDR_BEAM_OFF;
    float beam_loading = 1e-2f;
    int smooth_x = 0, smooth_y = 0, order_crit = CRSDR_ORDER_OFF, spectrum_kind = CRSDR_SPECTRUM_MUSIC, refine_levels = 0, esprit_mode = CRSDR_ESPRIT_OFF;
    bool smooth_fb = false;
    int augment_x = 0, augment_y = 0, refcancel = 0;
    std::string augment_mask;
    int sb_nfft = 0, sb_first = 0, sb_count = 1, sb_width = 1, sb_window = CRSDR_WINDOW_RECT;
    int sp_nfft = 0, sp_band_lo = 0, sp_band_hi = 0;
    bool sp_half = false;
    int caf_seg = 0, caf_lags = 0, caf_ref = 0, caf_frames = 1, caf_guard = 0;
    bool cfar_on = false;
    double cfar_db = 0.0;
    crsdr_cfar_desc cfar = {1, 1, 3, 4, 0.f, 1, 16};
    bool cfar_est_on = false, cfar_axis_on = false;
    crsdr_cfar_est_desc cfar_est = {CRSDR_CFAR_CA, 0, 0};
    bool cancel_on = false, bearing_on = false, beams_on = false, clean_on = false;
    crsdr_caf_clean_desc clean = {1, 100.f, 1, 1};
    int beams_mx = 0, beams_my = 0, beams_nx = 0, beams_ny = 0;
    bool adapt_on = false, adapt_region = false;
    crsdr_caf_beam_adapt_desc adapt = {0, 0, 0, 0, 1e-2f, 0u};
    crsdr_caf_bearing_desc bearing = {0, 0, 100, 100, 0.5f, CRSDR_BEARING_CONVENTIONAL, 1e-2f, 0, 0u};
    crsdr_caf_cancel_desc cancel = {0, 0};
    bool track_on = false;
    crsdr_caf_track_desc track = {16, CRSDR_TRACK_SRC_ARRAY, 0.5, 0.5, 9.0, 1.0, 1e-3, 1e-3, 1e-4, 0.0, 3, 5, 2, 4};
    bool integrate_on = false;
    double integrate_window = 0.0;
    crsdr_caf_integrate_desc integrate = {CRSDR_INTEGRATE_ARRAY, 0, 1.0, 0.0};
    bool engine_batches = false;
    int ranks = 1, rank = 0, device = 0;
    std::string idfile;
    std::vector<double> table_lags;
    int table_fs = 2048000;
    std::string replay;
    int pace_ms = 0;
    for (int i = 1; i < argc; ++i) {
        std::string a = argv[i];
        auto val = [&](int &v) { if (i + 1 < argc) v = std::atoi(argv[++i]); };
        if (a == "--nsig") val(nsig);
        else if (a == "--L") val(L);
        else if (a == "--blocks") val(blocks);
        else if (a == "--dmax") val(dmax);
        else if (a == "--faithful") mode = CRSDR_MODE_FAITHFUL;
        else if (a == "--dump" && i + 1 < argc) dump = argv[++i];
        else if (a == "--cdsp") run_cdsp = true;
        else if (a == "--servo") servo = true;      // closed loop: ccontrol model slews the synthetic delays to zero (f3)
        else if (a == "--threads") threads = true;  // streaming: producer thread per device, ccoherent thread, publish loop (f2)
        else if (a == "--zmq" && i + 1 < argc) zmqaddr = argv[++i];           // e.g. tcp://127.0.0.1:5555 (reference: tcp://*:5555)
        else if (a == "--zmq-debug" && i + 1 < argc) cpacketize::debugaddress = argv[++i];
        else if (a == "--pace-ms") val(pace_ms);
        else if (a == "--replay" && i + 1 < argc) { replay = argv[++i]; threads = true; }   // <prefix><row>.u8: raw uint8 IQ recordings (f2)
        else if (a == "--music") music = true;      // f4: the last packet through the beamformer chain (needs nsig = 7 x 3)
        else if (a == "--fs") val(table_fs);
        else if (a == "--bench") bench = true;      // pipelined batched engine over PCIe: blocks/s from C++, no Python in the loop
        else if (a == "--batch") val(batch);
        // with --bench: the reference-noise canceller with TAPS taps (crsdr_plan_set_refcancel); prints the mean residual share of every
        // timed batch in dB (read behind the batch's submit: that read waits for the batch, so the run is no longer fully pipelined)
        else if (a == "--refcancel") val(refcancel);
        else if (a == "--peaks") val(peaks);                   // with --bench --music: that many directions per estimate (crsdr_doa_set_peaks)
        else if (a == "--peak-radius") val(peak_radius);
        // with --bench --music: a beam toward every direction (crsdr_doa_set_beams), its power printed beside the direction
        else if (a == "--beams" && i + 1 < argc) {
            const std::string m = argv[++i];
            beam_mode = m == "conventional" ? CRSDR_BEAM_CONVENTIONAL : m == "mvdr" ? CRSDR_BEAM_MVDR : -1;
        }
        // with --bench --music: sub-arrays of SX x SY elements and / or forward-backward averaging (crsdr_doa_set_smoothing), the source
        // count per estimate (crsdr_doa_set_order), printed as k
        else if (a == "--smooth" && i + 1 < argc) { if (std::sscanf(argv[++i], "%dx%d", &smooth_x, &smooth_y) != 2) smooth_x = smooth_y = -1; }
        else if (a == "--fb") smooth_fb = true;
        // with --bench --music: the covariance of a filled VX x VY virtual array from the receivers of --mask (crsdr_doa_set_augment): BITS is
        // one character '0' / '1' per signal channel in element order, element i = character i; without --mask every receiver is used
        else if (a == "--augment" && i + 1 < argc) { if (std::sscanf(argv[++i], "%dx%d", &augment_x, &augment_y) != 2) augment_x = augment_y = -1; }
        else if (a == "--mask" && i + 1 < argc) augment_mask = argv[++i];
        else if (a == "--order" && i + 1 < argc) {
            const std::string c = argv[++i];
            order_crit = c == "mdl" ? CRSDR_ORDER_MDL : c == "aic" ? CRSDR_ORDER_AIC : -1;
        }
        // with --bench --music: a direction and a power per frequency band (crsdr_doa_set_subbands): COUNT bands of WIDTH bins of an
        // NFFT-point transform from bin FIRST on
        else if (a == "--subbands" && i + 1 < argc) {
            const int n = std::sscanf(argv[++i], "%d:%d:%d:%d", &sb_nfft, &sb_first, &sb_count, &sb_width);
            if (n < 3) sb_nfft = -1;
            if (n == 3) sb_width = 1;
        }
        // with --bench: per batch and packet the Welch spectra of every row and its alignment against row 0 (crsdr_spectra) on the packets
        // where the plan left them: NFFT-point segments, ":half" for half-overlapping ones, --window as for --subbands, --band LO:HI the
        // signed bins of the alignment figures (default +-NFFT/4).  One line per row: delay, phase, gain, coherence, strongest bin.
        else if (a == "--spectra" && i + 1 < argc) {
            const std::string s = argv[++i];
            sp_nfft = std::atoi(s.c_str());
            const size_t colon = s.find(':');
            sp_half = colon != std::string::npos && s.substr(colon + 1) == "half";
            if (sp_nfft <= 0 || (colon != std::string::npos && !sp_half)) sp_nfft = -1;
        }
        // with --bench: per batch, line and row the peak of the row's range-Doppler map against row REF (crsdr_caf) on the packets where the
        // plan left them: SEG-sample segments, LAGS lags, --caf-frames packets a line, --window as for --subbands over slow time, --guard G
        // to search outside |Doppler| < G.  One line per row and one for the array map: lag, Doppler bin, sub-cell offsets, power, ratio.
        else if (a == "--caf" && i + 1 < argc) {
            const int n = std::sscanf(argv[++i], "%d:%d:%d", &caf_seg, &caf_lags, &caf_ref);
            if (n < 2 || caf_seg <= 0) caf_seg = -1;
        }
        else if (a == "--caf-frames") val(caf_frames);
        // with --caf: a cell-averaging CFAR detector over every map (crsdr_caf_set_cfar): a cell is detected SNR_DB above the mean of its
        // training cells, GD, GR guard and TD, TR training half-widths over Doppler and lag (default 1:1:3:4), --max-det K detections kept
        // per map.  One line per detection of the array map: lag, Doppler bin, sub-cell offsets, snr, and the map's count.
        else if (a == "--cfar" && i + 1 < argc) {
            const int n = std::sscanf(argv[++i], "%lf:%d:%d:%d:%d", &cfar_db, &cfar.gd, &cfar.gr, &cfar.td, &cfar.tr);
            cfar_on = true;
            cfar.alpha = n == 1 || n == 5 ? (float)std::pow(10.0, cfar_db / 10.0) : -1.f;      // (refused below with the rest)
        }
        else if (a == "--max-det") val(cfar.max_det);
        // with --cfar: the noise estimate (crsdr_caf_set_cfar_estimator) in place of the mean of all training cells: go, so -- the greater
        // or smaller of the means of the window's two halves over lag, or over Doppler with --cfar-axis doppler -- or os[:RANK], the
        // RANK-th smallest training cell (default: three quarters of the window's cells)
        else if (a == "--cfar-est" && i + 1 < argc) {
            const std::string v = argv[++i];
            cfar_est_on = true;
            cfar_est.rank = 0;
            if (v == "go") cfar_est.estimator = CRSDR_CFAR_GO;
            else if (v == "so") cfar_est.estimator = CRSDR_CFAR_SO;
            else if (v == "os") cfar_est.estimator = CRSDR_CFAR_OS;
            else if (v.compare(0, 3, "os:") == 0 && std::sscanf(v.c_str() + 3, "%d", &cfar_est.rank) == 1 && cfar_est.rank > 0) cfar_est.estimator = CRSDR_CFAR_OS;
            else cfar_est.estimator = -1;                                                    // (refused below)
        }
        else if (a == "--cfar-axis" && i + 1 < argc) {
            const std::string v = argv[++i];
            cfar_axis_on = true;
            cfar_est.axis = v == "lag" ? 0 : v == "doppler" ? 1 : -1;                        // (refused below)
        }
        // with --caf: the least-squares canceller in front of the Doppler stage (crsdr_caf_set_cancel): the reference's first K delays, each
        // at -P .. P Doppler bins (default 0), projected out of every other row.  One line per line of the batch: the mean share of the
        // rows' power that stays, in dB.
        else if (a == "--cancel" && i + 1 < argc) {
            const int n = std::sscanf(argv[++i], "%d:%d", &cancel.taps, &cancel.dopp);
            cancel_on = true;
            if (n < 1) cancel.taps = -1;                                                     // (refused below with the rest)
        }
        // with --caf, --cancel and --cfar: the second cancellation stage (crsdr_caf_set_clean): up to T strong detections of the array map's
        // list, none under MIN_SNR_DB (20 by default), each a cluster of half-widths WL lags and WQ half bins (1:1), join the canceller's
        // basis; per line the picks and the residual's list are printed
        else if (a == "--clean" && i + 1 < argc) {
            double db = 20.0;
            const int n = std::sscanf(argv[++i], "%d:%lf:%d:%d", &clean.max_targets, &db, &clean.wl, &clean.wq);
            clean_on = true;
            clean.min_snr = (float)std::pow(10.0, db / 10.0);
            if (n < 1 || n == 3) clean.max_targets = -1;                                     // (refused below with the rest)
        }
        // with --caf and --cfar: a direction per detection of the array map (crsdr_caf_set_bearing), the signal rows as an MX x MY array on
        // an NC x NC grid (100); --adaptive LOADING whitens with the training cells' covariance, --bearing-levels L refines off the grid.
        // Prints one line per (batch, line, detection): cell, angles in degrees, fit
        else if (a == "--bearing" && i + 1 < argc) {
            int nc = 100;
            const int n = std::sscanf(argv[++i], "%dx%d:%d", &bearing.mx, &bearing.my, &nc);
            bearing_on = true;
            bearing.ncx = bearing.ncy = nc;
            if (n < 2) bearing.mx = -1;                                                      // (refused below with the rest)
        }
        // with --caf: a lattice of NX x NY conventional beams across the signal rows as an MX x MY array, on a 100 x 100 grid
        // (crsdr_caf_set_beams): direction ((100 i + 48) / NX, (100 j + 96) / NY) is beam NY i + j (8 x 8: 6 + 12.5 i, 12 + 12.5 j).  With --cfar every beam map is detected on
        // and the fused detections are printed with their beam's angles.
        else if (a == "--caf-beams" && i + 1 < argc) {
            const int n = std::sscanf(argv[++i], "%dx%d:%dx%d", &beams_mx, &beams_my, &beams_nx, &beams_ny);
            beams_on = true;
            if (n != 4) beams_mx = -1;                                                       // (refused below with the rest)
        }
        // with --caf-beams: per line MVDR weights from the covariance of the line's own cells in place of the lattice's
        // (crsdr_caf_set_beam_adapt).  The default region is the whole map less the zero-Doppler guard.  Prints per line the mean over
        // the beams of 10 log10(ainfo[b][0] / ainfo[b][1]): what the adaptation takes out of the training cells' power
        else if (a == "--caf-adapt" && i + 1 < argc) {
            const int n = std::sscanf(argv[++i], "%f:%d:%d:%d:%d", &adapt.loading, &adapt.d_lo, &adapt.d_n, &adapt.r_lo, &adapt.r_n);
            adapt_on = true;
            adapt_region = n == 5;
            if (n != 1 && n != 5) adapt.loading = -1.f;                                      // (refused below)
        }
        // with --caf and --cfar: tracks across the lines from the detections (crsdr_caf_set_track): M-of-N confirmation, GATE on d2 (9),
        // --track-max T slots (16), --track-sigma SR:SF measurement deviations in cells and bins (0.5:0.5), --track-q QR:QF:QG process
        // noise per line (1e-3:1e-3:1e-4), --coupling C lag cells per line per Doppler bin (0).  The source is the fused list with
        // --caf-beams, the array map's otherwise.  Prints per line the confirmed tracks: id, lag, Doppler, rate, age, and the beam or angles
        else if (a == "--track" && i + 1 < argc) {
            const int n = std::sscanf(argv[++i], "%d:%d:%lf", &track.m, &track.n, &track.gate);
            track_on = true;
            if (n < 2) track.m = -1;                                                         // (refused below with the rest)
        }
        else if (a == "--track-max") val(track.max_tracks);
        else if (a == "--track-sigma" && i + 1 < argc) { if (std::sscanf(argv[++i], "%lf:%lf", &track.sigma_r, &track.sigma_f) != 2) track.sigma_r = -1.0; }
        else if (a == "--track-q" && i + 1 < argc) { if (std::sscanf(argv[++i], "%lf:%lf:%lf", &track.q_r, &track.q_f, &track.q_g) != 3) track.q_r = -1.0; }
        else if (a == "--coupling" && i + 1 < argc) track.coupling = std::atof(argv[++i]);
        // with --caf: the array map integrated across the lines along the range walk, ahead of the detector (crsdr_caf_set_integrate):
        // a window of W lines (forget = 1 / W), COUPLING lag cells per line per Doppler bin (0; give --track the same with --coupling).
        // With --cfar the printed detections are the integrated map's; with --caf-beams the beam maps are integrated too
        else if (a == "--integrate" && i + 1 < argc) {
            const int n = std::sscanf(argv[++i], "%lf:%lf", &integrate_window, &integrate.coupling);
            integrate_on = true;
            if (n < 1) integrate_window = -1.0;                                              // (refused below with the rest)
        }
        else if (a == "--adaptive" && i + 1 < argc) { bearing.mode = CRSDR_BEARING_ADAPTIVE; bearing.loading = (float)std::atof(argv[++i]); }
        else if (a == "--bearing-levels") val(bearing.levels);
        else if (a == "--guard") val(caf_guard);
        else if (a == "--band" && i + 1 < argc) { if (std::sscanf(argv[++i], "%d:%d", &sp_band_lo, &sp_band_hi) != 2) sp_nfft = -1; }
        else if (a == "--window" && i + 1 < argc) {
            const std::string w = argv[++i];
            sb_window = w == "rect" ? CRSDR_WINDOW_RECT : w == "hann" ? CRSDR_WINDOW_HANN : -1;
        }
        // with --subbands: a beam per band toward that band's directions (crsdr_doa_set_subband_beams), its power beside the direction
        else if (a == "--band-beams" && i + 1 < argc) {
            const std::string m = argv[++i];
            band_beam_mode = m == "conventional" ? CRSDR_BEAM_CONVENTIONAL : m == "mvdr" ? CRSDR_BEAM_MVDR : -1;
        }
        // with --bench --music: the map the scan computes (crsdr_doa_set_spectrum); the two power maps print their peak values in dB
        // (of full scale, ((I + jQ) / 127)^2 = 1) and take --loading as Capon's diagonal loading
        else if (a == "--spectrum" && i + 1 < argc) {
            const std::string m = argv[++i];
            spectrum_kind = m == "music" ? CRSDR_SPECTRUM_MUSIC : m == "bartlett" ? CRSDR_SPECTRUM_BARTLETT : m == "capon" ? CRSDR_SPECTRUM_CAPON : -1;
        }
        // with --bench --music: every direction refined off the scan grid (crsdr_doa_set_refine; 5 levels unless a number follows), its
        // angles in degrees printed beside the grid point
        else if (a == "--refine") {
            refine_levels = 5;
            if (i + 1 < argc && argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9') refine_levels = std::atoi(argv[++i]);
        }
        // with --bench --music: every estimate's directions by 2-D ESPRIT (crsdr_doa_set_esprit) beside the scan, or with "only" in its
        // place; their angles in degrees and power are printed beside the grid direction
        else if (a == "--esprit") {
            esprit_mode = CRSDR_ESPRIT_BESIDE;
            if (i + 1 < argc && std::string(argv[i + 1]) == "only") { esprit_mode = CRSDR_ESPRIT_ONLY; ++i; }
        }
        else if (a == "--loading" && i + 1 < argc) beam_loading = (float)std::atof(argv[++i]);
        else if (a == "--batch-parity") batch_parity = true;   // the batched engine's packets == step()'s packets, bit for bit (own read counters, a masked row)
        else if (a == "--batched") batched = true;             // with --threads: the engine thread runs a batch at a time (ccoherent::start_batched)
        else if (a == "--engine-delay-ms") val(engine_delay_ms);
        else if (a == "--pace-us") val(pace_us_arg);
        // one process per GPU: --engine-batches --ranks G --rank r --device d --id-file <path>; start the G processes
        // yourself (a shell loop, mpirun, ...): rank 0 writes the exchange id to the file, the others wait for it
        else if (a == "--engine-batches") engine_batches = true;
        else if (a == "--ranks") val(ranks);
        else if (a == "--rank") val(rank);
        else if (a == "--device") val(device);
        else if (a == "--id-file" && i + 1 < argc) idfile = argv[++i];
        else if (a == "--servo-table" && i + 1 < argc) {      // comma-separated lags
            servo_table = true;
            for (char *tok = std::strtok(argv[++i], ","); tok; tok = std::strtok(nullptr, ",")) table_lags.push_back(std::atof(tok));
        }
    }
    if (cfar_est_on || cfar_axis_on) {
        // numbers only (no device): the limits are the library's own, asked of crsdr_caf_set_cfar_estimator behind --caf
        if (!cfar_on) { std::printf("cfar: --cfar-est and --cfar-axis need --cfar: there is no detector to estimate the noise for\nDEMO FAILED\n"); return 1; }
        const bool halves = cfar_est.estimator == CRSDR_CFAR_GO || cfar_est.estimator == CRSDR_CFAR_SO;
        if (!cfar_est_on || cfar_est.estimator < 0 || cfar_est.axis < 0 || (cfar_axis_on && !halves)) {
            std::printf("cfar: --cfar-est go|so|os[:RANK] [--cfar-axis lag|doppler] refused (the axis is greatest-of's and smallest-of's)\nDEMO FAILED\n");
            return 1;
        }
        if (cfar_est.estimator == CRSDR_CFAR_OS && !cfar_est.rank)
            cfar_est.rank = std::max(1, 3 * ((2 * (cfar.gd + cfar.td) + 1) * (2 * (cfar.gr + cfar.tr) + 1) - (2 * cfar.gd + 1) * (2 * cfar.gr + 1)) / 4);
        std::printf("cfar: estimator %s axis %s rank %d\n", cfar_est.estimator == CRSDR_CFAR_GO ? "go" : cfar_est.estimator == CRSDR_CFAR_SO ? "so" : "os",
                    halves ? (cfar_est.axis ? "doppler" : "lag") : "-", cfar_est.rank);
    }
    if (track_on) {
        // numbers only (no device): the tracker's limits are the library's own (crsdr_track_state_bytes checks them on the host)
        size_t state_bytes = 0;
        track.source = beams_on ? CRSDR_TRACK_SRC_FUSED : CRSDR_TRACK_SRC_ARRAY;
        if (!caf_seg || !cfar_on) { std::printf("track: --track needs --caf and --cfar: there are no detections to track\nDEMO FAILED\n"); return 1; }
        if (crsdr_track_state_bytes(&track, &state_bytes)) {
            std::printf("track: --track M:N[:GATE] [--track-max T] [--track-sigma SR:SF] [--track-q QR:QF:QG] [--coupling C] refused: %s\nDEMO FAILED\n", crsdr_last_error());
            return 1;
        }
        std::printf("track: %d of %d gate %g slots %d sigma %g:%g q %g:%g:%g coupling %g source %s\n", track.m, track.n, track.gate, track.max_tracks, track.sigma_r,
                    track.sigma_f, track.q_r, track.q_f, track.q_g, track.coupling, beams_on ? "fused" : "array");
    }
    if (integrate_on) {
        // numbers only (no device): the window and the coupling; the coupling against nd is the library's to judge behind --caf
        if (!caf_seg) { std::printf("integrate: --integrate needs --caf: there are no maps to integrate\nDEMO FAILED\n"); return 1; }
        if (!(integrate_window >= 1.0) || !std::isfinite(integrate_window) || !std::isfinite(integrate.coupling)) {
            std::printf("integrate: --integrate W[:COUPLING] refused (W at least 1 line, both finite)\nDEMO FAILED\n");
            return 1;
        }
        integrate.forget = 1.0 / integrate_window;
        integrate.what = CRSDR_INTEGRATE_ARRAY | (beams_on ? CRSDR_INTEGRATE_BEAMS : 0);
        std::printf("integrate: window %g forget %g coupling %g maps %s\n", integrate_window, integrate.forget, integrate.coupling, beams_on ? "array+beams" : "array");
    }
    int fails = 0;
    if (servo_table) {
        // f3, numbers only (no device): descent / hold time / hold blocks of the servo for every lag given after the flag,
        // printed with full precision for tests/test_host_cpp.py to compare with its restatement of src/ccontrol.cc
        for (double lg : table_lags) {
            const float lag = (float)lg;
            std::printf("servo lag %.9g correct %d p %.9g t %.17g blocks %d realfs %.17g\n", lag, (int)ccontrol::needs_correction(lag),
                        ccontrol::descent(lag), ccontrol::needs_correction(lag) ? ccontrol::hold_seconds(lag, (uint32_t)table_fs) : 0.0,
                        ccontrol::needs_correction(lag) ? ccontrol::hold_block_count(lag, (uint32_t)table_fs, 2 * (uint32_t)L) : 0,
                        ccontrol::realfs((uint32_t)table_fs));
        }
        return 0;
    }
    if (run_cdsp) fails += cdsp_selftest();

    const uint32_t B = 2 * (uint32_t)L;
    if (batch_parity) {
        // The batched engine against the per-block loop on the same synthetic stream: 3 batches of `batch` blocks.  Row 2's read
        // counter starts three ahead of the others (each device's OWN counter must reach the header, src/cpacketizer.cc:142,163)
        // and row 2 stops asking for a lag after the first batch (the per-device gate of src/ccoherent.cc:266).  Every published
        // message -- header, read counters, matrix, zero tail -- and every phase-factor payload must be equal bit for bit.
        typedef std::vector<std::vector<int8_t>> pkv;
        typedef std::vector<std::vector<std::complex<float>>> phv;
        const int T = batch, NB = 3;
        auto run = [&](bool use_batches, pkv &pk, phv &ph, std::vector<float> &lags) -> bool {
            csynthsource src(nsig, L, csynth_config_seed(1), dmax, false);
            crefsdr rdev(&src, B);
            lvector<csdrdevice *> dv;
            std::vector<std::unique_ptr<csyntheticsdr>> od;
            for (int k = 0; k < nsig; ++k) { od.emplace_back(new csyntheticsdr(&src, 1 + k, B)); dv.push_back(od.back().get()); }
            if (nsig >= 2) for (int i = 0; i < 3; ++i) od[1]->inc_readcnt();
            crefnoise rn;
            cpacketize::init("", false, 1 + nsig, B);
            cpacketize::sink = [&](const int8_t *p, size_t bytes, const std::complex<float> *phase, size_t n) {
                pk.emplace_back(p, p + bytes);
                ph.emplace_back(phase, phase + n);
            };
            ccoherent eng(&rdev, &dv, &rn, 8, mode, use_batches ? T : 1);
            auto request = [&](int block) { for (int k = 0; k < nsig; ++k) if (!(k == 1 && block >= T)) dv[k]->requestfft(); };
            bool ok = true;
            if (!use_batches) {
                for (int t = 0; t < NB * T && ok; ++t) { src.advance(); request(t); ok = eng.step(); cpacketize::send(); }
            } else {
                ok = eng.enable_batching(T);
                for (int bb = 0; bb < NB && ok; ++bb) {
                    request(bb * T);
                    ok = eng.fill_batch(0, T, [&](int) { src.advance(); }) && eng.submit_batch(0, T, 0) && eng.collect_batch(0);
                }
            }
            for (int k = 0; k < nsig; ++k) lags.push_back(dv[k]->get_lagp()->lag);
            cpacketize::sink = nullptr;
            cpacketize::cleanup();
            return ok;
        };
        pkv pa, pb; phv ha, hb; std::vector<float> la, lb;
        const bool oka = run(false, pa, ha, la), okb = run(true, pb, hb, lb);
        size_t bad = (!oka) + (!okb) + (pa.size() != (size_t)(NB * T)) + (pb.size() != pa.size());
        size_t own_cnt = 0, masked_ok = 0;
        for (size_t i = 0; i < pa.size() && i < pb.size(); ++i) {
            if (pa[i] != pb[i]) { if (bad < 5) std::printf("packet %zu differs (%zu vs %zu bytes)\n", i, pa[i].size(), pb[i].size()); ++bad; }
            if (ha[i].size() != hb[i].size() || std::memcmp(ha[i].data(), hb[i].data(), ha[i].size() * sizeof(std::complex<float>))) { if (bad < 5) std::printf("phase payload %zu differs\n", i); ++bad; }
            const uint32_t *rc = reinterpret_cast<const uint32_t *>(pb[i].data() + 16);
            if (nsig >= 2) own_cnt += (rc[2] == rc[1] + 3);              // row 2 carries its own, offset counter
        }
        if (nsig >= 2) bad += (own_cnt != pb.size());
        for (int k = 0; k < nsig; ++k) { bad += (la[k] != lb[k]); masked_ok += 1; }
        std::printf("batch parity: %zu + %zu packets of %zu bytes, %zu with row 2's own read counter, lags %s\n", pa.size(), pb.size(), pa.empty() ? 0 : pa[0].size(), own_cnt,
                    la == lb ? "equal" : "DIFFER");
        std::printf("%s\n", bad ? "DEMO FAILED" : "DEMO OK");
        return bad ? 1 : 0;
    }

    if (engine_batches) {
        // The batched engine as a program: synchronous synthetic source -> fill_batch -> submit_batch -> collect_batch, pipelined over
        // two slots, every block's packet published (sink: one digest line per packet).  With --id-file the signal rows are split over
        // --ranks processes, one per GPU: each owns a slab, the exchange (RCCL under the C ABI) assembles every block on its rotating
        // root, and each rank publishes the blocks it assembled -- the union over the ranks is the unsharded engine's output.
        // (Every rank generates the whole synthetic matrix; only row 0 and its slab go to its GPU.)
        unsigned char xid[CRSDR_EXCHANGE_ID_BYTES];
        ccoherent_shard sh;
        sh.ranks = ranks; sh.rank = rank; sh.device = device;
        if (!idfile.empty()) {
            if (rank == 0) {
                if (crsdr_exchange_unique_id(xid) != CRSDR_OK) { std::printf("exchange id: %s\nDEMO FAILED\n", crsdr_last_error()); return 1; }
                const std::string tmp = idfile + ".tmp";
                FILE *f = std::fopen(tmp.c_str(), "wb");
                if (!f || std::fwrite(xid, 1, sizeof(xid), f) != sizeof(xid)) { std::printf("cannot write %s\nDEMO FAILED\n", tmp.c_str()); return 1; }
                std::fclose(f);
                std::rename(tmp.c_str(), idfile.c_str());              // atomic: a reader never sees half an id
            } else {
                bool got = false;
                for (int spin = 0; spin < 1200 && !got; ++spin) {      // up to 60 s for rank 0 to come up
                    FILE *f = std::fopen(idfile.c_str(), "rb");
                    if (f) { got = std::fread(xid, 1, sizeof(xid), f) == sizeof(xid); std::fclose(f); }
                    if (!got) usleep(50 * 1000);
                }
                if (!got) { std::printf("rank %d: no exchange id in %s\nDEMO FAILED\n", rank, idfile.c_str()); return 1; }
            }
            sh.id = xid;
        }
        csynthsource src(nsig, L, csynth_config_seed(1), dmax, false);
        crefsdr rdev(&src, B);
        lvector<csdrdevice *> dv;
        std::vector<std::unique_ptr<csyntheticsdr>> od;
        for (int k = 0; k < nsig; ++k) { od.emplace_back(new csyntheticsdr(&src, 1 + k, B)); dv.push_back(od.back().get()); }
        crefnoise rn;
        cpacketize::init(zmqaddr, false, 1 + nsig, B);
        size_t npk = 0, badhdr = 0;
        cpacketize::sink = [&](const int8_t *p, size_t bytes, const std::complex<float> *phase, size_t n) {
            const hdr0 *h = reinterpret_cast<const hdr0 *>(p);
            uint64_t fnv = 1469598103934665603ull;
            for (size_t i = 0; i < bytes; ++i) { fnv ^= (uint8_t)p[i]; fnv *= 1099511628211ull; }
            for (size_t i = 0; i < n * sizeof(std::complex<float>); ++i) { fnv ^= reinterpret_cast<const uint8_t *>(phase)[i]; fnv *= 1099511628211ull; }
            std::printf("packet seq %u N %u L %u bytes %zu digest %016llx\n", h->globalseqn, h->N, h->L, bytes, (unsigned long long)fnv);
            badhdr += (h->N != (uint32_t)(1 + nsig)) + (h->L != (uint32_t)L);
            ++npk;
        };
        ccoherent eng(&rdev, &dv, &rn, 8, mode, batch, &sh);
        if (!eng.ok() || !eng.enable_batching(batch)) { std::printf("engine unavailable\nDEMO FAILED\n"); return 1; }
        const int nb = std::max(1, blocks / batch);
        bool ok = true;
        auto fill = [&](int b) { for (auto *d : dv) d->requestfft(); return eng.fill_batch(b & 1, batch, [&](int) { src.advance(); }); };
        ok = fill(0) && eng.submit_batch(0, batch, 0);
        for (int b = 1; b < nb && ok; ++b) {
            ok = fill(b) && eng.submit_batch(b & 1, batch, 0);          // batch b computes while batch b - 1 is exchanged and fetched
            ok = ok && eng.collect_batch((b - 1) & 1);
        }
        ok = ok && eng.collect_batch((nb - 1) & 1);
        const csynth_params *pp = src.get_params();
        int badlag = 0;
        const int per = nsig / ranks, lo = sh.id ? rank * per : 0, hi = sh.id ? lo + per : nsig;
        for (int k = lo; k < hi; ++k) badlag += ((long)dv[k]->get_lagp()->lag != (long)pp->d[k]);      // this process's own devices got their lags
        // blocks this rank assembled: runs of ceil(batch / ranks) per batch
        const int bpr = (batch + ranks - 1) / ranks, mine = std::max(0, std::min(bpr, batch - rank * bpr));
        const size_t expect = (size_t)nb * (size_t)(sh.id ? mine : batch);
        std::printf("engine batches: rank %d of %d on device %d, %d batches x %d blocks, published %zu packets (expected %zu), own lags %s\n", rank, ranks, device, nb, batch,
                    npk, expect, badlag ? "MISMATCH" : "ok");
        const bool fail = !ok || badlag || badhdr || npk != expect;
        cpacketize::sink = nullptr;
        cpacketize::cleanup();
        std::printf("%s\n", fail ? "DEMO FAILED" : "DEMO OK");
        return fail ? 1 : 0;
    }

    csynthsource source(nsig, L, csynth_config_seed(1), dmax, false);
    crefsdr ref(&source, B);
    lvector<csdrdevice *> devs;
    std::vector<std::unique_ptr<csyntheticsdr>> own;
    for (int k = 0; k < nsig; ++k) { own.emplace_back(new csyntheticsdr(&source, 1 + k, B)); devs.push_back(own.back().get()); }
    crefnoise refnoise;
    cpacketize::init(zmqaddr, false, 1 + nsig, B);             // src/main.cc:261 binds tcp://*:5555
    if (!zmqaddr.empty()) { std::printf("zmq publish on %s: %s\n", zmqaddr.c_str(), cpacketize::publishing() ? "bound" : "unavailable"); usleep(300 * 1000); }
    size_t packets = 0, last_bytes = 0; uint32_t last_seq = 0, last_N = 0, last_L = 0;
    std::vector<int8_t> last_packet;
    cpacketize::sink = [&](const int8_t *p, size_t bytes, const std::complex<float> *, size_t) {
        const hdr0 *h = reinterpret_cast<const hdr0 *>(p);
        last_seq = h->globalseqn; last_N = h->N; last_L = h->L; last_bytes = bytes; ++packets;
        if (music) last_packet.assign(p, p + bytes);
    };
    ccoherent coherent(&ref, &devs, &refnoise, 8, mode, (bench || batched) ? batch : 1);

    if (bench) {
        // The engine a batch at a time, pipelined: page-locked slots of `batch` blocks go over PCIe while the previous batch's
        // packets come back (crsdr_plan_submit_batch + crsdr_plan_fetch_batch_async; src/ccoherent.cc:245-294 is the per-block
        // loop this replaces).  Host rows in, host packets out for EVERY block -- the PCIe-inclusive rate, bounded by
        // (1 + nsig) * B bytes each way per block.  The synthetic source is far slower than the link, so four distinct blocks
        // are generated once and cycled through the slots; the transfers and the device work are the real ones.
        if (!coherent.enable_batching(batch)) { std::printf("bench: batching unavailable\nDEMO FAILED\n"); return 1; }
        const size_t blk = (size_t)(1 + nsig) * B;
        std::vector<int8_t> distinct(4 * blk);
        for (int t = 0; t < 4; ++t) { source.advance(); std::memcpy(distinct.data() + t * blk, source.row(0), blk); }
        for (int sl = 0; sl < 2; ++sl)
            for (int t = 0; t < batch; ++t) std::memcpy(coherent.batch_rows(sl) + (size_t)t * blk, distinct.data() + (size_t)((sl * batch + t) % 4) * blk, blk);
        const int nb = std::max(3, blocks / batch);
        const uint32_t fl = CRSDR_REFNOISE_ENABLED;
        bool ok = true;
        if (refcancel && coherent.set_refcancel(refcancel)) { std::printf("bench: --refcancel %d refused: %s\nDEMO FAILED\n", refcancel, crsdr_last_error()); return 1; }
        bool residuals = false;
        auto residual = [&](int b) {
            if (!refcancel || !residuals || !ok) return;
            std::vector<float> res((size_t)(1 + nsig));
            double sum = 0.0;
            for (int t = 0; t < batch; ++t) {
                if (crsdr_plan_fetch_refcancel(coherent.engine_plan(), t, nullptr, res.data(), nullptr) != CRSDR_OK) { ok = false; return; }
                for (int k = 1; k <= nsig; ++k) sum += res[(size_t)k];
            }
            std::printf("refcancel: batch %d: %d taps, mean residual %.2f dB\n", b, refcancel, 10.0 * std::log10(sum / ((double)batch * nsig)));
        };
        // --bench --music: a direction per block from the packets where the plan left them (cbeamformer::batch over crsdr_doa), enqueued
        // behind every batch on the plan's stream; the peaks are the only thing fetched.  The synthetic channels all carry the reference
        // noise: once aligned, one source at broadside, grid point (50, 50).
        std::unique_ptr<cbeamformer::batch> doa;
        if (music && !coherent.sharded()) {
            doa.reset(new cbeamformer::batch(1 + nsig, B, batch));
            if (nsig != cbeamformer::MX * cbeamformer::MY || !doa->ok()) { std::printf("doa: unavailable (needs --nsig 21)\nDEMO FAILED\n"); return 1; }
            // the bands first: what follows sizes its buffers by them
            if (sb_nfft && doa->set_subbands(sb_nfft, sb_first, sb_count, sb_width, sb_window)) {
                std::printf("doa: --subbands %d:%d:%d:%d --window (rect|hann) refused\nDEMO FAILED\n", sb_nfft, sb_first, sb_count, sb_width);
                return 1;
            }
            if (smooth_x || smooth_fb) {
                const int sx = smooth_x ? smooth_x : cbeamformer::MX, sy = smooth_x ? smooth_y : cbeamformer::MY;
                if (doa->set_smoothing(sx, sy, smooth_fb)) { std::printf("doa: --smooth %dx%d%s refused\nDEMO FAILED\n", sx, sy, smooth_fb ? " --fb" : ""); return 1; }
            }
            if (augment_x || !augment_mask.empty()) {
                uint64_t mask = 0;
                bool bits_ok = augment_x != 0 && (augment_mask.empty() || (int)augment_mask.size() == nsig);
                for (size_t i = 0; bits_ok && i < augment_mask.size(); ++i) {
                    if (augment_mask[i] == '1') mask |= (uint64_t)1 << i;
                    else if (augment_mask[i] != '0') bits_ok = false;
                }
                if (!bits_ok) { std::printf("doa: --augment VXxVY [--mask BITS]: BITS is %d characters 0 / 1, one per receiver\nDEMO FAILED\n", nsig); return 1; }
                if (doa->set_augment(augment_x, augment_y, mask)) {
                    std::printf("doa: --augment %dx%d --mask %s refused: %s\nDEMO FAILED\n", augment_x, augment_y, augment_mask.empty() ? "(all)" : augment_mask.c_str(),
                                crsdr_last_error());
                    return 1;
                }
                std::printf("doa: augment: %d receivers of %d -> %d x %d virtual array\n", doa->receivers(), nsig, doa->virtual_x(), doa->virtual_y());
            }
            if (order_crit && doa->set_order(order_crit)) { std::printf("doa: --order (mdl|aic) refused\nDEMO FAILED\n"); return 1; }
            if (spectrum_kind && doa->set_spectrum(spectrum_kind, beam_loading)) {
                std::printf("doa: --spectrum (music|bartlett|capon) --loading %g refused\nDEMO FAILED\n", (double)beam_loading);
                return 1;
            }
            if (peaks && doa->set_peaks(peaks, peak_radius)) { std::printf("doa: --peaks %d --peak-radius %d refused\nDEMO FAILED\n", peaks, peak_radius); return 1; }
            if (esprit_mode && doa->set_esprit(esprit_mode)) { std::printf("doa: --esprit refused\nDEMO FAILED\n"); return 1; }
            if (refine_levels && doa->set_refine(refine_levels)) { std::printf("doa: --refine %d refused (1..8 levels)\nDEMO FAILED\n", refine_levels); return 1; }
            if (beam_mode && doa->set_beams(beam_mode, beam_loading)) { std::printf("doa: --beams (conventional|mvdr) --loading %g refused\nDEMO FAILED\n", (double)beam_loading); return 1; }
            if (band_beam_mode && (!sb_nfft || doa->set_subband_beams(band_beam_mode, beam_loading))) {
                std::printf("doa: --band-beams (conventional|mvdr) --loading %g refused (it needs --subbands)\nDEMO FAILED\n", (double)beam_loading);
                return 1;
            }
        }
        bool report = false;
        auto directions = [&](int b) {
            if (!doa || !ok) return;
            ok = doa->submit(coherent.engine_plan()) == CRSDR_OK && doa->fetch() == CRSDR_OK;
            if (!ok || !report) return;
            const int n = doa->estimates();
            if (doa->virtual_x())
                std::printf("doa: batch %d: the directions below are from %d receivers on the %d x %d virtual array\n", b, doa->receivers(), doa->virtual_x(), doa->virtual_y());
            const double deg = 180.0 / 3.14159265358979323846;
            if (esprit_mode) {
                // every matrix (estimate, or estimate and band): the grid direction, then the ESPRIT slots in order of power
                const int ns = doa->esprit_slots();
                for (int e = 0; e < n; ++e) {
                    std::printf("doa: batch %d: esprit %d:", b, e);
                    if (esprit_mode != CRSDR_ESPRIT_ONLY) std::printf(" grid (%d, %d)", doa->peak[2 * e], doa->peak[2 * e + 1]);
                    std::printf(" found %d status %d:", doa->esprit_found[e], doa->esprit_status[e]);
                    for (int s = 0; s < doa->esprit_found[e]; ++s) {
                        const size_t x = (size_t)e * ns + s;
                        std::printf(" (%.3f, %.3f) deg power %.4g", deg * doa->esprit_angles[2 * x], deg * doa->esprit_angles[2 * x + 1], (double)doa->esprit_power[x]);
                    }
                    std::printf("\n");
                }
                if (esprit_mode == CRSDR_ESPRIT_ONLY) { std::printf("doa: batch %d: %d estimates by ESPRIT alone\n", b, n); return; }
            }
            if (doa->bands()) {
                // every estimate's bands: the direction at that frequency and the power that says whether to trust it
                const int nb_ = doa->bands();
                for (int e = 0; e < n / nb_; ++e)
                    for (int i = 0; i < nb_; ++i) {
                        const int x = e * nb_ + i, f0 = (sb_first + i * sb_width) % sb_nfft;
                        std::printf("doa: batch %d: estimate %d band %d (bins %d..%d of %d): (%d, %d)", b, e, i, f0, (f0 + sb_width - 1) % sb_nfft, sb_nfft,
                                    doa->peak[2 * x], doa->peak[2 * x + 1]);
                        if (refine_levels) {
                            const size_t r = 2 * (size_t)x * doa->refined_slots();
                            std::printf(" = (%.3f, %.3f) deg", deg * doa->refined_angles[r], deg * doa->refined_angles[r + 1]);
                        }
                        std::printf(" power %.4g", (double)doa->band_power[x]);
                        // the band's beam toward its strongest direction (slot 0 is the peak, with or without --peaks)
                        if (band_beam_mode) std::printf(" beam power %.4g", (double)doa->band_beam_power[(size_t)x * doa->band_beam_slots()]);
                        std::printf("\n");
                    }
            }
            if (order_crit) {
                std::string ks;
                for (int e = 0; e < n; ++e) ks += " " + std::to_string(doa->order[e]);
                std::printf("doa: batch %d: %d estimates of %d elements, k:%s\n", b, n, doa->subspace_size(), ks.c_str());
            }
            if (peaks) {
                // the first estimate's local peaks, strongest first
                std::string dirs;
                char buf[64];
                for (int i = 0; i < doa->found[0]; ++i) {
                    std::snprintf(buf, sizeof(buf), " (%d, %d)", doa->directions[2 * i], doa->directions[2 * i + 1]);
                    dirs += buf;
                    if (refine_levels) {
                        std::snprintf(buf, sizeof(buf), " = (%.3f, %.3f) deg", deg * doa->refined_angles[2 * i], deg * doa->refined_angles[2 * i + 1]);
                        dirs += buf;
                    }
                    if (spectrum_kind) { std::snprintf(buf, sizeof(buf), " value %.2f dB", 10.0 * std::log10((double)doa->direction_values[i])); dirs += buf; }
                    if (beam_mode) { std::snprintf(buf, sizeof(buf), " power %.4g", (double)doa->beam_power[i]); dirs += buf; }
                }
                std::printf("doa: batch %d: %d estimates, peaks of the first:%s\n", b, n, dirs.c_str());
                return;
            }
            int broadside = 0;
            for (int e = 0; e < n; ++e) broadside += doa->peak[2 * e] == 50 && doa->peak[2 * e + 1] == 50;
            if (spectrum_kind) std::printf("doa: batch %d: peak value of the first direction %.2f dB\n", b, 10.0 * std::log10((double)doa->peak_value[0]));
            if (beam_mode) std::printf("doa: batch %d: beam power of the first direction %.4g\n", b, (double)doa->beam_power[0]);
            if (refine_levels)
                std::printf("doa: batch %d: first direction (%d, %d) refined to (%.3f, %.3f) deg\n", b, doa->peak[0], doa->peak[1], deg * doa->refined_angles[0],
                            deg * doa->refined_angles[1]);
            std::printf("doa: batch %d: %d directions, first (%d, %d), last (%d, %d), %d at broadside\n", b, n, doa->peak[0], doa->peak[1], doa->peak[2 * n - 2],
                        doa->peak[2 * n - 1], broadside);
        };
        // --bench --spectra: cspectra::batch over crsdr_spectra, enqueued behind every batch on the plan's stream like the directions.  The
        // synthetic channels all carry the reference noise and the plan has taken the integer lag out: what is left is under a sample.
        std::unique_ptr<cspectra::batch> spectra;
        if (sp_nfft && !coherent.sharded()) {
            if (sp_nfft > 0) spectra.reset(new cspectra::batch(1 + nsig, B, batch, sp_nfft, sp_half, sb_window, sp_band_lo, sp_band_hi));
            if (!spectra || !spectra->ok()) { std::printf("spectra: --spectra NFFT[:half] [--window rect|hann] [--band LO:HI] refused\nDEMO FAILED\n"); return 1; }
        }
        auto alignment = [&](int b) {
            if (!spectra || !ok) return;
            ok = spectra->submit(coherent.engine_plan()) == CRSDR_OK && spectra->fetch() == CRSDR_OK;
            if (!ok || !report) return;
            for (int e = 0; e < spectra->lines(); ++e)
                for (int c = 0; c < spectra->nrows(); ++c) {
                    const float *f = &spectra->align[4 * ((size_t)e * spectra->nrows() + c)];
                    double db = 0.0;
                    const int bin = spectra->strongest_bin(e, c, &db);
                    std::printf("spectra: batch %d line %d row %d: delay %.6f phase %.6f gain %.6f coherence %.6f peak bin %d power %.2f dB\n", b, e, c, (double)f[0],
                                (double)f[1], (double)f[2], (double)f[3], bin, db);
                }
        };
        // --bench --caf: ccaf::batch over crsdr_caf, behind every batch on the plan's stream like the spectra.  The synthetic channels are
        // copies of the reference noise with the integer lag taken out: with --guard 0 every row peaks at lag 0, Doppler 0.
        std::unique_ptr<ccaf::batch> caf;
        std::vector<double> beam_xy;                                                         // [nbeams][2]: the lattice's cell coordinates
        if (caf_seg && !coherent.sharded()) {
            if (caf_seg > 0) caf.reset(new ccaf::batch(1 + nsig, B, batch, caf_seg, caf_lags, caf_ref, sb_window, caf_guard, caf_frames));
            if (!caf || !caf->ok()) { std::printf("caf: --caf SEG:LAGS[:REF] [--caf-frames F] [--guard G] [--window rect|hann] refused\nDEMO FAILED\n"); return 1; }
            if (cfar_on && caf->set_cfar(&cfar)) { std::printf("cfar: --cfar SNR_DB[:GD:GR:TD:TR] [--max-det K] refused\nDEMO FAILED\n"); return 1; }
            if (cfar_est_on && caf->set_cfar_estimator(&cfar_est)) { std::printf("cfar: --cfar-est go|so|os[:RANK] [--cfar-axis lag|doppler] refused\nDEMO FAILED\n"); return 1; }
            if (cancel_on && caf->set_cancel(&cancel)) { std::printf("cancel: --cancel K[:P] refused\nDEMO FAILED\n"); return 1; }
            if (clean_on && caf->set_clean(&clean)) { std::printf("clean: --clean T[:MIN_SNR_DB[:WL:WQ]] refused (it needs --cancel and --cfar): %s\nDEMO FAILED\n", crsdr_last_error()); return 1; }
            if (bearing_on && !cfar_on) { std::printf("bearing: --bearing needs --cfar: there are no detections to take a bearing of\nDEMO FAILED\n"); return 1; }
            // (the order of the setters is detector / beams, integration, bearings, tracker: with --integrate the bearings wait for it)
            auto set_bearing = [&]() {
                if (!bearing_on || !caf->set_bearing(&bearing)) return true;
                std::printf("bearing: --bearing MXxMY[:NC] [--adaptive LOADING] [--bearing-levels L] refused (MX MY must be --nsig = %d)\nDEMO FAILED\n", nsig);
                return false;
            };
            if (!integrate_on && !set_bearing()) return 1;
            if (beams_on) {
                const long long nbm = (long long)beams_nx * beams_ny;
                bool good = beams_mx >= 1 && beams_my >= 1 && (long long)beams_mx * beams_my == nsig && beams_nx >= 1 && beams_ny >= 1 && nbm <= 64;
                if (good) {
                    beam_xy.resize(2 * (size_t)nbm);
                    for (int i = 0; i < beams_nx; ++i)
                        for (int j = 0; j < beams_ny; ++j) {
                            beam_xy[2 * ((size_t)i * beams_ny + j)] = (100.0 * i + 48.0) / beams_nx;      // (inside the grid for any NX, NY)
                            beam_xy[2 * ((size_t)i * beams_ny + j) + 1] = (100.0 * j + 96.0) / beams_ny;
                        }
                    std::vector<float> w(2 * (size_t)nbm * nsig);
                    const crsdr_caf_beams_desc bd = {(int32_t)nbm, w.data(), 0u};
                    good = crsdr_caf_beam_steer(w.data(), beams_mx, beams_my, bearing.d, 100, 100, beam_xy.data(), (int)nbm) == CRSDR_OK && caf->set_beams(&bd) == CRSDR_OK;
                }
                if (!good) { std::printf("beams: --caf-beams MXxMY:NXxNY refused (MX MY must be --nsig = %d, NX NY at most 64)\nDEMO FAILED\n", nsig); return 1; }
            }
            if (adapt_on) {
                if (!adapt_region) { adapt.d_lo = caf_guard + 1; adapt.d_n = caf->nd() - 2 * caf_guard - 1; adapt.r_lo = 0; adapt.r_n = caf->nlags(); }
                if (!beams_on || caf->set_beam_adapt(&adapt)) {
                    std::printf("adapt: --caf-adapt LOADING[:D_LO:D_N:R_LO:R_N] refused (it needs --caf-beams; LOADING in [1e-6, 1])\nDEMO FAILED\n");
                    return 1;
                }
                std::printf("adapt: loading %g doppler %d+%d lags %d+%d\n", (double)adapt.loading, adapt.d_lo, adapt.d_n, adapt.r_lo, adapt.r_n);
            }
            if (integrate_on && caf->set_integrate(&integrate)) { std::printf("integrate: --integrate W[:COUPLING] refused: %s\nDEMO FAILED\n", crsdr_last_error()); return 1; }
            if (integrate_on && !set_bearing()) return 1;
            if (track_on && caf->set_track(&track)) { std::printf("track: --track refused: %s\nDEMO FAILED\n", crsdr_last_error()); return 1; }
        }
        auto ambiguity = [&](int b) {
            if (!caf || !ok) return;
            ok = caf->submit(coherent.engine_plan()) == CRSDR_OK && caf->fetch() == CRSDR_OK && (!cfar_on || caf->fetch_cfar() == CRSDR_OK) &&
                 (!cancel_on || caf->fetch_cancel(false) == CRSDR_OK) && (!bearing_on || caf->fetch_bearing() == CRSDR_OK) &&
                 (!beams_on || caf->fetch_beams() == CRSDR_OK) && (!adapt_on || caf->fetch_beam_adapt() == CRSDR_OK) && (!track_on || caf->fetch_track() == CRSDR_OK) &&
                 (!integrate_on || caf->fetch_integrate() == CRSDR_OK) && (!clean_on || caf->fetch_clean() == CRSDR_OK);
            if (!ok || !report) return;
            if (integrate_on) std::printf("integrate: batch %d: %d lines behind a window of %g%s\n", b, caf->lines(), integrate_window, cfar_on ? ": the detections are the integrated map's" : "");
            for (int e = 0; cancel_on && e < caf->lines(); ++e) {
                double sum = 0.0;
                int n = 0, singular = 0;
                for (int c = 0; c < caf->nrows(); ++c)
                    if (c != caf_ref) { sum += (double)caf->residual(e, c); ++n; singular |= caf->singular(e, c); }
                std::printf("cancel: batch %d line %d: taps %d dopp %d residual %.2f dB%s\n", b, e, cancel.taps, cancel.dopp, 10.0 * std::log10(sum / n),
                            singular ? " (singular)" : "");
            }
            for (int e = 0; cfar_on && e < caf->lines(); ++e)
                for (int k = 0; k < caf->held(e, caf->nrows()); ++k) {
                    const ccaf::det_t &d = caf->detection(e, caf->nrows(), k);
                    std::printf("cfar: batch %d line %d det %d of %d: lag %d%+.3f doppler %d%+.3f snr %.2f dB\n", b, e, k, (int)caf->count[(size_t)e * (caf->nrows() + 1) + caf->nrows()],
                                (int)d.lag, (double)d.dlag, (int)d.doppler, (double)d.ddop, d.snr_db());
                }
            for (int e = 0; clean_on && e < caf->lines(); ++e) {
                const int rows = caf->nrows(), st = (int)caf->tinfo[2 * ((size_t)e * rows + (caf_ref == 0 ? 1 : 0)) + 1];
                for (int t = 0; t < caf->ntgt[(size_t)e]; ++t) {
                    const ccaf::det_t &d = caf->picked(e, t);
                    std::printf("clean: batch %d line %d pick %d of %d: lag %d doppler %.3f snr %.2f dB\n", b, e, t, (int)caf->ntgt[(size_t)e], (int)d.lag,
                                (double)d.doppler + (double)d.ddop, d.snr_db());
                }
                std::printf("clean: batch %d line %d: %d picks status %d residual list %d\n", b, e, (int)caf->ntgt[(size_t)e], st, (int)caf->rcount[(size_t)e * (rows + 1) + rows]);
                for (int k = 0; k < caf->residual_held(e, rows); ++k) {
                    const ccaf::det_t &d = caf->residual_detection(e, rows, k);
                    std::printf("clean: batch %d line %d residual det %d: lag %d%+.3f doppler %d%+.3f snr %.2f dB\n", b, e, k, (int)d.lag, (double)d.dlag, (int)d.doppler,
                                (double)d.ddop, d.snr_db());
                }
            }
            for (int e = 0; bearing_on && e < caf->lines(); ++e)
                for (int k = 0; k < caf->held(e, caf->nrows()); ++k) {
                    const ccaf::dir_t &d = caf->bearing(e, k);
                    std::printf("bearing: batch %d line %d det %d: cell (%d, %d) alpha %.3f deg beta %.3f deg fit %.4f\n", b, e, k, (int)d.cx, (int)d.cy, d.alpha_deg(),
                                d.beta_deg(), (double)d.fit);
                }
            for (int e = 0; adapt_on && e < caf->lines(); ++e) {
                double sum = 0.0;
                int n = 0;
                for (int bm = 0; bm < caf->nbeams(); ++bm) {
                    const float *f = &caf->ainfo[2 * ((size_t)e * caf->nbeams() + bm)];
                    if (f[0] > 0.f && f[1] > 0.f) { sum += 10.0 * std::log10((double)f[0] / (double)f[1]); ++n; }
                }
                std::printf("adapt: batch %d line %d status %d mean gain %.2f dB over %d beams\n", b, e, (int)caf->astat[(size_t)e], n ? sum / n : 0.0, n);
            }
            if (beams_on && !cfar_on) std::printf("beams: %d maps per line (no detector: --cfar fuses their detections)\n", caf->nbeams());
            for (int e = 0; beams_on && cfar_on && e < caf->lines(); ++e)
                for (int k = 0; k < caf->fused_held(e); ++k) {
                    const ccaf::fused_t &d = caf->fused_at(e, k);
                    const int bm = (int)d.beam;
                    std::printf("beams: batch %d line %d fused %d of %d: lag %d%+.3f doppler %d%+.3f power %.6g snr %.2f dB beam %d alpha %.3f deg beta %.3f deg\n", b, e, k,
                                (int)caf->nfused[(size_t)e], (int)d.lag, (double)d.dlag, (int)d.doppler, (double)d.ddop, (double)d.power, d.snr_db(), bm,
                                beam_xy[2 * (size_t)bm] * 1.8, beam_xy[2 * (size_t)bm + 1] * 1.8);
                }
            for (int e = 0; track_on && e < caf->lines(); ++e)
                for (int i = 0; i < caf->max_tracks(); ++i) {
                    const ccaf::track_t &t = caf->track_at(e, i);
                    if (!t.confirmed()) continue;
                    char where[96] = "";
                    if (beams_on) std::snprintf(where, sizeof where, " beam %d", (int)t.aux0);
                    else if (bearing_on) std::snprintf(where, sizeof where, " alpha %.3f deg beta %.3f deg", (double)t.aux0 * 180.0 / bearing.ncx, (double)t.aux1 * 180.0 / bearing.ncy);
                    std::printf("track: batch %d line %d id %d: lag %.3f doppler %.3f rate %.4f age %d hits %d live %d%s\n", b, e, (int)t.id, (double)t.r, (double)t.f,
                                (double)t.g, (int)t.age, (int)t.hits, (int)caf->ntrk[4 * (size_t)e], where);
                }
            for (int e = 0; e < caf->lines(); ++e)
                for (int c = 0; c <= caf->nrows(); ++c) {
                    const ccaf::peak_t &k = caf->at(e, c);
                    char who[32];
                    if (c < caf->nrows()) std::snprintf(who, sizeof who, "row %d", c);
                    else std::snprintf(who, sizeof who, "map");
                    std::printf("caf: batch %d line %d %s: lag %d%+.3f doppler %d%+.3f power %.2f dB ratio %.2f dB\n", b, e, who, (int)k.lag, (double)k.dlag, (int)k.doppler,
                                (double)k.ddop, k.power_db(), k.ratio_db());
                }
        };
        auto run = [&](int n) {
            ok = ok && coherent.submit_batch(0, batch, fl);
            directions(0);
            alignment(0);
            ambiguity(0);
            residual(0);
            for (int b = 1; b < n && ok; ++b) {
                ok = ok && coherent.submit_batch(b & 1, batch, fl);       // upload of batch b overlaps the download of batch b - 1
                directions(b);
                alignment(b);
                ambiguity(b);
                residual(b);
                ok = ok && coherent.collect_batch((b - 1) & 1);
            }
            ok = ok && coherent.collect_batch((n - 1) & 1);
        };
        run(3);                                                           // warm-up: allocations, code objects, link
        report = true;
        residuals = true;
        const auto t0 = std::chrono::steady_clock::now();
        run(nb);
        const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (!ok) { std::printf("bench: engine error\nDEMO FAILED\n"); return 1; }
        const csynth_params *p = source.get_params();
        const int last = (nb - 1) & 1;
        int bad = 0;
        for (int t = 0; t < batch; ++t)
            for (int k = 0; k < nsig; ++k) bad += (coherent.batch_lag(last, t)[1 + k] != (int32_t)p->d[k]);
        const hdr0 *h = reinterpret_cast<const hdr0 *>(coherent.batch_packet(last, batch - 1));
        bad += (h->N != (uint32_t)(1 + nsig)) + (h->L != (uint32_t)L);
        const double bps = (double)nb * batch / dt, gbs = bps * (double)blk / 1e9;
        std::printf("bench: %d batches x %d blocks of (1 + %d) x %d in %.3f s: %.1f blocks/s, %.2f GB/s each way over PCIe, lags %s\n", nb, batch, nsig, L, dt,
                    bps, gbs, bad ? "MISMATCH" : "ok");
        cpacketize::cleanup();
        std::printf("%s\n", bad ? "DEMO FAILED" : "DEMO OK");
        return bad ? 1 : 0;
    }

    if (threads) {
        // f2: every device streams from its own producer thread into a ring (crtlsdr::asynch_threadf /
        // swapbuffer / read / consume), the engine runs in its thread (ccoherent::start) and this thread
        // is the publish loop of src/main.cc:277-279.  Per-row readcnt must be continuous in the packets.
        {
            // Real-time sources start below: warm the process first (code object, streams, page-locked staging, the kernels' first
            // launches) on a throwaway plan of the same shape, or a cold first step costs more than the rings' 8 blocks of slack and
            // the run starts with overruns that have nothing to do with the engine.
            crsdr_plan_desc wd;
            std::memset(&wd, 0, sizeof(wd));
            wd.nrows = 1 + nsig; wd.blocksize = B; wd.mode = mode; wd.device = device; wd.max_batch = std::max(1, batch);
            crsdr_plan *w = nullptr;
            if (crsdr_plan_create(&w, &wd) == CRSDR_OK) {
                std::vector<int8_t> z((size_t)(1 + nsig) * B * (size_t)wd.max_batch, 0);
                for (int i = 0; i < 2; ++i) {
                    (void)crsdr_plan_submit_batch(w, z.data(), CRSDR_MEM_HOST, wd.max_batch, 0, nullptr, nullptr, 0, CRSDR_REFNOISE_ENABLED);
                    (void)crsdr_plan_sync(w);
                }
                crsdr_plan_destroy(w);
            }
        }
        std::vector<uint32_t> lastcnt(1 + nsig, 0);
        size_t gaps = 0;
        std::atomic<size_t> npk{0};
        cpacketize::sink = [&](const int8_t *p, size_t, const std::complex<float> *, size_t) {
            const uint32_t *rc = reinterpret_cast<const uint32_t *>(p + 16);
            for (int c = 0; c <= nsig; ++c) { if (npk && rc[c] != lastcnt[c] + 1) ++gaps; lastcnt[c] = rc[c]; }
            ++npk;
        };
        const int pace_us = pace_us_arg >= 0 ? pace_us_arg : pace_ms ? pace_ms * 1000 : 3000;
        if (batched) {
            // the engine thread a batch at a time (ccoherent::start_batched): every block's packet is published from there with
            // each device's own read counter.  With --engine-delay-ms the reader is slower than the producers: rings overrun,
            // blocks are lost, and the ONLY trace of that is a jump in that row's read counter (README.md:42) -- which must
            // therefore show in the headers of the batched engine exactly as it does in step()'s.
            std::vector<uint32_t> first(1 + nsig, 0), last(1 + nsig, 0);
            size_t jumps = 0, backwards = 0, npk2 = 0;
            cpacketize::sink = [&](const int8_t *p, size_t, const std::complex<float> *, size_t) {
                const uint32_t *rc = reinterpret_cast<const uint32_t *>(p + 16);
                for (int c = 0; c <= nsig; ++c) {
                    if (!npk2) first[c] = rc[c];
                    else { jumps += rc[c] > last[c] + 1; backwards += rc[c] <= last[c]; }
                    last[c] = rc[c];
                }
                ++npk2;
            };
            ref.start(pace_us, blocks);
            for (auto &d : own) d->start(pace_us, blocks);
            coherent.start_batched(batch, engine_delay_ms * 1000);
            // wait until the producers are done and less than a batch is left in some ring (the engine cannot fill another one)
            for (int spin = 0; spin < 60000; ++spin) {
                bool done = ref.produced_all(blocks) && ref.backlog() < (uint32_t)batch;
                for (auto &d : own) done = done || (d->produced_all(blocks) && d->backlog() < (uint32_t)batch);
                bool all_prod = ref.produced_all(blocks);
                for (auto &d : own) all_prod = all_prod && d->produced_all(blocks);
                if (all_prod && done) break;
                usleep(1000);
            }
            usleep(200 * 1000);                          // the batch in flight
            coherent.request_exit();
            ref.stop();
            for (auto &d : own) d->stop();
            coherent.join();
            uint32_t over = ref.get_overruns();
            for (auto &d : own) over += d->get_overruns();
            size_t skipped = 0;
            for (int c = 0; c <= nsig; ++c) skipped += npk2 ? (last[c] - first[c] + 1) - npk2 : 0;
            std::printf("streaming batched: %zu packets, %zu read-counter jumps (%zu blocks skipped), %zu backwards, %u ring overruns\n", npk2, jumps, skipped, backwards, over);
            // every skipped count is a block a ring dropped; drops behind the last published block do not show
            fails += (npk2 == 0) + (backwards != 0) + (skipped > over) + (engine_delay_ms > 0 ? (over == 0 || jumps == 0) : (over != 0 || jumps != 0));
            cpacketize::cleanup();
            std::printf("%s\n", fails ? "DEMO FAILED" : "DEMO OK");
            return fails ? 1 : 0;
        }
        if (!replay.empty()) {
            // recorded streams: one raw offset-binary uint8 file per channel, row 0 = the reference-noise channel
            bool ok = ref.start_replay((replay + "0.u8").c_str(), pace_us, blocks);
            for (int k = 0; k < nsig; ++k) ok = own[k]->start_replay((replay + std::to_string(1 + k) + ".u8").c_str(), pace_us, blocks) && ok;
            if (!ok) { std::printf("DEMO FAILED\n"); return 1; }
        } else {
            ref.start(pace_us, blocks);
            for (auto &d : own) d->start(pace_us, blocks);
        }
        coherent.start();
        // a ring that overran has dropped a block: the engine then waits for a block that never comes and this loop for a packet that
        // never comes.  Watch for it -- every producer done, every ring empty, no packet for a second -- and let go, so that a lost block
        // is a FAILED line below, not a hang
        std::atomic<bool> fin{false};
        std::thread guard([&] {
            size_t seen = 0;
            int idle = 0;
            while (!fin.load()) {
                usleep(50 * 1000);
                bool starving = ref.drained((uint32_t)blocks);
                for (auto &d : own) starving = starving && d->drained((uint32_t)blocks);
                if (starving && npk.load() == seen) { if (++idle >= 20) { ref.packetize.request_exit(); break; } }
                else idle = 0;
                seen = npk.load();
            }
        });
        for (int t = 0; t < blocks; ++t)
            if (cpacketize::send() < 0) break;
        fin = true;
        guard.join();
        coherent.request_exit();
        ref.stop();
        for (auto &d : own) d->stop();
        coherent.join();
        const csynth_params *p = source.get_params();
        for (int k = 0; k < nsig; ++k) {
            if (!replay.empty()) std::printf("row %d: lag %ld\n", 1 + k, (long)devs[k]->get_lagp()->lag);   // the recording's truth is the caller's
            else fails += ((long)devs[k]->get_lagp()->lag != (long)p->d[k]);
        }
        uint32_t over = ref.get_overruns();
        for (auto &d : own) over += d->get_overruns();
        std::printf("streaming: %zu packets, %zu readcnt gaps, %u ring overruns, lags %s\n", npk.load(), gaps, over, fails ? "MISMATCH" : "ok");
        fails += (npk.load() != (size_t)blocks) + (gaps != 0) + (over != 0);
        cpacketize::cleanup();
        std::printf("%s\n", fails ? "DEMO FAILED" : "DEMO OK");
        return fails ? 1 : 0;
    }
    if (servo) {
        // f3: closed loop.  Each device's ccontrol reads the lag the engine reports, slews the (modelled)
        // resampler, re-measures, and marks the device synchronized at |lag| <= sync_threshold -- after which
        // nobody requests lags and the engine runs its locked cadence.
        std::vector<ccontrol> ctl;
        for (auto &d : own) ctl.emplace_back(d.get());
        int t = 0, synced_at = -1;
        for (; t < blocks; ++t) {
            source.advance();
            if (!coherent.step()) { std::fprintf(stderr, "step failed\n"); return 2; }
            cpacketize::send();
            int nsync = 0;
            for (size_t k = 0; k < ctl.size(); ++k) { ctl[k].on_block(); nsync += own[k]->get_synchronized(); }
            if (nsync == nsig && synced_at < 0) synced_at = t;
            if (synced_at >= 0 && t >= synced_at + 12) break;   // a dozen locked blocks for the EMA to settle
        }
        const csynth_params *p = source.get_params();
        for (int k = 0; k < nsig; ++k) {
            std::complex<float> ph = devs[k]->get_phasecorrect();
            const double resid = std::arg(std::complex<double>(ph.real(), ph.imag()) * std::polar(1.0, std::atan2(p->s[k], p->c[k])));
            const bool ok = own[k]->get_synchronized() && p->d[k] == 0 && devs[k]->get_lagp()->lag == 0.0f && std::fabs(resid) < 0.02;
            std::printf("row %d: synchronized %d, residual delay %ld, last lag %.0f, residual phase %+.5f rad  %s\n", 1 + k,
                        (int)own[k]->get_synchronized(), (long)p->d[k], devs[k]->get_lagp()->lag, resid, ok ? "ok" : "MISMATCH");
            fails += !ok;
        }
        std::printf("servo: all synchronized after %d blocks, %u locked (phase-only) blocks of %d\n", synced_at, coherent.get_locked_steps(), t + 1);
        fails += (synced_at < 0) + (coherent.get_locked_steps() < 10);
        cpacketize::cleanup();
        std::printf("%s\n", fails ? "DEMO FAILED" : "DEMO OK");
        return fails ? 1 : 0;
    }

    for (int t = 0; t < blocks; ++t) {
        source.advance();
        if (t == 0 && !dump.empty()) {
            FILE *f = std::fopen(dump.c_str(), "wb");
            if (f) { std::fwrite(source.row(0), 1, (size_t)(1 + nsig) * B, f); std::fclose(f); }
        }
        for (auto *d : devs) d->requestfft();                 // "track" cadence: every row asks for a lag every block
        if (!coherent.step()) { std::fprintf(stderr, "step failed\n"); return 2; }
        cpacketize::send();                                    // main-thread publish loop, src/main.cc:277-279
        if (pace_ms) usleep(pace_ms * 1000);
    }
    const csynth_params *p = source.get_params();
    for (int k = 0; k < nsig; ++k) {
        const lagpoint *lp = devs[k]->get_lagp();
        std::complex<float> ph = devs[k]->get_phasecorrect();
        const double phi = std::atan2(p->s[k], p->c[k]);
        const double resid = std::arg(std::complex<double>(ph.real(), ph.imag()) * std::polar(1.0, phi));
        const bool lag_ok = ((long)lp->lag == (long)p->d[k]);
        const bool ph_ok = (mode != CRSDR_MODE_DIGITAL) || (std::fabs(resid) < 0.02);
        std::printf("row %d: lag %6.0f (injected %6ld) mag %10.1f  phasor %+.4f%+.4fj  residual phase %+.5f rad  %s\n", 1 + k,
                    lp->lag, (long)p->d[k], lp->mag, ph.real(), ph.imag(), resid, (lag_ok && ph_ok) ? "ok" : "MISMATCH");
        fails += !(lag_ok && ph_ok);
    }
    if (music) {
        // what the reference's beamformer client does with a packet (beamformclient/heatmap2d2.cpp:185-203).  The
        // synthetic channels all carry the reference noise, so once aligned the array sees one source at
        // broadside: steering vector of all ones, alpha = beta = pi/2, grid point (50, 50).
        cmatrix Rxx, U;
        std::vector<float> S, pm;
        int M = 0;
        if (nsig != cbeamformer::MX * cbeamformer::MY || cbeamformer::covariance(last_packet.data(), Rxx, M) ||
            cbeamformer::noisesubspace(Rxx, M, U, &S) ||
            cbeamformer::pmusic2dvec(U, M, 1, cbeamformer::D, cbeamformer::MX, cbeamformer::MY, cbeamformer::CX, cbeamformer::CY, pm)) {
            std::printf("music: chain failed (needs --nsig 21)\n");
            ++fails;
        } else {
            size_t best = 0;
            for (size_t i = 1; i < pm.size(); ++i) if (pm[i] > pm[best]) best = i;
            const int cx = (int)(best / cbeamformer::CY), cy = (int)(best % cbeamformer::CY);
            std::printf("music: singular values %.4f %.4f .. %.4f, peak (%d, %d) of %d x %d\n", S[0], S[1], S[M - 1], cx, cy, cbeamformer::CX, cbeamformer::CY);
            fails += (mode == CRSDR_MODE_DIGITAL) && !(cx == 50 && cy == 50 && S[0] > 10 * S[1]);
        }
    }
    std::printf("packets sent %zu, last hdr {seq %u, N %u, L %u}, %zu bytes\n", packets, last_seq, last_N, last_L, last_bytes);
    fails += (packets != (size_t)blocks) + (last_N != (uint32_t)(1 + nsig)) + (last_L != (uint32_t)L) + (last_seq != (uint32_t)(blocks - 1));
    cpacketize::cleanup();
    std::printf("%s\n", fails ? "DEMO FAILED" : "DEMO OK");
    return fails ? 1 : 0;
}
