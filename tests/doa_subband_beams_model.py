"""fp64 numpy statement of the band beams (crsdr_doa_set_subband_beams / crsdr_subband_beamform, include/crsdr.h), the error bar of the
device against it, and the three-emitter scene its tests use.

Definition.  Subbands are on: N = nfft, first, nbands, width, window w (tests/doa_subband_model.py).  X_c[j][f] is the segment spectrum
of signal row c = 1 .. m of a packet: samples x = (I + jQ) / 127, window, forward transform, J = L / N segments per packet.  With
c_w = 1 / sqrt(N sum_n w[n]^2) and weights u [nbands][nbeams][m] (per (estimate, band) and slot, exactly crsdr_doa_set_beams' from that
band's vec, sv and directions: tests/doa_beams_model.py),

    Y[i][b][j][u] = c_w sum_c u_{i,b}[c - 1] X_c[j][(first + i width + u) mod N]                 NO conjugate

Empty slots have weights 0, so zeros.  c_w is the normalisation behind R_f: (1 / J') sum_j |Y|^2 over an estimate's segments and a
band's bins is u^H R_band u.

Error bar of an fp32 evaluation, per real and imaginary part of Y, u = 2^-24.  Two things are rounded: the transform and the sum.

  transform   An N-point fp32 FFT with correctly rounded twiddles has ||dX||_2 <= log2(N) eta ||X||_2 with eta < 7 u (Higham, Accuracy
              and Stability of Numerical Algorithms, Thm 24.2); the rounding of the fp32 window adds u; ||X||_2 = sqrt(N) ||w x[j]||_2.
              Spread over the N bins, as tests/doa_subband_model.py takes it: |dX_c[j][f]| <= (7 log2 N + 1) u ||w x_c[j]||_2.  A weight
              multiplies it by at most |Re u_c| + |Im u_c| per component.  The same holds when the weighted sum of the rows is transformed
              instead: the transform's input is then sum_c u_c w x_c, whose 2-norm is at most sum_c |u_c| ||w x_c[j]||_2.
  sum         A component of sum_c u_c z_c is a sum of 2 m products: evaluated in any order, fused or not, its error is at most
              gamma_2m = 2 m u / (1 - 2 m u) times the sum of the magnitudes of the products (doa_beams_model.beam_bound's argument,
              which takes (4 m + 4) u to cover unfused products and the 1 / 127); two more roundings are the scale c_w in fp32 and the
              multiplication by it: (4 m + 6) u.  The magnitudes: summed before the transform, z_c = w[n] x_c[n] and the error of
              every sample reaches the bin, sum_n w[n] (|I| + |Q|) / 127 per row; summed after it, z_c = X_c[j][f] itself,
              |Re X_c| + |Im X_c| at the bin.

    bar = c_w u sum_c (|Re u_c| + |Im u_c|) ((7 log2 N + 1) ||w x_c[j]||_2 + (4 m + 6) sum_n w[n] (|I_c| + |Q_c|) / 127)           either order
    bar_transform_first: the second term (4 m + 6) (|Re X_c[j][f]| + |Im X_c[j][f]|) where that is smaller

The device transforms every row first and then sums (csrc/subband_beams.hpp): its tests use bar_transform_first, which is never above
the bar for either order.  Nothing in either is measured."""
import numpy as np

import doa_beams_model as beams_model
import doa_peaks_model as peaks_model
import doa_subband_model as sb
import ura

WINDOW_RECT, WINDOW_HANN = sb.WINDOW_RECT, sb.WINDOW_HANN
CONVENTIONAL, MVDR = beams_model.CONVENTIONAL, beams_model.MVDR
U = 2.0 ** -24


def c_w(N, kind):
    w = sb.window(N, kind)
    return 1.0 / np.sqrt(N * np.sum(w * w))


def segments(matrix, N):
    """x [m][J][N] complex128 = (I + jQ) / 127 of the signal rows, cut into segments"""
    x = sb.samples(matrix)
    return x.reshape(x.shape[0], x.shape[1] // N, N)


def beams(matrix, weights, N, first, nbands, width, kind):
    """Y [nbands][nbeams][J][width] complex128 of one packet's matrix [1 + m][2 L] int8 and weights [nbands][nbeams][m] (used as given)."""
    w = np.asarray(weights).astype(np.complex128)
    X = np.fft.fft(segments(matrix, N) * sb.window(N, kind), axis=2)              # [m][J][N]
    bins = np.asarray(sb.band_bins(N, first, nbands, width))                      # [nbands][width]
    return c_w(N, kind) * np.einsum("ibc,cjiu->ibju", w, X[:, :, bins])


def bar(matrix, weights, N, first, nbands, width, kind, transform_first=False):
    """The docstring's bar, [nbands][nbeams][J][width]"""
    w = np.asarray(weights).astype(np.complex128)
    m = w.shape[2]
    win = sb.window(N, kind)
    seg = segments(matrix, N) * win                                               # [m][J][N]
    norm2 = np.sqrt(np.sum(np.abs(seg) ** 2, axis=2))                             # ||w x_c[j]||_2
    mag = np.sum(np.abs(seg.real) + np.abs(seg.imag), axis=2)                     # sum_n w[n] (|I| + |Q|) / 127
    wm = np.abs(w.real) + np.abs(w.imag)                                          # [nbands][nbeams][m]
    bins = np.asarray(sb.band_bins(N, first, nbands, width))
    second = np.broadcast_to(mag[:, :, None, None], mag.shape + bins.shape)       # [m][J][nbands][width]
    if transform_first:
        X = np.fft.fft(seg, axis=2)[:, :, bins]
        second = np.minimum(second, np.abs(X.real) + np.abs(X.imag))
    per_row = (7.0 * np.log2(N) + 1.0) * norm2[:, :, None, None] + (4.0 * m + 6.0) * second
    return c_w(N, kind) * U * np.einsum("ibc,cjiu->ibju", wm, per_row)


def worst_ratio(got, want, bars):
    """largest error / bar over the components; a zero bar (an all-zero row set or empty slot) allows no error at all"""
    err = np.maximum(np.abs(got.real - want.real), np.abs(got.imag - want.imag))
    if np.any((bars == 0) & (err > 0)):
        return np.inf
    return float(np.max(np.where(bars > 0, err / np.where(bars > 0, bars, 1.0), 0.0)))


# ---- the arithmetic in fp32, in both orders (numpy has no fmaf: products are rounded once more, inside the same bar) ----
def _rows32(matrix, N, kind):
    """[m][J][N] complex64: the integers times the fp32 window"""
    a = np.asarray(matrix)[1:].astype(np.float32)
    w32 = sb.window(N, kind).astype(np.float32)
    m, B = a.shape
    wn = w32[np.arange(B // 2) % N]
    return ((a[:, 0::2] * wn) + 1j * (a[:, 1::2] * wn)).astype(np.complex64).reshape(m, B // (2 * N), N)


def _scale32(N, kind):
    return np.float32(1.0 / (127.0 * np.sqrt(N * (N if kind == WINDOW_RECT else 0.375 * N))))


def beams_f32(matrix, weights, N, first, nbands, width, kind, order="transform_first"):
    w = np.asarray(weights).astype(np.complex64)
    tw = np.exp(-2j * np.pi * np.arange(N) / N).astype(np.complex64)
    x = _rows32(matrix, N, kind)
    m, J, _ = x.shape
    bins = sb.band_bins(N, first, nbands, width)
    out = np.zeros((nbands, w.shape[1], J, width), dtype=np.complex64)
    if order == "transform_first":
        X = sb._fft32(x, tw)
        for i in range(nbands):
            for b in range(w.shape[1]):
                acc = np.zeros((J, width), dtype=np.complex64)
                for c in range(m):
                    acc = (acc + w[i, b, c] * X[c][:, bins[i]]).astype(np.complex64)
                out[i, b] = acc
    else:
        for i in range(nbands):
            for b in range(w.shape[1]):
                z = np.zeros((J, N), dtype=np.complex64)
                for c in range(m):
                    z = (z + w[i, b, c] * x[c]).astype(np.complex64)
                out[i, b] = sb._fft32(z, tw)[:, bins[i]]
    return (out * _scale32(N, kind)).astype(np.complex64)


# ---- the model with one mistake in it: each must leave the bar ----
MUTATIONS = ["bin", "conjugate", "window", "sum_w2", "row", "segment"]


def mutated(matrix, weights, N, first, nbands, width, kind, which):
    w = np.asarray(weights).astype(np.complex128)
    if which == "bin":
        return beams(matrix, w, N, (first + 1) % N, nbands, width, kind)
    if which == "conjugate":
        return beams(matrix, w.conj(), N, first, nbands, width, kind)
    if which == "window":
        return beams(matrix, w, N, first, nbands, width, WINDOW_RECT if kind == WINDOW_HANN else WINDOW_HANN) * c_w(N, kind) / c_w(N, 1 - kind)
    if which == "sum_w2":
        return beams(matrix, w, N, first, nbands, width, kind) / c_w(N, kind) / N
    if which == "row":
        w = w.copy()
        w[:, :, -1] = 0.0
        return beams(matrix, w, N, first, nbands, width, kind)
    if which == "segment":
        return np.roll(beams(matrix, w, N, first, nbands, width, kind), 1, axis=2)
    raise ValueError(which)


def band_power(Y):
    """[nbands][nbeams]: (1 / J') sum |Y|^2 over the packets' segments and the band's bins; Y [packets][nbands][nbeams][J][width]"""
    Y = np.asarray(Y)
    return np.sum(np.abs(Y.astype(np.complex128)) ** 2, axis=(0, 3, 4)) / (Y.shape[0] * Y.shape[3])


# ---- the three-emitter scene: two emitters share a carrier, a third sits on another ----
# (alpha, beta, cycles per sample, amplitude); A and B are doa_subband_model.EMITTERS, C shares A's carrier at half its amplitude.  On the
# 100 x 100 grid of the X^H X convention: A (65, 60), C (40, 42), B (35, 38); nfft 16: A and C in bin 3, B in bin 11.
EMITTERS = [sb.EMITTERS[0], (0.60 * np.pi, 0.58 * np.pi, 3.0 / 16.0, 12.0), sb.EMITTERS[1]]
EMITTER_PEAKS = [(65, 60), (40, 42), (35, 38)]
EMITTER_BINS16 = [3, 3, 11]
SEED, L, NFFT, K, LOADING, COUNT, RADIUS = 5, 8192, 16, 2, 1e-2, 4, 2


def three_emitter_block(Lb=L, rng=None, n0=0, sigma_n=8.0, mx=ura.MX, my=ura.MY, d=ura.D, phi=None):
    """(int8 rows [1 + m][2 L], signals [3][L] complex128): receiver noise first, then per emitter its envelope (the draws of
    doa_subband_model.two_emitter_block, one emitter more).  phi: per-channel receiver phase offsets (what a plan's calibration removes)."""
    rng = np.random.default_rng(SEED) if rng is None else rng
    m = mx * my
    x = sigma_n * (rng.standard_normal((m + 1, Lb)) + 1j * rng.standard_normal((m + 1, Lb))) / np.sqrt(2.0)
    n = n0 + np.arange(Lb)
    sig = []
    for alpha, beta, f, amp in EMITTERS:
        s = amp * sb.envelope(Lb, rng) * np.exp(2j * np.pi * f * n)
        x[1:] += ura.steering(alpha, beta, d, mx, my)[:, None] * s[None, :]
        sig.append(s)
    if phi is not None:
        x[1:] *= np.exp(1j * np.asarray(phi))[:, None]
    return ura.quantise(x), np.stack(sig)


def channelised(sig, N, f, kind):
    """[n][J]: bin f of the segment spectra of signals [n][L], what a perfect beam toward one of them would carry"""
    s = np.asarray(sig)
    return np.fft.fft(s.reshape(s.shape[0], s.shape[1] // N, N) * sb.window(N, kind), axis=2)[:, :, f]


def fp64_band(blocks, f, kind=WINDOW_RECT, k=K):
    """The fp64 pipeline on bin f of one estimate (a list of int8 blocks): (found, peaks, vec complex64, sv float32) with
    set_peaks(COUNT, RADIUS), handed over in fp32 as the device publishes them."""
    Rf = sb.bin_covariances(blocks, NFFT, kind)[f]
    Uv, s, _ = np.linalg.svd(Rf)
    _, pm = sb.music_from_covariance(Rf, k)
    found, peaks, _ = peaks_model.directions(pm.astype(np.float32), COUNT, RADIUS)
    return found, peaks, Uv.astype(np.complex64), s.astype(np.float32)


def check_three_emitters(sig_bins, band, what):
    """The issue's conditions.  sig_bins: {bin: [3][J'] channelised emitter signals}; band: {bin: (found, peaks, Y_mvdr [nbeams][J'],
    Y_conv [nbeams][J'], power_mvdr [nbeams])} for bins 3 and 11."""
    f3, f11 = EMITTER_BINS16[0], EMITTER_BINS16[2]
    found, peaks, ym, yc, pw = band[f3]
    sa, sc_ = beams_model.slot_near(peaks, found, EMITTER_PEAKS[0]), beams_model.slot_near(peaks, found, EMITTER_PEAKS[1])
    S = sig_bins[f3]
    own_a, other_a = beams_model.rho(S[0], ym[sa]), beams_model.rho(S[1], ym[sa])
    own_c, other_c = beams_model.rho(S[1], ym[sc_]), beams_model.rho(S[0], ym[sc_])
    conv_leak = beams_model.rho(S[0], yc[sc_])
    print(f"{what}: bin 3 peaks {np.asarray(peaks)[:found].tolist()}: A slot {sa} own {own_a:.4f} other {other_a:.4f}; C slot {sc_} own {own_c:.4f} "
          f"other {other_c:.4f}, conventional leak {conv_leak:.4f}; MVDR power {np.asarray(pw).tolist()}")
    assert own_a >= 0.95 and other_a <= 0.05 and own_c >= 0.95 and other_c <= 0.05, (what, own_a, other_a, own_c, other_c)
    assert conv_leak >= 10.0 * other_c, (what, conv_leak, other_c)
    assert set(np.argsort(np.asarray(pw)[:found])[::-1][:2].tolist()) == {sa, sc_}, (what, pw, sa, sc_)
    found, peaks, ym, yc, pw = band[f11]
    sb_ = beams_model.slot_near(peaks, found, EMITTER_PEAKS[2])
    S = sig_bins[f11]
    own_b, others = beams_model.rho(S[2], ym[sb_]), max(beams_model.rho(S[0], ym[sb_]), beams_model.rho(S[1], ym[sb_]))
    print(f"{what}: bin 11 peaks {np.asarray(peaks)[:found].tolist()}: B slot {sb_} own {own_b:.4f} (the emitters of the other carrier, as they "
          f"leak into this bin: {others:.4f}); MVDR power {np.asarray(pw).tolist()}")
    assert own_b >= 0.95, (what, own_b)                                          # no other emitter on this carrier
