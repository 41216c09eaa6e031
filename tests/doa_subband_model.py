"""fp64 numpy statement of the subband covariance (crsdr_doa_set_subbands / crsdr_subband_covariance), the two-emitter scene its
tests use, and the error bar of the device against it.

Definition.  A signal row c = 1 .. m of a packet holds L = blocksize / 2 samples x_c[n] = (I + jQ) / 127.  Each row is cut into
J = L / N segments of N = nfft samples (never across packets; an estimate of `frames` packets has J' = frames * J), and

    X_c[j][f] = sum_n w[n] x_c[jN + n] exp(-2 pi i f n / N)
    R_f[a][b] = 1 / (J' N sum_n w[n]^2) * sum_j conj(X_a[j][f]) X_b[j][f]
    band i    = sum of R_f over the bins (first + i * width + u) mod N, u < width
    power[i]  = Re trace(band i) / m

w = 1 (WINDOW_RECT) or 0.5 - 0.5 cos(2 pi n / N) (WINDOW_HANN, periodic).  No mean is removed.

Error bar of the device, per component (a, b) of a band.  The device keeps the integers I, Q, multiplies by the fp32 window (one
rounding, u = 2^-24, exact for rect), transforms in fp32, accumulates conj(X_a) X_b over the T = ceil(J / spb) segments of a K slice in
fp32 with fmaf, and does everything behind that (slices, bins, scale) in fp64 with one final rounding.

  transform   An N-point fp32 FFT with correctly rounded twiddles has ||dX||_2 <= log2(N) eta ||X||_2, eta = u + gamma_4 (sqrt2 + u)
              < 7 u (Higham, Accuracy and Stability of Numerical Algorithms, Thm 24.2); the window's rounding adds u.  Spread over
              the N bins that is |dX_c[j][f]| <= (7 log2 N + 1) u ||w x_c[j]||_2.  By Cauchy-Schwarz over j, and with
              sum_j ||w x_c[j]||^2 = J' sum w^2 * sum_f R_f[c][c], the term sum_j |dX_a| |X_b| is, after the scale, at most
              (7 log2 N + 1) u sqrt(P_a R_f[b][b]) with P_a = (1/N) sum_f R_f[a][a] the row's mean bin power; summed over a band's bins
              (Cauchy-Schwarz again) sqrt(width P_a * R_band[b][b]).  Both factors carry it: twice.
  sums        A real or imaginary part is a chain of 2T fmaf: at most gamma_2T = 2 T u times sum_j |X_a| |X_b| <= sqrt(R_aa R_bb).
  rounding    u |R_ab| <= u sqrt(R_aa R_bb) for the one rounding to fp32 (fp64 work is 2^-29 of that).

With s_c = max(R_band[c][c], width * P_c) (equal for a white row; the second carries the transform's error into a band that is much
weaker than the rest of the spectrum):

    bar[a][b] = u (2 (7 log2 N + 1) + 2 T + 1) sqrt(s_a s_b),        u = 2^-24

on the real and on the imaginary part.  Nothing in it is measured."""
import numpy as np

import ura

WINDOW_RECT, WINDOW_HANN = 0, 1
U = 2.0 ** -24
SLICE_SEGMENTS, MAX_SPB = 64, 16

# the two-emitter scene: (alpha, beta, cycles per sample, amplitude); on the 100 x 100 grid of the X^H X convention (65, 60) and (35, 38)
EMITTERS = [(0.35 * np.pi, 0.40 * np.pi, 3.0 / 16.0, 25.0), (0.65 * np.pi, 0.62 * np.pi, -5.0 / 16.0, 18.0)]
EMITTER_PEAKS = [(65, 60), (35, 38)]
EMITTER_BINS16 = [3, 11]


def window(N, kind):
    return np.ones(N) if kind == WINDOW_RECT else 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N) / N)


def spb(B, N):
    """K slices per packet (csrc/subband.hpp: subband_spb): from (B, N) alone."""
    return min(max((B // (2 * N)) // SLICE_SEGMENTS, 1), MAX_SPB)


def slice_bounds(B, N):
    J, s = B // (2 * N), spb(B, N)
    return [(J * p // s, J * (p + 1) // s) for p in range(s)]


def terms(B, N):
    """T: the most segments an fp32 partial accumulates."""
    return max(hi - lo for lo, hi in slice_bounds(B, N))


def samples(matrix):
    """the signal rows of an int8 matrix [1 + m][B] as complex fp64 [m][L]"""
    x = np.asarray(matrix)[1:].astype(np.float64) / 127.0
    return x[:, 0::2] + 1j * x[:, 1::2]


def spectra(matrices, N, kind, w=None):
    """X [J'][m][N] of the packets of one estimate"""
    w = window(N, kind) if w is None else w
    out = []
    for mat in matrices:
        x = samples(mat)
        m, L = x.shape
        assert L % N == 0
        out.append(np.fft.fft(x.reshape(m, L // N, N) * w, axis=2).transpose(1, 0, 2))
    return np.concatenate(out, axis=0)


def bin_covariances(matrices, N, kind):
    """R_f [N][m][m] of one estimate (a list of `frames` int8 matrices)"""
    w = window(N, kind)
    X = spectra(matrices, N, kind, w)
    return np.einsum("jaf,jbf->fab", X.conj(), X) / (X.shape[0] * N * np.sum(w * w))


def band_bins(N, first, nbands, width):
    return [[(first + i * width + u) % N for u in range(width)] for i in range(nbands)]


def bands(Rf, first, nbands, width):
    """(rbands [nbands][m][m], power [nbands])"""
    N, m = Rf.shape[0], Rf.shape[1]
    rb = np.stack([Rf[idx].sum(axis=0) for idx in band_bins(N, first, nbands, width)])
    return rb, np.trace(rb, axis1=1, axis2=2).real / m


def subband_covariance(matrices, N, first, nbands, width, kind):
    return bands(bin_covariances(matrices, N, kind), first, nbands, width)


def bar(Rf, first, nbands, width, T):
    """bar [nbands][m][m] of the docstring, from the model's R_f"""
    N = Rf.shape[0]
    rb, _ = bands(Rf, first, nbands, width)
    mean_bin = np.einsum("faa->a", Rf).real / N
    s = np.maximum(np.einsum("iaa->ia", rb).real, width * mean_bin[None, :])
    return U * (2.0 * (7.0 * np.log2(N) + 1.0) + 2.0 * T + 1.0) * np.sqrt(s[:, :, None] * s[:, None, :])


def worst_ratio(got, want, bars):
    err = np.maximum(np.abs(got.real - want.real), np.abs(got.imag - want.imag))
    return float(np.max(err / bars))


# ---- the kernel's arithmetic in fp32 (numpy has no fmaf: products are rounded once more, inside the same bar) ----
def _fft32(x, tw):
    """radix-2 decimation in time along the last axis, complex64 throughout; tw = exp(-2 pi i t / N) in complex64"""
    N = x.shape[-1]
    if N == 1:
        return x
    e, o = _fft32(x[..., 0::2], tw[0::2]), _fft32(x[..., 1::2], tw[0::2])
    t = (o * tw[: N // 2]).astype(np.complex64)
    return np.concatenate([e + t, e - t], axis=-1).astype(np.complex64)


def subband_covariance_f32(matrices, N, first, nbands, width, kind):
    """what the device computes, restated in numpy float32: integers times the fp32 window, an fp32 transform, fp32 sums over each
    slice's segments in order, fp64 behind them, one rounding.  Not its bits (another butterfly network, no fmaf): its error class."""
    w32 = window(N, kind).astype(np.float32)
    tw = np.exp(-2j * np.pi * np.arange(N) / N).astype(np.complex64)
    total, nseg = None, 0
    for mat in matrices:
        a = np.asarray(mat)[1:].astype(np.float32)
        m, B = a.shape
        x = ((a[:, 0::2] * w32[np.arange(B // 2) % N]) + 1j * (a[:, 1::2] * w32[np.arange(B // 2) % N])).astype(np.complex64)
        X = _fft32(x.reshape(m, B // (2 * N), N), tw)                            # [m][J][N]
        for lo, hi in slice_bounds(B, N):
            acc = np.zeros((N, m, m), dtype=np.complex64)
            for j in range(lo, hi):
                v = X[:, j, :].T                                                  # [N][m]
                acc = (acc + v.conj()[:, :, None] * v[:, None, :]).astype(np.complex64)
            total = acc.astype(np.complex128) if total is None else total + acc.astype(np.complex128)
        nseg += B // (2 * N)
    sw2 = N if kind == WINDOW_RECT else 0.375 * N
    Rf = total / (127.0 * 127.0 * nseg * N * sw2)
    rb, pw = bands(Rf, first, nbands, width)
    return rb.astype(np.complex64), pw.astype(np.float32)


# ---- the model with one mistake in it: each must leave the bar ----
MUTATIONS = ["window", "bin", "conjugate", "last_segment", "sum_w2"]


def mutated(matrices, N, first, nbands, width, kind, which):
    w = window(N, kind)
    if which == "window":
        X = spectra(matrices, N, kind, window(N, WINDOW_RECT if kind == WINDOW_HANN else WINDOW_HANN))
    else:
        X = spectra(matrices, N, kind, w)
    if which == "last_segment":
        X = X[:-1]
    nseg = sum(np.asarray(mt).shape[1] // (2 * N) for mt in matrices)
    sw2 = N if which == "sum_w2" else np.sum(w * w)
    if which == "conjugate":
        Rf = np.einsum("jaf,jbf->fab", X, X.conj()) / (nseg * N * sw2)
    else:
        Rf = np.einsum("jaf,jbf->fab", X.conj(), X) / (nseg * N * sw2)
    return bands(Rf, (first + 1) % N if which == "bin" else first, nbands, width)


# ---- the two-emitter scene ----
def envelope(L, rng, taps=64):
    """unit-power complex Gaussian through a `taps`-tap boxcar"""
    g = (rng.standard_normal(L + taps - 1) + 1j * rng.standard_normal(L + taps - 1)) / np.sqrt(2.0)
    return np.convolve(g, np.ones(taps), mode="valid") / np.sqrt(taps)


def two_emitter_block(L, rng, n0=0, sigma_n=8.0, mx=ura.MX, my=ura.MY, d=ura.D):
    """int8 rows [1 + m][2L]: two band-limited emitters on different carriers and white receiver noise; n0: the block's first sample"""
    m = mx * my
    x = sigma_n * (rng.standard_normal((m + 1, L)) + 1j * rng.standard_normal((m + 1, L))) / np.sqrt(2.0)
    n = n0 + np.arange(L)
    for alpha, beta, f, amp in EMITTERS:
        s = amp * envelope(L, rng) * np.exp(2j * np.pi * f * n)
        x[1:] += ura.steering(alpha, beta, d, mx, my)[:, None] * s[None, :]
    return ura.quantise(x)


def music_from_covariance(R, k, d=ura.D, mx=ura.MX, my=ura.MY, ncx=100, ncy=100):
    """(sv, pm [ncx][ncy]) of ura.music_fp64, from a covariance"""
    Uv, s, _ = np.linalg.svd(R)
    Un = Uv[:, k:]
    ix, iy = np.tile(np.arange(mx), my), np.repeat(np.arange(my), mx)
    al, be = np.arange(ncx)[:, None] * np.pi / ncx, np.arange(ncy)[None, :] * np.pi / ncy
    ph = 2.0 * np.pi * float(d) * (ix[None, None, :] * (np.cos(al) * np.sin(be))[:, :, None] + iy[None, None, :] * np.cos(be)[:, :, None] * np.ones_like(al)[:, :, None])
    a = np.exp(1j * ph)                                                           # [ncx][ncy][m]
    den = np.sum(np.abs(a.conj() @ Un) ** 2, axis=2)
    return s, (mx * my / den) ** 2
