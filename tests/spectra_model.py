"""fp64 numpy statement of crsdr_spectra / crsdr_welch (include/crsdr.h, section (v)): Welch auto-spectra of every row, cross-spectra
against row 0, the four alignment figures, and the error bars of the device against it.

Definition.  A packet's matrix is [nrows][B] int8; row c = 0 .. nrows - 1 (row 0, the reference channel, included) holds L = B / 2
samples x_c[n] = (I + jQ) / 127.  N = nfft, the hop is H = N (overlap 0) or N / 2 (overlap 1); a packet has J = (L - N) / H + 1 segments,
segment j from sample jH on, never across packets.  A line is `frames` consecutive packets: J' = frames * J segments.

    X_c[t][j][f] = sum_n w[n] x_c[jH + n] exp(-2 pi i f n / N)
    P_c[f] = 1 / (J' N sum w^2) * sum_{t,j} |X_c[t][j][f]|^2                      psd   [nrows][N]
    S_c[f] = 1 / (J' N sum w^2) * sum_{t,j} conj(X_0[t][j][f]) X_c[t][j][f]       cross [nrows][N] complex;  S_0 = (P_0, 0)

w = 1 (WINDOW_RECT) or 0.5 - 0.5 cos(2 pi n / N) (WINDOW_HANN, periodic).  No mean is removed: DC lands in bin 0.

Alignment figures over the signed bins s_i = lo + i, i < K = hi - lo + 1, bin f_i = s_i mod N, in fp64 from the PUBLISHED fp32 P and S:

    A         = sum_{i < K-1} S_c[f_{i+1}] conj(S_c[f_i])
    delay     = -atan2(Im A, Re A) N / (2 pi)                       0 if A == 0       (row c = row 0 delayed by `delay` samples)
    z         = sum_i S_c[f_i] exp(+2 pi i s_i delay / N)
    phase     = atan2(Im z, Re z)
    gain      = |z| / sum_i P_0[f_i]                                0 if the denominator is 0
    coherence = min(1, sum_i |S_c[f_i]|^2 / sum_i P_0[f_i] P_c[f_i])        0 if the denominator is 0 (1 for J' = 1)

each rounded once to fp32.

Error bar of psd and cross, per bin.  The device keeps the integers I, Q, multiplies by the fp32 window (one rounding, u = 2^-24, exact
for rect), transforms in fp32, accumulates |X|^2 and conj(X_0) X over the T <= 32 segments of a chain in fp32 with fmaf (csrc/spectra.hpp:
SP_CHAIN; where a chain is cut depends on (B, N, overlap) alone: chains() below), and does everything behind that (chains, packets,
scale) in fp64 with one final rounding.

  transform   An N-point fp32 FFT with correctly rounded twiddles has ||dX||_2 <= log2(N) eta ||X||_2, eta < 7 u (Higham, Accuracy and
              Stability of Numerical Algorithms, Thm 24.2); the window's rounding adds u.  Spread over the N bins that is
              |dX_c[j][f]| <= (7 log2 N + 1) u ||w x_c[j]||_2.  By Cauchy-Schwarz over the segments, and with
              sum_j ||w x_c[j]||^2 = J' sum w^2 * sum_f P_c[f], the term sum_j |dX_a| |X_b| is, after the scale, at most
              (7 log2 N + 1) u sqrt(M_a P_b[f]) with M_a = (1/N) sum_f P_a[f] the row's mean bin power.  Both factors carry it: twice.
  sums        A real or imaginary part is a chain of 2T fmaf: at most gamma_2T = 2 T u times sum_j |X_a| |X_b| <= sqrt(P_a P_b).
  rounding    u |S| <= u sqrt(P_a P_b) for the one rounding to fp32 (the fp64 work is 2^-29 of that).

With s_c[f] = max(P_c[f], M_c) (the second carries the transform's error into a bin much weaker than the rest of the spectrum):

    bar[f] = u (2 (7 log2 N + 1) + 2 T + 1) sqrt(s_a[f] s_b[f]),        u = 2^-24,   a = b = c for psd, a = 0 and b = c for cross

on the real and on the imaginary part.  Nothing in it is measured.

Error bar of the alignment figures.  Device and model start from the same fp32 arrays, so only fp64 work and one fp32 rounding
separate them.  A sum of K fp64 terms t_i computed in any order is off by at most (K - 1) e sum |t_i| and each complex product by 2 e
of its size, e = 2^-53; 4 K e sum |t_i| covers both with room.  Carried through atan2 (|d angle| <= |dA| / |A|, plus atan2's own few e):

    d_delay = (4 K e * sum |t_i| / |A| + 8 e) N / (2 pi)
    dz      = sum_i |S_i| * (4 K e + 2 pi max|s_i| d_delay / N + 4 e (1 + max |theta_i|))     theta_i = 2 pi s_i delay / N, the device's
                                                                                              own delay and its sin / cos in it
    delay:      d_delay + u |delay|            phase:      dz / |z| + 8 e + u |phase|
    gain:       gain (dz / |z| + 4 K e + u)    coherence:  coherence (8 K e + u)

The condition numbers sum |t_i| / |A| and sum |S_i| / |z| are 1 for a coherent row and grow as the coherence falls: the test scenes
keep it high."""
import numpy as np

from doa_subband_model import WINDOW_HANN, WINDOW_RECT, _fft32, window

U = 2.0 ** -24
E64 = 2.0 ** -53
THREADS, POINTS, CHAIN = 256, 4096, 32       # csrc/spectra.hpp: SP_THREADS, SP_POINTS, SP_CHAIN


def hop(N, overlap):
    return N // 2 if overlap else N


def segments(B, N, overlap):
    return (B // 2 - N) // hop(N, overlap) + 1


def chains(B, N, overlap):
    """the fp32 chains of one packet, each a list of segment indices in the order they are added (csrc/spectra.hpp): a chunk is
    POINTS / N segments, taken round robin by THREADS / N lanes (one lane from N = 256 on); a lane's sums are cut after CHAIN segments"""
    J, spc, lanes = segments(B, N, overlap), POINTS // N, max(THREADS // N, 1)
    cpg = CHAIN * lanes // spc                   # chunks per chain
    out = {}
    for j in range(J):
        q, jj = divmod(j, spc)
        out.setdefault((q // cpg, jj % lanes), []).append(j)
    return [out[k] for k in sorted(out)]


def terms(B, N, overlap):
    """T: the most segments an fp32 chain accumulates"""
    return max(len(c) for c in chains(B, N, overlap))


def samples(matrix):
    """every row of an int8 matrix [nrows][B] as complex fp64 [nrows][L]"""
    x = np.asarray(matrix).astype(np.float64) / 127.0
    return x[:, 0::2] + 1j * x[:, 1::2]


def segment_spectra(matrices, N, overlap, kind, w=None, H=None):
    """X [J'][nrows][N] of the packets of one line"""
    w = window(N, kind) if w is None else w
    H = hop(N, overlap) if H is None else H
    out = []
    for mat in matrices:
        x = samples(mat)
        J = (x.shape[1] - N) // H + 1
        seg = np.stack([x[:, j * H:j * H + N] for j in range(J)])                 # [J][nrows][N]
        out.append(np.fft.fft(seg * w, axis=2))
    return np.concatenate(out, axis=0)


def welch(matrices, N, overlap, kind):
    """(psd [nrows][N], cross [nrows][N] complex) of one line (a list of `frames` int8 matrices), fp64"""
    w = window(N, kind)
    X = segment_spectra(matrices, N, overlap, kind, w)
    scale = 1.0 / (X.shape[0] * N * np.sum(w * w))
    psd = np.sum(np.abs(X) ** 2, axis=0) * scale
    cross = np.sum(X[:, :1, :].conj() * X, axis=0) * scale
    cross[0] = psd[0]
    return psd, cross


def bars(psd, N, T):
    """(bar of psd [nrows][N], bar of cross [nrows][N]) of the docstring, from the model's psd"""
    s = np.maximum(psd, psd.mean(axis=1, keepdims=True))
    c = U * (2.0 * (7.0 * np.log2(N) + 1.0) + 2.0 * T + 1.0)
    return c * s, c * np.sqrt(s[:1] * s)


def worst_ratio(got, want, bar):
    """max |got - want| / bar, real and imaginary part apart; 0 / 0 (an all-zero row) counts as 0"""
    got, want = np.asarray(got), np.asarray(want)
    err = np.maximum(np.abs(got.real - want.real), np.abs(got.imag - want.imag)) if np.iscomplexobj(got) or np.iscomplexobj(want) else np.abs(got - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0.0, 0.0, err / bar)
    return float(np.max(r))


# ---- the alignment figures ----
def band(N, lo, hi):
    """(signed bins s [K], bins f [K])"""
    assert -N // 2 <= lo < hi <= N // 2 - 1
    s = np.arange(lo, hi + 1)
    return s, s % N


def align(psd, cross, lo, hi, wrap=True):
    """(figures [nrows][4] fp64 = (delay, phase, gain, coherence), their bars [nrows][4]) from psd [nrows][N] and cross [nrows][N]
    (the published fp32 arrays, or the model's own).  wrap=False: the mistake of leaving the negative bins unwrapped."""
    psd, cross = np.asarray(psd, dtype=np.float64), np.asarray(cross, dtype=np.complex128)
    nrows, N = psd.shape
    s, f = band(N, lo, hi)
    if not wrap:
        f = np.abs(s)
    K = len(s)
    out, bar = np.zeros((nrows, 4)), np.zeros((nrows, 4))
    P0 = psd[0, f]
    for c in range(nrows):
        S, Pc = cross[c, f], psd[c, f]
        t = S[1:] * S[:-1].conj()
        A = t.sum()
        delay = 0.0 if A == 0 else -np.arctan2(A.imag, A.real) * N / (2.0 * np.pi)
        theta = 2.0 * np.pi * s * delay / N
        z = np.sum(S * np.exp(1j * theta))
        phase = np.arctan2(z.imag, z.real)
        den = P0.sum()
        gain = abs(z) / den if den > 0 else 0.0
        pp = np.sum(P0 * Pc)
        coh = min(1.0, np.sum(np.abs(S) ** 2) / pp) if pp > 0 else 0.0
        out[c] = delay, phase, gain, coh
        if abs(A) > 0 and abs(z) > 0:
            d_delay = (4 * K * E64 * np.abs(t).sum() / abs(A) + 8 * E64) * N / (2.0 * np.pi)
            dz = np.abs(S).sum() * (4 * K * E64 + 2.0 * np.pi * np.abs(s).max() * d_delay / N + 4 * E64 * (1.0 + np.abs(theta).max()))
            bar[c] = (d_delay + U * abs(delay), dz / abs(z) + 8 * E64 + U * abs(phase), gain * (dz / abs(z) + 4 * K * E64 + U), coh * (8 * K * E64 + U))
    return out, bar


def align_errors(got, want):
    """|got - want| [nrows][4], the phase compared on the circle"""
    e = np.abs(np.asarray(got, dtype=np.float64) - want)
    dphi = np.asarray(got, dtype=np.float64)[:, 1] - want[:, 1]
    e[:, 1] = np.abs((dphi + np.pi) % (2.0 * np.pi) - np.pi)
    return e


# ---- the kernel's arithmetic in fp32 (numpy has no fmaf: products are rounded once more, inside the same bar) ----
def welch_f32(matrices, N, overlap, kind):
    """what the device computes, restated in numpy float32: integers times the fp32 window, an fp32 transform, fp32 sums over each
    chain's segments in order, fp64 behind them, one rounding.  Not its bits (another butterfly network, no fmaf): its error class."""
    w32 = window(N, kind).astype(np.float32)
    tw = np.exp(-2j * np.pi * np.arange(N) / N).astype(np.complex64)
    H = hop(N, overlap)
    tp = tc = None
    nseg = 0
    for mat in matrices:
        a = np.asarray(mat).astype(np.float32)
        nrows, B = a.shape
        J = segments(B, N, overlap)
        seg = np.stack([a[:, 2 * j * H:2 * (j * H + N)] for j in range(J)])       # [J][nrows][2N]
        x = ((seg[:, :, 0::2] * w32) + 1j * (seg[:, :, 1::2] * w32)).astype(np.complex64)
        X = _fft32(x, tw)
        for chain in chains(B, N, overlap):
            p, s = np.zeros((nrows, N), dtype=np.float32), np.zeros((nrows, N), dtype=np.complex64)
            for j in chain:
                v = X[j]
                p = (p + (v.real * v.real + v.imag * v.imag).astype(np.float32)).astype(np.float32)
                s = (s + (v[:1].conj() * v).astype(np.complex64)).astype(np.complex64)
            tp = p.astype(np.float64) if tp is None else tp + p.astype(np.float64)
            tc = s.astype(np.complex128) if tc is None else tc + s.astype(np.complex128)
        nseg += J
    sw2 = N if kind == WINDOW_RECT else 0.375 * N
    scale = 1.0 / (127.0 * 127.0 * nseg * N * sw2)
    psd, cross = (tp * scale).astype(np.float32), (tc * scale).astype(np.complex64)
    cross[0] = psd[0]
    return psd, cross


# ---- the model with one mistake in it: each must leave the bar ----
MUTATIONS = ["last_segment", "hop", "frames", "conjugate", "sum_w"]      # (and align(wrap=False): the band's negative bins not wrapped)


def mutated(matrices, N, overlap, kind, which):
    w = window(N, kind)
    X = segment_spectra(matrices, N, overlap, kind, w, H=N if which == "hop" else None)
    if which == "last_segment":
        per = X.shape[0] // len(matrices)
        X = np.concatenate([X[t * per:(t + 1) * per - 1] for t in range(len(matrices))], axis=0)
    nseg = X.shape[0] // len(matrices) if which == "frames" else X.shape[0]
    den = nseg * N * (np.sum(w) if which == "sum_w" else np.sum(w * w))
    psd = np.sum(np.abs(X) ** 2, axis=0) / den
    cross = (np.sum(X[:, :1, :] * X.conj(), axis=0) if which == "conjugate" else np.sum(X[:, :1, :].conj() * X, axis=0)) / den
    cross[0] = psd[0]
    return psd, cross


# ---- inputs ----
def gaussian_matrix(nrows, B, seed, sigma=30.0, common=0.9):
    """int8 [nrows][B]: every row shares a Gaussian reference (weight `common`) under its own noise, so that the cross-spectra are not
    just noise and the coherence is high"""
    rng = np.random.default_rng(seed)
    ref = rng.standard_normal((1, B))
    x = sigma * (common * ref + np.sqrt(1.0 - common * common) * rng.standard_normal((nrows, B)))
    x[0] = sigma * ref[0]
    return np.clip(np.rint(x), -128, 127).astype(np.int8)


def tone_matrix(nrows, B, N, bin_, amp=50.0):
    """a tone exactly on bin `bin_` of an N-point segment in every row, row c rotated by 0.3 c rad"""
    n = np.arange(B // 2)
    out = np.zeros((nrows, B), dtype=np.int8)
    for c in range(nrows):
        x = amp * np.exp(2j * np.pi * bin_ * n / N + 0.3j * c)
        out[c, 0::2], out[c, 1::2] = np.rint(x.real), np.rint(x.imag)
    return out
