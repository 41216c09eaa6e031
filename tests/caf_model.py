"""fp64 numpy statement of crsdr_caf / crsdr_ambiguity (include/crsdr.h, section (w)): every row's range-Doppler map (cross-ambiguity
function) against row r, the array map, the peak figures, and the error bars of the device against it.

Definition.  A packet's matrix is [nrows][B] int8; row c holds L = B / 2 samples, used as the INTEGERS X_c[n] = I + jQ.  Ls = seg,
R = nlags, r = ref_row.  A packet has J = L / Ls segments, never across packets; a line is `frames` consecutive packets; slow time
k = t J + j < nd = frames J.

    y_c[k][tau]   = sum_{n < Ls} X_c[t][j Ls + n] conj(X_r[t][j Ls + n - tau])      tau < R, X_r[t][m] = 0 for m < 0: exact integers
    chi_c[d][tau] = 1 / (127^2 Ls sum_k w[k]) * sum_k w[k] y_c[k][tau] exp(-2 pi i d k / nd)        chi [nrows][nd][R] complex
    map[d][tau]   = sum_{c != r} |chi_c[d][tau]|^2                                                   from the published fp32 chi

w = 1 (WINDOW_RECT) or 0.5 - 0.5 cos(2 pi k / nd) (WINDOW_HANN, periodic) over k.

Peak figures of a map P [nd][R] (a row's re^2 + im^2 of the published chi, or the published map), all in fp64: s(d) = d for d < nd / 2,
else d - nd; S = {(d, tau): |s(d)| >= guard};

    lag, doppler = tau*, s(d*)     the first maximum of P over S in the order of d R + tau
    power        = P*
    ratio        = P* / mean of P over S                                0 if the mean is 0
    dlag         = 0.5 (P- - P+) / (P- - 2 P* + P+) from (d*, tau* -+ 1)      0 at tau* = 0 or R - 1, 0 if the denominator is >= 0
    ddop         = the same from (d* -+ 1 mod nd, tau*)                         0 if a neighbour is outside S, 0 if the denominator is >= 0

both offsets clamped to [-0.5, 0.5]; each figure rounded once to fp32.  Where P* = 0 (every searched cell is zero, as for an all-zero packet)
the position means nothing and all six figures are 0.

Error bar of chi, per cell, on the real and on the imaginary part.  The range stage is exact.  The device converts y to fp32 (one
rounding, u = 2^-24: |y| reaches 2^27), multiplies by the fp32 window (one more), transforms over k in fp32 and multiplies by the scale
once.  An nd-point fp32 FFT with correctly rounded twiddles has ||dX||_2 <= log2(nd) eta ||X||_2, eta < 7 u (Higham, Accuracy and
Stability of Numerical Algorithms, Thm 24.2) -- the transform term of spectra_model.py -- and the two roundings in front of it add 2 u
of the same norm:

    bar_c[tau] = u (7 log2 nd + 2) * scale * || w o y_c[:, tau] ||_2,          scale = 1 / (127^2 Ls sum w)

the same for every Doppler bin of the column.  Nothing in it is measured.  (chi_f32 below, a complex64 radix-2 restatement, stays
within 0.12 .. 0.58 of it at the shapes the tests use: tests/test_caf_model.py.)

Error bar of map.  From the device's own fp32 chi in fp64: nrows - 1 positive terms in any order, one rounding:
    |dev - model| <= map (u + nrows e),        e = 2^-53

Error bars of the peak figures, evaluated on the device's own published arrays (as spectra_model.align is).  P = re re + im im is the
same three IEEE fp64 operations on both sides, so the cells, and with them the first maximum, agree exactly:
    lag, doppler   0
    power          u P*                        (the one fp32 rounding; nothing else separates the two)
    ratio          ratio (u + n e)             n = |S|: a sum of n positive fp64 terms in any order is within (n - 1) e of itself
    dlag, ddop     |x| (u + 8 e (1 + (|P-| + 2 P* + |P+|) / |den|)) + 2^-149
                                               the two differences and the quotient in fp64, carried through the denominator's condition
"""
import numpy as np

from doa_subband_model import WINDOW_HANN, WINDOW_RECT, _fft32, window

U = 2.0 ** -24
E64 = 2.0 ** -53
MUTATIONS = ["conjugate", "lag_sign", "wrap", "cross_packet", "doppler_sign", "fast_window", "sum_w2"]      # (and peaks(strict=True): > for >=)


def parts(matrix):
    """(I, Q) [nrows][L] int64 of an int8 matrix [nrows][B]"""
    m = np.asarray(matrix).astype(np.int64)
    return m[:, 0::2], m[:, 1::2]


def range_stage(matrices, seg, nlags, ref, which=None):
    """y [nrows][nd][R] as (real, imag) int64 of one line (a list of `frames` int8 matrices): exact.  which: one of MUTATIONS"""
    I = np.concatenate([parts(m)[0][:, None, :] for m in matrices], axis=1)      # [nrows][frames][L]
    Q = np.concatenate([parts(m)[1][:, None, :] for m in matrices], axis=1)
    nrows, F, L = I.shape
    J = L // seg
    kind = np.float64 if which == "fast_window" else np.int64
    yr, yi = np.zeros((nrows, F * J, nlags), dtype=kind), np.zeros((nrows, F * J, nlags), dtype=kind)
    w_fast = window(seg, WINDOW_HANN)
    for tau in range(nlags):
        def shifted(a):
            a = a[ref]
            if which == "wrap":
                return np.roll(a, tau, axis=1)
            if which == "lag_sign":
                return np.concatenate([a[:, tau:], np.zeros((F, tau), dtype=a.dtype)], axis=1)
            if which == "cross_packet":                              # the reference reaches into the packet before
                flat = np.concatenate([np.zeros(tau, dtype=a.dtype), a.reshape(-1)])[:F * L]
                return flat.reshape(F, L)
            return np.concatenate([np.zeros((F, tau), dtype=a.dtype), a[:, :L - tau]], axis=1)
        Ir, Qr = shifted(I), shifted(Q)
        re = I * Ir + Q * Qr
        im = (I * Qr - Q * Ir) if which == "conjugate" else (Q * Ir - I * Qr)
        re, im = re.reshape(nrows, F * J, seg), im.reshape(nrows, F * J, seg)
        if which == "fast_window":                                   # (no longer integers)
            re, im = re * w_fast, im * w_fast
        yr[:, :, tau], yi[:, :, tau] = re.sum(axis=2), im.sum(axis=2)
    return yr, yi


def scale_of(seg, nd, kind):
    return 1.0 / (127.0 * 127.0 * seg * np.sum(window(nd, kind)))


def caf_from_y(yr, yi, seg, kind, which=None):
    """(chi [nrows][nd][R] complex128, bar [nrows][1][R]) from the range stage's sums"""
    y = yr.astype(np.float64) + 1j * yi.astype(np.float64)
    nd = y.shape[1]
    w = np.ones(nd) if which == "fast_window" else window(nd, kind)
    wy = y * w[None, :, None]
    sc = 1.0 / (127.0 * 127.0 * seg * (np.sum(w * w) if which == "sum_w2" else np.sum(w)))
    chi = (np.fft.ifft(wy, axis=1) * nd if which == "doppler_sign" else np.fft.fft(wy, axis=1)) * sc
    bar = U * (7.0 * np.log2(nd) + 2.0) * sc * np.sqrt(np.sum(np.abs(wy) ** 2, axis=1, keepdims=True))
    return chi, bar


def caf(matrices, seg, nlags, ref, kind, which=None):
    """(chi [nrows][nd][R] complex128, bar [nrows][1][R]) of one line (a list of `frames` int8 matrices), fp64"""
    return caf_from_y(*range_stage(matrices, seg, nlags, ref, which), seg, kind, which)


def caf_direct(matrices, seg, nlags, ref, kind):
    """chi by its definition, one sum per cell over every sample of the line: O(L nd R) per row, for small shapes"""
    F = len(matrices)
    X = [parts(m)[0].astype(np.float64) + 1j * parts(m)[1].astype(np.float64) for m in matrices]
    nrows, L = X[0].shape
    J = L // seg
    nd = F * J
    w = window(nd, kind)
    chi = np.zeros((nrows, nd, nlags), dtype=np.complex128)
    n = np.arange(L)
    k_of = n // seg
    for d in range(nd):
        for tau in range(nlags):
            for t in range(F):
                xr = np.where(n - tau >= 0, X[t][ref][np.maximum(n - tau, 0)], 0.0)
                k = t * J + k_of
                chi[:, d, tau] += np.sum(X[t] * np.conj(xr)[None, :] * (w[k] * np.exp(-2j * np.pi * d * k / nd))[None, :], axis=1)
    return chi * scale_of(seg, nd, kind)


def caf_f32(matrices, seg, nlags, ref, kind):
    """what the device computes, restated in numpy float32: exact integers, one rounding to fp32, times the fp32 window, an fp32
    transform, times the fp32 scale.  Not its bits (another butterfly network): its error class."""
    yr, yi = range_stage(matrices, seg, nlags, ref)
    nd = yr.shape[1]
    w32 = window(nd, kind).astype(np.float32)[None, :, None]
    x = ((yr.astype(np.float32) * w32) + 1j * (yi.astype(np.float32) * w32)).astype(np.complex64)
    tw = np.exp(-2j * np.pi * np.arange(nd) / nd).astype(np.complex64)
    X = _fft32(np.ascontiguousarray(np.swapaxes(x, 1, 2)), tw)                   # [nrows][R][nd]
    sc = np.float32(scale_of(seg, nd, kind))
    return np.swapaxes((X.real * sc) + 1j * (X.imag * sc), 1, 2).astype(np.complex64)


def worst_ratio(got, want, bar):
    """max |got - want| / bar, real and imaginary part apart; 0 / 0 counts as 0"""
    got, want = np.asarray(got), np.asarray(want)
    err = np.maximum(np.abs(got.real - want.real), np.abs(got.imag - want.imag)) if np.iscomplexobj(got) or np.iscomplexobj(want) else np.abs(got - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0.0, 0.0, err / np.broadcast_to(bar, err.shape))
    return float(np.max(r))


# ---- the array map and the peak figures, from published fp32 arrays ----
def power(chi32):
    c = np.asarray(chi32)
    re, im = c.real.astype(np.float64), c.imag.astype(np.float64)
    return re * re + im * im


def array_map(chi32, ref):
    """(map [nd][R] fp64, its bar) from chi [nrows][nd][R] complex64"""
    P = power(chi32)
    m = np.sum(np.delete(P, ref, axis=0), axis=0)
    return m, m * (U + P.shape[0] * E64)


def signed_bins(nd):
    d = np.arange(nd)
    return np.where(d < nd // 2, d, d - nd)


def in_set(nd, guard, strict=False):
    s = np.abs(signed_bins(nd))
    return s > guard if strict else s >= guard


def _vertex(pm, p0, pp):
    """(offset, bar)"""
    den = pm - 2.0 * p0 + pp
    if not den < 0.0:
        return 0.0, 0.0
    x = min(0.5, max(-0.5, 0.5 * (pm - pp) / den))
    return x, abs(x) * (U + 8.0 * E64 * (1.0 + (abs(pm) + 2.0 * abs(p0) + abs(pp)) / abs(den))) + 2.0 ** -149


def peaks(P, guard, strict=False):
    """(figures [6] fp64 = (lag, doppler, power, ratio, dlag, ddop), bars [6]) of P [nd][R] fp64.  strict: the mistake of > for >="""
    P = np.asarray(P, dtype=np.float64)
    nd, R = P.shape
    ok = in_set(nd, guard, strict)
    if not ok.any():
        return np.zeros(6), np.zeros(6)
    masked = np.where(ok[:, None], P, -np.inf)
    i = int(np.argmax(masked))                                                   # (numpy: the first maximum in C order)
    d, tau = divmod(i, R)
    best = P[d, tau]
    if not best > 0.0:
        return np.zeros(6), np.zeros(6)
    n = int(ok.sum()) * R
    mean = P[ok].sum() / n
    ratio = best / mean if mean > 0 else 0.0
    dlag, blag = _vertex(P[d, tau - 1], best, P[d, tau + 1]) if 0 < tau < R - 1 else (0.0, 0.0)
    dm, dp = (d - 1) % nd, (d + 1) % nd
    ddop, bdop = _vertex(P[dm, tau], best, P[dp, tau]) if ok[dm] and ok[dp] else (0.0, 0.0)
    fig = np.array([tau, signed_bins(nd)[d], best, ratio, dlag, ddop], dtype=np.float64)
    return fig, np.array([0.0, 0.0, U * best, ratio * (U + n * E64), blag, bdop])


def all_peaks(chi32, map32, guard):
    """(peak [nrows + 1][6], bars) as the device lays them out: the rows' |chi|^2, then the published map"""
    rows = [peaks(power(c), guard) for c in np.asarray(chi32)] + [peaks(np.asarray(map32, dtype=np.float64), guard)]
    return np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])


# ---- inputs ----
def random_matrix(nrows, B, seed):
    """int8 [nrows][B], every byte uniform over -128 .. 127"""
    return np.random.default_rng(seed).integers(-128, 128, size=(nrows, B), dtype=np.int64).astype(np.int8)


def quantise(x, rms=30.0):
    """complex [L] -> interleaved int8 [2 L] at `rms` LSB rms of the complex sample"""
    x = x * (rms / np.sqrt(np.mean(np.abs(x) ** 2)))
    out = np.zeros(2 * len(x), dtype=np.int8)
    out[0::2], out[1::2] = np.clip(np.rint(x.real), -128, 127), np.clip(np.rint(x.imag), -128, 127)
    return out


def echo_scene(B, frames, echoes, nrows=2, ref=0, seed=0, direct=0.8, noise=0.05):
    """a line of `frames` int8 matrices [nrows][B].  Row ref is complex white noise, one stream across the line's packets.  Every other row
    is direct * reference + its own weak noise, plus, per echo (row, t0, d0, a): a * (the reference delayed by t0 samples and rotated by
    d0 cycles per line).  Every row is quantised at 30 LSB rms."""
    rng = np.random.default_rng(seed)
    L = B // 2
    N = frames * L
    hist = max([t0 for _, t0, _, _ in echoes] + [0])
    cn = lambda n: (rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2.0)
    s = cn(N + hist)
    n = np.arange(N)
    rows = []
    for c in range(nrows):
        if c == ref:
            rows.append(s[hist:])
            continue
        x = direct * s[hist:] + noise * cn(N)
        for row, t0, d0, a in echoes:
            if row == c:
                x = x + a * s[hist - t0:hist - t0 + N] * np.exp(2j * np.pi * d0 * n / N)
        rows.append(x)
    q = np.stack([quantise(x) for x in rows])                                    # [nrows][2 N]
    return [np.ascontiguousarray(q[:, 2 * t * L:2 * (t + 1) * L]) for t in range(frames)]
