"""The reference-noise canceller's definition (include/crsdr.h, crsdr_plan_set_refcancel) in numpy: integer sums in int64, the solve
and the output sample in fp64, and a float32 restatement of the output sample (one rounding per operation, taps ascending) whose own
rounding excess sets the error bar of the device tests.  Rows are int8 [B] with I and Q interleaved, L = B / 2 complex samples."""
import numpy as np

MAX_TAPS = 9
STATUS_SINGULAR, STATUS_IDLE = 1, 2


def to_ints(row_i8):
    """int8 [2 L] -> (I, Q) int64 [L]"""
    r = np.asarray(row_i8, dtype=np.int8).astype(np.int64)
    return r[0::2], r[1::2]


def signed(rows, offset_binary=False):
    """the signed int8 counts of a block given as int8, or as offset-binary uint8"""
    r = np.asarray(rows)
    return (r.view(np.uint8) ^ np.uint8(0x80)).view(np.int8) if offset_binary else r.view(np.int8)


def shift(x, d):
    """y[n] = x[n + d] for 0 <= n + d < L, zero elsewhere (x any 1-D array)"""
    L = x.shape[0]
    y = np.zeros_like(x)
    if d >= 0:
        if d < L:
            y[:L - d] = x[d:]
    elif -d < L:
        y[-d:] = x[:L + d]
    return y


def tap_rows(r, K, direction=1):
    """[2 K + 1][L]: r_j[n] = r[n - j], j = -K .. K, zero-filled (direction = -1: the mutation r[n + j])"""
    return np.stack([shift(r, -direction * j) for j in range(-K, K + 1)])


def sums(y, R, conj_c=True):
    """(c [taps], G [taps][taps], E) as exact integers held in complex128 / float64 (every component below 2^53): y, R complex with
    integer parts.  c_j = sum y conj(r_j), G_ij = sum conj(r_i) r_j, E = sum |y|^2."""
    yi, yq = np.rint(y.real).astype(np.int64), np.rint(y.imag).astype(np.int64)
    ri, rq = np.rint(R.real).astype(np.int64), np.rint(R.imag).astype(np.int64)
    if conj_c:
        c = (ri @ yi + rq @ yq) + 1j * (ri @ yq - rq @ yi)
    else:                                                         # the mutation: the conjugate forgotten
        c = (ri @ yi - rq @ yq) + 1j * (ri @ yq + rq @ yi)
    G = (ri @ ri.T + rq @ rq.T) + 1j * (ri @ rq.T - rq @ ri.T)    # conj(r_i) r_j
    E = int(yi @ yi + yq @ yq)
    return c.astype(np.complex128), G.astype(np.complex128), E


def toeplitz_gram(r, K):
    """the Toeplitz approximation of G (every entry the full-row autocorrelation at lag j - i): what the definition is NOT"""
    L = r.shape[0]
    t = {m: np.sum(np.conj(r[:L - m]) * r[m:]) for m in range(0, 2 * K + 1)}          # sum conj(r[n]) r[n + m]
    G = np.zeros((2 * K + 1, 2 * K + 1), dtype=np.complex128)
    for i in range(2 * K + 1):
        for j in range(2 * K + 1):
            # conj(r[n - i]) r[n - j] = conj(r[m]) r[m + i - j]
            G[i, j] = t[i - j] if i >= j else np.conj(t[j - i])
    return G


def solve(G, c, E):
    """(g complex128 [taps], residual float64, status): Cholesky in fp64 with the pivot rule of the definition"""
    n = G.shape[0]
    floor = np.ldexp(G[n // 2, n // 2].real, -40)
    Lf = np.zeros((n, n), dtype=np.complex128)
    ok = True
    for k in range(n):
        d = G[k, k].real - np.sum(np.abs(Lf[k, :k]) ** 2)
        if not d > floor:
            ok = False
            break
        Lf[k, k] = np.sqrt(d)
        for i in range(k + 1, n):
            Lf[i, k] = (G[i, k] - np.sum(Lf[i, :k] * np.conj(Lf[k, :k]))) / Lf[k, k]
    g = np.zeros(n, dtype=np.complex128)
    if ok:
        y = np.zeros(n, dtype=np.complex128)
        for i in range(n):
            y[i] = (c[i] - np.sum(Lf[i, :i] * y[:i])) / Lf[i, i]
        for i in range(n - 1, -1, -1):
            g[i] = (y[i] - np.sum(np.conj(Lf[i + 1:, i]) * g[i + 1:])) / Lf[i, i].real
    return g, residual_share(E, g, c), 0 if ok else STATUS_SINGULAR


def residual_share(E, g, c):
    if E == 0:
        return 1.0
    return float(np.clip((E - np.sum(np.conj(g) * c).real) / E, 0.0, 1.0))


def output64(y, R, g, p):
    """w = p (y - sum_j g_j r_j) in fp64 (g, p as given: the published fp32 values widen exactly)"""
    g = np.asarray(g, dtype=np.complex128)
    return complex(p) * (y.astype(np.complex128) - g @ R.astype(np.complex128))


def output32(y, R, g, p):
    """the same in float32 arithmetic: one rounding per operation, taps ascending, products before sums"""
    f = np.float32
    zr, zi = y.real.astype(f), y.imag.astype(f)
    g = np.asarray(g, dtype=np.complex64)
    for j in range(R.shape[0]):
        gr, gi = f(g[j].real), f(g[j].imag)
        rI, rQ = R[j].real.astype(f), R[j].imag.astype(f)
        zr = zr - (gr * rI - gi * rQ)
        zi = zi - (gr * rQ + gi * rI)
    pr, pi = f(np.complex64(p).real), f(np.complex64(p).imag)
    return (pr * zr - pi * zi).astype(np.float64) + 1j * (pr * zi + pi * zr).astype(np.float64)


def quantise(w):
    """clip(rint(w), -128, 127), ties to even, I and Q interleaved: int8 [2 L]"""
    out = np.empty(2 * w.shape[0], dtype=np.int8)
    out[0::2] = np.clip(np.rint(w.real), -128, 127).astype(np.int8)
    out[1::2] = np.clip(np.rint(w.imag), -128, 127).astype(np.int8)
    return out


def excess(q_i8, w):
    """largest |q - clip(w, -128, 127)| - 0.5 over the I and Q of every sample: <= 0 for a correctly rounded row"""
    q = np.asarray(q_i8, dtype=np.int8).astype(np.float64)
    flat = np.empty(2 * w.shape[0])
    flat[0::2], flat[1::2] = w.real, w.imag
    return float(np.max(np.abs(q - np.clip(flat, -128.0, 127.0)))) - 0.5


def row_parts(block, row, d, K, direction=1):
    """(y, R) of one row of a signed block [nrows][B]: complex128 with integer parts"""
    si, sq = to_ints(block[row])
    ri, rq = to_ints(block[0])
    y = shift(si + 1j * sq, int(d))
    return y, tap_rows(ri + 1j * rq, K, direction)


def cancel_row(block, row, d, p, taps, mutation=None):
    """One row by the definition: dict(g, g32, residual, status, cond, y, R, w64 (from g32 and p), out).  mutation: None, or one of
    "tapdir" (r[n + j]), "noconj" (c_j without the conjugate), "toeplitz" (the Toeplitz Gram), "pconj" (p conjugated): a device
    that made that single mistake -- its coefficients, and its bytes from its own coefficients."""
    K = (taps - 1) // 2
    y, R = row_parts(block, row, d, K, -1 if mutation == "tapdir" else 1)
    c, G, E = sums(y, R, conj_c=mutation != "noconj")
    if mutation == "toeplitz":
        G = toeplitz_gram(R[K], K)
    g, res, status = solve(G, c, E)
    g32 = g.astype(np.complex64)
    with np.errstate(all="ignore"):
        ev = np.linalg.eigvalsh(G)
    cond = float(ev[-1] / ev[0]) if ev[0] > 0 else np.inf
    pp = np.conj(np.complex64(p)) if mutation == "pconj" else np.complex64(p)
    w64 = output64(y, R, g32, pp)
    return dict(g=g, g32=g32, residual=np.float32(res), status=status, cond=cond, y=y, R=R, w64=w64, out=quantise(w64), G=G, c=c, E=E)


def cancel_block(block, lag, phasor, taps):
    """The per-op call by the definition on a signed block [nrows][B]: dict(out [nrows][B] int8, coef [nrows][taps] complex64, residual,
    status, cond [nrows], g64 [nrows][taps]); row 0 copied, zeros in its per-row outputs."""
    block = np.asarray(block, dtype=np.int8)
    nrows, B = block.shape
    out = np.zeros((nrows, B), dtype=np.int8)
    out[0] = block[0]
    coef, g64 = np.zeros((nrows, taps), dtype=np.complex64), np.zeros((nrows, taps), dtype=np.complex128)
    res, st, cond = np.zeros(nrows, dtype=np.float32), np.zeros(nrows, dtype=np.int32), np.zeros(nrows)
    for r in range(1, nrows):
        m = cancel_row(block, r, int(lag[r]), phasor[r], taps)
        out[r], coef[r], g64[r], res[r], st[r], cond[r] = m["out"], m["g32"], m["g"], m["residual"], m["status"], m["cond"]
    return dict(out=out, coef=coef, residual=res, status=st, cond=cond, g64=g64)


# ---- a scene: band-limited reference noise, a row that carries it delayed by a fraction of a sample -----------------------------
def band_noise(rng, L, band, sigma):
    """complex noise of per-component standard deviation sigma occupying the centre `band` of the sampled band"""
    x = rng.standard_normal(L) + 1j * rng.standard_normal(L)
    f = np.fft.fftfreq(L)
    X = np.fft.fft(x) * (np.abs(f) <= band / 2)
    y = np.fft.ifft(X)
    return y * sigma / np.sqrt(np.mean(np.abs(y) ** 2) / 2)


def delay(x, D):
    """x delayed by D samples (band-limited interpolation, circular)"""
    f = np.fft.fftfreq(x.shape[0])
    return np.fft.ifft(np.fft.fft(x) * np.exp(-2j * np.pi * f * D))


def to_i8(x):
    out = np.empty(2 * x.shape[0], dtype=np.int8)
    out[0::2] = np.clip(np.rint(x.real), -128, 127).astype(np.int8)
    out[1::2] = np.clip(np.rint(x.imag), -128, 127).astype(np.int8)
    return out


def noise_scene(seed, L, D, nsig=1, band=0.8, sigma_noise=25.0, sigma_rx=4.0, gain=0.7):
    """(block int8 [1 + nsig][2 L], share [nsig]): row 0 the noise alone, every signal row gain * noise delayed by D plus receiver
    noise; share = the part of the row's power that is not the delayed noise (receiver noise and the row's own quantisation)."""
    rng = np.random.default_rng(seed)
    nz = band_noise(rng, L, band, sigma_noise)
    block = np.zeros((1 + nsig, 2 * L), dtype=np.int8)
    block[0] = to_i8(nz)
    share = np.zeros(nsig)
    for k in range(nsig):
        part = gain * delay(nz, D) * np.exp(1j * rng.uniform(0, 2 * np.pi))
        rx = sigma_rx * (rng.standard_normal(L) + 1j * rng.standard_normal(L))
        block[1 + k] = to_i8(part + rx)
        si, sq = to_ints(block[1 + k])
        y = si + 1j * sq
        share[k] = np.sum(np.abs(y - part) ** 2) / np.sum(np.abs(y) ** 2)
    return block, share
