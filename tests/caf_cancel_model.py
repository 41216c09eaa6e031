"""fp64 numpy statement of crsdr_caf's canceller (include/crsdr.h, section (w), "Cancellation"; crsdr_caf_set_cancel and
crsdr_ambiguity_cancel), on top of caf_model.py, and the error bars of the device against it.

Definition.  y, k, nd, Ls, R, r, w and scale are caf_model.py's.  taps = K, dopp = P, n = K (2 P + 1).  Basis member (m, p), index
j = (p + P) K + m, is in segment k the reference delayed by m samples (zeros in front of the packet) times phi_p[k] = exp(2 pi i p k / nd).

    G[k][m][tau]    = sum_{n < Ls} X_r[j Ls + n - m] conj(X_r[j Ls + n - tau])              exact integers, G[k][0][tau] = y_r[k][tau]
    c_(m',p')       = sum_k conj(phi_p'[k]) y_c[k][m']
    A_(m',p'),(m,p) = sum_k phi_(p-p')[k] G[k][m][m']                                       Hermitian, one per line
    E               = sum |X_c|^2 over the line
    A h_c = c;  a Cholesky pivot <= 2^-40 A_00 makes the line singular: h = 0, status 1
    y'_c[k][tau]    = y_c[k][tau] - sum_(m,p) h_c,(m,p) phi_p[k] G[k][m][tau]               row r untouched
    share           = clamp((E - Re sum conj(h) c) / E, 0, 1), 1 where E = 0

and chi is caf_model.caf_from_y of y'.

Error bars.  e = 2^-53, u = 2^-24.

h.  The device forms A and c by fp64 sums of nd products of an exactly converted integer and a phase (itself within 2 e of phi): each
entry is within 2 (nd + 6) e of the sum of the magnitudes of its terms (a complex product's two-term parts carry sqrt(2) gamma_2 < 2 e
each, the recursive sum nd e).  Call those perturbations dA (Frobenius norm over Aabs = sum_k |G|) and dc (over cabs = sum_k |y|).
The Cholesky solve is backward stable: (A + DA) h^ = c with |DA| <= gamma_(3n+1) |L| |L^H| (Higham, Accuracy and Stability of Numerical
Algorithms, Thm 10.4) and || |L| |L^H| ||_2 <= n ||A||_2 (his (10.7)); complex arithmetic costs a factor below 4 on gamma (his
Lemma 3.5), so ||DA||_2 <= 4 n (3 n + 1) e ||A||_2.  First-order perturbation theory then gives

    ||h^ - h||_2 <= ||A^-1||_2 ((4 n (3 n + 1) e ||A||_2 + 2 (nd + 6) e ||Aabs||_F) ||h||_2 + 2 (nd + 6) e ||cabs||_2)  =: dh

that is 2^-53 cond(A) times a constant of about 4 n (3 n + 1) + 4 (nd + 6), relative to ||h||.  The published coef adds one fp32 rounding
per part: bar_coef = dh + u |h_j|.  dh bounds every component.  cond(A) is computed here, and the scene builders assert cond(A) <= 16
so that this bar stays some 10^-10 of ||h||: it cannot hide a mistake.

chi.  caf_model's bar on y' (the one rounding of y' to fp32 is the rounding it already counts), plus what the error of the device's
fp64 h carries through G, plus the fp64 evaluation of the n + 1 term sum (each complex multiply-add within 4 e of its magnitude):

    bar_c[tau] = u (7 log2 nd + 2) scale ||w o y'_c[:, tau]||_2 + scale sum_k w[k] (dh sum_m,p |G[k][m][tau]| + 4 (n + 2) e T_c[k][tau])

with T = |y| + sum |h phi G| the sum of the term magnitudes (y' itself is a difference of large numbers and scales nothing here).

share.  |d share| <= (dh ||c||_2 + 2 (n + 2) e sum |h| |c|) / E + u share.  The status is exact.
"""
import numpy as np

import caf_model as M
from caf_model import E64, U

MUTATIONS = ["h_conj", "g_toeplitz", "front_zeros", "phi_sign_c", "phi_sign_sub", "a_transposed", "fp32_accumulate", "ref_cancelled", "window_first"]
STATUS_SINGULAR = 1


def basis(taps, dopp):
    return taps * (2 * dopp + 1)


def bad_limit(nd, R, lines, taps, dopp):
    """the number of the limit that fails (0: none), as csrc/caf_cancel_solve.hpp counts them"""
    if not 0 <= dopp <= 2:
        return 1
    if not 1 <= taps <= min(R, 32):
        return 2
    if basis(taps, dopp) > 48:
        return 3
    if 2 * dopp + 1 > nd:
        return 4
    if lines * nd * taps * R > 2 ** 24:
        return 5
    return 0


def delayed(matrices, ref, taps, wrap=False):
    """per packet an int8 matrix [taps + 1][B]: the reference delayed by m = 0 .. taps - 1 samples, zeros in front (wrap: the mistake of
    taking them from the packet's end), and the reference itself as the last row"""
    out = []
    for mt in matrices:
        x = np.asarray(mt)[ref]
        rows = []
        for m in range(taps):
            d = np.roll(x, 2 * m)
            if not wrap:
                d[:2 * m] = 0
            rows.append(d)
        out.append(np.stack(rows + [x]))
    return out


def ref_sums(matrices, seg, nlags, ref, taps, which=None):
    """G [nd][K][R] complex128, exact integers"""
    gr, gi = M.range_stage(delayed(matrices, ref, taps, wrap=which == "front_zeros"), seg, nlags, taps)
    G = np.swapaxes((gr + 1j * gi)[:taps].astype(np.complex128), 0, 1)
    if which == "g_toeplitz":                                                    # a function of tau - m alone: the segment's edge terms are lost
        T = G.copy()
        for m in range(taps):
            for tau in range(nlags):
                T[:, m, tau] = G[:, 0, tau - m] if tau >= m else np.conj(G[:, 0, m - tau])
        G = T
    return G


def phases(nd, dopp):
    """phi [2 P + 1][nd], p = -P .. P"""
    return np.exp(2j * np.pi * np.arange(-dopp, dopp + 1)[:, None] * np.arange(nd)[None, :] / nd)


def _cholesky_ok(A):
    """the pivot rule: every pivot > 2^-40 A_00"""
    floor_ = A[0, 0].real * 2.0 ** -40
    n = A.shape[0]
    L = np.zeros_like(A)
    for k in range(n):
        d = A[k, k].real - np.sum(np.abs(L[k, :k]) ** 2)
        if not d > floor_:
            return False
        L[k, k] = np.sqrt(d)
        L[k + 1:, k] = (A[k + 1:, k] - L[k + 1:, :k] @ np.conj(L[k, :k])) / L[k, k]
    return True


def normal_equations(y, G, dopp, weights=None):
    """(A [n][n], c [nrows][n], Aabs, cabs) from y [nrows][nd][R] and G [nd][K][R]"""
    nd, K, _ = G.shape
    P = dopp
    phi = phases(nd, P)
    wk = np.ones(nd) if weights is None else weights
    n = basis(K, P)
    A, Aabs = np.zeros((n, n), dtype=np.complex128), np.zeros((n, n))
    for pi in range(2 * P + 1):
        for pj in range(2 * P + 1):
            f = np.exp(2j * np.pi * (pj - pi) * np.arange(nd) / nd) * wk
            blk = np.einsum("k,kmt->tm", f, G[:, :, :K])                         # [m'][m]
            A[pi * K:(pi + 1) * K, pj * K:(pj + 1) * K] = blk
            Aabs[pi * K:(pi + 1) * K, pj * K:(pj + 1) * K] = np.einsum("k,kmt->tm", wk, np.abs(G[:, :, :K]))
    c = np.concatenate([np.einsum("k,rkm->rm", np.conj(phi[p]) * wk, y[:, :, :K]) for p in range(2 * P + 1)], axis=1)
    cabs = np.concatenate([np.einsum("k,rkm->rm", wk, np.abs(y[:, :, :K])) for p in range(2 * P + 1)], axis=1)
    return A, c, Aabs, cabs


def s_sums(G, dopp):
    """S [4 P + 1][K][K]: S[q + 2 P][m][m'] = sum_k phi_q[k] G[k][m][m'], as csrc/caf_cancel_solve.hpp's gram_entry reads it"""
    nd, K, _ = G.shape
    return np.stack([np.einsum("k,kmt->mt", np.exp(2j * np.pi * q * np.arange(nd) / nd), G[:, :, :K]) for q in range(-2 * dopp, 2 * dopp + 1)])


def energy(matrices):
    """E [nrows]: sum |X_c|^2 over the line, exact"""
    return sum((np.asarray(m).astype(np.int64) ** 2).sum(axis=1) for m in matrices).astype(np.float64)


def cancel(matrices, seg, nlags, ref, kind, taps, dopp, which=None):
    """one line (a list of `frames` int8 matrices) -> dict: chi [nrows][nd][R] complex128 and its bar [nrows][1][R]; h [nrows][n] and hbar;
    share [nrows] and sbar; status; cond; y, yc (= y'), terms (the term magnitudes T) [nrows][nd][R]; G; A; c.  which: one of MUTATIONS"""
    yr, yi = M.range_stage(matrices, seg, nlags, ref)
    y = yr.astype(np.float64) + 1j * yi.astype(np.float64)
    nrows, nd, R = y.shape
    K, P, n = taps, dopp, basis(taps, dopp)
    G = ref_sums(matrices, seg, nlags, ref, K, which)
    w = M.window(nd, kind)
    A, c, Aabs, cabs = normal_equations(y, G, P, weights=w if which == "window_first" else None)
    if which == "phi_sign_c":
        c = np.concatenate([c[:, (2 * P - p) * K:(2 * P - p + 1) * K] for p in range(2 * P + 1)], axis=1)
    if which == "a_transposed":
        A = A.T.copy()
    E = energy(matrices)
    ok = _cholesky_ok(A)
    h = np.zeros((nrows, n), dtype=np.complex128)
    cond, inv_norm = np.inf, np.inf
    if ok:
        sv = np.linalg.svd(A, compute_uv=False)
        cond, inv_norm = float(sv[0] / sv[-1]), float(1.0 / sv[-1])
        h = np.linalg.solve(A, c.T).T
        if which != "ref_cancelled":
            h[ref] = 0.0
    hn = np.linalg.norm(h, axis=1)
    if ok:
        a2 = float(np.linalg.norm(A, 2))
        dh = inv_norm * ((4.0 * n * (3 * n + 1) * E64 * a2 + 2.0 * (nd + 6) * E64 * np.linalg.norm(Aabs)) * hn + 2.0 * (nd + 6) * E64 * np.linalg.norm(cabs, axis=1))
        dh[ref] = 0.0
    else:
        dh = np.zeros(nrows)
    hbar = dh[:, None] + U * np.abs(h)
    phi = phases(nd, P)
    hs = np.conj(h) if which == "h_conj" else h
    ps = np.conj(phi) if which == "phi_sign_sub" else phi
    F = np.stack([ps[j // K][:, None] * G[:, j % K, :] for j in range(n)])       # [n][nd][R]: phi_p[k] G[k][m][tau]
    if which == "fp32_accumulate":
        acc = y.astype(np.complex64)
        for j in range(n):
            acc = (acc - (hs[:, j].astype(np.complex64)[:, None, None] * F[j].astype(np.complex64)[None])).astype(np.complex64)
        yc = acc.astype(np.complex128)
    else:
        yc = y - np.einsum("rj,jkt->rkt", hs, F)
    terms = np.abs(y) + np.einsum("rj,jkt->rkt", np.abs(h), np.abs(F))
    gsum = np.sum(np.abs(G), axis=1)                                             # [nd][R]
    with np.errstate(divide="ignore", invalid="ignore"):
        share = np.where(E > 0, np.clip((E - np.sum(np.conj(h) * c, axis=1).real) / np.where(E > 0, E, 1.0), 0.0, 1.0), 1.0)
        sbar = np.where(E > 0, (dh * np.linalg.norm(c, axis=1) + 2.0 * (n + 2) * E64 * np.sum(np.abs(h) * np.abs(c), axis=1)) / np.where(E > 0, E, 1.0), 0.0) + U * share
    share[ref], sbar[ref] = 1.0, 0.0
    chi, bar = M.caf_from_y(yc.real, yc.imag, seg, kind)
    sc = M.scale_of(seg, nd, kind)
    bar = bar + sc * np.einsum("k,rkt->rt", w, dh[:, None, None] * gsum[None] + 4.0 * (n + 2) * E64 * terms)[:, None, :]
    status = np.full(nrows, 0 if ok else STATUS_SINGULAR, dtype=np.float64)
    status[ref] = 0.0
    return dict(chi=chi, bar=bar, h=h, hbar=hbar, share=share, sbar=sbar, status=status, cond=cond, y=y, yc=yc, terms=terms, G=G, A=A, c=c, E=E)


def time_domain(matrices, seg, nlags, ref, taps, dopp, h):
    """ECA the long way: X' = X_c - sum h_(m,p) phi_p[k(n)] X_r[n - m] in complex128, then the range stage on it.  -> y' [nrows][nd][R]"""
    F = len(matrices)
    nrows, B = np.asarray(matrices[0]).shape
    L, J = B // 2, B // 2 // seg
    nd = F * J
    phi = phases(nd, dopp)
    out = np.zeros((nrows, nd, nlags), dtype=np.complex128)
    for t, mt in enumerate(matrices):
        I, Q = M.parts(mt)
        X = I.astype(np.float64) + 1j * Q.astype(np.float64)
        xr = X[ref]
        k = t * J + np.arange(L) // seg
        Xc = X.copy()
        for j in range(basis(taps, dopp)):
            m, p = j % taps, j // taps
            d = np.concatenate([np.zeros(m), xr[:L - m]])
            Xc -= h[:, j][:, None] * (phi[p][k] * d)[None, :]
        for tau in range(nlags):
            d = np.conj(np.concatenate([np.zeros(tau), xr[:L - tau]]))
            out[:, t * J:(t + 1) * J, tau] = (Xc * d[None, :]).reshape(nrows, J, seg).sum(axis=2)
    return out


# ---- scenes ----
def clutter_scene(seed, seg=64, nd=64, paths=((0, 0, 0.8), (1, 0, 0.3), (3, 0, 0.1)), echo=(20, 5, 0.01), thermal=2.0, rms=30.0, nrows=2, ref=0, per_segment=False,
                  frames=1):
    """a line of `frames` int8 matrices [nrows][B], B = 2 seg nd / frames.  Row ref: complex white noise at `rms` LSB rms, one stream.
    Every other row: per path (lag, bin, a) a * the reference delayed by lag samples and rotated by `bin` cycles per line, the echo
    likewise, plus thermal noise of `thermal` LSB rms; rounded and clipped to int8, nothing rescaled.  per_segment: the rotation is
    constant within a segment."""
    rng = np.random.default_rng(seed)
    N = seg * nd
    hist = 64
    cn = lambda n: (rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2.0)
    s = rms * cn(N + hist)
    nn = np.arange(N)
    rot = lambda b: np.exp(2j * np.pi * b * ((nn // seg) * seg if per_segment else nn) / N)
    rows = []
    for c in range(nrows):
        if c == ref:
            rows.append(s[hist:])
            continue
        x = thermal * cn(N)
        for lag, b, a in list(paths) + [echo]:
            x = x + a * s[hist - lag:hist - lag + N] * rot(b)
        rows.append(x)
    q = np.zeros((nrows, 2 * N), dtype=np.int8)
    for c, x in enumerate(rows):
        q[c, 0::2], q[c, 1::2] = np.clip(np.rint(x.real), -128, 127), np.clip(np.rint(x.imag), -128, 127)
    Bp = 2 * N // frames
    return [np.ascontiguousarray(q[:, t * Bp:(t + 1) * Bp]) for t in range(frames)]


DOPPLER_PATHS = ((0, 0, 0.8), (2, 1, 0.3), (4, -1, 0.2))


def over_mean_db(P, d, tau):
    return float(10.0 * np.log10(P[d, tau] / P.mean()))
