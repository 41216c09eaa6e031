"""fp64 numpy statement of crsdr_caf's second cancellation stage (include/crsdr.h, section (w), "Cleaning"; crsdr_caf_set_clean and
crsdr_ambiguity_clean), on top of caf_cancel_model.py, and the error bars of the device against it.

Definition.  y, G, k, nd, Ls, R, r, K = taps, P = dopp, n1 = K (2 P + 1) are caf_cancel_model.py's.  T = max_targets, wl, wq, min_snr.

Picks, from the array map's published list det [Kdet][8] float32 and its count, in fp64 on those figures (so exact): the first
min(count, Kdet) records in order, f = doppler + ddop, l = lag; skipped if snr < min_snr, if l - wl <= K - 1 and circ(f) < P + 1 + wq / 2,
or if |l - l'| <= 2 wl and circ(f - f') < wq + 1 for an accepted pick; circ(a) = |a|, or nd - |a| when |a| > nd / 2.  At most T.

Members: the canceller's n1 first; per pick, q = -wq .. wq outer, j = -wl .. wl inner, (m, g) = (l + j, f + q / 2), lags outside
0 .. R - 1 left out.  phi_g[k] = exp(2 pi i ((g k) / nd)), the product and the quotient rounded as fp64 rounds them.

    A_ij = sum_k phi_(g_j - g_i)[k] G[k][m_j][m_i]        c_i = sum_k conj(phi_(g_i)[k]) y_c[k][m_i]
    Cholesky by columns, pivot floor 2^-40 A_00: status 1 if a pivot of the first n1 fails (h = 0), 2 if a later one does (target h = 0,
    the canceller's h is stage 1's); either way the residual is stage 1's chi
    y''_c[k][tau] = y_c[k][tau] - sum_i h_i phi_(g_i)[k] G[k][m_i][tau]

and rchi is caf_model.caf_from_y of y''.

Error bars.  caf_cancel_model.py's derivation with n members in the place of its n, and a phase within 4 e of phi in the place of 2 e
(the argument (g k) / nd is formed with one rounding of the product, which the model shares bit for bit; sincospi and the model's
exp each add under 2 e): each entry of A and c is within 2 (nd + 8) e of the sum of the magnitudes of its terms, and

    ||h^ - h||_2 <= ||A^-1||_2 ((4 n (3 n + 1) e ||A||_2 + 2 (nd + 8) e ||Aabs||_F) ||h||_2 + 2 (nd + 8) e ||cabs||_2)  =: dh
    bar_coef = dh + u |h_j|
    bar_rchi[tau] = u (7 log2 nd + 2) scale ||w o y''_c[:, tau]||_2 + scale sum_k w[k] (dh sum_i |G[k][m_i][tau]| + 4 (n + 2) e T_c[k][tau])
    |d share| <= (dh ||c||_2 + 2 (n + 2) e sum |h| |c|) / E + u share

cond(A) enters through ||A^-1||_2 ||A||_2.  The bars stay some 10^-9 of ||h|| while cond(A) <= COND_MAX = 4096, which every scene's
test asserts: neighbouring lags and half-bin Dopplers of one pick are strongly correlated columns, so the joint matrix is far less
well conditioned than the canceller's own (whose scenes hold 16), and 4096 still leaves the bar five decades under fp32's rounding.
"""
import numpy as np

import caf_cancel_model as X
import caf_cfar_model as C
import caf_model as M
from caf_model import E64, U

MUTATIONS = ["integer_f", "phi_sign", "g_transposed", "cross_dropped", "doppler_not_wrapped", "lag_wrapped", "min_snr_ignored", "fp32_subtract", "touch_ignored"]
STATUS_SINGULAR, STATUS_TARGET = 1, 2
COND_MAX = 4096.0
LAUNCHES = 9


class Params:
    def __init__(self, max_targets=1, min_snr=100.0, wl=1, wq=1):
        self.T, self.wl, self.wq = int(max_targets), int(wl), int(wq)
        self.min_snr = np.float32(min_snr)                                       # what the device is handed

    @property
    def per(self):
        return (2 * self.wl + 1) * (2 * self.wq + 1)


def bad_limit(nd, R, lines, nrows, taps, dopp, prm):
    """the number of the limit that fails (0: none), as csrc/caf_clean_solve.hpp counts them"""
    if not 1 <= prm.T <= 8:
        return 1
    if not 0 <= prm.wl <= 2:
        return 2
    if not 0 <= prm.wq <= 2:
        return 3
    if X.basis(taps, dopp) + prm.T * prm.per > 64:
        return 4
    if not (np.isfinite(prm.min_snr) and prm.min_snr > 0):
        return 5
    if lines * nd * (taps + prm.T * (2 * prm.wl + 1)) * R > 2 ** 24:
        return 6
    if 2 * lines * nrows * nd * R > 2 ** 24:
        return 7
    return 0


def circular(a, nd):
    g = abs(a)
    return nd - g if g > nd / 2 else g


def _lf(rec, which=None):
    f = float(rec[1]) if which == "integer_f" else float(rec[1]) + float(rec[6])
    return int(rec[0]), f


def pick_walk(det, count, nd, taps, dopp, prm, which=None):
    """the indices of the accepted records of det [Kdet][8] (float32 as published), in their order"""
    det = np.asarray(det, dtype=np.float32)
    dist = (lambda a: abs(a)) if which == "doppler_not_wrapped" else (lambda a: circular(a, nd))
    picked = []
    for i in range(min(int(count), det.shape[0])):
        if len(picked) == prm.T:
            break
        l, f = _lf(det[i], which)
        if which != "min_snr_ignored" and float(det[i][3]) < float(prm.min_snr):
            continue
        if l - prm.wl <= taps - 1 and dist(f) < dopp + 1 + prm.wq / 2:
            continue
        if which != "touch_ignored" and any(abs(l - _lf(det[t], which)[0]) <= 2 * prm.wl and dist(f - _lf(det[t], which)[1]) < prm.wq + 1 for t in picked):
            continue
        picked.append(i)
    return picked


def target_members(det, picked, R, prm, which=None):
    """[(lag, g, owner, pos)] in member order"""
    out = []
    for o, i in enumerate(picked):
        l, f = _lf(np.asarray(det, dtype=np.float32)[i], which)
        for q in range(-prm.wq, prm.wq + 1):
            for j in range(-prm.wl, prm.wl + 1):
                m = l + j
                if not 0 <= m < R:
                    if which != "lag_wrapped":
                        continue
                    m %= R
                out.append((m, f + 0.5 * q, o, (q + prm.wq) * (2 * prm.wl + 1) + (j + prm.wl)))
    return out


def phase(g, nd):
    """phi_g [nd]: the argument as fp64 forms it, reduced to one turn exactly"""
    x = (np.float64(g) * np.arange(nd, dtype=np.float64)) / np.float64(nd)
    return np.exp(2j * np.pi * np.mod(x, 1.0))


def chol_columns(A):
    """(L, status): the factor by columns under the pivot rule; status None while every pivot holds, else the failing column"""
    n = A.shape[0]
    floor_ = A[0, 0].real * 2.0 ** -40
    L = np.zeros_like(A)
    for k in range(n):
        d = A[k, k].real - np.sum(np.abs(L[k, :k]) ** 2)
        if not d > floor_:
            return L, k
        L[k, k] = np.sqrt(d)
        L[k + 1:, k] = (A[k + 1:, k] - L[k + 1:, :k] @ np.conj(L[k, :k])) / L[k, k]
    return L, None


def joint_equations(y, Gf, lags, gs, n1, which=None):
    """(A [n][n], c [nrows][n], Aabs, cabs) from y [nrows][nd][R] and Gf [nd][R][R] over the members (lags[i], gs[i])"""
    nd = Gf.shape[0]
    n = len(lags)
    A, Aabs = np.zeros((n, n), dtype=np.complex128), np.zeros((n, n))
    for i in range(n):
        for j in range(n):
            g = Gf[:, lags[i], lags[j]] if which == "g_transposed" and max(i, j) >= n1 else Gf[:, lags[j], lags[i]]
            A[i, j] = np.sum(phase(gs[j] - gs[i], nd) * g)
            Aabs[i, j] = np.sum(np.abs(g))
    if which == "cross_dropped":
        A[n1:, :n1] = 0.0
        A[:n1, n1:] = 0.0
    c = np.zeros((y.shape[0], n), dtype=np.complex128)
    cabs = np.zeros((y.shape[0], n))
    for i in range(n):
        f = phase(gs[i], nd)
        if not (which == "phi_sign" and i >= n1):
            f = np.conj(f)
        c[:, i] = y[:, :, lags[i]] @ f
        cabs[:, i] = np.abs(y[:, :, lags[i]]).sum(axis=1)
    return A, c, Aabs, cabs


def full_ref_sums(matrices, seg, nlags, ref):
    """G [nd][R][R]: every lag m < R"""
    return X.ref_sums(matrices, seg, nlags, ref, nlags)


def clean(matrices, seg, nlags, ref, kind, taps, dopp, det, count, prm, which=None):
    """one line (a list of `frames` int8 matrices) and its array map's published list -> dict: picked, tgt [T][8] float32, ntgt; members;
    h [nrows][n] and hbar; tcoef [nrows][T][per] and tbar; share, sbar; status [nrows]; cond; rchi [nrows][nd][R] complex128 and rbar
    [nrows][1][R]; A, c, L; stage1 (caf_cancel_model.cancel's dict).  which: one of MUTATIONS"""
    det = np.asarray(det, dtype=np.float32)
    s1 = X.cancel(matrices, seg, nlags, ref, kind, taps, dopp)
    y, E = s1["y"], s1["E"]
    nrows, nd, R = y.shape
    K, P, n1 = taps, dopp, X.basis(taps, dopp)
    picked = pick_walk(det, count, nd, K, P, prm, which)
    tm = target_members(det, picked, R, prm, which)
    tgt = np.zeros((prm.T, 8), dtype=np.float32)
    tgt[:len(picked)] = det[picked]
    lags = [j % K for j in range(n1)] + [m[0] for m in tm]
    gs = [float(j // K - P) for j in range(n1)] + [m[1] for m in tm]
    n = len(lags)
    Gf = full_ref_sums(matrices, seg, nlags, ref)
    A, c, Aabs, cabs = joint_equations(y, Gf, lags, gs, n1, which)
    L, failed = chol_columns(A)
    st = 0 if failed is None else (STATUS_SINGULAR if failed < n1 else STATUS_TARGET)
    h = np.zeros((nrows, n), dtype=np.complex128)
    cond, inv_norm = np.inf, np.inf
    used = n
    if st == 0:
        sv = np.linalg.svd(A, compute_uv=False)
        cond, inv_norm = float(sv[0] / sv[-1]), float(1.0 / sv[-1])
        # (a line without picks has stage 1's equations: it takes stage 1's route, and so its values exactly)
        h = np.linalg.solve(A, c.T).T if tm else s1["h"].copy()
    elif st == STATUS_TARGET:
        h[:, :n1] = s1["h"]
        used = n1
    h[ref] = 0.0
    hn = np.linalg.norm(h, axis=1)
    if st == 0:
        a2 = float(np.linalg.norm(A, 2))
        dh = inv_norm * ((4.0 * n * (3 * n + 1) * E64 * a2 + 2.0 * (nd + 8) * E64 * np.linalg.norm(Aabs)) * hn + 2.0 * (nd + 8) * E64 * np.linalg.norm(cabs, axis=1))
        dh[ref] = 0.0
    else:
        dh = np.zeros(nrows)
    hbar = dh[:, None] + U * np.abs(h)
    tcoef, tbar = np.zeros((nrows, prm.T, prm.per), dtype=np.complex128), np.zeros((nrows, prm.T, prm.per))
    for i, (_, _, o, pos) in enumerate(tm):
        tcoef[:, o, pos], tbar[:, o, pos] = h[:, n1 + i], hbar[:, n1 + i]
    with np.errstate(divide="ignore", invalid="ignore"):
        Es = np.where(E > 0, E, 1.0)
        share = np.where(E > 0, np.clip((E - np.sum(np.conj(h[:, :used]) * c[:, :used], axis=1).real) / Es, 0.0, 1.0), 1.0)
        sbar = np.where(E > 0, (dh * np.linalg.norm(c, axis=1) + 2.0 * (n + 2) * E64 * np.sum(np.abs(h) * np.abs(c), axis=1)) / Es, 0.0) + U * share
    if st == STATUS_TARGET:
        sbar = s1["sbar"].copy()
    share[ref], sbar[ref] = 1.0, 0.0
    status = np.full(nrows, float(st))
    status[ref] = 0.0
    out = dict(picked=picked, tgt=tgt, ntgt=len(picked), members=tm, lags=lags, gs=gs, h=h, hbar=hbar, tcoef=tcoef, tbar=tbar, share=share, sbar=sbar, status=status,
               cond=cond, A=A, c=c, L=L, stage1=s1, n1=n1)
    if st != 0 or not tm:
        out.update(rchi=s1["chi"], rbar=s1["bar"], yres=s1["yc"])
        if st == 0:
            out.update(share=s1["share"], sbar=s1["sbar"], hbar=s1["hbar"])
        return out
    F = np.stack([phase(gs[i], nd)[:, None] * Gf[:, lags[i], :] for i in range(n)])  # [n][nd][R]
    if which == "fp32_subtract":
        acc = y.astype(np.complex64)
        for i in range(n):
            acc = (acc - (h[:, i].astype(np.complex64)[:, None, None] * F[i].astype(np.complex64)[None])).astype(np.complex64)
        yres = acc.astype(np.complex128)
    else:
        yres = y - np.einsum("ri,ikt->rkt", h, F)
    terms = np.abs(y) + np.einsum("ri,ikt->rkt", np.abs(h), np.abs(F))
    gsum = np.sum(np.abs(F), axis=0)
    rchi, rbar = M.caf_from_y(yres.real, yres.imag, seg, kind)
    w, sc = M.window(nd, kind), M.scale_of(seg, nd, kind)
    rbar = rbar + sc * np.einsum("k,rkt->rt", w, dh[:, None, None] * gsum[None] + 4.0 * (n + 2) * E64 * terms)[:, None, :]
    out.update(rchi=rchi, rbar=rbar, yres=yres)
    return out


def time_domain(matrices, seg, nlags, ref, lags, gs, h):
    """the joint cancellation the long way: X' = X_c - sum_i h_i phi_(g_i)[k(n)] X_r[n - m_i] in complex128, then the range stage on it.
    -> y'' [nrows][nd][R]"""
    F = len(matrices)
    nrows, B = np.asarray(matrices[0]).shape
    L, J = B // 2, B // 2 // seg
    nd = F * J
    out = np.zeros((nrows, nd, nlags), dtype=np.complex128)
    phis = [phase(g, nd) for g in gs]
    for t, mt in enumerate(matrices):
        I, Q = M.parts(mt)
        Xs = I.astype(np.float64) + 1j * Q.astype(np.float64)
        xr = Xs[ref]
        k = t * J + np.arange(L) // seg
        Xc = Xs.copy()
        for i, m in enumerate(lags):
            d = np.concatenate([np.zeros(m), xr[:L - m]])
            Xc -= h[:, i][:, None] * (phis[i][k] * d)[None, :]
        for tau in range(nlags):
            d = np.conj(np.concatenate([np.zeros(tau), xr[:L - tau]]))
            out[:, t * J:(t + 1) * J, tau] = (Xc * d[None, :]).reshape(nrows, J, seg).sum(axis=2)
    return out


def array_list(chi, ref, guard, cprm):
    """(map fp32, caf_cfar_model.detect's dict on it) of chi [nrows][nd][R]: the array map's list as the device would publish it from
    this chi (rounded to fp32 first, as it is published)"""
    chi32 = np.asarray(chi).astype(np.complex64)
    mp = M.array_map(chi32, ref)[0].astype(np.float32)
    return mp, C.detect(mp.astype(np.float64), guard, cprm)


# ---- the masking scene ----
# nrows 3, seg 32, nd 32, R 16.  The reference is white noise at 30 LSB rms.  Every other row: the direct path (lag 0, a 0.8), a strong
# mover (lag 6, 4.3 bins, a 0.6, its phase constant within a segment as the basis has it) and a weak echo (lag 11, -9 bins, a 0.04)
# over thermal noise of 1 LSB rms.  The mover's floor, 1 / (nd Ls) = -30 dB under its peak, lies 7 dB over the echo's peak / alpha.
MASK = dict(seg=32, nd=32, R=16, nrows=3, ref=0, taps=2, dopp=0, strong=(6, 4.3, 0.6), weak=(11, -9, 0.04))


def masking_scene(seed=0, strong=MASK["strong"], weak=MASK["weak"]):
    return X.clutter_scene(seed, seg=MASK["seg"], nd=MASK["nd"], paths=((0, 0, 0.8), strong), echo=weak, thermal=1.0, nrows=MASK["nrows"], ref=MASK["ref"],
                           per_segment=True)


def masking_detector():
    """the full window is 9 x 7 - 3 x 3 = 54 cells; 10^-6 per cell on one row's map, a little less on the array map of two rows"""
    return C.Params(C.cfar_alpha(1e-6, 54), gd=1, gr=1, td=3, tr=2, min_train=20, max_det=8)
