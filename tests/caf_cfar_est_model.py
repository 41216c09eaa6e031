"""fp64 numpy statement of the greatest-of, smallest-of and ordered-statistic CFAR estimators of crsdr_caf (include/crsdr.h, section
(w), "Estimators"; crsdr_caf_set_cfar_estimator, crsdr_cfar_est, crsdr_cfar_alpha_est), and the error bars of the device against it.
caf_cfar_model.py is imported and left as it is: P, S, guard, the training set, N, the 3 x 3 test, the order of the detections and the
eight figures are its own.  Only noise and ntrain change with the estimator.

Definition.  Nfull = (2 Hd + 1)(2 Hr + 1) - (2 gd + 1)(2 gr + 1).  A detected cell needs a noise estimate with noise > 0, P > t with
t = fp64(alpha) * noise, and the neighbourhood test.
    CA (0)   caf_cfar_model.detect.
    GO (1), SO (2)   axis 0 (lag) splits the training set into the cells with b < 0 and those with b > 0, axis 1 (Doppler) into a < 0 and
             a > 0; the centre line (b = 0, or a = 0) trains neither half.  A half counts iff its size N_h >= min_train; its mean is
             Z_h / N_h, Z_h by additions only.  noise is the larger (GO) or smaller (SO) mean over the halves that count, the lower half
             on equal means; ntrain is that half's N_h.  No counting half, or noise not above 0: no detection.
    OS (3)   1 <= rank <= Nfull.  With N >= min_train, k = max(1, ceil(rank N / Nfull)) in integers and noise is the k-th smallest P of
             the training set; ntrain = N.  A cell outside the lags or outside S is absent, not a zero; a cell of S with P = 0 is present.

Error bars (u = 2^-24, e = 2^-53), derived and not measured.
    OS       noise is a value of the map: the same bits on both sides, and t one fp64 product of the same two numbers.  Nothing is
             ambiguous; power, snr and noise carry their single fp32 roundings alone, so the device's figures equal fp32(model's).
    GO, SO   Z_h as caf_cfar_model's Z: two orders of the same N_h non-negative terms are within 2 (N_h - 1) e of each other, so a
             half's mean carries mean (N_h e).  max and min are 1-Lipschitz: noise keeps the bar noise (u + N_h e), and the rule
             |P - t| <= 2^-40 t marks the AMBIGUOUS cells.  In addition a cell whose two counting halves have different sizes and means
             within 2^-40 of each other, relatively, is HALF-AMBIGUOUS: the other half, and so another ntrain, could be chosen.
Tests assert that their inputs have none of either kind; the rule is never used to leave a detection out.

cfar_alpha_est is the exact false-alarm equation under exponential noise (Gandhi and Kassam, Analysis of CFAR processors in
nonhomogeneous background, IEEE Trans. AES 24 (1988); Rohling, Radar CFAR thresholding in clutter and multiple target situations, IEEE
Trans. AES 19 (1983)), solved by bisection in fp64 and rounded once to fp32:
    SO   2 (2 + T)^-n sum_{i < n} C(n - 1 + i, i) (2 + T)^-i,  T = alpha / n, n the cells of a half
    GO   2 (1 + T)^-n - P_SO
    OS   prod_{i < rank} (N - i) / (N - i + alpha)
"""
import math

import numpy as np

import caf_cfar_model as C
import caf_model as M

U, E64 = M.U, M.E64
AMBIGUOUS = C.AMBIGUOUS
CA, GO, SO, OS = 0, 1, 2, 3
LAG, DOPPLER = 0, 1
MUTATIONS = ["absent_as_zero", "rank_unscaled", "rank_off_by_one", "centre_trains", "go_so_exchanged", "small_half_counts", "ge"]


class Est:
    def __init__(self, est=CA, axis=LAG, rank=0):
        self.est, self.axis, self.rank = int(est), int(axis), int(rank)


def full_count(prm):
    return (2 * prm.Hd + 1) * (2 * prm.Hr + 1) - (2 * prm.gd + 1) * (2 * prm.gr + 1)


def os_rank(rank, N, Nfull):
    return max(1, -((-rank * N) // Nfull))


def _offsets(prm):
    return [(a, b) for a in range(-prm.Hd, prm.Hd + 1) for b in range(-prm.Hr, prm.Hr + 1) if not (abs(a) <= prm.gd and abs(b) <= prm.gr)]


def _side(a, b, axis, which=None):
    v = b if axis == LAG else a
    if v == 0:
        return -1 if which == "centre_trains" else 0
    return -1 if v < 0 else 1


def half_sums(P, guard, prm, axis, which=None):
    """(Zlo, Nlo, Zhi, Nhi) [nd][R] of every cell, by sums of shifted copies: additions only"""
    P = np.asarray(P, dtype=np.float64)
    nd, R = P.shape
    ok = M.in_set(nd, guard)
    Pm = np.where(ok[:, None], P, 0.0)
    Im = np.broadcast_to(ok[:, None], P.shape).astype(np.int64)
    Z = {-1: np.zeros_like(P), 1: np.zeros_like(P)}
    N = {-1: np.zeros(P.shape, dtype=np.int64), 1: np.zeros(P.shape, dtype=np.int64)}
    for a, b in _offsets(prm):
        s = _side(a, b, axis, which)
        if s == 0:
            continue
        Z[s] += C._shifted(Pm, a, b, prm.Hr, None)
        N[s] += C._shifted(Im, a, b, prm.Hr, None)
    return Z[-1], N[-1], Z[1], N[1]


def half_cell(P, guard, prm, axis, d, tau):
    """((Zlo, Nlo), (Zhi, Nhi)) of ONE cell by the letter: caf_cfar_model.train_cell's cells, each given to its half"""
    nd, R = P.shape
    cells = set(C.train_cell(P, guard, prm, d, tau)[2])
    out = {-1: [0.0, 0], 1: [0.0, 0]}
    for a in range(-prm.Hd, prm.Hd + 1):
        for b in range(-prm.Hr, prm.Hr + 1):
            dq, tq = (d + a) % nd, tau + b
            if abs(a) <= prm.gd and abs(b) <= prm.gr:
                continue
            s = _side(a, b, axis)
            if s == 0 or (dq, tq) not in cells or tq < 0 or tq >= R:
                continue
            out[s][0] += float(P[dq, tq])
            out[s][1] += 1
    return tuple(out[-1]), tuple(out[1])


def os_cell(P, guard, prm, rank, d, tau):
    """(x_(k), N, k) of ONE cell by the letter: the training cells' values sorted"""
    _, n, cells = C.train_cell(P, guard, prm, d, tau)
    if n == 0:
        return 0.0, 0, 0
    k = os_rank(rank, n, full_count(prm))
    return sorted(float(P[c]) for c in cells)[k - 1], n, k


def os_values(P, guard, prm, rank, which=None):
    """(noise [nd][R], N [nd][R]) of every cell: the shifted copies stacked, absent cells at +inf, sorted along the stack"""
    P = np.asarray(P, dtype=np.float64)
    nd, R = P.shape
    ok = M.in_set(nd, guard)
    absent = 0.0 if which == "absent_as_zero" else np.inf
    Pm = np.where(ok[:, None], P, np.inf)
    Im = np.broadcast_to(ok[:, None], P.shape).astype(np.int64)
    offs = _offsets(prm)
    stack = np.empty((len(offs), nd, R))
    N = np.zeros(P.shape, dtype=np.int64)
    for j, (a, b) in enumerate(offs):
        Y = np.roll(Pm, -a, axis=0)
        pad = np.full((nd, prm.Hr), np.inf)
        stack[j] = np.concatenate([pad, Y, pad], axis=1)[:, prm.Hr + b:prm.Hr + b + R]
        N += C._shifted(Im, a, b, prm.Hr, None)
    if which == "absent_as_zero":
        stack = np.where(np.isinf(stack), absent, stack)
        Nuse = np.full(P.shape, len(offs), dtype=np.int64)
    else:
        Nuse = N
    stack.sort(axis=0)
    Nfull = full_count(prm)
    if which == "rank_unscaled":
        k = np.minimum(rank, np.maximum(Nuse, 1))
    else:
        k = np.maximum(1, -((-rank * Nuse) // Nfull))
    if which == "rank_off_by_one":
        k = np.maximum(1, k - 1)
    k = np.minimum(k, len(offs))
    noise = np.take_along_axis(stack, (k - 1)[None], axis=0)[0]
    return np.where(N >= 1, noise, 0.0), N


def estimate(P, guard, prm, est, which=None):
    """(live [nd][R] bool, noise, ntrain, half_ambiguous [nd][R] bool): the estimate of every cell"""
    P = np.asarray(P, dtype=np.float64)
    nd, R = P.shape
    inS = M.in_set(nd, guard)[:, None]
    none = np.zeros(P.shape, dtype=bool)
    if est.est == OS:
        noise, N = os_values(P, guard, prm, est.rank, which)
        noise = np.where(np.isfinite(noise), noise, 0.0)
        return inS & (N >= prm.min_train) & (N >= 1) & (noise > 0.0), noise, N, none
    zlo, nlo, zhi, nhi = half_sums(P, guard, prm, est.axis, which)
    floor = 1 if which == "small_half_counts" else prm.min_train
    lo, hi = (nlo >= floor) & (nlo >= 1), (nhi >= floor) & (nhi >= 1)
    mlo, mhi = zlo / np.maximum(nlo, 1), zhi / np.maximum(nhi, 1)
    go = (est.est == GO) != (which == "go_so_exchanged")
    upper = ~lo | (hi & ((mhi > mlo) if go else (mhi < mlo)))
    noise = np.where(upper, mhi, mlo)
    n = np.where(upper, nhi, nlo)
    live = inS & (lo | hi) & (noise > 0.0)
    hamb = inS & lo & hi & (nlo != nhi) & (np.abs(mhi - mlo) <= AMBIGUOUS * np.maximum(mhi, mlo)) & (np.maximum(mhi, mlo) > 0.0)
    return live, np.where(lo | hi, noise, 0.0), np.where(lo | hi, n, 0), hamb


def detect(P, guard, prm, est, which=None):
    """caf_cfar_model.detect's dict under the estimator est, with half_ambiguous beside ambiguous.  CA goes through the same code below,
    on caf_cfar_model's own sums"""
    P = np.asarray(P, dtype=np.float64)
    nd, R = P.shape
    if est is None or est.est == CA:
        _, noise, N, _ = C.threshold(P, guard, prm)
        Z, _ = C.train_sums(P, guard, prm)
        live, hamb = M.in_set(nd, guard)[:, None] & (N >= prm.min_train) & (Z > 0.0), np.zeros(P.shape, dtype=bool)
    else:
        live, noise, N, hamb = estimate(P, guard, prm, est, which)
    t = np.float64(prm.alpha) * noise
    passed = live & ((P >= t) if which == "ge" else (P > t))
    amb = live & (np.abs(P - t) <= AMBIGUOUS * t) if (est is None or est.est != OS) else np.zeros(P.shape, dtype=bool)
    found = [(d, tau) for d, tau in zip(*np.nonzero(passed)) if C._local_max(P, guard, int(d), int(tau))]
    found.sort(key=lambda c: (-P[c], c[0] * R + c[1]))
    K = prm.max_det
    det, bar = np.zeros((K, 8)), np.zeros((K, 8))
    ok, s = M.in_set(nd, guard), M.signed_bins(nd)
    exact = est is not None and est.est == OS
    for k, (d, tau) in enumerate(found[:K]):
        p, nz, n = P[d, tau], noise[d, tau], int(N[d, tau])
        dlag, blag = M._vertex(P[d, tau - 1], p, P[d, tau + 1]) if 0 < tau < R - 1 else (0.0, 0.0)
        dm, dp = (d - 1) % nd, (d + 1) % nd
        ddop, bdop = M._vertex(P[dm, tau], p, P[dp, tau]) if ok[dm] and ok[dp] else (0.0, 0.0)
        snr = p / nz
        det[k] = [tau, s[d], p, snr, nz, dlag, ddop, n]
        bar[k] = [0.0, 0.0, U * p, snr * (U + (0 if exact else n + 2) * E64), nz * (U + (0 if exact else n) * E64), blag, bdop, 0.0]
    return dict(count=len(found), cells=[int(d) * R + int(tau) for d, tau in found], det=det, bar=bar, passed=int(passed.sum()), ambiguous=int(amb.sum()),
                half_ambiguous=int(hamb.sum()))


def pfa(est, n, rank, alpha):
    """the false-alarm probability of a cell under exponential noise at threshold factor alpha"""
    if est == CA:
        return (1.0 + alpha / n) ** -n
    if est == OS:
        p = 1.0
        for i in range(rank):
            p *= (n - i) / (n - i + alpha)
        return p
    T = alpha / n
    lx = -math.log(2.0 + T)
    so, lc = 0.0, 0.0
    for i in range(n):
        if i:
            lc += math.log((n - 1 + i) / i)
        so += math.exp(lc + (n + i) * lx)
    so *= 2.0
    return so if est == SO else 2.0 * math.exp(-n * math.log(1.0 + T)) - so


def cfar_alpha_est(p, ntrain, est):
    """crsdr_cfar_alpha_est: a bracket by doubling, bisection down to neighbouring doubles, one rounding to fp32"""
    if est is None or est.est == CA:
        return C.cfar_alpha(p, ntrain)
    lo, hi = 0.0, 1.0
    while pfa(est.est, ntrain, est.rank, hi) > p and hi < 1e300:
        hi *= 2.0
    for _ in range(2200):
        mid = 0.5 * (lo + hi)
        if not (lo < mid < hi):
            break
        if pfa(est.est, ntrain, est.rank, mid) > p:
            lo = mid
        else:
            hi = mid
    return np.float32(hi)
