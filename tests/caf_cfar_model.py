"""fp64 numpy statement of the cell-averaging CFAR detector of crsdr_caf (include/crsdr.h, section (w), "Detections"; crsdr_caf_set_cfar,
crsdr_cfar), and the error bars of the device against it.  caf_model.py is imported and left as it is: the map P, the signed bin s(d),
the searched set S = {(d, tau): |s(d)| >= guard}, the linear index i = d R + tau and the parabola are its own.

Definition.  P [nd][R] is a published array map, or re re + im im of a row's published fp32 chi in fp64 (caf_model.power).  Guard
half-widths gd, gr over Doppler and lag, training half-widths td, tr beyond them, Hd = gd + td, Hr = gr + tr.  The training set of a
cell (d, tau) of S is the set of cells (d + a mod nd, tau + b) with

    |a| <= Hd and |b| <= Hr;    NOT (|a| <= gd and |b| <= gr);    0 <= tau + b < R;    the Doppler bin in S.

Doppler wraps, lag does not, and the ridge that guard cuts out of the search trains nothing.  N is the set's size, Z the sum of P over
it.  The cell is detected if and only if

    N >= min_train;    Z > 0;    P > t,  noise = Z / N,  t = fp64(alpha) * noise;
    P beats its 3 x 3 neighbours: Doppler wraps, neighbours outside the lags or outside S do not count, and against a neighbour q the
    test is P > P_q, or P == P_q with i < i_q.

count is the number of detected cells; det holds the K = max_det of largest P, ties by smaller i, in that order, each as
(lag, doppler = s(d), power = P, snr = P / noise, noise, dlag, ddop, ntrain = N) with dlag, ddop as in caf_model.peaks, zeros behind them.

Here Z is a sum of shifted copies of the masked, zero-padded map, one per window offset: additions only, as on the device.

Error bars, derived and not measured (u = 2^-24, e = 2^-53).  P is the same three IEEE operations on both sides: exact.  N is an integer.
    Z        a sum of N <= (2 Hd + 1)(2 Hr + 1) non-negative fp64 terms: in any order it is within (N - 1) e of the exact sum, relatively
             (Higham, Accuracy and Stability of Numerical Algorithms, (4.4), every term of one sign: the condition number is 1), so two
             orders are within 2 (N - 1) e of each other to first order.  This needs every order to be a sum of the terms themselves: a
             window sum less a guard-block sum carries the rounding error of the cancelled cells, a target's among them, and has no such
             bound -- the device adds row sums and never subtracts.
    noise    one division more: noise (N e) against the model's own, and one rounding to fp32: noise (u + N e)
    t        one multiplication more: t (N + 1) e < 2^-43 t at N <= 561.  A cell with |P - t| <= 2^-40 t -- more than eight times that --
             is AMBIGUOUS: the only kind of cell on which device and model may disagree about the threshold.  Everything else in the
             decision is exact on both sides (comparisons of the same fp64 P, integers), so away from ambiguous cells the detection set,
             its order and count are equal.
    lag, doppler, ntrain    0
    power    u P                          (the one fp32 rounding)
    snr      snr (u + (N + 2) e)          (noise's N e, the division, the rounding)
    dlag, ddop   caf_model._vertex's bar
"""
import numpy as np

import caf_model as M

U, E64 = M.U, M.E64
AMBIGUOUS = 2.0 ** -40
MUTATIONS = ["guard_trains", "ridge_counts", "lag_wrap", "doppler_nowrap", "ge", "tie_reversed", "full_window_mean"]


class Params:
    def __init__(self, alpha, gd=1, gr=1, td=3, tr=4, min_train=1, max_det=16):
        self.gd, self.gr, self.td, self.tr, self.min_train, self.max_det = int(gd), int(gr), int(td), int(tr), int(min_train), int(max_det)
        self.alpha = np.float32(alpha)                                           # what the device is handed

    @property
    def Hd(self):
        return self.gd + self.td

    @property
    def Hr(self):
        return self.gr + self.tr


def cfar_alpha(pfa, ntrain):
    """the cell-averaging factor of ONE row's map under exponential noise, as crsdr_cfar_alpha rounds it"""
    return np.float32(ntrain * (pfa ** (-1.0 / ntrain) - 1.0))


def _shifted(X, a, b, Hr, which):
    """Y[d][tau] = X[d + a mod nd][tau + b], 0 outside the lags (which: the two mistakes about the edges)"""
    nd, R = X.shape
    if which == "doppler_nowrap":
        Y = np.zeros_like(X)
        lo, hi = max(0, -a), min(nd, nd - a)
        Y[lo:hi] = X[lo + a:hi + a]
    else:
        Y = np.roll(X, -a, axis=0)
    if which == "lag_wrap":
        return np.roll(Y, -b, axis=1)
    pad = np.zeros((nd, Hr), dtype=X.dtype)
    return np.concatenate([pad, Y, pad], axis=1)[:, Hr + b:Hr + b + R]


def train_sums(P, guard, prm, which=None):
    """(Z [nd][R] fp64, N [nd][R] int) of every cell, by sums of shifted copies: additions only.  which: one of MUTATIONS"""
    P = np.asarray(P, dtype=np.float64)
    nd, R = P.shape
    ok = np.ones(nd, dtype=bool) if which == "ridge_counts" else M.in_set(nd, guard)
    Pm = np.where(ok[:, None], P, 0.0)
    Im = np.broadcast_to(ok[:, None], P.shape).astype(np.int64)
    Z, N = np.zeros_like(P), np.zeros(P.shape, dtype=np.int64)
    for a in range(-prm.Hd, prm.Hd + 1):
        for b in range(-prm.Hr, prm.Hr + 1):
            if abs(a) <= prm.gd and abs(b) <= prm.gr and not (which == "guard_trains" and (a, b) != (0, 0)):
                continue
            Z += _shifted(Pm, a, b, prm.Hr, which)
            N += _shifted(Im, a, b, prm.Hr, which)
    return Z, N


def train_cell(P, guard, prm, d, tau):
    """(Z, N, cells) of ONE cell by the letter of the definition: every (a, b) tried, every condition tested"""
    nd, R = P.shape
    s = M.signed_bins(nd)
    z, cells = 0.0, []
    for a in range(-prm.Hd, prm.Hd + 1):
        for b in range(-prm.Hr, prm.Hr + 1):
            if abs(a) <= prm.gd and abs(b) <= prm.gr:
                continue
            dq, tq = (d + a) % nd, tau + b
            if tq < 0 or tq >= R or abs(s[dq]) < guard:
                continue
            z += float(P[dq, tq])
            cells.append((dq, tq))
    return z, len(cells), cells


def threshold(P, guard, prm, which=None):
    """(passed [nd][R] bool, noise, N, ambiguous [nd][R] bool): the threshold stage alone"""
    P = np.asarray(P, dtype=np.float64)
    nd, R = P.shape
    Z, N = train_sums(P, guard, prm, which)
    live = M.in_set(nd, guard)[:, None] & (N >= prm.min_train) & (Z > 0.0)
    if which == "full_window_mean":
        div = np.full(P.shape, (2 * prm.Hd + 1) * (2 * prm.Hr + 1) - (2 * prm.gd + 1) * (2 * prm.gr + 1), dtype=np.float64)
    else:
        div = np.maximum(N, 1).astype(np.float64)
    noise = Z / div
    t = np.float64(prm.alpha) * noise
    passed = live & ((P >= t) if which == "ge" else (P > t))
    return passed, noise, N, live & (np.abs(P - t) <= AMBIGUOUS * t)


def _local_max(P, guard, d, tau, which=None):
    nd, R = P.shape
    ok = M.in_set(nd, guard)
    i = d * R + tau
    for a in (-1, 0, 1):
        dq = (d + a) % nd
        if not ok[dq]:
            continue
        for b in (-1, 0, 1):
            tq = tau + b
            if (a, b) == (0, 0) or tq < 0 or tq >= R:
                continue
            iq = dq * R + tq
            first = i > iq if which == "tie_reversed" else i < iq
            if not (P[d, tau] > P[dq, tq] or (P[d, tau] == P[dq, tq] and first)):
                return False
    return True


def detect(P, guard, prm, which=None):
    """dict of: count; cells, every detection's linear index in the order of det; det [K][8] fp64 and bar [K][8]; passed, the number of
    cells the threshold alone let through; ambiguous, the number of cells too near the threshold to call"""
    P = np.asarray(P, dtype=np.float64)
    nd, R = P.shape
    passed, noise, N, amb = threshold(P, guard, prm, which)
    found = [(d, tau) for d, tau in zip(*np.nonzero(passed)) if _local_max(P, guard, int(d), int(tau), which)]
    found.sort(key=lambda c: (-P[c], c[0] * R + c[1]))
    K = prm.max_det
    det, bar = np.zeros((K, 8)), np.zeros((K, 8))
    ok, s = M.in_set(nd, guard), M.signed_bins(nd)
    for k, (d, tau) in enumerate(found[:K]):
        p, nz, n = P[d, tau], noise[d, tau], int(N[d, tau])
        dlag, blag = M._vertex(P[d, tau - 1], p, P[d, tau + 1]) if 0 < tau < R - 1 else (0.0, 0.0)
        dm, dp = (d - 1) % nd, (d + 1) % nd
        ddop, bdop = M._vertex(P[dm, tau], p, P[dp, tau]) if ok[dm] and ok[dp] else (0.0, 0.0)
        snr = p / nz
        det[k] = [tau, s[d], p, snr, nz, dlag, ddop, n]
        bar[k] = [0.0, 0.0, U * p, snr * (U + (n + 2) * E64), nz * (U + n * E64), blag, bdop, 0.0]
    return dict(count=len(found), cells=[int(d) * R + int(tau) for d, tau in found], det=det, bar=bar, passed=int(passed.sum()), ambiguous=int(amb.sum()))


def maps_of(chi32, map32):
    """the nrows + 1 maps of a line as the device's entries have them: the rows' |chi|^2, then the published map"""
    return [M.power(c) for c in np.asarray(chi32)] + [np.asarray(map32, dtype=np.float64)]


def snapshot(chi32, cells, K):
    """snap [K][nrows] complex64: chi of every row at the detections' cells, zeros behind them"""
    chi32 = np.asarray(chi32)
    nrows = chi32.shape[0]
    flat = chi32.reshape(nrows, -1)
    out = np.zeros((K, nrows), dtype=np.complex64)
    for k, i in enumerate(cells[:K]):
        out[k] = flat[:, i]
    return out
