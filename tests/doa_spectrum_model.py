"""Test helper: the Bartlett and Capon power maps of crsdr_doa_set_spectrum / crsdr_spectrum2d (include/crsdr.h) in fp64 numpy, with
the bound an fp32 evaluation in the header's expression order has to meet.  Plain numpy, independent of the kernels.

Definition (M = mx my, vec and sv the published fp32 subspace, a the steering vector of crsdr_pmusic2d on the grid):
    y_r = sum_i conj(vec[i][r]) a[i] for all r,   S = sum_r w_r |y_r|^2
    Bartlett  w_r = sv[r] / M^2,                                   pm = S
    Capon     w_r = 1 / (sv[r] + delta), delta = loading sv[0],    pm = 1 / S           (loading as the float32 the ABI takes)
    sv[0] == 0: pm = 0 everywhere.

Bound (first order in u = 2^-24, in the style of music_model.scan's docstring, whose terms it reuses).  The comparison is made on S:
the device's pm for Bartlett, 1 / pm for Capon (near a Capon peak S is small and pm ill-conditioned, as den is for MUSIC).
  * y_r.  music_model's per-element term dphi_i = 2 pi d (18u ix + 11u iy) + 11u + 3M u covers the fp32 steering vector in the
    reference's expression order and the 2M-term accumulation per component (fused multiply-adds round half as often and are inside
    it): |d y_r| <= dy_r = sum_i |vec[i][r]| dphi_i.
  * |y_r|^2 moves by 2 |y_r| dy_r + dy_r^2, weighted with w_r >= 0: sum_r w_r (2 |y_r| dy_r + dy_r^2).
  * roundings relative to S (no term of S is negative, so a relative error of a term or of a partial sum is at most that of S):
    w_r is fp64 rounded once to fp32: 1u (Bartlett's 1 / M^2 is inside it).  |y_r|^2 = yr yr + yi yi: two products and their sum, 2u.
    The product with w_r: 1u.  The M additions into S: M u.  Together (M + 4) u S for an evaluation without fused multiply-adds; one
    with them rounds less often.
  * Capon's reciprocal pm = 1 / S: one rounding, 1u of pm, so 1 / pm = S (1 +- u): 1u S more.
  bound = sum_r w_r (2 |y_r| dy_r + dy_r^2) + (M + 4 [+ 1 for Capon]) u S.
The fp64 weights are taken as exact (their own error is 1e-16)."""
import numpy as np

import music_model as mm

BARTLETT, CAPON = 1, 2
KINDS = {"bartlett": BARTLETT, "capon": CAPON}
U32 = mm.U32


def weights(sv, kind, loading):
    """w [M] in fp64 from the fp32 sv (not yet rounded to fp32)."""
    s = np.asarray(sv, dtype=np.float32).astype(np.float64)
    M = len(s)
    if kind == BARTLETT:
        return s / (float(M) * float(M))
    return 1.0 / (s + float(np.float32(loading)) * s[0])


def y_all(vec, d, mx, my, ncx, ncy, **kw):
    """(y [ncx][ncy][M] = v_r^H a, dy [M]) of every column."""
    M = mx * my
    y, un = mm._y(vec, 0, d, mx, my, ncx, ncy, **kw)
    ix, iy = mm.element_index(mx, my)
    dphi = 2.0 * np.pi * float(np.float32(d)) * U32 * (mm.CX_PHASE * ix + mm.CY_PHASE * iy) + (mm.C_ELEM + 3.0 * M) * U32
    return y, np.abs(un).T @ dphi


def maps(vec, sv, kind, loading, d, mx, my, ncx, ncy):
    """(S64 [ncx][ncy], bound [ncx][ncy]): S of the given fp32 vec and sv in fp64 and the absolute bound on |S_device - S64|, S_device =
    pm (Bartlett) or 1 / pm (Capon).  An all-zero estimate (sv[0] == 0) has S64 = 0 and bound 0 for Bartlett; Capon's pm is 0 by
    definition there and has no S: use power() for it."""
    M = mx * my
    w = weights(sv, kind, loading) if np.asarray(sv)[0] != 0 else np.zeros(M)
    y, dy = y_all(vec, d, mx, my, ncx, ncy)
    S = (w[None, None, :] * np.abs(y) ** 2).sum(axis=2)
    bound = (w[None, None, :] * (2.0 * np.abs(y) * dy[None, None, :] + (dy ** 2)[None, None, :])).sum(axis=2)
    bound = bound + (M + 4 + (kind == CAPON)) * U32 * S
    return S, bound


def power(S, kind):
    """The map itself, fp64: S, or 1 / S."""
    return S if kind == BARTLETT else 1.0 / S


def s_of(pm, kind):
    """The S an fp32 map stands for: pm, or 1 / pm (pm = 0 -> inf, pm = inf -> 0)."""
    pm = np.asarray(pm, dtype=np.float64)
    if kind == BARTLETT:
        return pm
    with np.errstate(divide="ignore"):
        return 1.0 / pm


def fractions(pm, kind, S, bound):
    """(worst |S_device - S64| / bound over the grid, median |S_device - S64| / S64).  A NaN or a negative pm counts as infinitely wrong."""
    pm = np.asarray(pm, dtype=np.float64)
    err = np.abs(s_of(pm, kind) - S)
    err = np.where(np.isnan(err) | (pm < 0), np.inf, err)
    return float((err / bound).max()), float(np.median(err / S))


def _peak_interval(S, bound, kind):
    """(lo, hi) of the quantity whose MAXIMUM is the map's peak: S for Bartlett, -S for Capon (pm = 1 / S is largest where S is least)."""
    return (S - bound, S + bound) if kind == BARTLETT else (-S - bound, -S + bound)


def admissible_peak(S, bound, kind, peak):
    """True when an fp32 map within the bound can have its maximum at `peak` (cx, cy)."""
    lo, hi = _peak_interval(S, bound, kind)
    p = tuple(int(v) for v in peak)
    return bool(hi[p] >= lo.max())


def certain_peak(S, bound, kind):
    """The grid point every fp32 map within the bound must report as its maximum, or None."""
    lo, hi = _peak_interval(S, bound, kind)
    p = np.unravel_index(np.argmax(lo), lo.shape)
    others = hi.copy()
    others[p] = -np.inf
    return tuple(int(v) for v in p) if lo[p] > others.max() else None


def local_peaks_within_bound(S, bound, kind, radius, region):
    """(certain, possible): the grid points of `region` (a pair of slices) that every / that some fp32 map within the bound has as a
    local maximum of radius `radius` (doa_peaks_model's window, clipped at the grid's edges), as sorted lists of (cx, cy); and the
    margin: the least gap that decides a point, as a multiple of the two bounds involved (> 1 everywhere: certain == possible)."""
    lo, hi = _peak_interval(S, bound, kind)
    ncx, ncy = S.shape
    certain, possible, margin = [], [], np.inf
    for cx in range(*region[0].indices(ncx)):
        for cy in range(*region[1].indices(ncy)):
            x0, x1, y0, y1 = max(cx - radius, 0), min(cx + radius, ncx - 1) + 1, max(cy - radius, 0), min(cy + radius, ncy - 1) + 1
            mid = (lo + hi)[x0:x1, y0:y1] / 2
            b = bound[x0:x1, y0:y1] + bound[cx, cy]
            gap = (mid[cx - x0, cy - y0] - mid) / b                   # > 1: certainly above that neighbour, < -1: certainly below
            gap[cx - x0, cy - y0] = np.inf
            if gap.min() > 1:
                certain.append((cx, cy))
            if gap.min() >= -1:
                possible.append((cx, cy))
            margin = min(margin, float(np.abs(gap).min()) if gap.min() > -1 else float(-gap.min()))
    return certain, possible, margin


# ---- the resolution scene (CPU test on the fp64 model, GPU test on the device, same block) ----
# 7 x 3 URA, two equal incoherent sources whose peaks sit six grid steps apart in cx on a 100 x 100 grid; set_peaks(4, RES_RADIUS);
# inside RES_REGION Bartlett has one local maximum and Capon (RES_LOADING) two.  tests/test_doa_spectrum_model.py states the margins.
RES_SEED, RES_L, RES_RADIUS, RES_LOADING = 5, 1024, 2, 1e-2
RES_PEAKS = ((47, 50), (53, 50))
RES_REGION = (slice(40, 61), slice(44, 57))


def resolution_block():
    import ura
    rng = np.random.default_rng(RES_SEED)
    return ura.scene(RES_L, [(*mm.mirrored_source(cx, cy, 100, 100), 1.0) for cx, cy in RES_PEAKS], rng)


def region_peaks(pm, radius=RES_RADIUS, region=RES_REGION):
    """[(cx, cy)] of the local maxima (doa_peaks_model's definition) of pm [100][100] inside the region."""
    import doa_peaks_model as pk
    mask = np.zeros(pm.shape, dtype=bool)
    mask[region] = True
    return [tuple(int(v) for v in p) for p in np.argwhere(pk.is_local_peak(np.asarray(pm, dtype=np.float32), radius) & mask)]


# ---- the power scene: two incoherent sources of different strength, far enough apart for both maps ----
POW_SEED, POW_L = 7, 4096
POW_PEAKS, POW_AMPS = ((35, 45), (65, 58)), (1.0, 2.0)             # amplitudes 1 : 2 are powers 1 : 4


def power_block():
    import ura
    rng = np.random.default_rng(POW_SEED)
    return ura.scene(POW_L, [(*mm.mirrored_source(cx, cy, 100, 100), a) for (cx, cy), a in zip(POW_PEAKS, POW_AMPS)], rng)
