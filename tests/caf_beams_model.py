"""fp64 numpy statement of crsdr_caf's coherent beam maps (include/crsdr.h, section (w), "Beams"; crsdr_caf_set_beams, crsdr_beam_maps,
crsdr_beam_fuse, crsdr_caf_beam_steer), and the error bars of the device against it.  caf_model, caf_cfar_model and caf_bearing_model
are imported and left as they are: the maps, the detector and the steering expression are their own.

Definition.  The rows c != ref_row in ascending order are the elements e = 0 .. m - 1, m = nrows - 1.  With the float32 weights
w [nb][m] and the published float32 chi, both promoted to fp64,
    z_b[d][tau] = sum_e w_b,e chi_c(e)[d][tau]                       bmap_b = |z_b|^2, published as a float32
The detector (caf_cfar_model.detect, unchanged) runs on every published beam map; bcount [nb], bdet [nb][K][8] as count and det.
Fusion.  The candidates are the slots q < min(bcount[b], K) of every beam.  A before A'  <=>  P > P', or P == P' and b < b', or those
equal and i < i' (i = d R + tau; one cell twice in one beam of a hand-made list: the earlier slot).  A candidate is suppressed iff some other candidate comes before it and lies within one cell of it
(lag difference at most 1, no wrap; Doppler difference at most 1 modulo nd), whether or not that other one is itself suppressed.
nfused: the number of survivors; fused [K][8]: the first K survivors in that order, each its bdet record with the eighth figure
replaced by the beam index; unused slots zero.

Error bars, derived and not measured (U = 2^-24, E = 2^-53).
    z        re z is a sum of the 2 m products wr cr, -wi ci.  However they are ordered, and whether each addition is fused with its
             multiplication or not, every product meets at most 2 m roundings on its way into the sum (its own and at most 2 m - 1
             additions; a fused multiply-add drops one), so by Higham's (3.4) the computed sum is sum_k p_k (1 + theta_k) with
             |theta_k| <= gamma_(2m), gamma_n = n U / (1 - n U):
                 b_re = gamma_(2m) sum_e (|wr||cr| + |wi||ci|),      b_im = gamma_(2m) sum_e (|wr||ci| + |wi||cr|)
             An intermediate that falls below the normal range is rounded absolutely, by at most 2^-150 each: 2 m 2^-150 more.
    bmap     the squares and their sum are taken in fp64 from the fp32 z: the products are exact (24-bit factors), the sum has one
             rounding E, and the result one rounding to fp32 (U, or 2^-150 below the normal range).  With |zr^2 - zr'^2| <=
             2 |zr| b_re + b_re^2, and likewise for the imaginary part:
                 d = 2 |zr| b_re + b_re^2 + 2 |zi| b_im + b_im^2,     bar(bmap) = d + (U + E)(P + d) + 2^-149
    bdet     the detector's own bars (caf_cfar_model) on the map it was given; fusion copies records: 0.
    steer    crsdr_caf_beam_steer against (a / sqrt(m)) rounded to float32: the phase is formed as the bearings form it, so a_e is off by
             at most caf_bearing_model's dphi_e with LIBM = 4 for the two libms (doa_refine_model's allowance); the scaling, the
             square root and their order: 3 E; the two roundings to fp32 may fall either side of a tie: 2 U.  Per part
                 |dw| <= (dphi_e + 3 E + 2 U) / sqrt(m)
AMBIGUOUS.  Detections are compared exactly.  The detector's model counts the cells too near the threshold to call
(caf_cfar_model.AMBIGUOUS); `ambiguous` here is their sum over the beams.  Every comparison first asserts that it is 0; no test may
use it to leave a detection out."""
import numpy as np

import caf_bearing_model as BM
import caf_cfar_model as CF
import caf_model as M
import music_model as mm

U, E64 = M.U, M.E64
TINY = 2.0 ** -149
MUTATIONS = ["w_conj", "im_sign", "ref_counts", "beam_fastest", "powers_summed"]
FUSE_MUTATIONS = ["lag_wrap", "doppler_nowrap", "same_cell", "tie_reversed", "dead_cannot_suppress"]


def gamma(n):
    return n * U / (1.0 - n * U)


def element_rows(nrows, ref, which=None):
    return BM.element_rows(nrows, ref, which)


def _weights(W, m, which):
    W = np.asarray(W).astype(np.complex64).astype(np.complex128)             # what the device is handed
    nb = len(W)
    if which == "beam_fastest":                                              # [m][nb] read where [nb][m] was written
        W = W.reshape(-1).reshape(m, nb).T
    if which == "w_conj":
        W = W.conj()
    return W


def beam_sums(chi32, ref, W, which=None):
    """(z [nb][nd][R] complex128, b_re, b_im) from chi [nrows][nd][R] complex64 and the weights [nb][m]"""
    chi32 = np.asarray(chi32)
    nrows = chi32.shape[0]
    m = nrows - 1
    W = _weights(W, m, which)
    x = chi32[element_rows(nrows, ref, which)].astype(np.complex128)         # [m][nd][R]
    wr, wi, cr, ci = W.real, W.imag, x.real, x.imag
    zr = np.einsum("be,edt->bdt", wr, cr) - np.einsum("be,edt->bdt", wi, ci)
    zi = np.einsum("be,edt->bdt", wr, ci) + np.einsum("be,edt->bdt", wi, cr)
    if which == "im_sign":
        zi = np.einsum("be,edt->bdt", wr, ci) - np.einsum("be,edt->bdt", wi, cr)
    g = gamma(2 * m)
    b_re = g * (np.einsum("be,edt->bdt", np.abs(wr), np.abs(cr)) + np.einsum("be,edt->bdt", np.abs(wi), np.abs(ci))) + 2 * m * TINY / 2
    b_im = g * (np.einsum("be,edt->bdt", np.abs(wr), np.abs(ci)) + np.einsum("be,edt->bdt", np.abs(wi), np.abs(cr))) + 2 * m * TINY / 2
    return zr + 1j * zi, b_re, b_im


def bmap(chi32, ref, W, which=None):
    """(P [nb][nd][R] fp64, bar [nb][nd][R]): the beam maps before their rounding to float32, and the device's bar against them"""
    z, b_re, b_im = beam_sums(chi32, ref, W, which)
    P = z.real ** 2 + z.imag ** 2
    if which == "powers_summed":
        chi32 = np.asarray(chi32)
        W2 = np.abs(_weights(W, chi32.shape[0] - 1, None)) ** 2
        P = np.einsum("be,edt->bdt", W2, M.power(chi32[element_rows(chi32.shape[0], ref)]))
    d = 2.0 * np.abs(z.real) * b_re + b_re ** 2 + 2.0 * np.abs(z.imag) * b_im + b_im ** 2
    return P, d + (U + E64) * (P + d) + TINY


def bmap_f32(chi32, ref, W, reverse=False, split=False):
    """a float32 restatement of the beam maps: every product and every addition rounded to float32 (no fused multiply-add), the
    elements ascending or descending, and with split the real and imaginary products in two sums joined at the end"""
    chi32 = np.asarray(chi32)
    nrows = chi32.shape[0]
    W = np.asarray(W).astype(np.complex64)
    x = chi32[element_rows(nrows, ref)]
    wr, wi = W.real.astype(np.float32), W.imag.astype(np.float32)
    cr, ci = x.real.astype(np.float32), x.imag.astype(np.float32)
    nb = len(W)
    shape = (nb,) + chi32.shape[1:]
    zr, zi, zr2, zi2 = (np.zeros(shape, dtype=np.float32) for _ in range(4))
    order = range(nrows - 2, -1, -1) if reverse else range(nrows - 1)
    for e in order:
        a, b = wr[:, e, None, None], wi[:, e, None, None]
        if split:
            zr, zr2 = zr + a * cr[e], zr2 + b * ci[e]
            zi, zi2 = zi + a * ci[e], zi2 + b * cr[e]
        else:
            zr = (zr + a * cr[e]) - b * ci[e]
            zi = (zi + b * cr[e]) + a * ci[e]
    if split:
        zr, zi = zr - zr2, zi + zi2
    assert zr.dtype == np.float32 and zi.dtype == np.float32
    return (zr.astype(np.float64) ** 2 + zi.astype(np.float64) ** 2).astype(np.float32)


def detect_beams(P32, guard, prm):
    """the detector on every published beam map [nb][nd][R]: dict(bdet [nb][K][8] fp64, bar, bcount [nb], cells (per beam), ambiguous)"""
    P32 = np.asarray(P32)
    nb, K = len(P32), prm.max_det
    out = dict(bdet=np.zeros((nb, K, 8)), bar=np.zeros((nb, K, 8)), bcount=np.zeros(nb, dtype=np.int64), cells=[], ambiguous=0)
    for b in range(nb):
        r = CF.detect(P32[b].astype(np.float64), guard, prm)
        out["bdet"][b], out["bar"][b], out["bcount"][b] = r["det"], r["bar"], r["count"]
        out["cells"].append(r["cells"])
        out["ambiguous"] += r["ambiguous"]
    return out


def _near(c1, c2, nd, R, which):
    (d1, t1), (d2, t2) = c1, c2
    if which == "same_cell":
        return (d1, t1) == (d2, t2)
    dt = min((t1 - t2) % R, (t2 - t1) % R) if which == "lag_wrap" else abs(t1 - t2)
    dd = abs(d1 - d2) if which == "doppler_nowrap" else min((d1 - d2) % nd, (d2 - d1) % nd)
    return dt <= 1 and dd <= 1


def fuse(bdet, bcount, nd, R, which=None, arrival=None):
    """(fused [K][8], nfused) of a line's lists bdet [nb][K][8], bcount [nb].  arrival: a permutation of the candidates' order of arrival,
    which must not matter.  which: one of FUSE_MUTATIONS"""
    bdet = np.asarray(bdet)
    nb, K, _ = bdet.shape
    cand = []
    for b in range(nb):
        for q in range(min(max(int(bcount[b]), 0), K)):
            rec = bdet[b, q]
            d, tau = int(rec[1]) % nd, int(rec[0])
            cand.append((rec[2], b, d * R + tau, (d, tau), q))
    if arrival is not None:
        cand = [cand[k] for k in arrival]

    def before(x, y):
        if x[0] != y[0]:
            return x[0] > y[0]
        if which == "tie_reversed":
            return (x[1], x[2], x[4]) > (y[1], y[2], y[4])
        return (x[1], x[2], x[4]) < (y[1], y[2], y[4])

    if which == "dead_cannot_suppress":                                         # greedy: only a survivor suppresses
        alive = []
        for x in sorted(cand, key=lambda c: (-c[0], c[1], c[2], c[4])):
            if not any(_near(y[3], x[3], nd, R, None) for y in alive):
                alive.append(x)
    else:
        alive = [x for x in cand if not any(y is not x and before(y, x) and _near(y[3], x[3], nd, R, which) for y in cand)]
        key = (lambda c: (-c[0], -c[1], -c[2], -c[4])) if which == "tie_reversed" else (lambda c: (-c[0], c[1], c[2], c[4]))
        alive.sort(key=key)
    fused = np.zeros((K, 8), dtype=bdet.dtype)
    for k, x in enumerate(alive[:K]):
        fused[k] = bdet[x[1], x[4]]
        fused[k, 7] = x[1]
    return fused, len(alive)


def line(chi32, ref, W, guard, prm, which=None):
    """a line, all of it: dict(bmap32 [nb][nd][R] float32, bar, bdet, bcount, fused, nfused, ambiguous)"""
    P, bar = bmap(chi32, ref, W, which)
    P32 = P.astype(np.float32)
    det = detect_beams(P32, guard, prm)
    nd, R = P.shape[1:]
    fused, nf = fuse(det["bdet"], det["bcount"], nd, R)
    return dict(bmap32=P32, bar=bar, bdet=det["bdet"], dbar=det["bar"], bcount=det["bcount"], fused=fused, nfused=nf, ambiguous=det["ambiguous"])


def hand_lists(entries, nb, K, nd):
    """(bdet [nb][K][8] float32, bcount [nb] int32) as the detector lays them out, from entries (beam, d, tau, P) in each beam's own
    order; snr, noise and ntrain are made up from the entry's position so that a copied record can be told from another"""
    bdet, bcount = np.zeros((nb, K, 8), dtype=np.float32), np.zeros(nb, dtype=np.int32)
    s = M.signed_bins(nd)
    for n, (b, d, tau, p) in enumerate(entries):
        q = int(bcount[b])
        if q < K:
            bdet[b, q] = [tau, s[d], p, 10.0 + n, p / (10.0 + n), 0.125, -0.25, 40 + n]
        bcount[b] += 1
    return bdet, bcount


# Hand-made lists on nd 8, R 6 (entries as hand_lists takes them) and what must survive, as (beam, d, tau) in order
HAND_ND, HAND_R = 8, 6
HAND_FUSE = {
    "two beams at the same cell": ([(0, 2, 3, 5.0), (1, 2, 3, 7.0)], [(1, 2, 3)]),
    "a chain A > B > C one cell apart each: only A survives": ([(0, 2, 1, 9.0), (1, 2, 2, 8.0), (2, 2, 3, 7.0)], [(0, 2, 1)]),
    "a diagonal chain across beams and Doppler": ([(3, 4, 1, 9.0), (3, 5, 2, 8.0), (0, 6, 3, 7.0)], [(3, 4, 1)]),
    "neighbours across the Doppler wrap": ([(0, 0, 2, 4.0), (1, 7, 2, 6.0), (2, 7, 3, 5.0)], [(1, 7, 2)]),
    "lags 0 and R - 1 are no neighbours": ([(0, 3, 0, 4.0), (1, 3, 5, 6.0), (2, 4, 5, 5.0)], [(1, 3, 5), (0, 3, 0)]),
    "equal powers in two beams": ([(2, 5, 2, 3.0), (1, 5, 3, 3.0), (3, 1, 1, 3.0), (0, 1, 4, 3.0)], [(0, 1, 4), (1, 5, 3), (3, 1, 1)]),
    "one record's cell twice in one beam: the earlier slot alone": ([(2, 3, 2, 5.0), (2, 3, 2, 5.0), (1, 6, 4, 5.0)], [(1, 6, 4), (2, 3, 2)]),
    "two cells apart: both survive": ([(0, 2, 1, 9.0), (1, 2, 3, 8.0), (1, 4, 1, 7.0)], [(0, 2, 1), (1, 2, 3), (1, 4, 1)]),
}


# ---- steering ----
def steer_weights(q, xy):
    """w [nb][m] complex64 = a(x, y) / sqrt(m), each part rounded once: what crsdr_caf_beam_steer states"""
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    return (BM.steer(q, xy[:, 0], xy[:, 1]) / np.sqrt(q.m)).astype(np.complex64)


def steer_bar(q):
    """the allowance per part of a weight [m] (module docstring)"""
    ix, iy = mm.element_index(q.mx, q.my)
    dphi = BM.LIBM * (2.0 * np.pi * q.d * E64 * (mm.CX_PHASE * ix + mm.CY_PHASE * iy) + (mm.C_ELEM + 3.0 * q.m) * E64)
    return (dphi + 3.0 * E64 + 2.0 * U) / np.sqrt(q.m)


def lattice(nx=8, ny=8, nc=100):
    """the nx x ny lattice of directions of the issue's bank on an nc x nc grid, beam index nx-major: for 8 x 8 on 100 x 100
    x = 6 + 12.5 i, y = 12 + 12.5 j, beam 8 i + j; in general x = (i + 0.48) nc / nx, y = (j + 0.96) nc / ny, inside the grid for any nx, ny"""
    return np.array([((nc * i + 0.48 * nc) / nx, (nc * j + 0.96 * nc) / ny) for i in range(nx) for j in range(ny)])


# ---- the scene of the model test and of the device's end-to-end test ----
# caf_bearing_model.SCENES[1] (7 x 3, 22 rows, B 2048, 2 frames, seg 32, 24 lags, nd 64) with the echo at amplitude 0.02 (0.6 LSB) at lag 7,
# Doppler 5, in grid cell (31, 62): under the array map's detector at any usable alpha, in beam 20 of the 8 x 8 bank at alpha 16
WEAK = dict(scene=1, amp=0.02, seeds=(0, 1, 2, 3), alpha=16.0, map_alphas=(4.0, 6.0, 8.0), cfar=dict(gd=1, gr=1, td=3, tr=4), guard=2, beam=20, max_det=16)


def weak_line(seed):
    """(chi32 [22][64][24], map32, desc, weights [64][21] complex64, the echo's (lag, doppler)) of the weak scene"""
    sc = BM.SCENES[WEAK["scene"]]
    blocks, q, _ = BM.scene_line(sc, amp=WEAK["amp"], seed=seed)
    chi32, map32 = BM.scene_maps(sc, blocks)
    return chi32, map32, q, steer_weights(q, lattice(8, 8, sc[3])), (sc[9], sc[10])
