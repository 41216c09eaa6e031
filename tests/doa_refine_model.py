"""Test helper: the zoom search of crsdr_doa_set_refine / crsdr_refine2d (include/crsdr.h) in fp64 numpy.  Plain numpy, independent of
the kernel.

Definition.  Cell coordinates x, y; alpha = x pi / ncx, beta = y pi / ncy; a_i = exp(2 pi j d (ix cos(alpha) sin(beta) + iy cos(beta)))
with d the float32 the ABI takes; y_r = v_r^H a from the given vec (fp32 as published, or any other precision: the model promotes it);
    MUSIC     f = (M / den)^2, den = sum_{r >= k} |y_r|^2
    Bartlett  f = S, Capon f = 1 / S,  S = sum_r w_r |y_r|^2 with doa_spectrum_model.weights (fp64, not rounded)
    sv[0] == 0: f = 0
    x = cx, y = cy, s = 1/2; L times: the 7 x 7 lattice of spacing s around (x, y), clamped to [0, ncx] x [0, ncy], in row-major order;
    a point replaces the best so far if it is strictly above the centre and strictly above the best; then s = s / 4.

Comparable quantity.  f is monotone in q = -den (MUSIC), S (Bartlett), -S (Capon), and the project's bounds are bounds on den and S:
the model compares q.  (f itself adds the quotient and the square, which those bounds already count.)

tol.  The bound of music_model.scan (MUSIC) or doa_spectrum_model.maps (the two maps) at the point, with u = 2^-53 in place of 2^-24,
times 4 for the device's libm sincos and argument formation, which those formulas count as single operations.  branches() follows
every choice a device within tol of this model can make: a point is a possible choice of a level when its q + tol reaches the
largest q - tol of the level."""
import numpy as np

import doa_spectrum_model as sm
import music_model as mm

MUSIC, BARTLETT, CAPON = 0, sm.BARTLETT, sm.CAPON
U64 = 2.0 ** -53
LIBM = 4.0
SIDE = 7                                                     # lattice points per axis and level; the spacing shrinks by 4


def points_y(vec, d, mx, my, ncx, ncy, xs, ys):
    """y [P][M] = v_r^H a at the cell coordinates (xs [P], ys [P])."""
    v = np.asarray(vec).astype(np.complex128)
    ix, iy = mm.element_index(mx, my)
    alpha = (np.asarray(xs, dtype=np.float64) * np.pi / ncx)[:, None]
    beta = (np.asarray(ys, dtype=np.float64) * np.pi / ncy)[:, None]
    a = np.exp(2j * np.pi * float(np.float32(d)) * (ix[None, :] * np.cos(alpha) * np.sin(beta) + iy[None, :] * np.cos(beta)))
    return a @ v.conj()


def q_points(vec, sv, kind, k, loading, d, mx, my, ncx, ncy, xs, ys, u=U64):
    """(q [P], tol [P], f [P]) at the points: the comparable quantity, the allowance on it, the map's value."""
    M = mx * my
    xs = np.atleast_1d(np.asarray(xs, dtype=np.float64))
    if np.asarray(sv)[0] == 0:
        z = np.zeros(len(xs))
        return z, z.copy(), z.copy()
    y = points_y(vec, d, mx, my, ncx, ncy, xs, np.atleast_1d(ys))
    v = np.asarray(vec).astype(np.complex128)
    ix, iy = mm.element_index(mx, my)
    dphi = 2.0 * np.pi * float(np.float32(d)) * u * (mm.CX_PHASE * ix + mm.CY_PHASE * iy) + (mm.C_ELEM + 3.0 * M) * u
    dy = np.abs(v).T @ dphi                                                       # [M]
    if kind == MUSIC:
        yn, dyn = y[:, k:], dy[k:]
        den = (np.abs(yn) ** 2).sum(axis=1)
        bound = (2.0 * np.abs(yn) * dyn[None, :] + (dyn ** 2)[None, :]).sum(axis=1) + (M - k + M + 30) * u * den
        with np.errstate(divide="ignore"):
            return -den, LIBM * bound, (M / den) ** 2
    w = sm.weights(sv, kind, loading)
    S = (w[None, :] * np.abs(y) ** 2).sum(axis=1)
    bound = (w[None, :] * (2.0 * np.abs(y) * dy[None, :] + (dy ** 2)[None, :])).sum(axis=1) + (M + 4 + (kind == CAPON)) * u * S
    with np.errstate(divide="ignore"):
        return (S, LIBM * bound, S) if kind == BARTLETT else (-S, LIBM * bound, 1.0 / S)


def lattice(x, y, s, ncx, ncy, side=SIDE):
    """(px [side^2], py [side^2]) in the definition's order (i major), clamped to the grid's range."""
    h = side // 2
    i, j = np.repeat(np.arange(-h, h + 1), side), np.tile(np.arange(-h, h + 1), side)
    return np.clip(x + i * s, 0.0, float(ncx)), np.clip(y + j * s, 0.0, float(ncy))


def refine(vec, sv, kind, k, loading, d, mx, my, ncx, ncy, peak, levels, side=SIDE, shrink=4.0):
    """The definition, literally.  ((x - cx, y - cy), (alpha, beta), f at the refined point).  side / shrink: another lattice (the
    definition's is 7 and 4) for the measurements of tests/test_doa_refine_model.py."""
    cx, cy = (int(p) for p in peak)
    x, y, s, centre, fbest = float(cx), float(cy), 0.5, (side * side) // 2, 0.0
    for _ in range(levels):
        px, py = lattice(x, y, s, ncx, ncy, side)
        q, _, f = q_points(vec, sv, kind, k, loading, d, mx, my, ncx, ncy, px, py)
        c = best = q[centre]
        bx, by, fbest = x, y, f[centre]
        for p in range(side * side):
            if p != centre and q[p] > c and q[p] > best:
                best, bx, by, fbest = q[p], float(px[p]), float(py[p]), f[p]
        x, y, s = bx, by, s / shrink
    return (x - cx, y - cy), (x * np.pi / ncx, y * np.pi / ncy), float(fbest)


def branches(vec, sv, kind, k, loading, d, mx, my, ncx, ncy, peak, levels):
    """The set of final offsets (x - cx, y - cy) a device within tol of this model can reach."""
    cx, cy = (int(p) for p in peak)
    states, s = {(float(cx), float(cy))}, 0.5
    for _ in range(levels):
        nxt = set()
        for x, y in states:
            px, py = lattice(x, y, s, ncx, ncy)
            q, tol, _ = q_points(vec, sv, kind, k, loading, d, mx, my, ncx, ncy, px, py)
            floor = (q - tol).max()
            for p in np.nonzero(q + tol >= floor)[0]:
                nxt.add((float(px[p]), float(py[p])))
        states, s = nxt, s / 4.0
    return {(x - cx, y - cy) for x, y in states}


def f_at(vec, sv, kind, k, loading, d, mx, my, ncx, ncy, x, y):
    """(q, tol, f) at one point."""
    q, tol, f = q_points(vec, sv, kind, k, loading, d, mx, my, ncx, ncy, [x], [y])
    return float(q[0]), float(tol[0]), float(f[0])


def q_of(value, kind, M):
    """The comparable quantity a device value stands for: -M / sqrt(f), f, -1 / f."""
    value = float(value)
    with np.errstate(divide="ignore"):
        if kind == MUSIC:
            return -M / np.sqrt(value)
        return value if kind == BARTLETT else -1.0 / value


# ---- the scenes of the model test and of the device's end-to-end test ----
import ura

SCENES = (dict(mx=3, my=2, d=0.5, nc=16, L=256, seed=1), dict(mx=7, my=3, d=float(ura.D), nc=100, L=1024, seed=2), dict(mx=8, my=8, d=0.5, nc=32, L=512, seed=3))
OFFSETS = ((0.37, -0.29), (0.5, 0.5), (-0.45, 0.1))
LEVELS = 5


def scene_id(sc, off):
    return f"{sc['mx']}x{sc['my']}-{sc['nc']}-{off[0]:+.2f}{off[1]:+.2f}"


def true_cell(sc, off):
    return 0.45 * sc["nc"] + off[0], 0.55 * sc["nc"] + off[1]


def scene_block(sc, off):
    """int8 rows [1 + M][2 L]: one emitter whose map peak sits at true_cell."""
    tx, ty = true_cell(sc, off)
    rng = np.random.default_rng(sc["seed"])
    return ura.scene(sc["L"], [(*mm.mirrored_source(tx, ty, sc["nc"], sc["nc"]), 1.0)], rng, mx=sc["mx"], my=sc["my"], d=np.float32(sc["d"]))


def fp64_subspace(block):
    """(sv, vec) in fp64 of the model's own covariance (music_model.rxx_reference's definition without its rounding), numpy eigh."""
    x = np.asarray(block)[1:].astype(np.float64) / 127.0
    X = (x[:, 0::2] + 1j * x[:, 1::2]).T
    X = X - X.mean(axis=0, keepdims=True)
    return mm.eigh_by_magnitude(X.conj().T @ X / X.shape[0])


def grid_peak(vec, sv, kind, k, loading, d, mx, my, ncx, ncy):
    """The grid point with the largest q (lowest index among equals, as the device's peak key orders)."""
    gx, gy = np.repeat(np.arange(ncx), ncy), np.tile(np.arange(ncy), ncx)
    q, _, _ = q_points(vec, sv, kind, k, loading, d, mx, my, ncx, ncy, gx, gy)
    p = int(np.argmax(q))
    return int(gx[p]), int(gy[p])
