"""Test helper: fp64 numpy restatement of crsdr_doa_set_augment (include/crsdr.h (iv)), the bar the GPU tests hold the device to, and
the scenes the feature was specified from.  Plain numpy; nothing here calls the library.

Augmentation.  augment() is the header's definition, term for term.  Physical array mx x my, element i = iy * mx + ix; bit i of the mask
set = element i present (0 = all).  Virtual array vx x vy, element j = jy * vx + jx.  For every lag u = (ux, uy) of the half-plane
(uy > 0, or uy == 0 and ux >= 0; |ux| < vx, uy < vy), P(u) = the pairs (p, q) of present elements with pos_q - pos_p = u by ascending
p, c(u) = |P(u)|, and in fp64 from the fp32 entries, in that order,

    r(u) = (1 / c(u)) sum_{(p, q) in P(u)} rxx[p][q],        ra[a][b] = r(pos_b - pos_a) for a <= b,

the diagonal's imaginary part exactly 0, the lower triangle the conjugate of the upper one.  It returns the UNROUNDED fp64 value.
Bar, per component (real and imaginary apart):

    |dev - model| <= 2^-24 |model| + 2^-45 max|rxx|                                                        (augment_bar)

max|rxx| is taken over the entries the definition can read: rows and columns of present elements (an absent receiver's row may hold
anything, NaN included, and must not widen the bar).  The inputs are exact fp32 numbers.  An fp64 sum of c(u) <= 64 of them has at most
63 additions with a relative error of 2^-53 each on partial sums of at most 64 max|rxx|: below 63 * 64 * 2^-53 max|rxx| < 2^-41 max|rxx|
in whatever order they are taken -- but device and model take them in the SAME order (the definition fixes it: ascending p), so both
hold the same fp64 sum and this term only has to cover a compiler that reassociates; 2^-45 max|rxx| is what the issue sets (smoothing's
form) and it is kept.  The division by c(u) is one more fp64 rounding, the same on both sides (2^-53 relative, far inside the first term
if it were not).  The single rounding to fp32 is half an ulp: 2^-24 |model| for normal numbers; results below the normal range
(|x| < 2^-126) are covered by the absolute term as long as max|rxx| > 2^-81, and an all-zero rxx gives exact zeros.
"""
import functools

import numpy as np

import doa_smooth_model as smooth_model
import ura

DEG = np.pi / 180.0
SOURCES = [(60 * DEG, 70 * DEG, 1.0), (110 * DEG, 100 * DEG, 0.9), (85 * DEG, 130 * DEG, 0.8)]
SEEDS = range(8)
L = 4096
THINNED = "110001111101001010101"        # 12 of the 21 elements of the 7 x 3 array
THINNED11 = "101000110000011111011"      # 11 of them
RULER = "1100101"                        # 7 x 1: elements 0, 1, 4, 6 cover every lag 0 .. 6


def mask_of(mask, m):
    """int mask with "0 = all" resolved: from an int, a string of '0' / '1' in element order, or the indices that are present"""
    if isinstance(mask, str):
        assert len(mask) == m and not set(mask) - {"0", "1"}
        mask = sum(1 << i for i, ch in enumerate(mask) if ch == "1")
    elif not isinstance(mask, (int, np.integer)):
        mask = sum(1 << int(i) for i in mask)
    return int(mask) if mask else (1 << m) - 1


def dead(m, gone):
    """the mask of an m-element array without the elements `gone`"""
    return ((1 << m) - 1) & ~sum(1 << int(i) for i in gone)


def present(mask, m):
    mask = mask_of(mask, m)
    return [i for i in range(m) if (mask >> i) & 1]


def half_plane(vx, vy):
    """the lags in the kernel's order: uy, then ux"""
    return [(ux, uy) for uy in range(vy) for ux in range(-(vx - 1) if uy else 0, vx)]


def pairs(mx, my, ux, uy, mask):
    """P(u): [(p, q)] by ascending p"""
    m = mx * my
    mask = mask_of(mask, m)
    out = []
    for p in range(m):
        ixq, iyq = p % mx + ux, p // mx + uy
        if 0 <= ixq < mx and 0 <= iyq < my:
            q = iyq * mx + ixq
            if (mask >> p) & 1 and (mask >> q) & 1:
                out.append((p, q))
    return out


def lag_counts(mx, my, vx, vy, mask=0):
    """(counts [vy][2 vx - 1] with c(u) at [uy][ux + vx - 1], row 0's negative ux mirrored; the number of uncovered half-plane lags)"""
    counts = np.zeros((vy, 2 * vx - 1), dtype=np.int32)
    missing = 0
    for ux, uy in half_plane(vx, vy):
        c = len(pairs(mx, my, ux, uy, mask))
        counts[uy, ux + vx - 1] = c
        if uy == 0:
            counts[0, vx - 1 - ux] = c
        missing += c == 0
    return counts, missing


def lag_means(rxx, mx, my, vx, vy, mask=0):
    """{(ux, uy): r(u)} complex, each sum taken entry by entry in the definition's order"""
    r = np.asarray(rxx).astype(np.complex128)
    out = {}
    for ux, uy in half_plane(vx, vy):
        P = pairs(mx, my, ux, uy, mask)
        assert P, ("uncovered lag", ux, uy)
        re = im = 0.0
        for p, q in P:
            re += float(r[p, q].real)
            im += float(r[p, q].imag)
        out[(ux, uy)] = complex(re / len(P), im / len(P))
    return out


def augment(rxx, mx, my, vx, vy, mask=0):
    """ra [mv][mv] complex128, unrounded"""
    lag = lag_means(rxx, mx, my, vx, vy, mask)
    mv = vx * vy
    out = np.zeros((mv, mv), dtype=np.complex128)
    for a in range(mv):
        for b in range(a, mv):
            v = lag[(b % vx - a % vx, b // vx - a // vx)]
            if a == b:
                v = complex(v.real, 0.0)
            out[a, b] = v
            out[b, a] = np.conj(v)
    return out


def readable_top(rxx, mx, my, mask=0):
    """max |component| over the rows and columns of present elements"""
    s = present(mask, mx * my)
    r = np.asarray(rxx)[np.ix_(s, s)]
    return max(np.abs(r.real).max(), np.abs(r.imag).max())


def augment_bar(model, top):
    """per component: (bar_re, bar_im); top = readable_top"""
    return 2.0 ** -24 * np.abs(model.real) + 2.0 ** -45 * top, 2.0 ** -24 * np.abs(model.imag) + 2.0 ** -45 * top


def within_bar(dev, model, top):
    """(all inside, the largest error / bar)"""
    bre, bim = augment_bar(model, top)
    d = np.asarray(dev).astype(np.complex128)
    ere, eim = np.abs(d.real - model.real), np.abs(d.imag - model.imag)
    worst = max(float((ere / np.maximum(bre, 1e-300)).max()), float((eim / np.maximum(bim, 1e-300)).max()))
    return bool((ere <= bre).all() and (eim <= bim).all()), worst


def assert_augmented(dev, rxx, mx, my, vx, vy, mask=0, what=""):
    """the device's ra against the restatement fed with the device's own rxx; returns the largest error / bar"""
    ok, worst = within_bar(dev, augment(rxx, mx, my, vx, vy, mask), readable_top(rxx, mx, my, mask))
    assert ok, (what, worst)
    return worst


# ---- the scenes: np.random.default_rng(1000 + seed), seed 0 .. 7, from each generator in order ura.scene(L, SOURCES[:k], rng) for
# k = 1, 2, 3 on the 7 x 3 array ----
@functools.lru_cache(maxsize=None)
def scenes():
    """[(seed, k, block int8 [22][2 L])], 24 of them; shared, never written to"""
    out = []
    for seed in SEEDS:
        rng = np.random.default_rng(1000 + seed)
        for k in (1, 2, 3):
            blk = ura.scene(L, SOURCES[:k], rng)
            blk.setflags(write=False)
            out.append((seed, k, blk))
    return out


def overwrite_absent(block, mask, value=127):
    """a copy of the block with the rows of absent receivers (row 1 + i for element i) full-scale garbage"""
    m = block.shape[0] - 1
    out = np.array(block)
    gone = [1 + i for i in range(m) if i not in present(mask, m)]
    out[gone] = value
    return out


def scene_covariance(block, mask):
    """complex64 covariance of the block with its absent rows overwritten"""
    return smooth_model.covariance(overwrite_absent(block, mask)).astype(np.complex64)


CONFIGS = [  # (name, mask, vx, vy) on the 7 x 3 array
    ("full", 0, 7, 3),
    ("dead {4, 16}", dead(21, (4, 16)), 7, 3),
    ("12 of 21", mask_of(THINNED, 21), 7, 3),
    ("dead {4, 16} -> 5 x 2", dead(21, (4, 16)), 5, 2),
]
