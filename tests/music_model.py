"""Test helper: the beamformer chain (covariance -> noise subspace -> 2-D MUSIC scan) restated in fp64 numpy, with the bars a correct
fp32 / fp64 implementation has to meet.  Plain numpy, independent of the kernels and of the C oracle; tests/test_music_model.py holds
the C oracle to these bars on the CPU, tests/test_gpu_music_shapes.py the device.

u = 2^-24 is the unit roundoff of fp32 (one rounding to nearest moves a value by at most u of its magnitude).

Subspace bars (subspace_fractions).  The decomposition runs in fp64 and its outputs vec and sv are rounded once to fp32; the reference
is numpy.linalg.eigh of the input promoted to complex128, ordered by |lambda| (what an SVD of a Hermitian matrix returns), lambda_0 the
largest.  With v the fp64 vectors and dv their rounding, |dv_ir| <= u |v_ir|:
  * |V^H V - I|max <= 2^-22.  (V^H V)_rs moves by sum_i (|v_ir| |dv_is| + |dv_ir| |v_is|) <= 2u sum_i |v_ir| |v_is| <= 2u = 2^-23
    (Cauchy-Schwarz, unit columns); the fp64 rotations themselves lose about m * 1e-16.  The bar is twice the rounding term.
  * |sv_r - |lambda_r|| <= 2^-23 |lambda_r| + 1e-12 lambda_0: one rounding (u |lambda_r|, the bar takes 2u) plus the absolute accuracy
    of a backward-stable fp64 eigenvalue solver, a few m * 1.1e-16 * lambda_0 (< 1e-13 lambda_0 at m = 64), taken ten times.
  * |R v_r - sv_r v_r|max <= 2^-22 lambda_0: the fp32 outputs add R dv (<= |R|_2 |dv|_2 <= u lambda_0), sv dv (<= u lambda_0) and
    d(sv) v (<= u lambda_0) to the fp64 residual: 3u < 4u = 2^-22.
  * noise projector P = Un Un^H at an index where the spectrum has a gap: |P - P64|max <= 2^-22 + 1e-13 lambda_0 / gap.  Rounding moves
    P_ik by sum_j (|v_ij| |dv_kj| + |dv_ij| |v_kj|) <= 2u (rows of a unitary matrix have unit norm); the subspace itself is determined
    to backward error / gap (Davis-Kahan), with the backward error of the fp64 iterations below 1e-13 lambda_0 as above.

Scan bar (scan).  den64 is the MUSIC denominator |Un^H a|^2 of the exact steering vector in fp64; the bound is a first-order worst-case
bound on |m / sqrt(pm) - den64| for an fp32 evaluation in the reference's expression order (heatmap2d2.cpp:103-147):
  * pi_f = (float) pi = pi (1 + 0.47u).  alpha = (float)cx * pi_f / (float)Cx: two roundings, |d alpha| <= 2.47u alpha <= 7.76u.
  * cosf / sinf / sincosf results are taken as good to 2 ulp = 4u of the result (the documented bound of the device's math library; a
    correctly rounded libm is inside it).  So ca = cosf(alpha) is off by at most (7.76 |sin alpha| + 4 |cos alpha|) u, likewise sb, cb.
  * px = 2 pi_f ix d ca sb evaluated left to right: 2 pi_f is exact, then four rounded products, (4 + 0.47) u |ca sb| relative to
    2 pi d ix, plus the errors of ca and sb.  Over all angles 7.76 sa sb + 8 ca sb + 7.76 ca cb <= 12.73 and 4.47 ca sb <= 4.47:
    |d px| <= 18u * 2 pi d ix.  py = 2 pi_f iy d cb: three products, (3.47 |cb| + 7.76 |sb| + 4 |cb|) u <= 10.8u: |d py| <= 11u * 2 pi d iy.
    (At ix = 63, d = 0.506: 2.1e-4 rad.)
  * each sincosf result is off by at most 4u in the complex plane, their product by 8u; the complex product itself (two rounded
    products and a sum per component) by 3u.  |e^{jx} - e^{jy}| <= |x - y|, so every term is an absolute error of the element a_i:
    e_i = 2 pi d (18u ix + 11u iy) + 11u.
  * y_j = sum_i conj(u_ij) a_i accumulated in fp32: 2m terms per component summed in sequence, at most 2m u sum_i |u_ij| per component,
    2 sqrt(2) m u < 3m u sum_i |u_ij| in the plane.  Folded into the per-element term: dphi_i = e_i + 3m u,  dy_j = sum_i |u_ij| dphi_i.
  * den = sum_j |y_j|^2: |d den| <= sum_j (2 |y_j| dy_j + dy_j^2) from the y_j, and (nn + 3) u den from the squares and the nn additions.
  * pm = (a2 / den)^2 with a2 = sum_i |a_i|^2 in fp32: |a_i|^2 = 1 within 2 * 11u, m additions and the sum of two squares (m + 2) u;
    the quotient u, the square u, of which the square root keeps half: m / sqrt(pm) = den (1 + (m + 27) u).
  bound = sum_j (2 |y_j| dy_j + dy_j^2) + (nn + m + 30) u den64.
The terms are first order in u; the neglected products of two of them are below 1e-12.  The bound does not depend on which points are
peaks: near a peak den is small and pm ill-conditioned, which is why the comparison is made on den (a device inf is den = 0)."""
import numpy as np

U32 = 2.0 ** -24
CX_PHASE, CY_PHASE, C_ELEM = 18.0, 11.0, 11.0


# ---- covariance --------------------------------------------------------------------------------------------------------------------

def rxx_reference(rows):
    """beamformclient/heatmap2d2.cpp:189-199 in exact integer sums (int8 products summed in float64: |sum| <= 2^14 L, exact far beyond
    any L used) and the fp64 epilogue crsdr_covariance uses: (1/L) sum conj(x_a) x_b - conj(mean_a) mean_b with x = (I + jQ) / 127,
    rounded once to float.  rows [1 + m][2L] int8; row 0 is the reference-noise channel and is left out."""
    x = np.asarray(rows)[1:].astype(np.float64)
    I, Q = x[:, 0::2], x[:, 1::2]
    L = I.shape[1]
    g1 = I @ I.T + Q @ Q.T
    g3, g2 = I @ Q.T, Q @ I.T
    si, sq = I.sum(axis=1), Q.sum(axis=1)
    scale = 1.0 / (127.0 * 127.0)
    re = (g1 / L - (np.outer(si, si) + np.outer(sq, sq)) / (L * L)) * scale
    im = ((g3 - g2) / L - (np.outer(si, sq) - np.outer(sq, si)) / (L * L)) * scale
    return (re + 1j * im).astype(np.complex64)


def rxx_reference_frames(blocks):
    """The same for F stacked frames (X = [X; Xc] of measurement_script.m): blocks [F][1 + m][B] int8 are one record of L = F B / 2
    samples per channel, one mean and one covariance over all of it."""
    blocks = np.asarray(blocks)
    assert blocks.ndim == 3
    return rxx_reference(np.concatenate(list(blocks), axis=1))


# ---- inputs of the decomposition ---------------------------------------------------------------------------------------------------

def hermitian32(R):
    """complex64 matrix that is Hermitian to the bit: the upper triangle of R rounded and mirrored, the diagonal real.  The device
    decomposes the matrix as given, the C oracle its Hermitian part; on such input they mean the same matrix."""
    R = np.asarray(R).astype(np.complex64)
    up = np.triu(R, 1)
    out = up + up.conj().T
    out[np.diag_indices_from(out)] = R.diagonal().real
    return out


FAMILIES = ("wishart", "clustered", "geometric", "rank3", "stairs")


def family(m, name, seed=0):
    """(R, gaps): an m x m test covariance of the named spectrum family as hermitian32, and the indices k (signal dimension) at which the
    spectrum has a gap, the only places where the subspace vec[:, k:] is determined and compared."""
    rng = np.random.default_rng(1000 * m + 17 * FAMILIES.index(name) + seed)
    if name == "wishart":
        g = rng.standard_normal((m, 3 * m)) + 1j * rng.standard_normal((m, 3 * m))
        return hermitian32(g @ g.conj().T / (3 * m)), []
    q = m // 4
    if name == "clustered":
        w = np.concatenate([[1e4, 3e3], np.ones(max(m - 2, 0))])[:m]
        gaps = [g for g in (1, 2) if g < m]
    elif name == "geometric":
        w, gaps = np.logspace(0, -6, m), []
    elif name == "rank3":
        w = np.concatenate([[5.0, 2.0, 1.0], np.zeros(max(m - 3, 0))])[:m]
        gaps = [3] if m > 3 else []
    elif name == "stairs":
        w = np.concatenate([np.full(q, 1e3), np.full(q, 10.0), np.full(m - 2 * q, 1e-2)])
        gaps = [q, 2 * q] if q else []
    else:
        raise ValueError(name)
    z = rng.standard_normal((m, m)) + 1j * rng.standard_normal((m, m))
    Q, _ = np.linalg.qr(z)
    return hermitian32((Q * w[None, :]) @ Q.conj().T), gaps


def eigh_by_magnitude(R):
    """(|lambda| descending, vectors in that order) of the input promoted to complex128."""
    w, V = np.linalg.eigh(np.asarray(R).astype(np.complex128))
    order = np.argsort(-np.abs(w), kind="stable")
    return np.abs(w[order]), V[:, order]


def sv_fraction(sv, lam):
    """worst |sv_r - |lambda_r|| as a fraction of its bar 2^-23 |lambda_r| + 1e-12 lambda_0."""
    sv, lam = np.asarray(sv, dtype=np.float64), np.asarray(lam, dtype=np.float64)
    return float((np.abs(sv - lam) / (2.0 ** -23 * lam + 1e-12 * lam[0] + 1e-300)).max())


def subspace_fractions(R, vec, sv, gaps=()):
    """Each subspace quantity as a fraction of its bar (module docstring): {"orth", "sv", "resid", "proj"}; all must be <= 1."""
    R64 = np.asarray(R).astype(np.complex128)
    V = np.asarray(vec).astype(np.complex128)
    s = np.asarray(sv, dtype=np.float64)
    m = R64.shape[0]
    lam, E = eigh_by_magnitude(R64)
    lam0 = max(lam[0], 1e-300)
    out = {"orth": float(np.abs(V.conj().T @ V - np.eye(m)).max() / 2.0 ** -22),
           "sv": sv_fraction(s, lam) if lam[0] > 0 else float(np.abs(s).max() > 0),
           "resid": float(np.abs(R64 @ V - V * s[None, :]).max() / (2.0 ** -22 * lam0)),
           "proj": 0.0}
    for k in gaps:
        gap = lam[k - 1] - lam[k]
        P, P64 = V[:, k:] @ V[:, k:].conj().T, E[:, k:] @ E[:, k:].conj().T
        out["proj"] = max(out["proj"], float(np.abs(P - P64).max() / (2.0 ** -22 + 1e-13 * lam0 / gap)))
    return out


# ---- scan --------------------------------------------------------------------------------------------------------------------------

def element_index(mx, my):
    """(ix, iy) of the array element stored at index iy*mx + ix (s_vecd2d, heatmap2d2.cpp:103-115)."""
    return np.tile(np.arange(mx), my), np.repeat(np.arange(my), mx)


def _y(vec, k, d, mx, my, ncx, ncy, order="row", col0=None, sign_y=1.0):
    """y [ncx][ncy][nn] = Un^H a in fp64 on the grid alpha = cx pi / ncx, beta = cy pi / ncy.  The keyword arguments are the places an
    implementation can get wrong (the mutants of tests/test_music_model.py); the defaults are the definition."""
    v = np.asarray(vec).astype(np.complex128)
    m = mx * my
    assert v.shape == (m, m)
    ix, iy = element_index(mx, my) if order == "row" else (np.repeat(np.arange(mx), my), np.tile(np.arange(my), mx))
    nn = m - k
    if col0 is None or col0 == k:
        un = v[:, k:]
    else:                                       # nn columns from col0 of the row-major matrix, as a kernel with a wrong offset reads them
        flat = np.concatenate([v.reshape(-1), np.zeros(m, dtype=np.complex128)])
        un = np.stack([flat[i * m + col0: i * m + col0 + nn] for i in range(m)])
    alpha = (np.arange(ncx) * np.pi / ncx)[:, None]
    beta = (np.arange(ncy) * np.pi / ncy)[None, :]
    px = (np.cos(alpha) * np.sin(beta))[:, :, None] * ix[None, None, :]
    py = (np.cos(beta) * np.ones_like(alpha))[:, :, None] * iy[None, None, :]
    a = np.exp(2j * np.pi * float(np.float32(d)) * (px + sign_y * py))
    return a @ un.conj(), un


def scan(vec, k, d, mx, my, ncx, ncy):
    """(den64 [ncx][ncy], bound [ncx][ncy]): den64[cx, cy] = sum_j |sum_i conj(u_ij) a_i|^2 of the given fp32 vec in fp64, and the
    absolute bound on |m / sqrt(pm) - den64| for an fp32 scan (module docstring)."""
    m = mx * my
    nn = m - k
    y, un = _y(vec, k, d, mx, my, ncx, ncy)
    den = (np.abs(y) ** 2).sum(axis=2)
    ix, iy = element_index(mx, my)
    dphi = 2.0 * np.pi * float(np.float32(d)) * U32 * (CX_PHASE * ix + CY_PHASE * iy) + (C_ELEM + 3.0 * m) * U32
    dy = np.abs(un).T @ dphi                                                      # [nn]
    bound = (2.0 * np.abs(y) * dy[None, None, :] + (dy ** 2)[None, None, :]).sum(axis=2) + (nn + m + 30) * U32 * den
    return den, bound


def den_of(pm, m):
    """The denominator an fp32 spectrum stands for: pm = (a2 / den)^2 with a2 = m.  inf -> 0."""
    with np.errstate(divide="ignore"):
        return m / np.sqrt(np.asarray(pm, dtype=np.float64))


def scan_fractions(pm, m, den64, bound):
    """(worst |m / sqrt(pm) - den64| / bound over the grid, median |m / sqrt(pm) - den64| / den64).  A NaN counts as infinitely wrong."""
    err = np.abs(den_of(pm, m) - den64)
    err = np.where(np.isnan(err), np.inf, err)
    return float((err / bound).max()), float(np.median(err / den64))


def admissible_peak(den64, bound, peak):
    """True when an fp32 scan within the bound can have its maximum of pm (minimum of den) at `peak` (cx, cy): the least den the point
    can have is not above the largest den of every point.  Ties (a line array is mirror-symmetric in beta) are admissible on both sides."""
    p = tuple(int(v) for v in peak)
    return bool(den64[p] - bound[p] <= (den64 + bound).min())


def certain_peak(den64, bound):
    """The grid point every fp32 scan within the bound must report, or None: its largest possible den is below the least possible den
    of every other point."""
    p = np.unravel_index(np.argmin(den64), den64.shape)
    others = (den64 - bound).copy()
    others[p] = np.inf
    return tuple(int(v) for v in p) if den64[p] + bound[p] < others.min() else None


def mirrored_source(cx, cy, ncx, ncy):
    """(alpha, beta) of the far-field source whose MUSIC peak sits on grid point (cx, cy): Rxx = X^H X of heatmap2d2.cpp:197 has
    conj(a) as its principal vector, so the peak is at (pi - alpha, pi - beta)."""
    return np.pi - cx * np.pi / ncx, np.pi - cy * np.pi / ncy


# ---- the shapes both test modules run ------------------------------------------------------------------------------------------------

_SPOTS = ((0.3, 0.4), (0.7, 0.65), (0.5, 0.25), (0.15, 0.75), (0.85, 0.5))


def scan_case(mx, my, k, ncx, ncy, nsrc=None, find=True, flat=False):
    nsrc = k if nsrc is None else nsrc
    src = [(int(round(fx * ncx)) % ncx, int(round(fy * ncy)) % ncy) for fx, fy in _SPOTS[:nsrc]]
    return dict(mx=mx, my=my, k=k, ncx=ncx, ncy=ncy, src=src, find=find, flat=flat)


# find: the array resolves both angles and the scene has k sources, so the fp64 minimum of den must be one of them.  Not so for a line
# array (a whole curve of the grid shares the steering vector), for m = 2, and for k above the number of sources in the scene (a
# one-column noise subspace has nulls of its own).
SCAN_CASES = (
    scan_case(2, 1, 1, 24, 36, find=False),
    scan_case(1, 2, 1, 33, 17, find=False),
    scan_case(4, 2, 3, 30, 20),
    scan_case(7, 3, 2, 100, 100),
    scan_case(3, 7, 2, 24, 36),
    scan_case(11, 3, 2, 33, 17),
    scan_case(16, 4, 5, 30, 20),
    scan_case(8, 8, 1, 24, 36),
    scan_case(8, 8, 4, 33, 17),
    scan_case(8, 8, 63, 30, 20, nsrc=2, find=False),
    scan_case(7, 3, 20, 24, 36, nsrc=2, find=False),
    scan_case(64, 1, 1, 33, 17, find=False),
    scan_case(1, 64, 1, 30, 20, find=False),
    scan_case(11, 3, 1, 1, 50),
    # beta = 0 on the whole grid: sin(beta) = 0 and every point has the same steering vector, so there is no peak to locate; the value
    # itself still depends on the element order, the columns and the sign (every mutant but none of the grid's shows on it)
    scan_case(3, 7, 1, 50, 1, find=False, flat=True),
)


def case_id(c):
    return f"{c['mx']}x{c['my']}-k{c['k']}-{c['ncx']}x{c['ncy']}"


def case_scene(c, L=2048, frames=1, seed=0):
    """int8 blocks [frames][1 + m][2L] of the array of case c looking at sources whose peaks sit on the grid points c['src']."""
    import ura
    rng = np.random.default_rng(7919 * c["mx"] + 131 * c["my"] + 17 * c["k"] + c["ncx"] + seed)
    sources = [(*mirrored_source(cx, cy, c["ncx"], c["ncy"]), 1.0) for cx, cy in c["src"]]
    return np.stack([ura.scene(L, sources, rng, mx=c["mx"], my=c["my"]) for _ in range(frames)])
