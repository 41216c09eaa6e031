"""fp64 numpy statement of crsdr_caf's bearings (include/crsdr.h, section (w), "Bearings"; crsdr_caf_set_bearing, crsdr_bearing), and
the error bars of the device against it.  caf_model, caf_cfar_model and ura are imported and left as they are: the searched set, the
detector's training set and the array are their own.

Definition.  The rows c != ref_row in ascending order are the elements e = iy mx + ix of an mx x my array, m = nrows - 1.  At the
cell coordinates (x, y): alpha = x pi / ncx, beta = y pi / ncy, a_e = exp(2 pi j d (ix cos(alpha) sin(beta) + iy cos(beta))) with d
the float32 the ABI takes.  For slot q < min(count, K) of the array map's detections, at its cell (d*, tau*):
    u_e = conj(chi_c[d*][tau*])                                     the published fp32 chi promoted to fp64
    W   = I (conventional), or (Q + loading trace(Q) / m I)^-1 with Q = (1 / N) sum_train u_t u_t^H over the detector's training set
          of the cell (caf_cfar_model.train_cell); N = 0 or trace(Q) = 0: W = I and status bit 1
    T(x, y) = |a^H W u|^2 / ((a^H W a)(u^H W u))                    u^H u = 0: T = 0, every figure 0, status bit 0
    (cx, cy) = the first maximum of T over the grid in row-major order; then `levels` levels of doa_refine_model's zoom on f = T.
dir = (cx, cy, T at the grid peak, x - cx, y - cy, alpha, beta, status); spec = T on the grid.

Error bars, derived and not measured (u32 = 2^-24, e = 2^-53).  T <= 1, so the bars on T are absolute.
    steering   a_e is off by at most dphi_e = LIBM (2 pi d e (18 ix + 11 iy) + (11 + 3 m) e) in the complex plane: music_model's phase
               formation with e in place of 2^-24, times LIBM = 4 for the device's libm sincos, as doa_refine_model takes it.
               The perturbation of a has norm at most sqrt(sum dphi_e^2); measured in the W-norm against |a|_W it grows by at most
               sqrt(cond(W)):  eta_a = sqrt(cond) sqrt(mean_e dphi_e^2).  The phases of the polynomial form of a^H W a (below) are formed
               the same way: eta_a is taken twice.
    summation  every entry of N Q is a sum of N products; |dQ_ik| <= (N + 2) e sqrt(Q_ii Q_kk) (Higham (3.5), Cauchy-Schwarz on the
               terms' magnitudes), so |dQ|_F <= (N + 2) e trace(Q), which against lambda_min(Q') >= loading trace(Q) / m is a relative
               perturbation of Q' (as an operator inequality) of (N + 2) e m / loading <= (N + 2) e cond.
    Cholesky   the factor of a complex m x m matrix has backward error |dA| <= gamma |L| |L^H| with gamma <= 3 (m + 1) e, norm
               <= 3 (m + 1) m e |A|_2 (Higham, Theorem 10.3); relative to lambda_min: 3 (m + 1) m e cond.  The columns of L^-1 by
               substitution: column j is exact for L + dL_j, |dL_j| <= 3 m e |L|, which moves W's forms like a perturbation of the
               vectors of relative W-norm 3 m^2 e cond.  Together below 8 m^2 e cond.
    polynomial a^H W a = sum over co-array lags of C[p][q] z, C the sums of W_ef over at most m pairs, W_ef sums of at most m products:
               |d| <= 2 m e sum |W_ef| <= 2 m^2 e lambda_max(W), against a^H W a >= m lambda_min(W): 2 m e cond.  W u and u^H W u:
               sums of m terms, 2 m e cond likewise.  Together below 8 m^2 e cond as well.
               eta_w = e cond (N + 2 + 16 m^2)  with cond = 1 + m / loading;   conventional (and W = I): eta_w = 4 m e.
    T          the squared cosine of the angle between a and u in the W-inner product.  A relative perturbation eta of W moves each of
               the three forms by eta of sqrt(aWa uWu) at most: |dT| <= 4 eta.  A perturbation of a of relative W-norm eta turns the
               angle by at most asin(eta): |dT| <= 2 eta.  One quotient and one product more: 8 e.
                   bar(T) = 4 eta_w + 4 eta_a + 8 e
    figures    cx, cy, the offsets, the status: 0.  T, alpha, beta: one rounding to fp32 more, u32 of the value.
AMBIGUOUS.  Positions are compared exactly.  A grid point (a lattice point of a zoom level) other than the winner is ambiguous when its
T is within the two points' bars of the winner's and differs from it: there, and only there, device and model may name different
positions.  Points whose T equals the winner's bit for bit do not count: they are the same expression of the same operands on both
sides (a line array's map does not depend on one coordinate, whose term is an exact zero; lattice points clamped onto one border
point), and the first-index rule decides them alike."""
import numpy as np

import caf_cfar_model as CF
import caf_model as M
import doa_refine_model as RF
import music_model as mm
import ura  # noqa: F401  (the array of the scenes; D is its spacing)

U, E64 = M.U, M.E64
LIBM = RF.LIBM
CONVENTIONAL, ADAPTIVE = 1, 2
STATUS_ZERO, STATUS_IDENTITY, STATUS_CELL = 1, 2, 4
MUTATIONS = ["no_conj", "ref_counts", "xy_swapped", "guard_trains", "no_denominator", "no_loading", "doppler_nowrap"]


class Desc:
    def __init__(self, mx, my, d, ncx=100, ncy=100, mode=CONVENTIONAL, loading=1e-2, levels=0):
        self.mx, self.my, self.ncx, self.ncy, self.mode, self.levels = int(mx), int(my), int(ncx), int(ncy), int(mode), int(levels)
        self.d, self.loading = float(np.float32(d)), float(np.float32(loading))       # what the device is handed

    @property
    def m(self):
        return self.mx * self.my


def steer(q, xs, ys, which=None):
    """a [P][m] at the cell coordinates"""
    ix, iy = mm.element_index(q.mx, q.my)
    if which == "xy_swapped":
        ix, iy = np.repeat(np.arange(q.mx), q.my), np.tile(np.arange(q.my), q.mx)
    alpha = (np.atleast_1d(np.asarray(xs, dtype=np.float64)) * np.pi / q.ncx)[:, None]
    beta = (np.atleast_1d(np.asarray(ys, dtype=np.float64)) * np.pi / q.ncy)[:, None]
    return np.exp(2j * np.pi * q.d * (ix[None, :] * np.cos(alpha) * np.sin(beta) + iy[None, :] * np.cos(beta)))


def element_rows(nrows, ref, which=None):
    return list(range(nrows - 1)) if which == "ref_counts" else [c for c in range(nrows) if c != ref]


def snapshot(chi32, ref, d, tau, which=None):
    x = np.asarray(chi32)[element_rows(len(chi32), ref, which), d, tau].astype(np.complex128)
    return x if which == "no_conj" else x.conj()


def train_cells(nd, R, guard, prm, d, tau, which=None):
    """the detector's training cells of (d, tau), by caf_cfar_model.train_cell; which: the two mistakes about the set"""
    if which == "guard_trains":
        wide = CF.Params(prm.alpha, gd=-1, gr=-1, td=prm.Hd + 1, tr=prm.Hr + 1)      # nothing is guard, the cell itself included
        return CF.train_cell(np.zeros((nd, R)), guard, wide, d, tau)[2]
    cells = CF.train_cell(np.zeros((nd, R)), guard, prm, d, tau)[2]
    if which == "doppler_nowrap":
        cells = [(dq, tq) for dq, tq in cells if abs(dq - d) <= prm.Hd]
    return cells


def weight(chi32, ref, guard, prm, q, d, tau, which=None):
    """(W [m][m] complex128, N, status, cond bound)"""
    m = q.m
    if q.mode != ADAPTIVE:
        return np.eye(m, dtype=np.complex128), 0, 0, 1.0
    nrows, nd, R = np.asarray(chi32).shape
    cells = train_cells(nd, R, guard, prm, d, tau, which)
    N = len(cells)
    if N == 0:
        return np.eye(m, dtype=np.complex128), 0, STATUS_IDENTITY, 1.0
    Ut = np.stack([snapshot(chi32, ref, dq, tq, which) for dq, tq in cells])     # [N][m]
    Q = Ut.T @ Ut.conj() / N
    tr = float(np.trace(Q).real)
    if not tr > 0.0:
        return np.eye(m, dtype=np.complex128), N, STATUS_IDENTITY, 1.0
    load = 0.0 if which == "no_loading" else q.loading
    Qp = Q + load * (tr / m) * np.eye(m)
    try:
        W = np.linalg.inv(Qp)
    except np.linalg.LinAlgError:                                                # (only the mistake of no loading at N < m comes here)
        W = np.full((m, m), np.nan, dtype=np.complex128)
    return W, N, 0, 1.0 + m / q.loading


def stat(W, u, a, which=None):
    """T [P] of the steering vectors a [P][m]"""
    Wu = W @ u
    num = np.abs(a.conj() @ Wu) ** 2
    uWu = float((u.conj() @ Wu).real)
    aWa = np.full(len(a), float(len(u))) if which == "no_denominator" else np.einsum("pe,ef,pf->p", a.conj(), W, a).real
    return num / (aWa * uWu)


def coefficients(W, mx, my):
    """C [mx][2 my - 1]: the sums of W_ef over the pairs with (fx - ex, fy - ey) = (p, q), p >= 0, q = -(my - 1) .. my - 1"""
    ix, iy = mm.element_index(mx, my)
    C = np.zeros((mx, 2 * my - 1), dtype=np.complex128)
    for e in range(mx * my):
        for f in range(mx * my):
            p, qq = ix[f] - ix[e], iy[f] - iy[e]
            if p >= 0:
                C[p, qq + my - 1] += W[e, f]
    return C


def awa_polynomial(W, q, xs, ys):
    """a^H W a by the co-array polynomial: C[0][0] + 2 Re sum over the half plane of C[p][q] exp(j 2 pi d (p ca sb + q cb))"""
    C = coefficients(W, q.mx, q.my)
    alpha, beta = np.asarray(xs, dtype=np.float64) * np.pi / q.ncx, np.asarray(ys, dtype=np.float64) * np.pi / q.ncy
    kx, ky = np.cos(alpha) * np.sin(beta), np.cos(beta)
    out = np.full(len(alpha), C[0, q.my - 1].real)
    for p in range(q.mx):
        for qq in range(-(q.my - 1), q.my):
            if p > 0 or qq > 0:
                out += 2.0 * (C[p, qq + q.my - 1] * np.exp(2j * np.pi * q.d * (p * kx + qq * ky))).real
    return out


def t_bar(q, N, cond):
    """the absolute bar on T (module docstring)"""
    m = q.m
    ix, iy = mm.element_index(q.mx, q.my)
    dphi = LIBM * (2.0 * np.pi * q.d * E64 * (mm.CX_PHASE * ix + mm.CY_PHASE * iy) + (mm.C_ELEM + 3.0 * m) * E64)
    eta_a = np.sqrt(cond) * np.sqrt(np.mean(dphi ** 2))
    eta_w = E64 * cond * (N + 2 + 16.0 * m * m) if cond > 1.0 else 4.0 * m * E64
    return 4.0 * eta_w + 4.0 * eta_a + 8.0 * E64


def grid_points(q):
    return np.repeat(np.arange(q.ncx), q.ncy).astype(np.float64), np.tile(np.arange(q.ncy), q.ncx).astype(np.float64)


def _rivals(T, w, bar, same):
    """the number of points other than the winner w within the bars of it, equal values and `same` positions apart"""
    near = (T + 2.0 * bar >= T[w]) & (T != T[w]) & ~same
    near[w] = False
    return int(near.sum())


def one(chi32, ref, guard, prm, q, d, tau, which=None):
    """one detection: dict(dir [8] fp64, bar [8], spec [ncx][ncy], tbar, ambiguous, N)"""
    u = snapshot(chi32, ref, d, tau, which)
    if not np.any(u):
        out = np.zeros(8)
        out[7] = STATUS_ZERO
        return dict(dir=out, bar=np.zeros(8), spec=np.zeros((q.ncx, q.ncy)), tbar=0.0, ambiguous=0, N=0)
    W, N, status, cond = weight(chi32, ref, guard, prm, q, d, tau, which)
    bar = t_bar(q, N, cond)
    gx, gy = grid_points(q)
    T = stat(W, u, steer(q, gx, gy, which), which)
    w = int(np.argmax(T))                                                        # (numpy: the first maximum in C order)
    amb = _rivals(T, w, bar, np.zeros(len(T), dtype=bool))
    cx, cy, tg = int(gx[w]), int(gy[w]), float(T[w])
    x, y, s = float(cx), float(cy), 0.5
    for _ in range(q.levels):
        px, py = RF.lattice(x, y, s, q.ncx, q.ncy)
        f = stat(W, u, steer(q, px, py, which), which)
        centre = len(f) // 2
        c = best = f[centre]
        k = centre
        for p in range(len(f)):
            if p != centre and f[p] > c and f[p] > best:
                best, k = f[p], p
        amb += _rivals(f, k, bar, (px == px[k]) & (py == py[k]))
        x, y, s = float(px[k]), float(py[k]), s / 4.0
    fig = np.array([cx, cy, tg, x - cx, y - cy, x * np.pi / q.ncx, y * np.pi / q.ncy, status], dtype=np.float64)
    fb = np.array([0.0, 0.0, bar + U * tg, 0.0, 0.0, U * fig[5], U * fig[6], 0.0])
    return dict(dir=fig, bar=fb, spec=T.reshape(q.ncx, q.ncy), tbar=bar, ambiguous=amb, N=N)


def cell_of(det_row, nd):
    """(d, tau) of a detection's figures"""
    return int(det_row[1]) % nd, int(det_row[0])


def bearing(chi32, det, count, ref, guard, prm, q, which=None):
    """a line: dict(dir [K][8] fp64, bar [K][8], spec [K][ncx][ncy], sbar [K] (the bar on every spec value before its rounding),
    ambiguous, N [K]) from chi [nrows][nd][R] complex64 and the array map's det [K][8] and count"""
    chi32 = np.asarray(chi32)
    nd = chi32.shape[1]
    K = prm.max_det
    out = dict(dir=np.zeros((K, 8)), bar=np.zeros((K, 8)), spec=np.zeros((K, q.ncx, q.ncy)), sbar=np.zeros(K), ambiguous=0, N=np.zeros(K, dtype=np.int64))
    for k in range(min(int(count), K)):
        d, tau = cell_of(np.asarray(det)[k], nd)
        r = one(chi32, ref, guard, prm, q, d, tau, which)
        out["dir"][k], out["bar"][k], out["spec"][k], out["sbar"][k], out["N"][k] = r["dir"], r["bar"], r["spec"], r["tbar"], r["N"]
        out["ambiguous"] += r["ambiguous"]
    return out


def noise_chi(nrows, nd, R, seed, floor=None, scale=1e-3):
    """chi [nrows][nd][R] complex64 of noise, with one spatial signature's floor (floor [nrows]) in every cell where asked for: the
    interference the adaptive mode whitens"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((nrows, nd, R)) + 1j * rng.standard_normal((nrows, nd, R))
    if floor is not None:
        x = x + 3.0 * np.asarray(floor)[:, None, None] * (rng.standard_normal((nd, R)) + 1j * rng.standard_normal((nd, R)))[None]
    return (x * scale).astype(np.complex64)


def plant(chi, ref, q, d, tau, x, y, amp=0.05):
    """a target from the cell coordinates (x, y) in cell (d, tau): chi_c = amp conj(a_e), so that u = amp a; the reference row keeps its value"""
    rows = element_rows(len(chi), ref)
    chi[rows, d, tau] = (amp * steer(q, [x], [y])[0].conj()).astype(np.complex64)
    return chi


def hand_det(cells, nd, K):
    """det [K][8] float32 as the detector lays it out, of which only lag and Doppler are read, for the cells (d, tau) in this order"""
    det = np.zeros((K, 8), dtype=np.float32)
    s = M.signed_bins(nd)
    for k, (d, tau) in enumerate(cells[:K]):
        det[k, 0], det[k, 1], det[k, 2] = tau, s[d], 1.0
    return det


# ---- the scenes of the model test and of the device's end-to-end test ----
ALPHA, CFAR = 8.0, dict(gd=1, gr=1, td=2, tr=3)
# (mx, my, d, nc, B, frames, seg, R, cell, lag, doppler, amp, seed)
SCENES = (
    (3, 2, 0.5, 16, 1024, 2, 16, 16, (5, 9), 5, 3, 0.3, 1),
    (7, 3, float(ura.D), 100, 2048, 2, 32, 24, (31, 62), 7, 5, 0.3, 3),
    (8, 8, 0.5, 32, 2048, 1, 32, 16, (20, 11), 4, -6, 0.3, 4),
)
OFFSETS = ((0.37, -0.29), (-0.45, 0.1), (0.5, 0.5))
# The scenes of the echo OFF the grid.  The first two as above.  The third on a 64 x 64 grid (the same direction: cell (40, 22)): the
# adaptive statistic of 64 elements whose training cells hold the echo's own ambiguity floor is so selective that with the echo 0.4 cell
# off a 32 x 32 grid no grid point lies inside its main lobe -- T is 0.04 at the nearest one and the grid's first maximum is elsewhere
# (this model, 8 x 8 at 32 x 32: 13 cells off).  The scene is changed, not the bound: the grid must sample the adaptive main lobe.
OFF_SCENES = SCENES[:2] + ((8, 8, 0.5, 64, 2048, 1, 32, 16, (40, 22), 4, -6, 0.3, 4),)
WEAK = dict(scene=1, amp=0.05, seeds=(0, 1, 2, 3), alpha=6.0, cfar=dict(gd=1, gr=1, td=3, tr=4), guard=2, loading=1e-2)


def scene_id(sc):
    return f"{sc[0]}x{sc[1]}-{sc[3]}"


def scene_line(sc, off=(0.0, 0.0), amp=None, seed=None, direct=0.8):
    """(line of int8 matrices [1 + m][B], desc, the echo's (x, y)): every element row gets the echo with the complex amplitude
    amp * conj(a(x, y))[e]; row 0 is the reference"""
    mx, my, d, nc, B, frames, seg, R, cell, lag, dop, a0, s0 = sc
    q = Desc(mx, my, d, nc, nc)
    x, y = cell[0] + off[0], cell[1] + off[1]
    a = steer(q, [x], [y])[0]
    amp = a0 if amp is None else amp
    echoes = [(1 + e, lag, dop, amp * np.conj(a[e])) for e in range(q.m)]
    return M.echo_scene(B, frames, echoes, nrows=1 + q.m, ref=0, seed=s0 if seed is None else seed, direct=direct), q, (x, y)


def scene_maps(sc, line):
    """(chi32 [nrows][nd][R] complex64, map32 [nd][R] float32) of a line, as the device publishes them (caf_model.caf_f32)"""
    chi32 = M.caf_f32(line, sc[6], sc[7], 0, M.WINDOW_HANN)
    m64, _ = M.array_map(chi32, 0)
    return np.asarray(chi32), m64.astype(np.float32)
