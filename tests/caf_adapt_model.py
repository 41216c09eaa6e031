"""fp64 numpy statement of crsdr_caf's adaptive beams (include/crsdr.h, section (w), "Adaptive beams"; crsdr_caf_set_beam_adapt,
crsdr_beam_adapt), and the error bars of the device against it.  caf_model, caf_bearing_model and caf_beams_model are imported and left
as they are: the maps, the steering expression, the beam maps and their detector are their own.

Definition.  Elements e = 0 .. m - 1 are the rows c != ref_row, ascending.  Training cells: Doppler (d_lo + a) mod nd, a < d_n; lags
r_lo + b, b < r_n; N = d_n r_n.  u_e = conj(chi_c(e)[cell]) of the published float32 chi, promoted to fp64.
    Q = (1 / N) sum u u^H       Q' = Q + loading (trace(Q) / m) I       g = Q'^-1 v_b (numpy.linalg.solve)
    w_b = (v_b^H v_b / v_b^H g) g       aw = w as float32       ainfo = (w^H Q w, v^H Q v) as float32
A beam with v = 0 keeps it.  Fallback (aw = v, ainfo = 0): trace(Q) == 0: status 1; trace(Q) not finite: status 2.

Error bars, derived and not measured (U = 2^-24, E = 2^-53).
    Q      every product of two fp32 values is exact in fp64 (48-bit product), so whatever the order -- tiles, matrix instructions,
           trees -- an entry is a sum of 2 N exact terms (4 N off the diagonal) with at most N + 1 roundings on any term's way, one more
           for the division by N.  Every partial sum of |terms| of entry (i, j) is at most N sqrt(Q_ii Q_jj) by Cauchy-Schwarz, hence
               |dQ_ij| <= (N + 2) E sqrt(Q_ii Q_jj)                                   (the sum bar)
    w      kappa = cond(Q') <= (tr Q + delta) / delta <= 1 + m / loading, delta = loading tr Q / m, since Q is positive semidefinite
           with lambda_max <= tr Q.  The device solves (Q' + dA) g = v exactly, where dA collects the sum bar, ||dQ||_F <= (N + 2) E tr Q
           <= (N + 2) m E ||Q'||_2 (||Q'||_2 >= tr Q' / m), the rounding of the loading (3 E), and the Cholesky factor with its two
           triangular products, backward stable with ||dA|| <= 4 m (3 m + 1) E ||Q'||_2 (Higham, Theorem 10.4 with the constant of
           caf_cancel_model).  eps_b = ((N + 2) m + 4 m (3 m + 1) + 8 m) E.  Then ||dg|| <= kappa eps_b ||g||, and with
           den = v^H g = g^H Q' g >= lambda_min ||g||^2:  |d den| = |g^H dA g| <= kappa eps_b den.  w = (v^H v / den) g:
               ||dw||_2 <= 2 kappa eps_b ||w||_2 = dwn        per part of aw:  bar_w = dwn + U |w_e| + 2^-149
           (U |w_e|: half an ulp of fp32; the numpy solve of this model has the same bound and is counted in the factor 2 -> 4.)
    ainfo  p = x^H Q x.  From dx: 2 sqrt(p tr Q) ||dx|| + tr Q ||dx||^2; from dQ: (N + 2) E tr Q ||x||^2; from the 2 m^2 additions of
           the form: 4 m E tr Q ||x||^2; one rounding to fp32.  x = w: ||dx|| = dwn; x = v: 0.
    mean   the mean of the published bmap over the training cells against ainfo[0]: bmap is formed with aw = w + dw32,
           ||dw32|| <= U ||w|| + dwn, so its exact mean is (w + dw32)^H Q (w + dw32): 2 sqrt(p tr Q) ||dw32|| + tr Q ||dw32||^2, plus the
           mean of caf_beams_model's bars on bmap, plus the bar on ainfo[0], plus N E of the mean's own sum.
MUTATIONS: eight single mistakes, each of which must miss a bar or change the scene's outcome (test_caf_adapt_model.py)."""
import numpy as np

import caf_bearing_model as BM
import caf_beams_model as B
import caf_cfar_model as CF
import caf_model as M

U, E64 = M.U, M.E64
TINY = 2.0 ** -149
STATUS_ZERO, STATUS_SOLVE = 1, 2
CHUNK, MAX_TILES = 64, 64
MUTATIONS = ["no_conj", "q_transposed", "absolute_loading", "unscaled", "doppler_nowrap", "lag_short", "ref_counts", "last_tile_dropped"]


class Desc:
    def __init__(self, loading, d_lo, d_n, r_lo, r_n):
        self.loading, self.d_lo, self.d_n, self.r_lo, self.r_n = float(np.float32(loading)), int(d_lo), int(d_n), int(r_lo), int(r_n)

    @property
    def N(self):
        return self.d_n * self.r_n


def whole(nd, R, loading=1e-2, guard=None):
    """the whole map, or the whole map less the zero-Doppler guard"""
    return Desc(loading, 0, nd, 0, R) if guard is None else Desc(loading, guard + 1, nd - 2 * guard - 1, 0, R)


def tile_cells(N):
    chunks = (N + CHUNK - 1) // CHUNK
    return ((chunks + MAX_TILES - 1) // MAX_TILES) * CHUNK


def tiles_of(N):
    return (N + tile_cells(N) - 1) // tile_cells(N)


def train_cells(q, nd, R, which=None):
    """[(d, tau)] in the order t = a r_n + b"""
    cells = []
    for a in range(q.d_n):
        d = q.d_lo + a
        if which == "doppler_nowrap":
            if d >= nd:
                continue
        else:
            d %= nd
        for b in range(q.r_n - 1 if which == "lag_short" else q.r_n):
            cells.append((d, q.r_lo + b))
    if which == "last_tile_dropped" and tiles_of(q.N) > 1:
        cells = cells[:(tiles_of(q.N) - 1) * tile_cells(q.N)]
    return cells


def snapshots(chi32, ref, q, which=None):
    """u [N][m] complex128"""
    chi32 = np.asarray(chi32)
    nrows, nd, R = chi32.shape
    cells = train_cells(q, nd, R, which)
    x = chi32[BM.element_rows(nrows, ref, which)].astype(np.complex128)
    u = np.stack([x[:, d, t] for d, t in cells]) if cells else np.zeros((0, nrows - 1), dtype=np.complex128)
    return u if which == "no_conj" else u.conj()


def covariance(chi32, ref, q, which=None):
    """(Q [m][m] complex128, its sum bar [m][m]): Q = (1 / N) sum u u^H over the declared N"""
    u = snapshots(chi32, ref, q, which)
    with np.errstate(all="ignore"):
        Q = np.einsum("ti,tj->ij", u, u.conj()) / q.N
        if which == "q_transposed":
            Q = Q.T
        dg = np.abs(np.diag(Q).real)
        return Q, (q.N + 2) * E64 * np.sqrt(np.outer(dg, dg))


def covariance_by_cells(chi32, ref, q):
    """the same by a cell-by-cell enumeration with Python integers for the indices"""
    chi32 = np.asarray(chi32)
    nrows, nd, R = chi32.shape
    rows = [c for c in range(nrows) if c != ref]
    Q = np.zeros((len(rows), len(rows)), dtype=np.complex128)
    for t in range(q.d_n * q.r_n):
        a, b = divmod(t, q.r_n)
        d, tau = (q.d_lo + a) % nd, q.r_lo + b
        u = np.array([np.conj(complex(chi32[c, d, tau])) for c in rows])
        Q += np.outer(u, u.conj())
    return Q / (q.d_n * q.r_n)


def kappa_bound(m, q):
    return 1.0 + m / q.loading


def eps_b(m, N):
    return ((N + 2) * m + 4 * m * (3 * m + 1) + 8 * m) * E64


def adapt(chi32, ref, V, q, which=None):
    """a line: dict(w [nb][m] complex128, wbar [nb][m] per part, dwn [nb], info [nb][2] fp64, ibar [nb][2], status, Q, qbar, Ql)"""
    V = np.asarray(V).astype(np.complex64).astype(np.complex128)
    nb, m = V.shape
    Q, qbar = covariance(chi32, ref, q, which)
    tr = float(np.trace(Q).real)
    out = dict(Q=Q, qbar=qbar, status=0, w=V.copy(), wbar=np.zeros((nb, m)), dwn=np.zeros(nb), info=np.zeros((nb, 2)), ibar=np.zeros((nb, 2)), Ql=None)
    if tr == 0.0:
        out["status"] = STATUS_ZERO
        return out
    if not np.isfinite(tr) or not np.all(np.isfinite(Q)):
        out["status"] = STATUS_SOLVE
        return out
    delta = q.loading if which == "absolute_loading" else q.loading * tr / m
    Ql = Q + delta * np.eye(m)
    out["Ql"] = Ql
    k = kappa_bound(m, q)
    for b in range(nb):
        v = V[b]
        vv = float(np.vdot(v, v).real)
        if vv == 0.0:
            continue
        g = np.linalg.solve(Ql, v)
        den = float(np.vdot(v, g).real)
        w = g if which == "unscaled" else (vv / den) * g
        wn = float(np.linalg.norm(w))
        dwn = 4.0 * k * eps_b(m, q.N) * wn
        out["w"][b], out["dwn"][b] = w, dwn
        out["wbar"][b] = dwn + U * np.maximum(np.abs(w.real), np.abs(w.imag)) + TINY
        for j, (x, dx) in enumerate(((w, dwn), (v, 0.0))):
            p = float(np.vdot(x, Q @ x).real)
            xn2 = float(np.vdot(x, x).real)
            d = 2.0 * np.sqrt(max(p, 0.0) * tr) * dx + tr * dx * dx + (q.N + 2 + 4 * m) * E64 * tr * xn2
            out["info"][b, j], out["ibar"][b, j] = p, d + U * (p + d) + TINY
    return out


def mean_bar(chi32, ref, r, b, q):
    """the bar of (mean of the published bmap of beam b over the training cells) against ainfo[b][0], aw32 the published weights"""
    w = r["w"][b]
    aw32 = w.astype(np.complex64)
    _, pbar = B.bmap(chi32, ref, aw32[None])
    nd, R = np.asarray(chi32).shape[1:]
    cells = train_cells(q, nd, R)
    mb = float(np.mean([pbar[0, d, t] for d, t in cells]))
    tr, p = float(np.trace(r["Q"]).real), r["info"][b, 0]
    d32 = U * float(np.linalg.norm(w)) * np.sqrt(2.0) + r["dwn"][b]
    return 2.0 * np.sqrt(max(p, 0.0) * tr) * d32 + tr * d32 * d32 + mb + r["ibar"][b, 0] + q.N * E64 * (p + mb) + U * p


def beam_mean(bmap_b, q):
    nd, R = bmap_b.shape
    return float(np.mean([float(bmap_b[d, t]) for d, t in train_cells(q, nd, R)]))


# ---- the scene of the model test and of the device's end-to-end test ----
# caf_bearing_model.SCENES[1]'s array (7 x 3, 22 rows, B 2048, 2 frames, seg 32, 24 lags, nd 64, Hann).  The direct path arrives in every
# signal row from grid cell DIRECT at lag 0, Doppler 0, at amplitude `direct`; its ambiguity floor covers the whole map.  The echo
# comes from SCENES[1]'s cell (31, 62) at lag 7, Doppler 5.  The bank is caf_beams_model's 8 x 8 lattice; the beam nearest the echo is 20.
SCENE = dict(scene=1, direct_cell=(45.0, 62.0), direct=0.8, amp=0.004, seed=5, alpha=50.0, cfar=dict(gd=1, gr=1, td=3, tr=4), guard=2, max_det=16,
             loading=1e-2, beam=20)


def scene_line():
    """(line of int8 matrices, chi32, desc of the array, weights [64][21], the echo's (lag, doppler))"""
    sc = BM.SCENES[SCENE["scene"]]
    mx, my, d, nc, Bs, frames, seg, R, cell, lag, dop, _, _ = sc
    qa = BM.Desc(mx, my, d, nc, nc)
    a_echo = BM.steer(qa, [cell[0]], [cell[1]])[0]
    a_dir = BM.steer(qa, [SCENE["direct_cell"][0]], [SCENE["direct_cell"][1]])[0]
    echoes = [(1 + e, 0, 0, SCENE["direct"] * np.conj(a_dir[e])) for e in range(qa.m)] + [(1 + e, lag, dop, SCENE["amp"] * np.conj(a_echo[e])) for e in range(qa.m)]
    line = M.echo_scene(Bs, frames, echoes, nrows=1 + qa.m, ref=0, seed=SCENE["seed"], direct=0.0)
    chi32, _ = BM.scene_maps(sc, line)
    return line, chi32, qa, B.steer_weights(qa, B.lattice(8, 8, nc)), (lag, dop)


def scene_ratios(P, cell):
    """per beam the largest (cell / the detector's noise estimate) in dB over the cells within one cell of `cell` = (d, tau), and at it"""
    nd, R = P.shape[1:]
    d0, t0 = cell
    near = [((d0 + a) % nd, t0 + b) for a in (-1, 0, 1) for b in (-1, 0, 1) if 0 <= t0 + b < R]
    out = np.zeros((len(P), 2))
    with np.errstate(divide="ignore"):
        for b in range(len(P)):
            _, noise, _, _ = CF.threshold(P[b].astype(np.float64), SCENE["guard"], scene_params())
            out[b] = 10.0 * np.log10(max(P[b][c] / noise[c] for c in near)), 10.0 * np.log10(P[b][d0 % nd, t0] / noise[d0 % nd, t0])
    return out


def scene_params():
    return CF.Params(alpha=SCENE["alpha"], min_train=1, max_det=SCENE["max_det"], **SCENE["cfar"])


def scene_fused(chi32, W, which=None, adaptive=True):
    """(fused, nfused, bmap fp64, ambiguous, the model's dict or None) of the scene's line with the caller's weights or the adaptive ones"""
    nd, R = chi32.shape[1:]
    r = None
    if adaptive:
        r = adapt(chi32, 0, W, whole(nd, R, SCENE["loading"], SCENE["guard"]), which)
        W = r["w"].astype(np.complex64)
    ln = B.line(chi32, 0, W, SCENE["guard"], scene_params())
    return ln["fused"], ln["nfused"], ln, r
