"""fp64 numpy model of the gridless directions (include/crsdr.h: crsdr_doa_set_esprit, crsdr_esprit2d): 2-D ESPRIT on the signal
subspace of a uniform rectangular array.

The definition, per matrix (vec [M][M] complex64 as published, column r = v_r; sv [M]; k sources; the array sx x sy, element
i = iy sx + ix; d).  All arithmetic in fp64:
    E = vec[:, :k];  E1x / E2x = the rows with ix <= sx-2 / ix >= 1 (paired (ix, iy) -> (ix+1, iy)), E1y / E2y likewise along y
    Gx = E1x^H E1x, Hx = E1x^H E2x, Psi_x = Gx^-1 Hx (Cholesky);  Psi_y likewise
    Psi_c = Psi_x + gamma Psi_y, gamma = (1 + j) / 2;  Psi_c V = V diag(w)
    lambda_x_i = (V^-1 Psi_x V)_ii, lambda_y_i = (V^-1 Psi_y V)_ii;  mu_i = arg lambda_x_i, nu_i = arg lambda_y_i
    cb = nu / (2 pi d), clamped to [-1, 1] (flag bit 0);  sb = sqrt(1 - cb^2);  ca = sb > 0 ? mu / (2 pi d sb) : 0, clamped (flag bit 1,
    also when sb == 0);  beta = acos(cb), alpha = acos(ca)
    power_i = sum_r sv[r] |v_r^H a_i|^2 / M^2, a_i the steering vector at (alpha_i, beta_i)
    slots by descending power, then ascending mu, then nu
    found = k; 0 with status 0 when sv[0] == 0, with status bit 1 when a Cholesky pivot is <= 2^-40, with status bit 0 when the
    eigenvalue iteration did not finish within 40 k steps.  Empty slots: phases (0, 0), angles (-1, -1), modulus (-1, -1), power -1, flags 0.

Two routes to V.  "eig": numpy's.  "qr": the device's own algorithm (Householder reduction to Hessenberg form, explicit shifted QR
steps with Givens rotations and Wilkinson's shift, deflation from the bottom, the eigenvectors of the triangular factor by back
substitution, lambda_i as the i-th entry of the solution of Y z = (Q^H Psi Q) y_i).  The diagonal of V^-1 Psi V does not depend on the
order or the scaling of V's columns, so the two agree to rounding where the w_i are distinct.

`dtype` runs the whole chain in another precision (complex64: what fp32 arithmetic would give); `mistake` plants one single error.

The bar.  BAR = 1e-11 rad on mu and nu between two fp64 evaluations from the same fp32 vec, for scenes with cond(Gx), cond(Gy) <= 4,
cond(V) <= 4 (unit-norm columns) and min |w_i - w_j| >= 0.1: the two routes here disagree by some 1e-15 on such scenes and a complex64
run errs by 1e-8 and more, the bar sits between.  DIRECTION_BAR = pi / 100: one cell of a 100 x 100 grid, for the estimated against the
true (mirrored) direction on arrays >= 7 x 3 with L >= 2048."""
import numpy as np

import ura

BAR = 1e-11
DIRECTION_BAR = np.pi / 100
GAMMA = 0.5 + 0.5j
PIVOT_MIN = 2.0 ** -40
MAX_K = 16
MISTAKES = ("no_inverse", "gamma_zero", "wrong_slot", "exchanged", "conjugate")


def selections(sx, sy):
    """element indices of (E1x, E2x, E1y, E2y)"""
    ix, iy = np.tile(np.arange(sx), sy), np.repeat(np.arange(sy), sx)
    i = np.arange(sx * sy)
    return i[ix <= sx - 2], i[ix >= 1], i[iy <= sy - 2], i[iy >= 1]


def rank_limit(sx, sy):
    return min((sx - 1) * sy, sx * (sy - 1), MAX_K)


def _cholesky_solve(G, H):
    """(G^-1 H, smallest pivot): the pivot is the diagonal entry a column starts from, before its square root"""
    k = G.shape[0]
    L = np.zeros_like(G)
    worst = np.inf
    for j in range(k):
        p = (G[j, j] - np.sum(L[j, :j] * L[j, :j].conj())).real
        worst = min(worst, float(p))
        if not p > PIVOT_MIN:
            return None, worst
        L[j, j] = np.sqrt(p)
        for i in range(j + 1, k):
            L[i, j] = (G[i, j] - np.sum(L[i, :j] * L[j, :j].conj())) / L[j, j]
    Y = np.zeros_like(H)
    for i in range(k):
        Y[i] = (H[i] - L[i, :i] @ Y[:i]) / L[i, i]
    X = np.zeros_like(H)
    for i in range(k - 1, -1, -1):
        X[i] = (Y[i] - L[i + 1:, i].conj() @ X[i + 1:]) / L[i, i]
    return X, worst


def _givens(a, b):
    """(c, s) with [[c, s], [-conj(s), c]] (a, b)^T = (r, 0)^T, c real"""
    na, nb = abs(a), abs(b)
    if nb == 0:
        return 1.0, 0.0 * b
    if na == 0:
        return 0.0, b.conj() / nb
    r = np.hypot(na, nb)
    return na / r, (a / na) * b.conj() / r


def schur_qr(A, max_steps):
    """(T, Q, steps) with A = Q T Q^H, T upper triangular; None in T's place if max_steps QR steps were not enough"""
    cx, rl = A.dtype.type, A.real.dtype.type
    k = A.shape[0]
    T, Q = A.copy(), np.eye(k, dtype=A.dtype)
    eps = np.finfo(rl).eps
    for j in range(k - 2):                                  # Householder: column j below the subdiagonal
        x = T[j + 1:, j].copy()
        if not np.any(x[1:] != 0):
            continue
        nx = np.sqrt(np.sum(np.abs(x) ** 2))
        ph = x[0] / abs(x[0]) if x[0] != 0 else cx(1)
        v = x.copy()
        v[0] += ph * nx
        v /= np.sqrt(np.sum(np.abs(v) ** 2))
        T[j + 1:, :] -= 2 * np.outer(v, v.conj() @ T[j + 1:, :])
        T[:, j + 1:] -= 2 * np.outer(T[:, j + 1:] @ v, v.conj())
        Q[:, j + 1:] -= 2 * np.outer(Q[:, j + 1:] @ v, v.conj())
        T[j + 2:, j] = 0
    n, steps = k, 0
    while n > 1:
        if abs(T[n - 1, n - 2]) <= eps * (abs(T[n - 2, n - 2]) + abs(T[n - 1, n - 1])):
            T[n - 1, n - 2] = 0
            n -= 1
            continue
        if steps >= max_steps:
            return None, Q, steps
        steps += 1
        a, b, c, dd = T[n - 2, n - 2], T[n - 2, n - 1], T[n - 1, n - 2], T[n - 1, n - 1]
        # Wilkinson: the eigenvalue of the trailing 2 x 2 block nearer to its last entry
        h = (a - dd) / 2
        root = np.sqrt(h * h + b * c)
        den = h + root if abs(h + root) >= abs(h - root) else h - root
        sigma = dd - (b * c / den if den != 0 else cx(0))
        rot = []
        for i in range(n):
            T[i, i] -= sigma
        for i in range(n - 1):                               # R = G_{n-2} .. G_0 (T - sigma)
            c_, s_ = _givens(T[i, i], T[i + 1, i])
            rot.append((c_, s_))
            ri, rj = T[i, i:].copy(), T[i + 1, i:].copy()
            T[i, i:] = c_ * ri + s_ * rj
            T[i + 1, i:] = -np.conj(s_) * ri + c_ * rj
            T[i + 1, i] = 0
        for i, (c_, s_) in enumerate(rot):                   # R G_0^H .. G_{n-2}^H, and Q likewise
            for Mx, rows in ((T, min(i + 2, n)), (Q, k)):
                ci, cj = Mx[:rows, i].copy(), Mx[:rows, i + 1].copy()
                Mx[:rows, i] = c_ * ci + np.conj(s_) * cj
                Mx[:rows, i + 1] = -s_ * ci + c_ * cj
        for i in range(n):
            T[i, i] += sigma
    return T, Q, steps


def triangular_vectors(T):
    """Y unit upper triangular with T Y = Y diag(T)"""
    k = T.shape[0]
    Y = np.eye(k, dtype=T.dtype)
    tiny = np.finfo(T.real.dtype).tiny
    for i in range(k):
        for j in range(i - 1, -1, -1):
            den = T[j, j] - T[i, i]
            if den == 0:
                den = T.dtype.type(tiny)
            Y[j, i] = -(T[j, j + 1:i + 1] @ Y[j + 1:i + 1, i]) / den
    return Y


def _diag_qr(T, Q, Y, Psi):
    """diag(V^-1 Psi V) for V = Q Y: entry i of the solution z of Y z = (Q^H Psi Q) y_i"""
    k = T.shape[0]
    S = Q.conj().T @ Psi @ Q
    out = np.zeros(k, dtype=T.dtype)
    for i in range(k):
        u = S @ Y[:, i]
        z = u.copy()
        for p in range(k - 1, i - 1, -1):
            z[p] = u[p] - Y[p, p + 1:] @ z[p + 1:]
        out[i] = z[i]
    return out


def _empty(slots):
    return dict(found=0, status=0, phases=np.zeros((slots, 2)), angles=np.full((slots, 2), -1.0, dtype=np.float32),
                modulus=np.full((slots, 2), -1.0, dtype=np.float32), power=np.full(slots, -1.0, dtype=np.float32), flags=np.zeros(slots, dtype=np.int32),
                mu=np.zeros(0), nu=np.zeros(0))


def esprit(vec, sv, k, d, sx, sy, route="eig", dtype=np.complex128, mistake=None, slots=None):
    """The definition on one matrix.  phases [slots][2] float64, angles and modulus [slots][2] float32, power [slots] float32, flags
    [slots] int32, found, status; with them cond_gx, cond_gy, cond_v, gap (the scene's conditioning) and steps (route "qr")."""
    rl = np.float64 if dtype == np.complex128 else np.float32
    slots = k if slots is None else slots
    vec = np.asarray(vec, dtype=np.complex64)
    sv = np.asarray(sv, dtype=np.float32)
    M = sx * sy
    out = _empty(slots)
    if sv[0] == 0:
        return out
    E = vec[:, :k].astype(dtype)
    s1x, s2x, s1y, s2y = selections(sx, sy)
    if mistake == "exchanged":
        s1x, s2x, s1y, s2y = s2x, s1x, s2y, s1y
    psi, conds = [], []
    for s1, s2 in ((s1x, s2x), (s1y, s2y)):
        G, H = E[s1].conj().T @ E[s1], E[s1].conj().T @ E[s2]
        if mistake == "conjugate":
            H = H.conj()
        conds.append(float(np.linalg.cond(G.astype(np.complex128))))
        X, pivot = _cholesky_solve(G, H)
        if X is None:
            out["status"] = 2
            return out
        psi.append(H if mistake == "no_inverse" else X)
    px, py = psi
    pc = px + dtype(0 if mistake == "gamma_zero" else GAMMA) * py
    steps = 0
    if route == "eig":
        w, V = np.linalg.eig(pc)
        Vi = np.linalg.inv(V)
        lx, ly = np.diag(Vi @ px @ V), np.diag(Vi @ py @ V)
    else:
        T, Q, steps = schur_qr(pc, 40 * k)
        if T is None:
            out["status"] = 1
            return out
        Y = triangular_vectors(T)
        V, w = Q @ Y, np.diag(T).copy()
        lx, ly = _diag_qr(T, Q, Y, px), _diag_qr(T, Q, Y, py)
    if mistake == "wrong_slot":
        ly = np.roll(ly, 1)
    lx, ly = lx.astype(np.complex128), ly.astype(np.complex128)
    mu, nu = np.arctan2(lx.imag, lx.real), np.arctan2(ly.imag, ly.real)
    if rl is np.float32:
        mu, nu = mu.astype(np.float32).astype(np.float64), nu.astype(np.float32).astype(np.float64)
    # the angles in the scan's convention
    two_pi_d = 2.0 * np.pi * float(np.float32(d))
    flags = np.zeros(k, dtype=np.int32)
    cb = nu / two_pi_d
    flags[np.abs(cb) > 1] |= 1
    cb = np.clip(cb, -1.0, 1.0)
    sb = np.sqrt(1.0 - cb * cb)
    ca = np.where(sb > 0, mu / (two_pi_d * np.where(sb > 0, sb, 1.0)), 0.0)
    flags[(sb == 0) | (np.abs(ca) > 1)] |= 2
    ca = np.clip(ca, -1.0, 1.0)
    alpha, beta = np.arccos(ca), np.arccos(cb)
    v64, s64 = vec.astype(np.complex128), sv.astype(np.float64)
    power = np.array([float(np.sum(s64 * np.abs(v64.conj().T @ ura.steering(a_, b_, np.float32(d), sx, sy)) ** 2)) / (M * M) for a_, b_ in zip(alpha, beta)])
    order = sorted(range(k), key=lambda i: (-power[i], mu[i], nu[i]))
    Vn = V.astype(np.complex128) / np.linalg.norm(V.astype(np.complex128), axis=0)
    gap = min([abs(w[i] - w[j]) for i in range(k) for j in range(i)], default=np.inf)
    out.update(found=k, mu=mu[order], nu=nu[order], cond_gx=conds[0], cond_gy=conds[1], cond_v=float(np.linalg.cond(Vn)), gap=float(gap), steps=steps)
    out["phases"][:k] = np.stack([mu, nu], axis=1)[order]
    out["angles"][:k] = np.stack([alpha, beta], axis=1)[order].astype(np.float32)
    out["modulus"][:k] = np.stack([np.abs(lx), np.abs(ly)], axis=1)[order].astype(np.float32)
    out["power"][:k] = power[order].astype(np.float32)
    out["flags"][:k] = flags[order]
    return out


def well_conditioned(r):
    return r["cond_gx"] <= 4 and r["cond_gy"] <= 4 and r["cond_v"] <= 4 and r["gap"] >= 0.1


def phase_error(a, b):
    """largest |difference| of two phases arrays, modulo 2 pi"""
    dlt = np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)
    return float(np.abs((dlt + np.pi) % (2 * np.pi) - np.pi).max()) if dlt.size else 0.0


# ---- scenes --------------------------------------------------------------------------------------------------------------------------

def phases_of(alpha, beta, d):
    """(mu, nu) of the direction (alpha, beta) in the scan's convention"""
    return 2 * np.pi * float(d) * np.cos(alpha) * np.sin(beta), 2 * np.pi * float(d) * np.cos(beta)


def direction_of(mu, nu, d):
    cb = nu / (2 * np.pi * float(d))
    sb = np.sqrt(1 - cb * cb)
    return float(np.arccos(mu / (2 * np.pi * float(d) * sb))), float(np.arccos(cb))


def lattice_sources(k, d, span=0.62):
    """k directions (in the scan's convention: where MUSIC peaks) on a lattice of the (mu, nu) plane inside the visible disc, no two
    sharing mu or nu: rows of the lattice are sheared a little"""
    n = int(np.ceil(np.sqrt(k)))
    r = 2 * np.pi * float(d) * span
    pts = []
    for a in range(n):
        for c in range(n):
            u = ((a + 0.5) / n * 2 - 1 + 0.11 * (c - (n - 1) / 2) / n) * r
            v = ((c + 0.5) / n * 2 - 1 + 0.07 * (a - (n - 1) / 2) / n) * r
            pts.append((u, v))
    pts.sort(key=lambda p: p[0] ** 2 + p[1] ** 2)
    return [direction_of(u, v, d) for u, v in pts[:k]]


def shared_directions(which, d=ura.D):
    """two directions with the same mu ("mu") or the same nu ("nu")"""
    r = 2 * np.pi * 0.5
    pts = ((0.9, -1.1), (0.9, 0.8)) if which == "mu" else ((-1.2, 0.7), (1.0, 0.7))
    assert all(u * u + v * v < r * r for u, v in pts)
    return [direction_of(u, v, d) for u, v in pts]


# (sx, sy, k): the shapes of tests/test_gpu_doa_esprit.py
SHAPES = ((2, 2, 1), (3, 2, 3), (2, 5, 2), (5, 2, 2), (7, 3, 1), (7, 3, 2), (7, 3, 3), (7, 3, 5), (8, 8, 6), (8, 8, 16))


def shape_d(sx, sy):
    return float(ura.D) if (sx, sy) == (7, 3) else 0.5


def shape_scene(sx, sy, k, L=2048, seed=0, directions=None):
    """(block int8 [1 + M][2L], the k directions where MUSIC peaks (alpha, beta), amplitudes descending)"""
    d = shape_d(sx, sy)
    dirs = lattice_sources(k, 0.5 if d > 0.5 else d) if directions is None else list(directions)
    rng = np.random.default_rng(1000 * sx + 100 * sy + k + seed)
    amps = [1.0 - 0.5 * i / max(k, 1) for i in range(k)]
    src = [(np.pi - a, np.pi - b_, amp) for (a, b_), amp in zip(dirs, amps)]
    return ura.scene(L, src, rng, mx=sx, my=sy, d=np.float32(d)), dirs


def fp64_subspace(block):
    """(vec complex64 [M][M], sv float32 [M]) of a block: fp64 covariance and SVD, rounded once, as the engine publishes them"""
    x = block[1:].astype(np.float64) / 127.0
    X = (x[:, 0::2] + 1j * x[:, 1::2]).T
    X = X - X.mean(axis=0, keepdims=True)
    U, s, _ = np.linalg.svd(X.conj().T @ X / X.shape[0])
    return U.astype(np.complex64), s.astype(np.float32)


def match_error(angles, dirs):
    """largest distance (either angle) between the directions and the nearest estimated one, each estimate used once"""
    import itertools
    angles = np.asarray(angles, dtype=np.float64)
    if len(dirs) <= 6:
        return min(max(max(abs(angles[j][0] - a), abs(angles[j][1] - b_)) for j, (a, b_) in zip(perm, dirs)) for perm in itertools.permutations(range(len(angles)), len(dirs)))
    left, worst = list(range(len(angles))), 0.0
    for a, b_ in dirs:                                       # greedy: the scenes' directions lie many bars apart
        j = min(left, key=lambda q: max(abs(angles[q][0] - a), abs(angles[q][1] - b_)))
        worst = max(worst, max(abs(angles[j][0] - a), abs(angles[j][1] - b_)))
        left.remove(j)
    return worst
