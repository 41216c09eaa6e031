"""Test helper: a numpy fp64 restatement of crsdr_doa_set_beams / crsdr_doa_fetch_beams / crsdr_beamform (include/crsdr.h), from the
definition alone.

Per estimate and beam slot: a direction (alpha, beta) -- a grid point (cx, cy) as alpha = cx pi / ncx, beta = cy pi / ncy, or the caller's
angles -- its steering vector a[iy mx + ix] = exp(2 pi j d (ix cos(alpha) sin(beta) + iy cos(beta))) (tests/ura.py's, d promoted from
float32), and from the published fp32 subspace vec (column r = v_r) and singular values sv, in fp64:

    conventional  u = a / m                                                          power = sum_r sv[r] |v_r^H a|^2 / m^2
    MVDR          delta = loading sv[0],  z = sum_r v_r (v_r^H a) / (sv[r] + delta)   u = z / Re(a^H z)     power = 1 / Re(a^H z)
                  sv[0] == 0:  u = a / m, power 0

both rounded once to fp32 by the callers that compare with the device.  Beam: y[n] = sum_c u[c - 1] (I_c[n] + j Q_c[n]) / 127 over the
signal rows c = 1 .. m of a matrix [1 + m][2 L] int8, NO conjugate.  Empty slots (b >= found): weights 0, power -1, samples 0."""
import numpy as np

import doa_peaks_model as peaks_model
import ura

CONVENTIONAL, MVDR = 1, 2


def grid_angles(cx, cy, ncx=100, ncy=100):
    return cx * np.pi / ncx, cy * np.pi / ncy


def steering(alpha, beta, d=ura.D, mx=ura.MX, my=ura.MY):
    return ura.steering(float(alpha), float(beta), np.float32(d), mx, my)


def weights(vec, sv, a, mode, loading=0.0):
    """(u [m] complex128, power float) of one slot.  vec [m][m] and sv [m] as published (any float type: promoted), a [m] complex128.
    Takes any loading >= 0 (the ABI restricts it to [1e-6, 1])."""
    V = np.asarray(vec).astype(np.complex128)
    s = np.asarray(sv).astype(np.float64)
    a = np.asarray(a, dtype=np.complex128)
    m = len(a)
    g = V.conj().T @ a                                   # g[r] = v_r^H a
    if mode == CONVENTIONAL or s[0] == 0.0:
        return a / m, float(np.sum(s * np.abs(g) ** 2)) / (m * m)
    delta = float(np.float32(loading)) * s[0]
    z = V @ (g / (s + delta))
    den = np.vdot(a, z).real                             # Re(a^H z)
    return z / den, 1.0 / den


def slot_weights(vec, sv, slots, mode, loading, d=ura.D, mx=ura.MX, my=ura.MY):
    """One estimate: slots = [(alpha, beta) or None (an empty slot)] -> (weights [n][m] complex64, power [n] float32), rounded as the
    device rounds them."""
    m = mx * my
    w = np.zeros((len(slots), m), dtype=np.complex64)
    p = np.full(len(slots), -1.0, dtype=np.float32)
    for b, ang in enumerate(slots):
        if ang is None:
            continue
        u, pw = weights(vec, sv, steering(ang[0], ang[1], d, mx, my), mode, loading)
        w[b] = (u.real.astype(np.float32) + 1j * u.imag.astype(np.float32)).astype(np.complex64)
        p[b] = np.float32(pw)
    return w, p


def following_slots(found, peaks, ncx=100, ncy=100):
    """The slots of an estimate whose beams follow its directions: peaks [count][2] with found of them valid."""
    return [grid_angles(int(cx), int(cy), ncx, ncy) if b < found else None for b, (cx, cy) in enumerate(peaks)]


def samples(matrix):
    """x [m][L] complex128 = (I + j Q) of the signal rows (not yet divided by 127)."""
    x = np.asarray(matrix)[1:].astype(np.float64)
    return x[:, 0::2] + 1j * x[:, 1::2]


def beams(matrix, w):
    """y [n][L] complex128 of weights w [n][m] (used as given: fp32 weights promoted) on matrix [1 + m][2 L] int8."""
    return (np.asarray(w).astype(np.complex128) @ samples(matrix)) / 127.0


def beam_bound(matrix, w):
    """[n][L]: (4 m + 4) 2^-24 sum_c (|Re u_c| + |Im u_c|) (|I_c[n]| + |Q_c[n]|) / 127, the bar per sample and component for an fp32
    evaluation in any order, fused or not, with the 1/127 applied anywhere."""
    w = np.asarray(w).astype(np.complex128)
    x = np.abs(np.asarray(matrix)[1:].astype(np.float64))
    mag = (np.abs(w.real) + np.abs(w.imag)) @ (x[:, 0::2] + x[:, 1::2]) / 127.0
    return (4 * w.shape[1] + 4) * 2.0 ** -24 * mag


def scene(L, sources, rng, mx=ura.MX, my=ura.MY, d=ura.D, sigma_s=25.0, sigma_n=8.0):
    """tests/ura.py's scene (the same draws in the same order, so the same block for the same generator state) with the source signals
    returned as well: (int8 rows [1 + M][2 L], signals [k][L] complex128)."""
    M = mx * my
    x = sigma_n * (rng.standard_normal((M + 1, L)) + 1j * rng.standard_normal((M + 1, L))) / np.sqrt(2)
    sig = []
    for alpha, beta, amp in sources:
        s = sigma_s * amp * (rng.standard_normal(L) + 1j * rng.standard_normal(L)) / np.sqrt(2)
        x[1:] += ura.steering(alpha, beta, d, mx, my)[:, None] * s[None, :]
        sig.append(s)
    return ura.quantise(x), np.stack(sig)


def rho(s, y):
    """|<s, y>| / (|s| |y|)"""
    return float(np.abs(np.vdot(s, y)) / (np.linalg.norm(s) * np.linalg.norm(y)))


def mirrored_source(gx, gy, nc=100):
    """(alpha, beta) of a source that MUSIC on X^H X shows at grid (gx, gy): the mirror image (pi - alpha, pi - beta)."""
    return np.pi - gx * np.pi / nc, np.pi - gy * np.pi / nc


# ---- the separation scenes (CPU test on the fp64 pipeline, GPU test on the device's beams, same seed) ----
# 7 x 3 URA, L = 8192, k = 2, source 0 at amplitude 1 beside source 1 at amplitude 3; set_peaks(4, 2); MVDR loading 1e-2 (at 1e-4 a
# half-grid-step pointing error makes MVDR null its own source: textbook behaviour, the reason loading is a parameter).
SEED, L, K, LOADING = 1, 8192, 2, 1e-2
ON_GRID = ((50, 50), (55, 58))                 # where MUSIC shows the two sources (their mirror images)
OFF_GRID = ((50.5, 50.5), (56.4, 59.5))        # MUSIC peaks (51, 51), (56, 59), and two side-lobe peaks


def separation_block(grid_pts):
    """(int8 block, source signals [2][L]) of one of the two scenes."""
    rng = np.random.default_rng(SEED)
    return scene(L, [(*mirrored_source(*grid_pts[0]), 1.0), (*mirrored_source(*grid_pts[1]), 3.0)], rng)


def separation_scene(grid_pts):
    """The block, the source signals and the fp64 pipeline's (found, peaks, vec, sv) for one of the two scenes (set_peaks(4, 2))."""
    blk, sig = separation_block(grid_pts)
    _, U, s, pm = ura.music_fp64(blk, K)
    found, peaks, _ = peaks_model.directions(pm.astype(np.float32), 4, 2)
    return blk, sig, found, peaks, U.astype(np.complex64), s.astype(np.float32)


def slot_near(peaks, found, pt):
    """the slot within 1.5 grid points (both coordinates) of pt"""
    hits = [j for j in range(found) if abs(peaks[j][0] - pt[0]) <= 1.5 and abs(peaks[j][1] - pt[1]) <= 1.5]
    assert len(hits) == 1, (peaks, pt)
    return hits[0]


def check_separation(sig, beams_mvdr, beams_conv, power_mvdr, peaks, found, grid_pts, what):
    """The issue's conditions for the weak source's beam, and the two largest MVDR powers at the two sources."""
    weak, strong = slot_near(peaks, found, grid_pts[0]), slot_near(peaks, found, grid_pts[1])
    own, other = rho(sig[0], beams_mvdr[weak]), rho(sig[1], beams_mvdr[weak])
    conv_other = rho(sig[1], beams_conv[weak])
    print(f"{what}: peaks {np.asarray(peaks)[:found].tolist()} weak slot {weak}: MVDR rho_own {own:.4f} rho_other {other:.4f}, "
          f"conventional rho_other {conv_other:.4f}; MVDR power {np.asarray(power_mvdr).tolist()}")
    assert own >= 0.95 and other <= 0.10, (what, own, other)
    assert conv_other >= 0.5, (what, conv_other)
    top2 = set(np.argsort(np.asarray(power_mvdr)[:found])[::-1][:2].tolist())
    assert top2 == {weak, strong}, (what, power_mvdr, weak, strong)
