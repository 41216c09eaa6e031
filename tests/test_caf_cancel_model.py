"""The numpy model of crsdr_caf's canceller (tests/caf_cancel_model.py) against itself: the lag-domain result is ECA done the long way,
the residual is orthogonal to the basis, the identities of the definition hold, the two scenes of the change behave as measured, and
every single mistake the device could make misses a bar or the peak.  CPU only."""
import numpy as np
import pytest

import caf_cancel_model as X
import caf_cfar_model as C
import caf_model as M

RECT, HANN = M.WINDOW_RECT, M.WINDOW_HANN
ECHO = (5, 20)                                                                   # (Doppler bin, lag) of the scenes' echo
# gd = gr = 1, td = 3, tr = 4: 9 x 11 - 3 x 3 = 90 training cells, and crsdr_cfar_alpha's factor for 10^-6 per cell.  That factor is made for
# the full set: a cell at a lag edge trains on about half of it and runs at a higher rate (include/crsdr.h says so), so min_train = 90
# tests only the cells the factor is made for -- 0.002 false alarms expected per map of 2048 cells.
ALPHA, MIN_TRAIN = C.cfar_alpha(1e-6, 90), 90


def _noise_line(nrows, B, frames, seed, ref=0, echoes=()):
    return M.echo_scene(B, frames, list(echoes), nrows=nrows, ref=ref, seed=seed)


def _cancel(line, seg, R, ref, kind, K, P, which=None):
    r = X.cancel(line, seg, R, ref, kind, K, P, which)
    if which is None and np.isfinite(r["cond"]):
        assert r["cond"] <= 16.0, r["cond"]                                      # the bars of h stay tight
    return r


SHAPES = [(3, 256, 1, 16, 16, 0, 2, 0), (3, 256, 1, 16, 16, 1, 2, 2), (3, 512, 2, 16, 20, 2, 17, 0), (2, 4096, 1, 64, 32, 0, 16, 1), (3, 1024, 4, 16, 16, 0, 5, 1)]


@pytest.mark.parametrize("shape", SHAPES)
def test_lag_domain_equals_eca_in_the_time_domain(shape):
    nrows, B, frames, seg, R, ref, K, P = shape
    line = _noise_line(nrows, B, frames, 11, ref)
    r = _cancel(line, seg, R, ref, HANN, K, P)
    td = X.time_domain(line, seg, R, ref, K, P, r["h"])
    # fp64 on both sides: Ls products and n + 1 terms, each within 4 e of its magnitude -- scaled by the terms, not by the small y'
    bar = 4.0 * (seg + X.basis(K, P) + 4) * X.E64 * r["terms"]
    assert np.all(np.abs(td - r["yc"]) <= bar), np.max(np.abs(td - r["yc"]) / bar)
    others = [c for c in range(nrows) if c != ref]
    assert np.sum(np.abs(r["yc"][others]) ** 2) < 0.5 * np.sum(np.abs(r["y"][others]) ** 2)      # something was taken out


@pytest.mark.parametrize("shape", SHAPES)
def test_the_residual_is_orthogonal_to_the_basis(shape):
    nrows, B, frames, seg, R, ref, K, P = shape
    line = _noise_line(nrows, B, frames, 12, ref)
    r = _cancel(line, seg, R, ref, RECT, K, P)
    nd = r["y"].shape[1]
    phi = X.phases(nd, P)
    n = X.basis(K, P)
    # sum_k conj(phi_p[k]) y'[k][m] = c - A h: zero to the solve's bar carried through A
    proj = np.concatenate([np.einsum("k,rkm->rm", np.conj(phi[p]), r["yc"][:, :, :K]) for p in range(2 * P + 1)], axis=1)
    hb64 = r["hbar"] - X.U * np.abs(r["h"])                                      # (the fp64 part of the bar: the model's h is not rounded)
    tol = (np.linalg.norm(r["A"], 2) * np.sqrt(n) * hb64.max(axis=1) + 4.0 * (n + nd) * X.E64 * np.einsum("rkt->r", r["terms"][:, :, :K]))[:, None]
    others = [c for c in range(nrows) if c != ref]
    assert np.all(np.abs(proj[others]) <= tol[others]), np.max(np.abs(proj[others]) / tol[others])
    # so with rect chi' is zero at the Doppler bins p mod nd and the lags < K
    sc = M.scale_of(seg, nd, RECT)
    for p in range(-P, P + 1):
        cell = r["chi"][others][:, p % nd, :K]
        assert np.all(np.abs(cell) <= sc * tol[others]), (p, np.max(np.abs(cell)))
    assert np.max(np.abs(r["chi"][others][:, (P + 1) % nd, :])) > 1e3 * sc * tol.max()      # (and not everywhere)


def test_identities():
    nrows, B, seg, R, K, P = 4, 512, 16, 16, 4, 1
    line = _noise_line(nrows, B, 1, 13, ref=1)
    # row 2 lies in the span: 3 X_r[n] - 2 X_r[n - 2]; row 3 is all zero
    x = line[0].astype(np.int64)
    d2 = np.concatenate([np.zeros(4, dtype=np.int64), x[1][:-4]])
    line[0][2] = np.clip((3 * (x[1] // 8)) - 2 * (d2 // 8), -128, 127).astype(np.int8)
    line[0][1] = ((x[1] // 8) * 1).astype(np.int8)
    line[0][3] = 0
    r = _cancel(line, seg, R, 1, HANN, K, P)
    off, _ = M.caf(line, seg, R, 1, HANN)
    assert np.array_equal(r["chi"][1], off[1]) and not r["h"][1].any() and (r["share"][1], r["status"][1]) == (1.0, 0.0)      # row r untouched
    want = np.zeros(X.basis(K, P), dtype=np.complex128)
    want[K + 0], want[K + 2] = 3.0, -2.0
    assert np.all(np.abs(r["h"][2] - want) <= r["hbar"][2] + 1e-12) and r["share"][2] <= r["sbar"][2] + 1e-12
    assert np.all(np.abs(r["chi"][2]) <= r["bar"][2]) and np.max(np.abs(off[2])) > 1e6 * np.max(r["bar"][2])
    assert not r["h"][3].any() and r["share"][3] == 1.0 and np.all(np.isfinite(r["chi"])) and not r["chi"][3].any()
    line[0][1] = 0                                                               # an all-zero reference: singular, the canceller-off chi
    z = X.cancel(line, seg, R, 1, HANN, K, P)
    off, _ = M.caf(line, seg, R, 1, HANN)
    assert list(z["status"]) == [1.0, 0.0, 1.0, 1.0] and not z["h"].any() and np.array_equal(z["chi"], off) and np.all(z["share"] == 1.0)


def _row_map(chi):
    return np.abs(chi.astype(np.complex64).astype(np.complex128)) ** 2


@pytest.mark.parametrize("seed", range(4))
def test_the_static_scene(seed):
    """noise reference of 30 LSB rms, seg 64, nd 64, 32 lags, Hann; direct path 0.8, clutter 0.3 at lag 1 and 0.1 at lag 3, thermal noise
    of 2 LSB rms, an echo of 0.01 (0.3 LSB) at lag 20, Doppler bin 5.  Measured, seeds 0 .. 3: canceller off the echo cell is -8.7, -14.6,
    -0.4, -3.0 dB against the map's mean and the guard-2 peak sits at (lag, Doppler) (8, -26), (30, -15), (26, -14), (8, -32); with
    K = 8, P = 0 the echo cell is the guard-0 peak at 18.4, 17.9, 17.1, 17.3 dB over the mean, cond(A) 1.10 .. 1.18, 0.0063 .. 0.0066 of
    the row's power stays."""
    line = X.clutter_scene(seed)
    off, _ = M.caf(line, 64, 32, 0, HANN)
    fig = M.peaks(_row_map(off[1]), 2)[0]
    assert (fig[1], fig[0]) != ECHO
    r = _cancel(line, 64, 32, 0, HANN, 8, 0)
    P = _row_map(r["chi"][1])
    fig = M.peaks(P, 0)[0]
    db = X.over_mean_db(P, *ECHO)
    print(f"seed {seed}: echo {db:.1f} dB over the mean, cond {r['cond']:.3f}, share {r['share'][1]:.4f}")
    assert (fig[1], fig[0]) == ECHO and 16.0 < db < 20.0 and r["cond"] < 1.5 and 0.004 < r["share"][1] < 0.009
    det = C.detect(P, 0, C.Params(ALPHA, 1, 1, 3, 4, min_train=MIN_TRAIN))
    assert det["count"] == 1 and (det["det"][0][1], det["det"][0][0]) == ECHO and det["ambiguous"] == 0


@pytest.mark.parametrize("per_segment", [False, True], ids=["continuous", "per segment"])
@pytest.mark.parametrize("seed", range(4))
def test_the_doppler_scene(seed, per_segment):
    """the same with the clutter 0.3 at lag 2 shifted by +1 Doppler bin and 0.2 at lag 4 shifted by -1 bin.  Measured: P = 0 leaves the
    peak at (Doppler 1, lag 2) and keeps 0.173 .. 0.176 of the power; P = 1 puts it on the echo, 17.1 .. 18.5 dB over the mean, and keeps
    0.0062 .. 0.0066, cond(A) 1.26 .. 1.35."""
    line = X.clutter_scene(seed, paths=X.DOPPLER_PATHS, per_segment=per_segment)
    r0 = _cancel(line, 64, 32, 0, HANN, 8, 0)
    fig = M.peaks(_row_map(r0["chi"][1]), 0)[0]
    assert (fig[1], fig[0]) == (1, 2) and 0.15 < r0["share"][1] < 0.2
    r1 = _cancel(line, 64, 32, 0, HANN, 8, 1)
    P = _row_map(r1["chi"][1])
    fig = M.peaks(P, 0)[0]
    assert (fig[1], fig[0]) == ECHO and 16.0 < X.over_mean_db(P, *ECHO) < 20.0 and 0.004 < r1["share"][1] < 0.009


@pytest.mark.parametrize("which", X.MUTATIONS)
def test_single_mistakes_miss_a_bar_or_the_peak(which):
    # a line of two packets (the second one's front has a packet before it), a reference in the middle, complex clutter with Doppler
    line = X.clutter_scene(5, seg=32, nd=32, paths=((0, 0, 0.8 * np.exp(0.7j)), (2, 1, 0.3j), (4, -1, 0.2)), echo=(9, 5, 0.05), nrows=3, ref=1, frames=2)
    good = _cancel(line, 32, 16, 1, HANN, 6, 1)
    bad = X.cancel(line, 32, 16, 1, HANN, 6, 1, which)
    miss_chi = M.worst_ratio(bad["chi"], good["chi"], good["bar"])
    miss_h = float(np.max(np.abs(bad["h"] - good["h"]) / np.maximum(good["hbar"], 1e-300)))
    print(f"{which}: chi misses its bar by {miss_chi:.3g}, h by {miss_h:.3g}")
    assert miss_chi > 1.0 or miss_h > 1.0
    if which == "fp32_accumulate":
        assert miss_chi > 1.0 and miss_h == 0.0                                  # (h is the same: only the subtraction differs)
