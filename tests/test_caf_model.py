"""CPU checks of tests/caf_model.py, the fp64 statement of crsdr_caf (include/crsdr.h, section (w)) that the GPU tests hold the device
against: the two-stage route against the definition, a complex64 restatement against the derived bar, echo scenes whose peak must land
where the echo was put, single mistakes that must show, and the peak figures' rules."""
import numpy as np
import pytest

import caf_model as M

RECT, HANN = M.WINDOW_RECT, M.WINDOW_HANN

# (nrows, B, seg, frames, nlags): the shapes the GPU tests use where the bar is tightest (nd = 16, 32, 4096, 8)
BAR_SHAPES = [(2, 512, 16, 1, 16), (3, 2048, 64, 2, 17), (2, 16384, 16, 8, 5), (2, 8192, 4096, 8, 33)]

# (B, seg, frames, nlags, t0, d0, a)
SCENES = [(2048, 64, 2, 16, 5, 3, 0.3), (2048, 64, 2, 16, 11, -7, 0.3), (1024, 16, 1, 8, 3, 5, 0.3), (4096, 128, 4, 32, 20, -9, 0.1)]


def _line(nrows, B, frames, seed):
    return [M.random_matrix(nrows, B, seed + t) for t in range(frames)]


@pytest.mark.parametrize("kind", [RECT, HANN])
@pytest.mark.parametrize("nrows,B,seg,frames,nlags,ref", [(2, 512, 16, 1, 16, 1), (3, 1024, 64, 2, 9, 1)])
def test_two_stage_route_is_the_definition(nrows, B, seg, frames, nlags, ref, kind):
    line = _line(nrows, B, frames, 3)
    chi, _ = M.caf(line, seg, nlags, ref, kind)
    want = M.caf_direct(line, seg, nlags, ref, kind)
    assert chi.shape == (nrows, frames * B // (2 * seg), nlags)
    assert np.max(np.abs(chi - want)) <= 1e-12 * np.max(np.abs(want))


@pytest.mark.parametrize("kind", [RECT, HANN])
@pytest.mark.parametrize("nrows,B,seg,frames,nlags", BAR_SHAPES)
def test_complex64_restatement_meets_the_bar(nrows, B, seg, frames, nlags, kind):
    line = _line(nrows, B, frames, 10 + seg)
    chi, bar = M.caf(line, seg, nlags, 0, kind)
    r = M.worst_ratio(M.caf_f32(line, seg, nlags, 0, kind).astype(np.complex128), chi, bar)
    print(f"rows {nrows} B {B} seg {seg} frames {frames} lags {nlags} window {kind}: largest error / bar {r:.3f}")
    assert 0.0 < r <= 1.0


def test_full_scale_cannot_overflow():
    yr, yi = M.range_stage([np.full((2, 8192), -128, dtype=np.int8)], 4096, 3, 0)
    assert yr.max() == 2 ** 27 and np.abs(yi).max() == 0 and yr[0, 0, 2] == 2 ** 15 * (4096 - 2)


def _scene_peak(scene, kind, guard, which=None, strict=False):
    B, seg, frames, nlags, t0, d0, a = scene
    line = M.echo_scene(B, frames, [(1, t0, d0, a)], seed=B + t0)
    chi, bar = M.caf(line, seg, nlags, 0, kind, which)
    P = np.abs(chi[1]) ** 2
    return chi, bar, P, M.peaks(P, guard, strict)[0]


@pytest.mark.parametrize("kind", [RECT, HANN])
@pytest.mark.parametrize("scene", SCENES)
def test_echo_scenes(scene, kind):
    B, seg, frames, nlags, t0, d0, a = scene
    _, _, P, fig = _scene_peak(scene, kind, 2)
    assert (fig[0], fig[1]) == (t0, d0), fig
    nd = P.shape[0]
    ok = M.in_set(nd, 2)
    second = np.sort(np.where(ok[:, None], P, 0.0).ravel())[-2]
    ratio_db, gap_db = 10 * np.log10(fig[3]), 10 * np.log10(fig[2] / second)
    print(f"scene {scene} window {kind}: peak / mean {ratio_db:.1f} dB, gap to the second cell {gap_db:.1f} dB, dlag {fig[4]:+.3f} ddop {fig[5]:+.3f}")
    # The echo integrates coherently over the line's N samples, the floor is the reference's own correlation noise: per cell
    # a^2 N / (row power 0.64 + a^2 + noise) above the floor, and the peak's own share of the mean over |S| cells takes some of it
    # back.  Half of that (3 dB) is asked for; Hann's equivalent noise bandwidth (1.5 bins) costs 1.8 dB more.
    N, n = frames * B // 2, int(ok.sum()) * nlags
    snr = a * a * N / (0.64 + a * a + 0.0025)
    expect = snr / (1.0 + snr / n)
    assert fig[3] >= 0.5 * expect / (1.5 if kind == HANN else 1.0), (fig[3], expect)
    # rect: every other cell is floor; Hann: the neighbouring Doppler bin holds a quarter of the peak (-6 dB) plus floor
    assert gap_db >= (3.0 if kind == HANN else 8.0)
    assert abs(fig[4]) <= 0.5 and abs(fig[5]) <= 0.5
    fig0 = M.peaks(P, 0)[0]
    assert (fig0[0], fig0[1]) == (0, 0), fig0                                     # the direct path


@pytest.mark.parametrize("which", M.MUTATIONS)
def test_single_mistakes_show(which):
    """each mistake leaves the bar of the true chi on the first scene (Hann: rect hides sum w^2), or moves the peak off the echo"""
    chi, bar, _, fig = _scene_peak(SCENES[0], HANN, 2)
    bad, _, _, bad_fig = _scene_peak(SCENES[0], HANN, 2, which)
    r = M.worst_ratio(bad, chi, bar)
    moved = (bad_fig[0], bad_fig[1]) != (fig[0], fig[1])
    print(f"{which}: largest error / bar {r:.3g}, peak {'moved' if moved else 'kept'}")
    assert r > 1.0 or moved


def test_guard_is_inclusive():
    # an echo at Doppler 3 with guard 3: |s| >= guard keeps it, |s| > guard loses it
    _, _, _, fig = _scene_peak(SCENES[0], RECT, 3)
    _, _, _, bad = _scene_peak(SCENES[0], RECT, 3, strict=True)
    assert (fig[0], fig[1]) == (5, 3) and (bad[0], bad[1]) != (5, 3)


def test_guard_set():
    assert M.in_set(8, 0).all()
    assert list(M.in_set(8, 1)) == [False] + [True] * 7                          # 2 g - 1 = 1 bin cut
    assert list(M.in_set(8, 2)) == [False, False, True, True, True, True, True, False]
    assert list(M.in_set(8, 4)) == [False] * 4 + [True] + [False] * 3             # only s = -nd / 2 is left


def test_tie_rule_and_plateaus():
    P = np.zeros((8, 4))
    P[5, 2] = P[3, 1] = P[3, 3] = 7.0
    fig, _ = M.peaks(P, 0)
    assert (fig[0], fig[1], fig[2]) == (1, 3, 7.0)                                # the first in the order of d R + tau
    fig, _ = M.peaks(P, 4)                                                        # only d = 4 (s = -4) is searched: all zero there
    assert not fig.any()
    P[:] = 2.0                                                                    # a plateau: the first searched cell, flat parabolas
    fig, _ = M.peaks(P, 2)
    assert list(fig) == [0, 2, 2.0, 1.0, 0.0, 0.0]


def test_edge_guards_and_clamp():
    P = np.ones((8, 5))
    P[2, 0] = 9.0
    P[2, 1] = 5.0
    fig, _ = M.peaks(P, 2)
    assert (fig[0], fig[1], fig[4], fig[5]) == (0, 2, 0.0, 0.0)                   # tau* = 0; d* - 1 is inside the guard
    P = np.ones((8, 5))
    P[3, 4], P[2, 4], P[4, 4] = 9.0, 5.0, 3.0
    fig, _ = M.peaks(P, 2)
    assert (fig[0], fig[1], fig[4]) == (4, 3, 0.0) and fig[5] == 0.5 * (5 - 3) / (5 - 18 + 3)      # tau* = R - 1
    P = np.ones((8, 5))
    P[0, 2], P[7, 2], P[1, 2] = 9.0, 4.0, 6.0                                     # the Doppler neighbours wrap: d = -1 is bin 7
    fig, _ = M.peaks(P, 0)
    assert (fig[0], fig[1]) == (2, 0) and fig[5] == 0.5 * (4 - 6) / (4 - 18 + 6) and fig[4] == 0.0
    assert M._vertex(0.0, 1.0, 1.5)[0] == 0.5 and M._vertex(1.5, 1.0, 0.0)[0] == -0.5      # beyond the neighbour: clamped
    assert M._vertex(1.0, 1.0, 1.0) == (0.0, 0.0) and M._vertex(3.0, 1.0, 3.0) == (0.0, 0.0)


def test_all_zero_map():
    fig, bar = M.peaks(np.zeros((16, 3)), 2)
    assert not fig.any() and np.all(np.isfinite(fig)) and not bar[:4].any()
    chi, bar = M.caf([np.zeros((2, 512), dtype=np.int8)], 16, 4, 0, HANN)
    assert not chi.any() and not bar.any()
    assert M.worst_ratio(chi, chi, bar) == 0.0
