"""CPU checks of tests/caf_cfar_model.py, the fp64 statement of crsdr_caf's CFAR detector (include/crsdr.h (w), "Detections"): its sums of
shifted maps against a literal enumeration of every cell's training set, the detections of two echo scenes, the false-alarm rate of the
threshold stage on exponential noise, and that single mistakes in the definition do not pass unseen."""
import functools

import numpy as np
import pytest

import caf_cfar_model as C
import caf_model as M

HANN = M.WINDOW_HANN


def _noise(nd, R, seed):
    return np.random.default_rng(seed).exponential(1.0, size=(nd, R))


# (nd, R, guard, gd, gr, td, tr): guard 0, 1 and nd / 2; R below Hr, R = 1; the window on nearly the whole Doppler axis (2 Hd + 1 = nd - 1 at
# a power of two, = nd at nd = 9: the model takes any nd); no guard cells but the cell; training over one axis only
BOXES = [(8, 1, 0, 1, 1, 2, 4), (8, 5, 1, 1, 1, 2, 15), (8, 20, 0, 0, 0, 3, 0), (9, 7, 2, 1, 2, 3, 2), (16, 3, 8, 1, 1, 3, 4), (16, 20, 1, 2, 0, 1, 3),
         (32, 17, 16, 1, 1, 3, 4), (32, 20, 0, 3, 5, 5, 11), (32, 11, 1, 0, 2, 0, 9), (16, 13, 2, 1, 1, 6, 15)]


@pytest.mark.parametrize("box", BOXES)
def test_sums_and_counts_against_the_enumerated_training_set(box):
    nd, R, guard, gd, gr, td, tr = box
    prm = C.Params(3.0, gd, gr, td, tr)
    P = _noise(nd, R, 17 * nd + R)
    Z, N = C.train_sums(P, guard, prm)
    s = M.signed_bins(nd)
    for d in range(nd):
        for tau in range(R):
            z, n, cells = C.train_cell(P, guard, prm, d, tau)
            assert len(set(cells)) == n and (d, tau) not in cells                # no cell twice, never the cell itself
            assert all(0 <= t < R and abs(s[q]) >= guard for q, t in cells)
            assert N[d, tau] == n, (box, d, tau)
            assert abs(Z[d, tau] - z) <= 2.0 * max(n - 1, 0) * C.E64 * z, (box, d, tau)
    if guard == nd // 2:
        assert N[nd // 2].max() <= 2 * tr                                        # one bin left: it trains on its own lags only
    if guard == 0 and R > 2 * (gr + tr):
        assert N.max() == (2 * (gd + td) + 1) * (2 * (gr + tr) + 1) - (2 * gd + 1) * (2 * gr + 1)


def test_nothing_to_train_on_behind_the_whole_guard():
    nd, R = 16, 12
    P = _noise(nd, R, 3)
    prm = C.Params(1.5, 1, 1, 3, 0)                                              # training over Doppler only, and guard leaves one bin
    Z, N = C.train_sums(P, nd // 2, prm)
    assert not N[nd // 2].any() and not Z[nd // 2].any()                         # (the one searched bin)
    r = C.detect(P, nd // 2, prm)
    assert r["count"] == 0 and not r["det"].any() and r["passed"] == 0


# ---- the echo scenes: (B, frames, seg, R, nrows, echoes, seed) ----
ALPHA = C.cfar_alpha(1e-6, 90)
SCENES = {"two": (4096, 4, 64, 32, 3, [(1, 9, 20, 0.2), (2, 17, -13, 0.15)], 0), "one": (2048, 2, 16, 16, 2, [(1, 5, 11, 0.3)], 1)}


@functools.lru_cache(maxsize=None)
def scene_maps(name):
    """the nrows + 1 maps of a scene from fp64 chi rounded to complex64 (Hann), never changed by a test"""
    B, frames, seg, R, nrows, echoes, seed = SCENES[name]
    line = M.echo_scene(B, frames, echoes, nrows=nrows, seed=seed)
    chi = M.caf(line, seg, R, 0, HANN)[0].astype(np.complex64)
    mp = M.array_map(chi, 0)[0].astype(np.float32)
    return tuple(C.maps_of(chi, mp))


def _where(r):
    return [(int(x[0]), int(x[1])) for x in r["det"][:r["count"]]]


def _db(r):
    return [round(10.0 * np.log10(x[3]), 1) for x in r["det"][:r["count"]]]


def test_alpha_of_the_scenes():
    assert abs(float(ALPHA) - 14.93) < 0.005
    assert ALPHA == np.float32(90.0 * (1e-6 ** (-1.0 / 90.0) - 1.0))
    assert abs(float(C.cfar_alpha(0.5, 1)) - 1.0) < 1e-6                         # N = 1: alpha = 1 / pfa - 1


def test_scene_of_two_echoes():
    prm = C.Params(ALPHA, 1, 1, 3, 4)
    maps = scene_maps("two")
    arr = C.detect(maps[3], 2, prm)
    assert arr["ambiguous"] == 0
    assert _where(arr) == [(9, 20), (17, -13)] and arr["count"] == 2, arr["det"][:4]
    assert _db(arr) == [22.6, 19.6], _db(arr)
    row = C.detect(maps[1], 2, prm)
    assert row["ambiguous"] == 0 and _where(row) == [(9, 20)] and _db(row) == [25.4], row["det"][:2]
    ref = C.detect(maps[0], 2, prm)                                              # the reference against itself: nothing off the ridge
    assert ref["count"] == 0
    # the threshold alone lets the Hann main lobe's other cells through: the neighbourhood test is what leaves one per echo
    assert 3 <= arr["passed"] <= 5 and 3 <= row["passed"] <= 5, (arr["passed"], row["passed"])
    assert np.all(arr["det"][:2, 7] == 90)                                       # interior cells: the whole window trains
    assert np.all(np.abs(arr["det"][:2, 5:7]) <= 0.5) and arr["det"][:2, 5:7].any()


def test_scene_of_one_echo():
    prm = C.Params(ALPHA, 1, 1, 3, 4)
    arr = C.detect(scene_maps("one")[2], 2, prm)
    assert arr["ambiguous"] == 0 and arr["count"] == 1 and _where(arr) == [(5, 11)] and _db(arr) == [23.2], arr["det"][:2]
    assert 3 <= arr["passed"] <= 5


@pytest.mark.parametrize("pfa", [1e-2, 1e-3])
def test_false_alarm_rate_on_exponential_noise(pfa):
    nd, R, n = 256, 64, 90
    prm = C.Params(C.cfar_alpha(pfa, n), 1, 1, 3, 4)
    passed, _, N, amb = C.threshold(_noise(nd, R, 2024), 0, prm)
    inner = N == n                                                               # the cells whose whole window is inside the lags
    cells = int(inner.sum())
    assert cells == nd * (R - 2 * prm.Hr) == 13824
    rate = passed[inner].sum() / cells
    band = 4.0 * np.sqrt(pfa * (1.0 - pfa) / cells)
    print(f"pfa {pfa}: {int(passed[inner].sum())} of {cells} interior cells over the threshold, rate {rate:.5f}, band +-{band:.5f}")
    assert abs(rate - pfa) <= band, (rate, pfa, band)
    assert not amb.any()


# ---- single mistakes ----
def _flat(nd, R, spots):
    P = np.ones((nd, R))
    for (d, t), v in spots.items():
        P[d, t] = v
    return P


@functools.lru_cache(maxsize=None)
def mistake_inputs():
    """(P, guard, prm) on which every one of MUTATIONS shows"""
    four = C.Params(4.0, 1, 1, 3, 4)
    ridge = _noise(32, 24, 5)
    ridge[0] *= 1e4                                                              # a direct path's ridge at Doppler 0 ...
    ridge[3, 12] = 60.0                                                          # ... and a target three bins from it
    edge = _noise(32, 24, 6)
    edge[10, 1], edge[10, 23] = 40.0, 3e3                                        # a target at lag 1; a strong cell at the other end of the lags
    return (
        (scene_maps("two")[3], 2, C.Params(ALPHA, 1, 1, 3, 4)),                  # the main lobe lies in the guard cells
        (scene_maps("two")[3], 0, C.Params(ALPHA, 1, 1, 3, 4)),                  # the direct path at (0, 0): Doppler wraps, and N < 90 at the lag edge
        (ridge, 2, C.Params(ALPHA, 1, 1, 3, 4)),
        (edge, 0, C.Params(ALPHA, 1, 1, 3, 4)),
        (_flat(16, 24, {(5, 6): 4.0, (11, 17): 5.0}), 0, four),                  # integers: noise = 1, t = 4 exactly; P = 4 is no detection
        (_flat(16, 24, {(5, 6): 9.0, (5, 7): 9.0, (6, 6): 9.0}), 0, four),       # a plateau: its first cell
    )


def _shows(which):
    for P, guard, prm in mistake_inputs():
        good, bad = C.detect(P, guard, prm), C.detect(P, guard, prm, which)
        if good["cells"] != bad["cells"] or np.any(np.abs(good["det"] - bad["det"]) > good["bar"]):
            return True
    return False


def test_the_inputs_of_the_mistakes_are_what_they_claim():
    ins = mistake_inputs()
    assert _where(C.detect(*ins[1]))[0] == (0, 0)
    assert (12, 3) in _where(C.detect(*ins[2])) and (1, 10) in _where(C.detect(*ins[3]))
    r = C.detect(*ins[4])
    assert r["cells"] == [11 * 24 + 17] and r["det"][0, 4] == 1.0 and r["det"][0, 3] == 5.0      # P == t at (5, 6): not a detection
    assert C.detect(*ins[5])["cells"] == [5 * 24 + 6]
    assert all(C.detect(*i)["ambiguous"] == (1 if k == 4 else 0) for k, i in enumerate(ins))      # (the cell put exactly AT the threshold is the one ambiguous cell)


@pytest.mark.parametrize("which", C.MUTATIONS)
def test_a_single_mistake_shows(which):
    assert _shows(which), which


def test_zero_map_and_snapshot():
    prm = C.Params(ALPHA, 1, 1, 3, 4, max_det=4)
    r = C.detect(np.zeros((16, 8)), 0, prm)
    assert r["count"] == 0 and not r["det"].any() and np.all(np.isfinite(r["det"])) and r["ambiguous"] == 0
    chi = (np.arange(3 * 8 * 4).reshape(3, 8, 4) * (1 + 2j)).astype(np.complex64)
    s = C.snapshot(chi, [5, 30], 4)
    assert s.shape == (4, 3) and s[0, 1] == chi[1, 1, 1] and s[1, 2] == chi[2, 7, 2] and not s[2:].any()
