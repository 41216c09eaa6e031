"""The numpy model of crsdr_caf's second cancellation stage (tests/caf_clean_model.py) against itself: the joint solve is cancellation
done the long way in the time domain, the residual is orthogonal to every member, a line without picks is the first stage exactly, the
leading block of the factor is the first stage's, the masking scene behaves as measured -- with the margins DESIGN.md records -- and
every single mistake the device could make misses a bar or changes a list.  CPU only."""
import numpy as np
import pytest

import caf_cancel_model as X
import caf_cfar_model as C
import caf_clean_model as Z
import caf_model as M

RECT, HANN = M.WINDOW_RECT, M.WINDOW_HANN
MK = Z.MASK
PRM = Z.Params(2, 100.0, 1, 1)


def _first_pass(line, kind=HANN, guard=0, q=None):
    s1 = X.cancel(line, MK["seg"], MK["R"], MK["ref"], kind, MK["taps"], MK["dopp"])
    mp, d1 = Z.array_list(s1["chi"], MK["ref"], guard, q or Z.masking_detector())
    assert d1["ambiguous"] == 0
    return s1, mp, d1


def _clean(line, d1, prm=PRM, which=None, kind=HANN):
    r = Z.clean(line, MK["seg"], MK["R"], MK["ref"], kind, MK["taps"], MK["dopp"], d1["det"].astype(np.float32), d1["count"], prm, which)
    if which is None and np.isfinite(r["cond"]):
        assert r["cond"] <= Z.COND_MAX, r["cond"]                                # the bound the bars assume
    return r


def _cells(d):
    return [(int(r[0]), int(r[1])) for r in d["det"][:d["count"]]]


STRONG, WEAK = (MK["strong"][0], int(round(MK["strong"][1]))), (MK["weak"][0], MK["weak"][1])


@pytest.mark.parametrize("wl, wq", [(1, 1), (0, 2), (2, 0), (2, 2)])
def test_the_joint_solve_equals_cancellation_in_the_time_domain(wl, wq):
    line = Z.masking_scene(3)
    _, _, d1 = _first_pass(line)
    r = _clean(line, d1, Z.Params(2, 100.0, wl, wq))
    assert r["ntgt"] == 1 and len(r["members"]) == (2 * wl + 1) * (2 * wq + 1)
    td = Z.time_domain(line, MK["seg"], MK["R"], MK["ref"], r["lags"], r["gs"], r["h"])
    n = len(r["lags"])
    terms = np.abs(r["stage1"]["y"]) + np.einsum("ri,ikt->rkt", np.abs(r["h"]), np.stack(
        [np.abs(Z.full_ref_sums(line, MK["seg"], MK["R"], MK["ref"])[:, m, :]) for m in r["lags"]]))
    bar = 4.0 * (MK["seg"] + n + 4) * X.E64 * terms
    assert np.all(np.abs(td - r["yres"]) <= bar), np.max(np.abs(td - r["yres"]) / bar)


def test_the_residual_is_orthogonal_to_every_member():
    line = Z.masking_scene(4)
    _, _, d1 = _first_pass(line)
    r = _clean(line, d1)
    nd = MK["nd"]
    proj = np.stack([r["yres"][:, :, m] @ np.conj(Z.phase(g, nd)) for m, g in zip(r["lags"], r["gs"])], axis=1)      # c - A h
    scale = np.abs(r["c"]).max()
    others = [c for c in range(MK["nrows"]) if c != MK["ref"]]
    assert np.all(np.abs(proj[others]) <= 1e-9 * scale), np.abs(proj[others]).max() / scale          # cond 4096 x a few hundred e
    assert np.abs(r["c"][others]).max() > 1e-2 * scale


def test_a_line_without_picks_is_the_first_stage_exactly_and_the_leading_block_is_its_factor():
    line = Z.masking_scene(5)
    s1, _, d1 = _first_pass(line)
    none = _clean(line, d1, Z.Params(2, 1e30, 1, 1))
    assert none["ntgt"] == 0 and not none["tgt"].any() and not none["tcoef"].any()
    assert np.array_equal(none["A"], s1["A"]) and np.array_equal(none["L"], Z.chol_columns(s1["A"])[0])
    assert np.array_equal(none["h"], s1["h"]) and np.array_equal(none["rchi"], s1["chi"]) and np.array_equal(none["rbar"], s1["bar"])
    assert np.array_equal(none["share"], s1["share"]) and np.array_equal(none["c"], s1["c"])
    r = _clean(line, d1)
    n1 = r["n1"]
    assert r["ntgt"] == 1 and np.array_equal(r["A"][:n1, :n1], s1["A"]) and np.array_equal(r["L"][:n1, :n1], none["L"])
    # the picks are copied, the members' order is q outer, j inner, and tcoef's index follows it
    assert np.array_equal(r["tgt"][0], d1["det"][0].astype(np.float32)) and not r["tgt"][1].any()
    f = float(np.float32(d1["det"][0][1])) + float(np.float32(d1["det"][0][6]))
    assert [(m[0], m[1]) for m in r["members"]] == [(STRONG[0] + j, f + q / 2) for q in (-1, 0, 1) for j in (-1, 0, 1)]
    assert [m[3] for m in r["members"]] == list(range(9)) and np.array_equal(r["tcoef"][:, 0, :], r["h"][:, n1:])


@pytest.mark.parametrize("seed", range(4))
def test_the_masking_scene(seed):
    """the first pass lists the mover alone; the residual lists the echo alone; wq = 0 at the integer bin leaves the mover listed"""
    line = Z.masking_scene(seed)
    q = Z.masking_detector()
    s1, mp, d1 = _first_pass(line)
    assert _cells(d1) == [STRONG]
    r = _clean(line, d1)
    rmap, d2 = Z.array_list(r["rchi"], MK["ref"], 0, q)
    assert d2["ambiguous"] == 0 and _cells(d2) == [WEAK]
    d, dw = STRONG[1] % MK["nd"], WEAK[1] % MK["nd"]
    depth = 10.0 * np.log10(mp[d, STRONG[0]] / rmap[d, STRONG[0]])
    # margins to the threshold alpha * noise: the echo's cell before (under it) and after (over it), the mover's cell after (under it)
    before = C.threshold(mp.astype(np.float64), 0, q)[1][dw, WEAK[0]]
    after = C.threshold(rmap.astype(np.float64), 0, q)[1]
    m_before = 10.0 * np.log10(mp[dw, WEAK[0]] / (float(q.alpha) * before))
    m_after = 10.0 * np.log10(rmap[dw, WEAK[0]] / (float(q.alpha) * after[dw, WEAK[0]]))
    m_strong = 10.0 * np.log10(rmap[d, STRONG[0]] / (float(q.alpha) * after[d, STRONG[0]]))
    print(f"seed {seed}: depth {depth:.1f} dB, cond {r['cond']:.1f}; echo {m_before:+.1f} dB of its threshold before, {m_after:+.1f} dB after; mover's cell {m_strong:+.1f} dB after")
    assert depth > 40.0 and m_before < -3.0 and m_after > 6.0 and m_strong < -3.0
    # why the member is fractional: one member at the integer bin takes some 20 dB, and the mover is still on the list
    coarse = _clean(line, d1, Z.Params(2, 100.0, 1, 0), which="integer_f")
    cmap, d3 = Z.array_list(coarse["rchi"], MK["ref"], 0, q)
    shallow = 10.0 * np.log10(mp[d, STRONG[0]] / cmap[d, STRONG[0]])
    assert shallow < 30.0 and any(c[0] == STRONG[0] and c != WEAK for c in _cells(d3)), (shallow, _cells(d3))


def _lists_scene():
    """a line whose walk meets every rule: a pick across the wrap, a record that touches it, one under min_snr"""
    det = np.zeros((8, 8), dtype=np.float32)
    det[0] = [6, 15, 9.0, 900.0, 0.01, 0.0, 0.4, 54]
    det[1] = [7, -16, 8.0, 800.0, 0.01, 0.0, -0.2, 54]                           # 0.4 bins from the first around the circle
    det[2] = [12, 4, 7.0, 40.0, 0.2, 0.0, 0.1, 54]                               # under min_snr
    det[3] = [15, -7, 6.0, 600.0, 0.01, 0.0, 0.0, 54]                            # its cluster is clipped at R - 1
    return det, 4


@pytest.mark.parametrize("which", Z.MUTATIONS)
def test_every_single_mistake_misses_a_bar_or_changes_a_list(which):
    line = Z.masking_scene(6)
    q = Z.masking_detector()
    _, _, d1 = _first_pass(line)
    good = _clean(line, d1)
    _, dg = Z.array_list(good["rchi"], MK["ref"], 0, q)
    det, count = _lists_scene()
    nd, R, K, P = MK["nd"], MK["R"], MK["taps"], MK["dopp"]
    walk_good = Z.pick_walk(det, count, nd, K, P, Z.Params(3, 100.0, 1, 1))
    assert walk_good == [0, 3] and len(Z.target_members(det, walk_good, R, Z.Params(3, 100.0, 1, 1))) == 15
    if which in ("doppler_not_wrapped", "min_snr_ignored", "touch_ignored"):     # the walk's mistakes: another list of picks
        assert Z.pick_walk(det, count, nd, K, P, Z.Params(3, 100.0, 1, 1), which) != walk_good
        return
    if which == "lag_wrapped":                                                   # a left-out lag wrapped in: more members, and a residual off its bar
        assert len(Z.target_members(det, walk_good, R, Z.Params(3, 100.0, 1, 1), which)) == 18
        edge = Z.masking_scene(6, strong=(15, 4.3, 0.6))
        _, _, de = _first_pass(edge)
        assert _cells(de) == [(15, 4)]
        good, bad = _clean(edge, de), _clean(edge, de, which=which)
        assert len(bad["members"]) == len(good["members"]) + 3
    else:
        bad = _clean(line, d1, which=which)
    ratio = M.worst_ratio(bad["rchi"].astype(np.complex64), good["rchi"], good["rbar"])
    _, db = Z.array_list(bad["rchi"], MK["ref"], 0, q)
    print(f"{which}: residual off its bar by a factor {ratio:.3g}; lists {_cells(dg)} -> {_cells(db)}")
    assert ratio > 2.0, (which, ratio)
    assert M.worst_ratio(good["rchi"].astype(np.complex64), good["rchi"], good["rbar"]) <= 1.0     # (and the bar holds fp32's own rounding)


def test_status_2_keeps_the_first_stage_and_status_1_nothing():
    """a reference confined to one segment: the cluster's second Doppler repeats its first up to a unit factor"""
    line = [Z.masking_scene(7)[0].copy()]
    keep = line[0][MK["ref"]].copy()
    line[0][MK["ref"]] = 0
    a = 2 * MK["seg"] * 5
    line[0][MK["ref"], a:a + 24] = keep[a:a + 24]
    s1 = X.cancel(line, MK["seg"], MK["R"], MK["ref"], HANN, 1, 0)
    det = np.zeros((8, 8), dtype=np.float32)
    det[0] = [6, 4, 9.0, 900.0, 0.01, 0.0, 0.3, 54]
    r = Z.clean(line, MK["seg"], MK["R"], MK["ref"], HANN, 1, 0, det, 1, Z.Params(1, 100.0, 0, 1))
    assert r["ntgt"] == 1 and r["status"].tolist() == [0.0, 2.0, 2.0] and not r["tcoef"].any()
    assert np.array_equal(r["h"][:, :1], s1["h"]) and np.array_equal(r["rchi"], s1["chi"]) and np.array_equal(r["share"], s1["share"])
    line[0][MK["ref"]] = 0
    r = Z.clean(line, MK["seg"], MK["R"], MK["ref"], HANN, 1, 0, det, 1, Z.Params(1, 100.0, 0, 1))
    assert r["status"].tolist() == [0.0, 1.0, 1.0] and not r["h"].any() and np.array_equal(r["rchi"], M.caf(line, MK["seg"], MK["R"], MK["ref"], HANN)[0])


def test_the_limits():
    ok = Z.Params(2, 100.0, 1, 1)
    assert Z.bad_limit(32, 16, 1, 3, 2, 0, ok) == 0
    assert Z.bad_limit(32, 16, 1, 3, 2, 0, Z.Params(0, 100.0, 1, 1)) == 1 and Z.bad_limit(32, 16, 1, 3, 2, 0, Z.Params(9, 100.0, 0, 0)) == 1
    assert Z.bad_limit(32, 16, 1, 3, 2, 0, Z.Params(1, 100.0, 3, 1)) == 2 and Z.bad_limit(32, 16, 1, 3, 2, 0, Z.Params(1, 100.0, 1, -1)) == 3
    assert Z.bad_limit(32, 16, 1, 3, 4, 0, Z.Params(4, 100.0, 2, 1)) == 0 and Z.bad_limit(32, 16, 1, 3, 5, 0, Z.Params(4, 100.0, 2, 1)) == 4     # 64 and 65 members
    assert [Z.bad_limit(32, 16, 1, 3, 2, 0, Z.Params(1, v, 1, 1)) for v in (0.0, -1.0, np.inf, np.nan)] == [5, 5, 5, 5]
    assert Z.bad_limit(4096, 1024, 1, 2, 1, 0, Z.Params(1, 100.0, 1, 0)) == 0 and Z.bad_limit(4096, 1024, 1, 2, 2, 0, Z.Params(1, 100.0, 1, 0)) == 6      # 2^24, and past it
    assert Z.bad_limit(4096, 1024, 1, 3, 1, 0, Z.Params(1, 100.0, 1, 0)) == 7                                                                              # 2 x 3 x 2^22
