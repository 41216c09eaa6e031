"""The integration across lines as the fp64 model states it (tests/caf_integrate_model.py): the properties that follow from the
definition, the scene that is the reason for the feature -- an echo that the per-line detector loses and the detector behind the
integration finds in every line, and only with the shift along the range walk -- and the single mistakes, each of which must show.
CPU only; the device is held against this model byte for byte in tests/test_gpu_caf_integrate.py."""
import itertools

import numpy as np
import pytest

import caf_cfar_model as CF
import caf_integrate_model as IM

GUARD = 2


def _prm(alpha):
    return CF.Params(alpha, gd=1, gr=1, td=3, tr=4, min_train=8, max_det=16)


def _maps(seed, L, nd, R, nmaps=1):
    rng = np.random.default_rng(seed)
    return rng.exponential(1.0, size=(L, nmaps, nd, R)).astype(np.float32)


def test_line_0_is_the_map():
    maps = _maps(1, 1, 16, 9)
    for a, c in ((1.0, 0.0), (0.125, 2.75), (2.0 ** -20, -0.5)):
        out, state = IM.run(maps, a, c)
        assert out.tobytes() == maps.tobytes()
        assert state[:16].view("<i8").tolist() == [1, 0] and np.array_equal(state[16:].view(np.float64), maps.reshape(-1).astype(np.float64))


def test_the_warm_up_is_the_cumulative_mean():
    W, nd, R = 8, 8, 5
    maps = _maps(2, 12, nd, R)
    out, _ = IM.run(maps, 1.0 / W, 0.0)
    mean = np.cumsum(maps.astype(np.float64), axis=0) / np.arange(1, 13)[:, None, None, None]
    # the running mean by updates against the mean by one sum: a few roundings of fp64 each, and imap's one of fp32
    assert np.allclose(out[:W], mean[:W], rtol=2.0 ** -23, atol=0.0)
    assert not np.allclose(out[W + 2:], mean[W + 2:], rtol=1e-3, atol=0.0)          # and forgetting from then on
    with_walk, _ = IM.run(maps, 1.0 / W, 1.0)
    assert with_walk[0].tobytes() == out[0].tobytes() and with_walk[1:].tobytes() != out[1:].tobytes()


def test_constant_maps_stay_constant():
    maps = np.full((20, 2, 16, 7), np.float32(3.7), dtype=np.float32)
    for a, c in ((1.0, 0.5), (0.125, -2.75), (2.0 ** -20, 3.0), (0.3, 0.05)):
        out, _ = IM.run(maps, a, c)
        assert out.tobytes() == maps.tobytes(), (a, c)


def test_every_cut_of_12_lines_gives_the_same_bytes():
    L, nd, R = 12, 8, 3
    maps = _maps(3, L, nd, R)
    whole, wstate = IM.run(maps, 0.25, 0.5)
    n = 0
    for bits in itertools.product((0, 1), repeat=L - 1):                             # all 2^11 compositions of 12
        cuts = [0] + [k + 1 for k, b in enumerate(bits) if b] + [L]
        state, parts = None, []
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            out, state = IM.run(maps[lo:hi], 0.25, 0.5, state=state)
            parts.append(out)
        assert np.concatenate(parts).tobytes() == whole.tobytes() and state.tobytes() == wstate.tobytes(), cuts
        n += 1
    assert n == 2048


def test_offsets_agree_with_integers_for_dyadic_couplings():
    for nd in (8, 64, 4096):
        s = CF.M.signed_bins(nd).astype(np.int64)
        for num, k in ((0, 0), (1, 1), (-1, 1), (11, 2), (1, 4), (-3, 3), (3, 0), (1, 10)):
            c = num / 2.0 ** k
            if abs(c) * (nd // 2) > 1024:
                continue
            for m in (0, 1, 2, 3, 7, 8, 1000, 12345, 2 ** 20 + 1):
                want = IM.offset_by_integers(m, num, k, s)
                assert np.array_equal(IM.offsets(m, c, nd), want), (nd, num, k, m)
                if m:
                    assert np.array_equal(IM.steps(m, c, nd), want - IM.offset_by_integers(m - 1, num, k, s))
        assert not IM.steps(0, 2.75, nd).any()


def _found(P, alpha, cell):
    """(the echo's cell is among the detections, the other detections, ambiguous cells)"""
    d = CF.detect(P, GUARD, _prm(alpha))
    i = cell[0] * IM.R + cell[1]
    return i in d["cells"], [c for c in d["cells"] if c != i], d["ambiguous"]


@pytest.fixture(scope="module")
def scenes():
    """(seed, case) -> (maps, cells, imap with the shift, imap with coupling 0)"""
    out = {}
    for seed in IM.SEEDS:
        for sd, lag0 in IM.CASES:
            maps, cells = IM.scene(seed, sd, lag0)
            out[seed, sd, lag0] = (maps, cells, IM.run(maps[:, None], IM.FORGET, IM.COUPLING)[0][:, 0], IM.run(maps[:, None], IM.FORGET, 0.0)[0][:, 0])
    return out


@pytest.mark.parametrize("seed", IM.SEEDS)
@pytest.mark.parametrize("sd,lag0", IM.CASES)
def test_the_echo_is_lost_per_line_and_found_behind_the_integration(scenes, seed, sd, lag0):
    maps, cells, imap, flat = scenes[seed, sd, lag0]
    per_line = [_found(maps[m], 6.0, cells[m]) for m in range(IM.NLINES)]
    with_shift = [_found(imap[m], 2.0, cells[m]) for m in range(IM.WARM, IM.NLINES)]
    without = [_found(flat[m], 2.0, cells[m]) for m in range(IM.WARM, IM.NLINES)]
    print(seed, sd, lag0, "per line", sum(f for f, _, _ in per_line), "integrated", sum(f for f, _, _ in with_shift), "others", sum(len(o) for _, o, _ in with_shift),
          "coupling 0", sum(f for f, _, _ in without))
    assert sum(a for _, _, a in per_line + with_shift + without) == 0                 # no cell anywhere near a threshold: nothing is left out
    assert sum(f for f, _, _ in per_line) <= 3
    assert all(f for f, _, _ in with_shift) and not any(o for _, o, _ in with_shift)
    assert sum(f for f, _, _ in without) <= 1


def test_noise_alone_gives_nothing_behind_the_integration():
    total = 0
    for seed in IM.SEEDS:
        maps, _ = IM.scene(seed, *IM.CASES[0], echo=False)
        imap = IM.run(maps[:, None], IM.FORGET, IM.COUPLING)[0][:, 0]
        for m in range(IM.WARM, IM.NLINES):
            d, p = CF.detect(imap[m], GUARD, _prm(2.0)), CF.detect(maps[m], GUARD, _prm(2.0))
            assert d["count"] == 0 and d["ambiguous"] == 0 and p["ambiguous"] == 0, (seed, m)
            total += p["count"]
    print("per-line detections at alpha 2.0:", total)
    assert total > 2000                                                              # the per-line maps: thousands at that factor


@pytest.mark.parametrize("which", IM.MUTATIONS)
def test_single_mistakes_show(scenes, which):
    """each changes imap's bytes, and flips a stated outcome of the first scene or moves a cell by more than 1e-3; the float32 state is
    caught by the bytes alone"""
    maps, cells, imap, _ = scenes[IM.SEEDS[0], IM.CASES[0][0], IM.CASES[0][1]]
    bad = IM.run(maps[:, None], IM.FORGET, IM.COUPLING, which=which)[0][:, 0]
    differ = int((bad.view(np.uint32) != imap.view(np.uint32)).sum())
    rel = float(np.max(np.abs(bad.astype(np.float64) - imap) / imap))
    found = [_found(bad[m], 2.0, cells[m]) for m in range(IM.WARM, IM.NLINES)]
    flipped = not all(f for f, _, _ in found) or any(o for _, o, _ in found)
    print(which, "cells that differ", differ, "of", imap.size, "max relative", rel, "outcome flipped", flipped)
    assert differ > 0
    if which == "float32_state":
        assert rel < 1e-6
    else:
        assert flipped or rel > 1e-3
        if which != "update_first":
            assert differ >= 25000
