"""CPU checks of the fp64 model of crsdr_caf's coherent beam maps (tests/caf_beams_model.py), whose docstring derives the bars: float32
restatements in other orders meet them; the identities that tie the beam maps to the bearings' statistic and to the array map; the
fusion does not depend on the candidates' order of arrival; the weak scene of the issue, which the array map's detector does not see
and the bank does; and every single mistake about the maps misses a bar and changes the scene's fused list, every one about the
fusion changes a hand-made line's.  The scene also needs the
library's own steering helper (crsdr_caf_beam_steer), so that a build without the beams fails here."""
import importlib

import numpy as np
import pytest

import caf_beams_model as B
import caf_bearing_model as BM
import caf_cfar_model as CF
import caf_model as M

U, E64 = M.U, M.E64


def _chi(nrows, nd, R, seed, scale=1e-3):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((nrows, nd, R)) + 1j * rng.standard_normal((nrows, nd, R))) * scale
    return x.astype(np.complex64)


def _w(nb, m, seed):
    rng = np.random.default_rng(seed)
    return ((rng.standard_normal((nb, m)) + 1j * rng.standard_normal((nb, m))) / np.sqrt(2 * m)).astype(np.complex64)


@pytest.mark.parametrize("m, nb, ref", [(1, 1, 0), (2, 3, 2), (21, 33, 5), (64, 64, 64)])
def test_float32_restatements_in_other_orders_meet_the_bars(m, nb, ref):
    chi = _chi(m + 1, 8, 5, 10 + m)
    chi[:, 1, 2] = 0
    chi[:, 2, 3] *= np.float32(1e-36)                                           # fp32 subnormals
    W = _w(nb, m, 20 + m)
    W[nb // 2] = 0
    P, bar = B.bmap(chi, ref, W)
    worst = 0.0
    for kw in (dict(), dict(reverse=True), dict(split=True), dict(reverse=True, split=True)):
        got = B.bmap_f32(chi, ref, W, **kw).astype(np.float64)
        assert np.all(np.isfinite(got))
        assert np.all(np.abs(got - P) <= bar), (kw, float(np.max(np.abs(got - P) / bar)))
        worst = max(worst, float(np.max(np.abs(got - P) / bar)))
    print(f"m {m} nb {nb}: worst error / bar {worst:.3f}")
    assert not P[nb // 2].any() and not P[:, 1, 2].any()
    # the bar is no blanket: it is a few units of the last place of the terms' magnitudes
    assert np.all(bar <= 16.0 * m * U * (np.abs(W).astype(np.float64) ** 2).sum(1)[:, None, None] * M.array_map(chi, ref)[0][None] + 1e-40)


@pytest.mark.parametrize("sc", BM.SCENES[:2], ids=[BM.scene_id(s) for s in BM.SCENES[:2]])
def test_steered_beams_are_the_bearings_statistic_times_the_array_map(sc):
    line, q, _ = BM.scene_line(sc)
    chi, _ = BM.scene_maps(sc, line)
    nc = sc[3]
    xy = np.array([sc[8], (1.0, 1.0), (nc / 2, nc / 2), (nc - 1.5, 3.25), (0.0, nc - 1.0)], dtype=np.float64)
    W = B.steer_weights(q, xy)
    P, bar = B.bmap(chi, 0, W)
    amap = M.array_map(chi, 0)[0]
    tbar = BM.t_bar(q, 0, 1.0)
    nd, R = chi.shape[1:]
    worst = 0.0
    # (the weights are rounded once to float32 on the way: far inside the map's own bar, which is gamma_(2m) of the same terms)
    for d, tau in [(0, 0), (sc[10] % nd, sc[9]), (nd - 1, R - 1), (nd // 2, 1)]:
        T = BM.stat(np.eye(q.m), BM.snapshot(chi, 0, d, tau), BM.steer(q, xy[:, 0], xy[:, 1]))
        err = np.abs(P[:, d, tau] - T * amap[d, tau])
        worst = max(worst, float(np.max(err / (bar[:, d, tau] + tbar * amap[d, tau]))))
        assert np.all(err <= bar[:, d, tau] + tbar * amap[d, tau]), (d, tau, err, bar[:, d, tau])
    print(f"scene {BM.scene_id(sc)}: worst error over the sum of the two bars {worst:.3f}")
    # and the beam toward the echo holds most of its cell's power
    assert P[0, sc[10] % nd, sc[9]] > 0.5 * amap[sc[10] % nd, sc[9]]


@pytest.mark.parametrize("m", [1, 6, 21, 64])
def test_a_unitary_bank_sums_to_the_array_map(m):
    chi = _chi(m + 1, 8, 6, 30 + m)
    ref = m // 2
    F = (np.exp(2j * np.pi * np.outer(np.arange(m), np.arange(m)) / m) / np.sqrt(m)).astype(np.complex64)
    P, bar = B.bmap(chi, ref, F)
    amap = M.array_map(chi, ref)[0]
    # the rounded bank is unitary to |dF|_F <= sqrt(2 m) U: |F x|^2 is off by at most (2 |dF| + |dF|^2) |x|^2
    assert np.all(np.abs(P.sum(0) - amap) <= bar.sum(0) + 3.0 * np.sqrt(2.0 * m) * U * amap)


def test_the_fusion_does_not_depend_on_the_order_of_arrival():
    rng = np.random.default_rng(5)
    nb, K, nd, R = 6, 5, 8, 6
    entries = []
    for b in range(nb):
        cells = rng.choice(nd * R, size=(7, 3, 0, 6, 5, 4)[b], replace=False)
        powers = np.sort(rng.integers(1, 6, size=len(cells)).astype(np.float64))[::-1]      # many ties across the beams
        entries += [(b, int(c) // R, int(c) % R, float(p)) for c, p in zip(cells, powers)]
    bdet, bcount = B.hand_lists(entries, nb, K, nd)
    want, nf = B.fuse(bdet, bcount, nd, R)
    n = int(np.minimum(bcount, K).sum())
    assert 0 < nf <= n and bcount.max() > K
    for seed in range(6):
        got, gnf = B.fuse(bdet, bcount, nd, R, arrival=np.random.default_rng(seed).permutation(n))
        assert gnf == nf and np.array_equal(got, want)
    # a survivor has no survivor within one cell of it, and every suppressed candidate has an earlier one beside it
    live = [(int(r[1]) % nd, int(r[0])) for r in want[:min(nf, K)]]
    assert all(not B._near(live[i], live[j], nd, R, None) for i in range(len(live)) for j in range(i))


@pytest.mark.parametrize("name", list(B.HAND_FUSE), ids=list(B.HAND_FUSE))
def test_hand_made_lists_fuse_as_the_definition_says(name):
    entries, survivors = B.HAND_FUSE[name]
    nb, K = 4, 4
    bdet, bcount = B.hand_lists(entries, nb, K, B.HAND_ND)
    fused, nf = B.fuse(bdet, bcount, B.HAND_ND, B.HAND_R)
    assert nf == len(survivors)
    s = M.signed_bins(B.HAND_ND)
    for k, (b, d, tau) in enumerate(survivors):
        assert (fused[k][7], fused[k][1], fused[k][0]) == (b, s[d], tau), (name, fused)
        assert np.array_equal(fused[k][:7], bdet[b][[q for q in range(K) if (bdet[b][q][0], bdet[b][q][1]) == (tau, s[d])][0]][:7])
    assert not fused[len(survivors):].any()


@pytest.fixture(scope="module")
def binding():
    b = importlib.import_module("coherent-rtlsdr_amd.binding")
    b.build()
    return b


@pytest.fixture(scope="module")
def weak():
    """the weak scene's lines, seeds 0 .. 3, each with its model result at alpha 16: computed once"""
    w = B.WEAK
    prm = CF.Params(w["alpha"], max_det=w["max_det"], **w["cfar"])
    out = []
    for seed in w["seeds"]:
        chi, map32, q, W, echo = B.weak_line(seed)
        out.append((chi, map32, q, W, echo, B.line(chi, 0, W, w["guard"], prm)))
    return out


@pytest.mark.parametrize("k", range(4), ids=[f"seed {s}" for s in B.WEAK["seeds"]])
def test_the_bank_detects_the_echo_the_array_map_misses(weak, binding, k):
    w = B.WEAK
    chi, map32, q, W, (lag, dop), got = weak[k]
    # the library's own weights are the model's within the allowance, and the lattice is the issue's
    xy = B.lattice(8, 8, q.ncx)
    assert tuple(xy[20]) == (31.0, 62.0) and tuple(xy[0]) == (6.0, 12.0) and tuple(xy[63]) == (93.5, 99.5)
    lib = binding.beam_steer(q.mx, q.my, q.d, xy, q.ncx, q.ncy)
    dw = lib.astype(np.complex128) - W.astype(np.complex128)
    assert np.all(np.abs(dw.real) <= B.steer_bar(q)[None]) and np.all(np.abs(dw.imag) <= B.steer_bar(q)[None])
    assert got["ambiguous"] == 0
    nd = chi.shape[1]
    hits = [b for b in range(64) for r in got["bdet"][b][:min(int(got["bcount"][b]), w["max_det"])] if (r[0], r[1]) == (lag, dop)]
    others = [(b, r[0], r[1]) for b in range(64) for r in got["bdet"][b][:min(int(got["bcount"][b]), w["max_det"])] if (r[0], r[1]) != (lag, dop)]
    P = got["bmap32"].astype(np.float64)
    ratio, aratio = P[w["beam"], dop % nd, lag] / np.median(P), float(map32[dop % nd, lag]) / float(np.median(map32))
    print(f"seed {w['seeds'][k]}: the echo's cell in beams {hits}, fused {got['fused'][:got['nfused']]}, over the median {ratio:.0f} (array map {aratio:.1f})")
    assert got["nfused"] == 1 and tuple(got["fused"][0][[0, 1, 7]]) == (lag, dop, w["beam"]), got["fused"][:got["nfused"]]
    assert not got["fused"][1:].any() and w["beam"] in hits and len(hits) >= 2 and not others
    assert ratio > 100.0 and aratio < 10.0
    for alpha in w["map_alphas"]:
        r = CF.detect(map32.astype(np.float64), w["guard"], CF.Params(alpha, max_det=64, **w["cfar"]))
        assert r["ambiguous"] == 0 and r["count"] <= 64
        assert (dop % nd) * chi.shape[2] + lag not in r["cells"], alpha


@pytest.mark.parametrize("which", B.MUTATIONS)
def test_every_single_mistake_in_the_maps_misses_a_bar_or_changes_the_list(weak, which):
    chi, map32, q, W, echo, good = weak[0]
    P, bar = B.bmap(chi, 0, W)
    bad = B.bmap(chi, 0, W, which)[0]
    w = B.WEAK
    wrong = B.line(chi, 0, W, w["guard"], CF.Params(w["alpha"], max_det=w["max_det"], **w["cfar"]), which)
    misses = bool(np.any(np.abs(bad - P) > bar))
    changes = wrong["nfused"] != good["nfused"] or not np.array_equal(wrong["fused"], good["fused"])
    print(f"{which}: misses a bar {misses}, changes the fused list {changes}")
    assert misses and changes, which


# the hand-made list on which each mistake of the fusion shows
FUSE_SHOWS = {"lag_wrap": "lags 0 and R - 1 are no neighbours", "doppler_nowrap": "neighbours across the Doppler wrap",
              "same_cell": "a chain A > B > C one cell apart each: only A survives", "tie_reversed": "equal powers in two beams",
              "dead_cannot_suppress": "a chain A > B > C one cell apart each: only A survives"}


@pytest.mark.parametrize("which", B.FUSE_MUTATIONS)
def test_every_single_mistake_in_the_fusion_changes_the_list(which):
    entries, _ = B.HAND_FUSE[FUSE_SHOWS[which]]
    bdet, bcount = B.hand_lists(entries, 4, 4, B.HAND_ND)
    good, nf = B.fuse(bdet, bcount, B.HAND_ND, B.HAND_R)
    bad, bnf = B.fuse(bdet, bcount, B.HAND_ND, B.HAND_R, which)
    assert bnf != nf or not np.array_equal(bad, good), which
