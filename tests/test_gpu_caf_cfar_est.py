"""GPU checks of the greatest-of, smallest-of and ordered-statistic CFAR estimators (crsdr_caf_set_cfar_estimator, crsdr_cfar_est) against
the fp64 numpy model in tests/caf_cfar_est_model.py, whose docstring derives the bars used here.  The model is always run on the
device's own inputs.  Every comparison first asserts that the model finds NO ambiguous cell (|P - t| <= 2^-40 t) and NO half-ambiguous
cell (two counting halves of different sizes with means within 2^-40) in them: away from such cells every decision is exact on both
sides, so

    the detection set, its order and count     equal
    lag, doppler, ntrain                       equal
    OS: power, snr, noise                      the model's rounded once to fp32, bit for bit
    GO, SO: power, snr, noise, dlag, ddop      within the fp64 bars

Maps of small integers are the ordered statistic's alone here (its noise is a map value: nothing is ambiguous): on a constant floor
every pair of unequal halves has equal means."""
import importlib

import numpy as np
import pytest

import caf_cfar_est_model as E
import caf_cfar_model as C
import caf_model as M

pytestmark = pytest.mark.gpu
EINVAL, ESTATE = -1, -5
RECT, HANN = M.WINDOW_RECT, M.WINDOW_HANN
TILE_D, TILE_L = 16, 64                                                          # the kernels' tile (csrc/caf_cfar_kernels.hpp)


@pytest.fixture(scope="module")
def b():
    binding = importlib.import_module("coherent-rtlsdr_amd.binding")
    if binding.device_count() < 1:
        pytest.fail("no HIP device: the product path has no CPU fallback")
    return binding


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


def _desc(b, q):
    return b.cfar_desc(alpha=q.alpha, gd=q.gd, gr=q.gr, td=q.td, tr=q.tr, min_train=q.min_train, max_det=q.max_det)


def _est(b, est):
    return b.CfarEstDesc(est.est, est.axis, est.rank)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same_bits(a, c):
    return a.shape == c.shape and np.array_equal(_bits(a), _bits(c))


def _name(est):
    return {E.CA: "ca", E.GO: f"go axis {est.axis}", E.SO: f"so axis {est.axis}", E.OS: f"os rank {est.rank}"}[est.est]


def _hold(det, count, src, guard, q, est, tag):
    """one map's detections against the model on the same array; returns the model's result"""
    P = M.power(src) if np.iscomplexobj(src) else np.asarray(src, dtype=np.float64)
    want = E.detect(P, guard, q, est)
    tag = f"{tag}, {_name(est)}"
    assert want["ambiguous"] == 0 and want["half_ambiguous"] == 0, f"{tag}: the model finds {want['ambiguous']} ambiguous and {want['half_ambiguous']} half-ambiguous cell(s)"
    assert np.all(np.isfinite(det)), tag
    assert int(count) == want["count"], (tag, int(count), want["count"])
    assert np.array_equal(det[:, [0, 1, 7]].astype(np.float64), want["det"][:, [0, 1, 7]]), (tag, det, want["det"])
    err = np.abs(det.astype(np.float64) - want["det"])
    assert np.all(err <= want["bar"]), (tag, det, want["det"], want["bar"])
    if est.est == E.OS:
        assert _same_bits(np.ascontiguousarray(det[:, [2, 3, 4]]), np.ascontiguousarray(want["det"][:, [2, 3, 4]].astype(np.float32))), (tag, det, want["det"])
    assert not det[min(want["count"], q.max_det):].any(), tag
    return want


def _per_op(b, src, guard, q, est, tag):
    det, count = b.cfar_est(src, guard, _desc(b, q), _est(b, est))
    want = _hold(det, count, src, guard, q, est, tag)
    print(f"{tag}, {_name(est)}: {src.shape} guard {guard}: count {count}, over the threshold {want['passed']}, first {det[0][:5]} ntrain {det[0][7]}")
    return det, count, want


def _floor(nd, R, seed, complex_=False):
    rng = np.random.default_rng(seed)
    if complex_:
        return (np.sqrt(0.5) * (rng.standard_normal((nd, R)) + 1j * rng.standard_normal((nd, R)))).astype(np.complex64)
    return rng.exponential(1.0, size=(nd, R)).astype(np.float32)


def _plant(a, cells, base=200.0):
    """distinct powers at `cells`, an uneven neighbour beside each for offsets that are not zero"""
    nd, R = a.shape
    for k, (d, t) in enumerate(cells):
        a[d, t] = base + 7.0 * k
        if t + 1 < R and (d, t + 1) not in cells:
            a[d, t + 1] = 20.0
    return a


def _ests(q, ranks=None):
    """all three new estimators, both axes, and the ranks 1, Nfull / 2 and Nfull"""
    Nfull = E.full_count(q)
    ranks = ranks or sorted({1, max(1, Nfull // 2), Nfull})
    return [E.Est(E.GO, E.LAG), E.Est(E.GO, E.DOPPLER), E.Est(E.SO, E.LAG), E.Est(E.SO, E.DOPPLER)] + [E.Est(E.OS, 0, r) for r in ranks]


# (tag, nd, R, guard, Params, planted cells, complex): the smallest shapes at which each path can go wrong
SHAPES = [
    ("nd 8 under Hd 3", 8, 40, 0, C.Params(6.0, 1, 1, 2, 4), [(0, 0), (7, 39), (4, 20)], False),
    ("nd 8 under Hd 3, behind a guard", 8, 40, 2, C.Params(6.0, 1, 1, 2, 4), [(2, 0), (6, 39), (4, 20)], True),
    ("R 1", 32, 1, 1, C.Params(5.0, 0, 0, 3, 0), [(1, 0), (16, 0), (26, 0)], False),
    ("R 5 under Hr 16", 16, 5, 0, C.Params(6.0, 1, 1, 2, 15), [(0, 0), (15, 4), (8, 2)], True),
    ("R 65, a lag tile of one", 32, 65, 2, C.Params(6.0, 1, 1, 3, 4), [(2, 64), (30, 63), (16, 0), (15, 64)], False),
    ("guard nd / 2", 16, 40, 8, C.Params(6.0, 1, 1, 3, 4), [(8, 20), (8, 0)], False),
    ("Hd 0", 32, 70, 0, C.Params(6.0, 0, 1, 0, 9), [(0, 0), (31, 69), (15, 63), (16, 65)], False),
    ("Hr 0", 32, 70, 1, C.Params(6.0, 1, 0, 5, 0), [(1, 0), (31, 69), (15, 64), (16, 62)], True),
    ("gd 0 and gr 0", 16, 66, 0, C.Params(6.0, 0, 0, 2, 5), [(0, 0), (15, 65), (7, 64)], False),
    ("the largest window", 32, 70, 0, C.Params(6.0, 2, 4, 6, 12), [(0, 0), (31, 69), (15, 62), (16, 64)], False),
]


@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_shapes_per_op(b, shape):
    tag, nd, R, guard, q, cells, complex_ = shape
    a = _plant(_floor(nd, R, 31 * nd + R, complex_), cells)
    s = M.signed_bins(nd)
    for est in _ests(q):
        det, count, want = _per_op(b, a, guard, q, est, tag)
        if est.est == E.OS and est.rank == max(1, E.full_count(q) // 2):         # (the median is above no planted cell: K = 16 holds them all)
            assert {(t, int(s[d])) for d, t in cells} <= {(int(x[0]), int(x[1])) for x in det[:count]}, (tag, det)
    if tag == "Hr 0":                                                            # over lag both halves are empty: no estimate anywhere
        for kind in (E.GO, E.SO):
            det, count = b.cfar_est(a, guard, _desc(b, q), b.CfarEstDesc(kind, 0, 0))
            assert count == 0 and not det.any()


def test_two_by_two_tiles_with_cells_either_side_of_every_edge(b):
    """nd 32, R 96: 2 x 2 tiles, the lag tile ragged; a planted cell on either side of every tile edge, the cyclic wrap and the map's
    edges included; cells that would be neighbours go to different maps"""
    nd, R = 32, 96
    q = C.Params(6.0, 1, 1, 3, 4, max_det=32)
    s = M.signed_bins(nd)
    for k in range(4):
        ds = (TILE_D - 1, nd - 1) if k < 2 else (TILE_D, 0)
        ls = (TILE_L - 1, R - 1) if k % 2 == 0 else (0, TILE_L)
        cells = [(d, t) for d in ds for t in ls]
        a = _plant(_floor(nd, R, 170 + k), cells)
        for est in _ests(q, ranks=[1, 67, 90]):
            det, count, _ = _per_op(b, a, 0, q, est, f"tile edges, map {k}")
            if est.est == E.OS and est.rank == 67:
                assert [(int(x[0]), int(x[1])) for x in det[:len(cells)]] == [(t, int(s[d])) for d, t in reversed(cells)], (k, det[:8])


def test_min_train_and_nothing_to_train_on(b):
    a = _plant(_floor(16, 40, 9), [(8, 20), (3, 1)])
    for est in _ests(C.Params(2.0, 1, 1, 3, 0)):
        det, count, _ = _per_op(b, a, 8, C.Params(2.0, 1, 1, 3, 0), est, "guard nd / 2, training over Doppler only")
        assert count == 0 and not det.any()
    q = C.Params(4.0, 0, 0, 1, 2, min_train=4, max_det=32)                        # at lag 1 the lower lag half holds three cells: it does not count
    for est in _ests(q):
        _per_op(b, a, 0, q, est, "a half below min_train")
    q = C.Params(4.0, 0, 0, 1, 2, min_train=15, max_det=32)                       # above Nfull = 14
    for est in _ests(q):
        det, count, _ = _per_op(b, a, 0, q, est, "min_train above every N")
        assert count == 0 and not det.any()


def test_integer_plateaus_and_duplicated_values_across_tile_edges(b):
    """the ordered statistic on maps of three small integers, each many times in every window, with plateaus across the tile edges: ties
    in the selection, and a plateau gives its first cell"""
    nd, R = 32, 96
    a = np.tile(np.array([1.0, 2.0, 3.0], dtype=np.float32), (nd, R // 3))
    for d, t in ((15, 63), (15, 64), (16, 63), (16, 64), (3, 94), (3, 95), (15, 10), (16, 10), (31, 80), (0, 80)):
        a[d, t] = 90.0
    for q in (C.Params(4.0, 1, 1, 3, 4, max_det=8), C.Params(4.0, 2, 4, 6, 12, max_det=8)):
        Nfull = E.full_count(q)
        for rank in (1, Nfull // 3, Nfull // 3 + 1, Nfull // 2, (2 * Nfull) // 3, (2 * Nfull) // 3 + 1, Nfull):
            det, count, _ = _per_op(b, a, 0, q, E.Est(E.OS, 0, rank), f"integers, Hd {q.Hd}")
            if rank <= (2 * Nfull) // 3:
                assert count == 4 and [(int(x[0]), int(x[1])) for x in det[:4]] == [(80, 0), (94, 3), (10, 15), (63, 15)], det[:6]
                assert set(det[:4, 4]) <= {1.0, 2.0, 3.0}
    c = (a * (1 + 0j)).astype(np.complex64)                                       # powers 1, 4, 9 and 8100 from a chi
    _per_op(b, c, 0, C.Params(4.0, 1, 1, 3, 4, max_det=8), E.Est(E.OS, 0, 45), "integers from a chi")


def test_true_zeros_next_to_the_lag_edge_and_the_ridge(b):
    """cells of S whose P is 0 are present and absent cells are not zeros: zeros on both lag edges and on the bins next to the ridge"""
    nd, R, guard = 16, 70, 3
    a = _floor(nd, R, 5)
    a[:, 0], a[:, R - 1], a[3, :], a[nd - 3, :] = 0.0, 0.0, 0.0, 0.0
    a[4, 1], a[9, R - 2], a[5, 30], a[nd - 4, 64] = 30.0, 30.0, 30.0, 30.0
    q = C.Params(3.0, 1, 1, 2, 4, max_det=32)
    for g in (0, guard):
        for est in _ests(q, ranks=[1, 2, 6, 20, 60, E.full_count(q)]):
            _per_op(b, a, g, q, est, f"true zeros, guard {g}")
    half0 = _floor(nd, R, 6)
    half0[:, :10] = 0.0                                                          # an all-zero lower lag half beside lags 10 .. 14
    half0[6, 10], half0[9, 40] = 20.0, 20.0
    det, count, _ = _per_op(b, half0, 0, q, E.Est(E.SO, E.LAG), "smallest-of beside an all-zero half")
    assert (10.0, 6.0) not in {(float(x[0]), float(x[1])) for x in det[:count]}
    det, count, _ = _per_op(b, half0, 0, q, E.Est(E.GO, E.LAG), "greatest-of beside an all-zero half")
    assert (10.0, 6.0) in {(float(x[0]), float(x[1])) for x in det[:count]}
    for rank in (1, 25, 26, 50):
        _per_op(b, half0, 0, q, E.Est(E.OS, 0, rank), "the ordered statistic beside zeros")


@pytest.mark.parametrize("K", [1, 5, 64])
def test_more_detections_than_slots(b, K):
    """count exceeds K; the K kept are those of largest power, ties by index -- inside one tile, and spread over all four"""
    nd, R = 32, 96
    q = C.Params(2.0, 0, 0, 1, 1, max_det=K)
    a = _floor(nd, R, 8)
    a[::4, ::3] = (90.0 + (np.arange(32) % 7)[None, :]).astype(np.float32)       # 256 cells of seven powers over the four tiles
    for est in (E.Est(E.GO, E.LAG), E.Est(E.SO, E.DOPPLER), E.Est(E.OS, 0, 4)):
        det, count, _ = _per_op(b, a, 0, q, est, f"many tiles, K {K}")
        assert count >= 256 and np.all(det[:min(K, 32), 2] == 96)
    one = _floor(nd, R, 9)
    one[0:16:2, 0:64:2] = (90.0 + (np.arange(32) % 5)[None, :]).astype(np.float32)
    for est in (E.Est(E.SO, E.LAG), E.Est(E.OS, 0, 5)):
        det, count, _ = _per_op(b, one, 0, q, est, f"one tile, K {K}")
        assert count >= 256 and np.all(det[:min(K, 48), 2] == 94)


def test_zero_and_full_scale(b):
    q = C.Params(6.0, 1, 1, 3, 4, max_det=64)
    for est in _ests(q):
        for a in (np.zeros((32, 70), dtype=np.float32), np.zeros((8, 1), dtype=np.complex64)):
            qq = C.Params(6.0, 0, 0, 3, 0, max_det=64) if a.shape[1] == 1 else q
            det, count = b.cfar_est(a, 0, _desc(b, qq), _est(b, E.Est(est.est, est.axis, min(est.rank, E.full_count(qq)))))
            assert count == 0 and not det.any() and np.all(np.isfinite(det))
    full = (_floor(32, 70, 4) * np.float32(1e36)).astype(np.float32)
    full[5, 5], full[20, 69] = 3.4e38, 3.0e38                                     # the largest fp32 there is
    for est in _ests(q):
        det, count, _ = _per_op(b, full, 0, q, est, "full scale")
        if est.est != E.OS or est.rank < 90:
            assert count >= 2 and (det[0][0], det[0][1], det[1][0], det[1][1]) == (5, 5, 69, -12)


def test_cell_averaging_through_cfar_est_is_cfar(b, torch):
    q = C.Params(5.0, 1, 1, 3, 4, max_det=16)
    for a, guard in ((_plant(_floor(32, 96, 3), [(0, 0), (15, 63), (16, 64)]), 0), (_plant(_floor(16, 40, 4, True), [(2, 0), (14, 39)]), 2)):
        want = b.cfar(a, guard, _desc(b, q))
        for e in (None, b.CfarEstDesc(0, 0, 0), b.CfarEstDesc(0, 7, -3)):
            det, count = b.cfar_est(a, guard, _desc(b, q), e)
            assert _same_bits(det, want[0]) and count == want[1] and count >= 2
    dev = torch.device("cuda", 0)
    a = _plant(_floor(32, 96, 3), [(0, 0), (15, 63)])
    src = torch.from_numpy(a.copy()).to(dev)
    for e in (None, b.CfarEstDesc(3, 0, 67), b.CfarEstDesc(2, 1, 0)):
        dd, dn = torch.zeros(q.max_det * 8, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
        b.cfar_est_device(dd.data_ptr(), dn.data_ptr(), src.data_ptr(), 1, 32, 96, 0, _desc(b, q), e)
        det, count = b.cfar_est(a, 0, _desc(b, q), e)
        assert _same_bits(dd.cpu().numpy().reshape(q.max_det, 8), det) and int(dn.cpu()[0]) == count


# ---- through the engine ----
class Packets:
    """T packet-shaped slots on the device, as a plan lays them out: packet t at base + t * stride, its matrix [nrows][B] at + 16 + 4 nrows"""

    def __init__(self, torch, blocks, pad=0):
        blocks = np.ascontiguousarray(blocks)
        self.T, self.nrows, self.B = blocks.shape
        self.offset = 16 + 4 * self.nrows
        self.stride = self.offset + self.nrows * self.B + pad
        host = np.full((self.T, self.stride), 0x55, dtype=np.int8)
        host[:, self.offset:self.offset + self.nrows * self.B] = blocks.reshape(self.T, -1)
        self.buf = torch.from_numpy(host).to(torch.device("cuda", 0))
        self.ptr = self.buf.data_ptr()


def _run(b, torch, blocks, seg, nlags, ref, kind, guard, frames, q, est, pad=0, max_batch=None):
    """every line of `blocks` [T][nrows][B] through the engine with the detector on under est -> {chi, map, peak, det, count, snap}"""
    T, nrows, B = blocks.shape
    pk = Packets(torch, blocks, pad)
    cf = b.Caf(nrows, B, seg, nlags, ref, kind, guard, max_batch=max_batch or T, frames=frames)
    cf.set_cfar(_desc(b, q))
    cf.set_cfar_estimator(None if est is None else _est(b, est))
    cf.submit(pk.ptr, pk.stride, pk.offset, T)
    assert cf._last() == (T // frames, 5)                                        # (as many launches as under cell averaging)
    out = {**cf.fetch(), **cf.fetch_cfar()}
    cf.close()
    return out


def _hold_line(out, e, guard, q, est, tag):
    chi, mp = out["chi"][e], out["map"][e]
    wants = [_hold(out["det"][e][entry], out["count"][e][entry], src, guard, q, est, f"{tag} entry {entry}") for entry, src in enumerate(list(chi) + [mp])]
    snap = C.snapshot(chi, wants[-1]["cells"], q.max_det)
    assert _same_bits(out["snap"][e].view(np.float32), snap.view(np.float32)), tag
    return wants


def test_the_masking_scene_as_echoes(b, torch):
    """row 1 carries an echo at lag 9 and one 11 dB down four lags on, at the same Doppler; row 2 one of its own.  Cell averaging and
    greatest-of lose the weaker echo under the stronger one's share of the mean; smallest-of and the ordered statistic report it"""
    B, frames, seg, R, nrows, guard = 4096, 4, 64, 32, 3, 2
    line = M.echo_scene(B, frames, [(1, 9, 20, 0.3), (1, 13, 20, 0.08), (2, 17, -13, 0.15)], nrows=nrows, seed=0)
    for est, n, row1, arr in ((E.Est(E.CA), 90, [(9, 20)], [(9, 20), (17, -13)]), (E.Est(E.GO, E.LAG), 42, [(9, 20)], [(9, 20), (17, -13)]),
                              (E.Est(E.SO, E.LAG), 42, [(9, 20), (13, 20)], [(9, 20), (17, -13), (13, 20)]),
                              (E.Est(E.OS, 0, 67), 90, [(9, 20), (13, 20)], [(9, 20), (17, -13), (13, 20)])):
        q = C.Params(b.cfar_alpha_est(1e-6, n, _est(b, est)), 1, 1, 3, 4)
        out = _run(b, torch, np.stack(line), seg, R, 0, HANN, guard, frames, q, est)
        _hold_line(out, 0, guard, q, est, "masking scene")
        got1 = [(int(x[0]), int(x[1])) for x in out["det"][0][1][:out["count"][0][1]]]
        gota = [(int(x[0]), int(x[1])) for x in out["det"][0][nrows][:out["count"][0][nrows]]]
        print(_name(est), "row 1", got1, "array map", gota)
        assert got1 == row1 and gota == arr, (_name(est), got1, gota)


def _same_line(x, e, y, f):
    return all(_same_bits(x[k][e].view(np.float32) if np.iscomplexobj(x[k]) else x[k][e], y[k][f].view(np.float32) if np.iscomplexobj(y[k]) else y[k][f])
               for k in ("chi", "map", "peak", "det", "count", "snap"))


@pytest.mark.parametrize("est", [E.Est(E.GO, E.DOPPLER), E.Est(E.SO, E.LAG), E.Est(E.OS, 0, 60)], ids=_name)
def test_a_line_has_its_bits_anywhere_and_from_the_per_op_call(b, torch, est):
    nrows, B, seg, nlags, ref, kind, guard = 3, 2048, 64, 17, 2, HANN, 1
    q = C.Params(3.0, 1, 1, 3, 4, max_det=8)                                     # a low threshold on noise: lists that are not empty
    blocks = np.stack([M.random_matrix(nrows, B, 900 + t) for t in range(8)])
    blocks[7] = blocks[0]
    alone = _run(b, torch, blocks[:1], seg, nlags, ref, kind, guard, 1, q, est, max_batch=8)
    batch = _run(b, torch, blocks, seg, nlags, ref, kind, guard, 1, q, est, pad=40)
    assert alone["count"][0].min() >= 1
    assert _same_line(alone, 0, batch, 0) and _same_line(alone, 0, batch, 7)
    assert not _same_line(alone, 0, batch, 1)
    _hold_line(batch, 3, guard, q, est, "line 3 of 8")
    for entry, src in enumerate(list(alone["chi"][0]) + [alone["map"][0]]):      # the per-op call on the fetched arrays
        det, count = b.cfar_est(src, guard, _desc(b, q), _est(b, est))
        assert _same_bits(det, alone["det"][0][entry]) and count == alone["count"][0][entry], entry


def test_the_ordered_statistic_on_the_beam_maps(b, torch):
    nrows, B, seg, nlags, guard = 4, 2048, 64, 16, 1
    q, est = C.Params(3.0, 1, 1, 2, 3, max_det=8), E.Est(E.OS, 0, 40)
    blocks = np.stack([M.random_matrix(nrows, B, 700 + t) for t in range(2)])
    pk = Packets(torch, blocks)
    rng = np.random.default_rng(12)
    w = (rng.standard_normal((3, nrows - 1)) + 1j * rng.standard_normal((3, nrows - 1))).astype(np.complex64)
    cf = b.Caf(nrows, B, seg, nlags, 0, HANN, guard, max_batch=2)
    cf.set_cfar(_desc(b, q))
    plain = b.Caf(nrows, B, seg, nlags, 0, HANN, guard, max_batch=2)
    plain.set_cfar(_desc(b, q))
    plain.set_beams(w)
    plain.submit(pk.ptr, pk.stride, pk.offset, 2)
    cf.set_cfar_estimator(_est(b, est))
    cf.set_beams(w)
    cf.submit(pk.ptr, pk.stride, pk.offset, 2)
    assert cf._last() == plain._last()                                           # the launches of a submit do not change
    out = cf.fetch_beams(lists=True)
    hits = 0
    for e in range(2):
        for k in range(3):
            det, count = b.cfar_est(out["bmap"][e][k], guard, _desc(b, q), _est(b, est))
            assert _same_bits(det, out["bdet"][e][k]) and count == out["bcount"][e][k], (e, k)
            _hold(out["bdet"][e][k], out["bcount"][e][k], out["bmap"][e][k], guard, q, est, f"beam map {e} {k}")
            hits += int(count)
    assert hits >= 1
    cf.close()
    plain.close()


def test_set_cfar_puts_the_estimator_back(b, torch):
    nrows, B, seg, nlags, guard = 3, 2048, 64, 16, 1
    q = C.Params(3.0, 1, 1, 3, 4, max_det=8)
    blocks = np.stack([M.random_matrix(nrows, B, 40)])
    pk = Packets(torch, blocks)
    plain = _run(b, torch, blocks, seg, nlags, 0, HANN, guard, 1, q, None)
    cf = b.Caf(nrows, B, seg, nlags, 0, HANN, guard, max_batch=1)
    cf.set_cfar(_desc(b, q))
    cf.set_cfar_estimator(b.CfarEstDesc(3, 0, 20))
    cf.submit(pk.ptr, pk.stride, pk.offset, 1)
    other = cf.fetch_cfar()
    assert not _same_bits(other["det"], plain["det"])
    cf.set_cfar(_desc(b, q))                                                     # the same descriptor again: cell averaging
    with pytest.raises(b.CrsdrError) as e:
        cf.fetch_cfar()
    assert e.value.code == ESTATE
    cf.submit(pk.ptr, pk.stride, pk.offset, 1)
    back = cf.fetch_cfar()
    assert all(_same_bits(back[k].view(np.float32) if k == "snap" else back[k], plain[k].view(np.float32) if k == "snap" else plain[k]) for k in ("det", "count", "snap"))
    cf.set_cfar_estimator(b.CfarEstDesc(1, 1, 0))
    with pytest.raises(b.CrsdrError) as e:
        cf.fetch_cfar()                                                          # nothing submitted since the estimator was set
    assert e.value.code == ESTATE
    cf.set_cfar_estimator(None)                                                  # NULL: cell averaging
    cf.submit(pk.ptr, pk.stride, pk.offset, 1)
    assert _same_bits(cf.fetch_cfar()["det"], plain["det"])
    cf.set_cfar(None)
    with pytest.raises(b.CrsdrError) as e:
        cf.set_cfar_estimator(b.CfarEstDesc(1, 1, 0))                            # no detector set
    assert e.value.code == ESTATE
    cf.close()


def test_refusals(b, torch):
    good = dict(gd=1, gr=1, td=3, tr=4, alpha=14.93, min_train=1, max_det=16)    # Nfull 90
    bad = [(-1, 0, 1), (4, 0, 1), (1, -1, 0), (1, 2, 0), (2, 2, 0), (3, 0, 0), (3, 0, 91), (3, 0, -1)]
    cf = b.Caf(4, 2048, 64, 16, max_batch=2)
    with pytest.raises(b.CrsdrError) as e:
        cf.set_cfar_estimator(b.CfarEstDesc(1, 0, 0))
    assert e.value.code == ESTATE                                                # no detector set
    cf.set_cfar(b.cfar_desc(**good))
    for est in bad:
        with pytest.raises(b.CrsdrError) as e:
            cf.set_cfar_estimator(b.CfarEstDesc(*est))
        assert e.value.code == EINVAL, est
        with pytest.raises(b.CrsdrError) as e:
            b.cfar_est(np.ones((16, 16), dtype=np.float32), 0, b.cfar_desc(**good), b.CfarEstDesc(*est))
        assert e.value.code == EINVAL, est
    cf.set_cfar_estimator(b.CfarEstDesc(3, 0, 90))
    # while bearings, beams or the tracker are on the estimator stays as it is
    cf.set_bearing(b.bearing_desc(3, 1, 0.5, ncx=20, ncy=20))
    with pytest.raises(b.CrsdrError) as e:
        cf.set_cfar_estimator(None)
    assert e.value.code == ESTATE
    cf.set_bearing(None)
    cf.set_beams(np.ones((2, 3), dtype=np.complex64))
    with pytest.raises(b.CrsdrError) as e:
        cf.set_cfar_estimator(b.CfarEstDesc(1, 0, 0))
    assert e.value.code == ESTATE
    cf.set_beams(None)
    cf.set_track(b.track_desc(8))
    with pytest.raises(b.CrsdrError) as e:
        cf.set_cfar_estimator(b.CfarEstDesc(2, 1, 0))
    assert e.value.code == ESTATE
    cf.set_track(None)
    cf.set_cfar_estimator(b.CfarEstDesc(2, 1, 0))
    cf.close()
