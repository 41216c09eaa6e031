"""GPU checks of crsdr_caf's CFAR detector (crsdr_caf_set_cfar, crsdr_cfar) against the fp64 numpy model in tests/caf_cfar_model.py, whose
docstring derives the bars used here.  The model is always run on the device's own published chi and map, as the peak tests do.  Every
comparison first asserts that the model finds NO ambiguous cell (|P - t| <= 2^-40 t) in those arrays: away from such cells every
decision is exact on both sides, so

    the detection set, its order and count     equal
    lag, doppler, ntrain                       equal
    power, snr, noise, dlag, ddop              within the fp64 bars
    snap                                       the fetched chi cells, bit for bit

The one exception is stated where it is made: maps of small integers, whose sums, quotient and product are exact in every order, with
cells put exactly AT the threshold -- there device and model must agree on every cell, the ambiguous ones included."""
import importlib

import numpy as np
import pytest

import caf_cfar_model as C
import caf_model as M

pytestmark = pytest.mark.gpu
EINVAL, ESTATE = -1, -5
RECT, HANN = M.WINDOW_RECT, M.WINDOW_HANN
TILE_D, TILE_L = 16, 64                                                          # the kernel's tile (csrc/caf_cfar_kernels.hpp)


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


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same_bits(a, c):
    return a.shape == c.shape and np.array_equal(_bits(a), _bits(c))


def _hold(det, count, src, guard, q, tag, integers=False):
    """one map's detections against the model on the same array; returns the model's result"""
    P = M.power(src) if np.iscomplexobj(src) else np.asarray(src, dtype=np.float64)
    want = C.detect(P, guard, q)
    if integers:                                                                 # exact in every order: nothing is ambiguous in fact
        assert np.array_equal(P, np.rint(P)) and P.sum() < 2.0 ** 53 and float(q.alpha) == int(q.alpha), tag
    else:
        assert want["ambiguous"] == 0, f"{tag}: the model finds {want['ambiguous']} ambiguous cell(s) in the device's arrays"
    assert np.all(np.isfinite(det)), tag
    assert int(count) == want["count"], (tag, int(count), want["count"])
    assert np.array_equal(det[:, [0, 1, 7]].astype(np.float64), want["det"][:, [0, 1, 7]]), (tag, det, want["det"])
    err = np.abs(det.astype(np.float64) - want["det"])
    assert np.all(err <= want["bar"]), (tag, det, want["det"], want["bar"])
    assert not det[min(want["count"], q.max_det):].any(), tag
    return want


def _per_op(b, src, guard, q, tag, integers=False):
    det, count = b.cfar(src, guard, _desc(b, q))
    want = _hold(det, count, src, guard, q, tag, integers)
    print(f"{tag}: {src.shape} guard {guard}: count {count}, over the threshold {want['passed']}, first {det[0][:4]}")
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


# (tag, nd, R, guard, Params, planted cells, complex): every shape at which the kernels take another path
SHAPES = [
    ("nd 8, the window on nearly the whole axis", 8, 40, 0, C.Params(8.0, 1, 1, 2, 4), [(0, 0), (7, 39), (4, 20)], False),
    ("nd 8, the same behind a guard", 8, 40, 2, C.Params(8.0, 1, 1, 2, 4), [(2, 0), (6, 39), (4, 20)], True),
    ("R 1", 32, 1, 1, C.Params(6.0, 0, 0, 3, 0), [(1, 0), (16, 0), (26, 0)], False),
    ("R 5 under Hr 16", 16, 5, 0, C.Params(8.0, 1, 1, 2, 15), [(0, 0), (15, 4), (8, 2)], True),
    ("R 65, a lag tile of one", 32, 65, 2, C.Params(8.0, 1, 1, 3, 4), [(2, 64), (30, 63), (16, 0), (15, 64)], False),
    ("R 1024 by nd 8", 8, 1024, 0, C.Params(10.0, 1, 1, 2, 4), [(0, 0), (7, 1023), (3, 63), (5, 64), (5, 511), (2, 960)], False),
    ("nd 4096 by R 3", 4096, 3, 3, C.Params(10.0, 1, 0, 7, 1), [(3, 0), (4093, 2), (2048, 0), (15, 2), (16, 0), (2047, 2)], True),
    ("guard nd / 2, lags to train on", 16, 40, 8, C.Params(8.0, 1, 1, 3, 4), [(8, 20), (8, 0)], False),
    ("Hd 0", 32, 70, 0, C.Params(8.0, 0, 1, 0, 9), [(0, 0), (31, 69), (15, 63), (16, 65)], False),
    ("Hr 0", 32, 70, 1, C.Params(8.0, 1, 0, 5, 0), [(1, 0), (31, 69), (15, 64), (16, 62)], True),
    ("Hd 0 and gr 0", 16, 66, 0, C.Params(8.0, 0, 0, 0, 16), [(0, 0), (15, 65), (7, 64)], False),
    ("the widest window", 32, 130, 0, C.Params(8.0, 2, 4, 6, 12), [(0, 0), (31, 129), (15, 63), (16, 128)], False),
]


@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_shapes_per_op(b, shape):
    tag, nd, R, guard, q, cells, complex_ = shape
    a = _plant(_floor(nd, R, 31 * nd + R, complex_), cells)
    det, count, want = _per_op(b, a, guard, q, tag)
    found = {(int(x[0]), int(x[1])) for x in det[:count]}
    s = M.signed_bins(nd)
    assert {(t, int(s[d])) for d, t in cells} <= found, (tag, found)              # (K = 16 holds them all: they are the strongest cells)


def test_nothing_to_train_on(b):
    """guard = nd / 2 leaves one Doppler bin; with training over Doppler only nothing trains it: N = 0, no detections"""
    a = _plant(_floor(16, 40, 9), [(8, 20)])
    det, count, _ = _per_op(b, a, 8, C.Params(2.0, 1, 1, 3, 0), "guard nd / 2, nothing to train on")
    assert count == 0 and not det.any()
    det, count, _ = _per_op(b, a, 8, C.Params(2.0, 0, 0, 0, 2, min_train=5), "min_train above every N")
    assert count == 0 and not det.any()


def test_tile_corners_and_edges(b):
    """a planted cell at each corner of a tile and on either side of every tile edge, the cyclic wrap included; cells that would be
    neighbours go to different maps"""
    nd, R = 32, 130
    q = C.Params(8.0, 1, 1, 3, 4, max_det=32)
    for k in range(4):
        ds = (TILE_D - 1, nd - 1) if k < 2 else (TILE_D, 0)
        ls = (TILE_L - 1, 2 * TILE_L - 1, R - 1) if k % 2 == 0 else (0, TILE_L, 2 * TILE_L)
        cells = [(d, t) for d in ds for t in ls]
        a = _plant(_floor(nd, R, 70 + k), cells)
        det, count, _ = _per_op(b, a, 0, q, f"tile edges, map {k}")
        s = M.signed_bins(nd)
        assert [(int(x[0]), int(x[1])) for x in det[:len(cells)]] == [(t, int(s[d])) for d, t in reversed(cells)], (k, det[:8])


def test_integer_plateaus_across_tile_edges(b):
    """flat maps of ones: noise = 1 and t = 4 exactly.  A plateau gives its first cell, across a tile edge and across tiles of the merge"""
    nd, R = 32, 130
    q = C.Params(4.0, 1, 1, 3, 4, max_det=8)
    a = np.ones((nd, R), dtype=np.float32)
    for d, t in ((15, 63), (15, 64), (16, 63), (16, 64), (3, 127), (3, 128), (15, 10), (16, 10), (31, 100), (0, 100)):
        a[d, t] = 9.0
    det, count, _ = _per_op(b, a, 0, q, "plateaus", integers=True)
    # four plateaus of one power: each gives its cell of smallest index ((0, 100) across the wrap), in the order of the index
    assert count == 4 and [(int(x[0]), int(x[1])) for x in det[:4]] == [(100, 0), (127, 3), (10, 15), (63, 15)], det[:6]


def test_integer_cells_exactly_at_the_threshold(b):
    nd, R = 32, 130
    q = C.Params(4.0, 1, 1, 3, 4, max_det=8)
    a = np.ones((nd, R), dtype=np.float32)
    at = [(15, 63), (16, 70), (2, 128), (31, 0)]
    for d, t in at:
        a[d, t] = 4.0                                                            # P == t: not a detection
    a[8, 30], a[24, 100] = 5.0, 6.0
    det, count, want = _per_op(b, a, 0, q, "P == t", integers=True)
    assert want["ambiguous"] == len(at)                                          # (they are AT the threshold, and only they)
    assert count == 2 and [(int(x[0]), int(x[1])) for x in det[:2]] == [(100, -8), (30, 8)] and list(det[0][2:5]) == [6, 6, 1]
    c = np.ones((nd, R), dtype=np.complex64)
    c[15, 63], c[8, 30] = 2.0, 1.0 + 2.0j                                        # |.|^2 = 4 and 5
    det, count, _ = _per_op(b, c, 0, q, "P == t, from a chi", integers=True)
    assert count == 1 and list(det[0]) == [30, 8, 5, 5, 1, 0, 0, 90]


@pytest.mark.parametrize("K", [1, 5, 64])
def test_more_detections_than_slots(b, K):
    """count exceeds K; the K kept are those of largest power, ties by index -- inside one tile, and spread over many"""
    nd, R = 32, 130
    q = C.Params(4.0, 0, 0, 1, 1, max_det=K)
    one = np.ones((nd, R), dtype=np.float32)
    one[0:16:2, 0:64:2] = 9.0 + (np.arange(32) % 5)[None, :]                     # 256 detections in tile (0, 0), five powers
    det, count, _ = _per_op(b, one, 0, q, f"one tile, K {K}", integers=True)
    top = min(K, 48)                                                             # 48 cells share the largest power
    assert count == 256 and np.all(det[:top, 2] == 13) and np.all(np.diff(det[:top, 1] * R + det[:top, 0]) > 0)
    spread = np.ones((nd, R), dtype=np.float32)
    spread[::4, ::3] = 9.0 + (np.arange(44) % 7)[None, :]                        # 352 detections over all six tiles, seven powers
    det, count, _ = _per_op(b, spread, 0, q, f"many tiles, K {K}", integers=True)
    assert count == 352 and np.all(det[:min(K, 48), 2] == 15)


def test_zero_and_full_scale(b):
    q = C.Params(8.0, 1, 1, 3, 4, max_det=64)
    for a in (np.zeros((32, 70), dtype=np.float32), np.zeros((8, 1), dtype=np.complex64)):
        det, count = b.cfar(a, 0, _desc(b, C.Params(8.0, 0, 0, 3, 0, max_det=64) if a.shape[1] == 1 else q))
        assert count == 0 and not det.any() and np.all(np.isfinite(det))
    full = (_floor(32, 70, 4) * np.float32(1e36)).astype(np.float32)
    full[5, 5], full[20, 69] = 3.4e38, 3.0e38                                     # the largest fp32 there is
    det, count, _ = _per_op(b, full, 0, q, "full scale")
    assert count >= 2 and (det[0][0], det[0][1], det[1][0], det[1][1]) == (5, 5, 69, -12)


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


def _run(b, torch, blocks, seg, nlags, ref, kind, guard, frames, q, pad=0, max_batch=None):
    """every line of `blocks` [T][nrows][B] through the engine with the detector on -> {chi, map, peak, det, count, snap}"""
    T, nrows, B = blocks.shape
    pk = Packets(torch, blocks, pad)
    cf = b.Caf(nrows, B, seg, nlags, ref, kind, guard, max_batch=max_batch or T, frames=frames)
    cf.set_cfar(_desc(b, q))
    cf.submit(pk.ptr, pk.stride, pk.offset, T)
    assert cf._last() == (T // frames, 5)
    out = {**cf.fetch(), **cf.fetch_cfar()}
    cf.close()
    assert out["det"].shape == (T // frames, nrows + 1, q.max_det, 8) and out["count"].shape == (T // frames, nrows + 1)
    assert out["snap"].shape == (T // frames, q.max_det, nrows)
    return out


def _hold_line(out, e, guard, q, tag):
    """a line's nrows + 1 detection lists and its snapshots against the model on the line's own published chi and map"""
    chi, mp = out["chi"][e], out["map"][e]
    wants = []
    for entry, src in enumerate(list(chi) + [mp]):
        wants.append(_hold(out["det"][e][entry], out["count"][e][entry], src, guard, q, f"{tag} entry {entry}"))
    snap = C.snapshot(chi, wants[-1]["cells"], q.max_det)
    assert _same_bits(out["snap"][e].view(np.float32), snap.view(np.float32)), tag
    return wants


ALPHA = C.cfar_alpha(1e-6, 90)
# (B, frames, seg, R, nrows, echoes, seed): the two lines of tests/test_caf_cfar_model.py
SCENES = [(4096, 4, 64, 32, 3, [(1, 9, 20, 0.2), (2, 17, -13, 0.15)], 0), (2048, 2, 16, 16, 2, [(1, 5, 11, 0.3)], 1)]


@pytest.mark.parametrize("kind", [RECT, HANN])
@pytest.mark.parametrize("scene", SCENES, ids=["two echoes", "one echo"])
def test_echo_scenes(b, torch, scene, kind):
    B, frames, seg, R, nrows, echoes, seed = scene
    q = C.Params(ALPHA, 1, 1, 3, 4)
    line = M.echo_scene(B, frames, echoes, nrows=nrows, seed=seed)
    out = _run(b, torch, np.stack(line), seg, R, 0, kind, 2, frames, q)
    wants = _hold_line(out, 0, 2, q, f"scene {scene[:5]} window {kind}")
    arr = out["det"][0][nrows]
    print(f"scene {scene[:5]} window {kind}: array map count {out['count'][0][nrows]}, snr dB {np.round(10 * np.log10(arr[:len(echoes), 3]), 1)}; over the threshold {wants[-1]['passed']}")
    # the array map's detections are exactly the echoes, strongest first; a row's map gives exactly its own echo
    assert out["count"][0][nrows] == len(echoes) and [(int(x[0]), int(x[1])) for x in arr[:len(echoes)]] == [(t0, d0) for _, t0, d0, _ in echoes], arr[:4]
    for row, t0, d0, _ in echoes:
        assert out["count"][0][row] == 1 and (out["det"][0][row][0][0], out["det"][0][row][0][1]) == (t0, d0)
    assert out["snap"][0][:len(echoes)].any() and not out["snap"][0][len(echoes):].any()


def _same_line(x, e, y, f):
    return all(_same_bits(x[k][e].view(np.float32) if np.iscomplexobj(x[k]) else x[k][e], y[k][f].view(np.float32) if np.iscomplexobj(y[k]) else y[k][f])
               for k in ("chi", "map", "peak", "det", "count", "snap"))


def test_a_line_has_its_bits_anywhere_and_from_the_per_op_call(b, torch):
    nrows, B, seg, nlags, ref, kind, guard = 3, 2048, 64, 17, 2, HANN, 1
    q = C.Params(3.0, 1, 1, 3, 4, max_det=8)                                     # a low threshold on noise: lists that are not empty
    blocks = np.stack([M.random_matrix(nrows, B, 900 + t) for t in range(8)])
    blocks[7] = blocks[0]
    alone = _run(b, torch, blocks[:1], seg, nlags, ref, kind, guard, 1, q, max_batch=8)
    batch = _run(b, torch, blocks, seg, nlags, ref, kind, guard, 1, q, pad=40)
    assert alone["count"][0].min() >= 1
    assert _same_line(alone, 0, batch, 0) and _same_line(alone, 0, batch, 7)
    assert not _same_line(alone, 0, batch, 1)
    _hold_line(batch, 3, guard, q, "line 3 of 8")
    for entry, src in enumerate(list(alone["chi"][0]) + [alone["map"][0]]):      # the per-op call on the fetched arrays
        det, count = b.cfar(src, guard, _desc(b, q))
        assert _same_bits(det, alone["det"][0][entry]) and count == alone["count"][0][entry], entry
    dev = torch.device("cuda", 0)
    nd = B // (2 * seg)
    src = torch.from_numpy(alone["map"][0].copy()).to(dev)
    dd, dn = torch.zeros(q.max_det * 8, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    b.cfar_device(dd.data_ptr(), dn.data_ptr(), src.data_ptr(), 1, nd, nlags, guard, _desc(b, q))
    assert _same_bits(dd.cpu().numpy().reshape(q.max_det, 8), alone["det"][0][nrows]) and int(dn.cpu()[0]) == alone["count"][0][nrows]


def test_behind_a_plan_and_off_again(b, torch):
    """behind a plan's batch on the plan's stream; set_cfar(NULL) restores three launches and leaves chi, map and peak as those of a Caf
    that never had the detector"""
    nrows, B, seg, nlags, frames, nblocks = 3, 2048, 64, 16, 2, 8
    q = C.Params(3.0, 1, 1, 2, 3, max_det=4)
    rows = np.stack([M.echo_scene(B, 1, [(1, 5, 0, 0.3)], nrows=nrows, seed=300 + t)[0] for t in range(nblocks)])
    plan = b.Plan(nrows, B, b.MODE_DIGITAL, max_batch=8)
    cf = b.Caf(nrows, B, seg, nlags, 0, HANN, 2, max_batch=8, frames=frames)
    never = b.Caf(nrows, B, seg, nlags, 0, HANN, 2, max_batch=8, frames=frames)
    plan.submit(rows, seq=0)
    cf.submit_plan(plan)
    assert cf._last() == (nblocks // frames, 3)
    with pytest.raises(b.CrsdrError) as e:
        cf.fetch_cfar()                                                          # no detector set
    assert e.value.code == ESTATE
    cf.set_cfar(_desc(b, q))
    with pytest.raises(b.CrsdrError) as e:
        cf.fetch_cfar()                                                          # nothing submitted since it was set
    assert e.value.code == ESTATE
    cf.submit_plan(plan)
    assert cf._last() == (nblocks // frames, 5) and cf.last_launches() == 5
    out = {**cf.fetch(), **cf.fetch_cfar()}
    for e_ in range(nblocks // frames):
        _hold_line(out, e_, 2, q, f"behind a plan, line {e_}")
    assert set(cf.fetch_cfar(det=False, snap=False)) == {"count"} and all(cf.cfar_device_buffers().values())
    cf.set_cfar(_desc(b, C.Params(5.0, 0, 0, 1, 1, max_det=64)))                 # another detector: other buffers, the same maps
    cf.submit_plan(plan)
    again = {**cf.fetch(), **cf.fetch_cfar()}
    assert again["det"].shape[2] == 64 and all(_same_bits(again[k].view(np.float32) if k == "chi" else again[k], out[k].view(np.float32) if k == "chi" else out[k])
                                               for k in ("chi", "map", "peak"))
    cf.set_cfar(None)
    cf.submit_plan(plan)
    never.submit_plan(plan)
    assert cf._last() == (nblocks // frames, 3) and never._last() == (nblocks // frames, 3)
    off, base = cf.fetch(), never.fetch()
    assert all(_same_bits(off[k].view(np.float32) if k == "chi" else off[k], base[k].view(np.float32) if k == "chi" else base[k]) for k in ("chi", "map", "peak"))
    assert all(_same_bits(off[k].view(np.float32) if k == "chi" else off[k], out[k].view(np.float32) if k == "chi" else out[k]) for k in ("chi", "map", "peak"))
    with pytest.raises(b.CrsdrError) as e:
        cf.fetch_cfar()
    assert e.value.code == ESTATE
    cf.close()
    never.close()
    plan.close()


def test_refusals(b, torch):
    good = dict(gd=1, gr=1, td=3, tr=4, alpha=14.93, min_train=1, max_det=16)
    bad = [dict(gd=-1), dict(gr=-1), dict(td=-1), dict(tr=-1), dict(gd=5, td=4), dict(gr=12, tr=5), dict(td=0, tr=0), dict(gd=4, td=4), dict(alpha=0.0),
           dict(alpha=float("inf")), dict(alpha=float("nan")), dict(min_train=0), dict(max_det=0), dict(max_det=65)]
    cf = b.Caf(3, 2048, 64, 16, max_batch=2)                                     # nd = 16: gd + td = 8 is beyond 2 Hd + 1 <= nd
    for over in bad:
        with pytest.raises(b.CrsdrError) as e:
            cf.set_cfar(b.cfar_desc(**{**good, **over}))
        assert e.value.code == EINVAL, over
        with pytest.raises(b.CrsdrError) as e:
            b.cfar(np.ones((16, 16), dtype=np.float32), 0, b.cfar_desc(**{**good, **over}))
        assert e.value.code == EINVAL, over
    pk = Packets(torch, np.stack([M.random_matrix(3, 2048, 1)]))
    cf.submit(pk.ptr, pk.stride, pk.offset, 1)
    cf.set_cfar(b.cfar_desc(**good))
    with pytest.raises(b.CrsdrError) as e:
        cf.fetch_cfar()                                                          # set behind the submit: nothing of its own yet
    assert e.value.code == ESTATE
    cf.submit(pk.ptr, pk.stride, pk.offset, 1)
    assert cf.fetch_cfar()["det"].shape == (1, 4, 16, 8)
    cf.close()
