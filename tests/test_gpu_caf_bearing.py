"""GPU checks of crsdr_caf's bearings (crsdr_caf_set_bearing, crsdr_bearing) against the fp64 numpy model in tests/caf_bearing_model.py,
whose docstring derives the bars used here.  The model is always run on the arrays the device itself was given or published.  Every
comparison first asserts that the model finds NO ambiguous grid or lattice point; away from such points

    cx, cy, the offsets, the status            equal
    T, alpha, beta                             within the bars
    spec                                       within the bar on T and its one rounding
    engine, per-op call, batch positions       bit for bit"""
import importlib

import numpy as np
import pytest

import caf_bearing_model as BM
import caf_cfar_model as C
import caf_model as M

pytestmark = pytest.mark.gpu
EINVAL, ESTATE = -1, -5
HANN = M.WINDOW_HANN
U = M.U


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


def _cfd(b, q):
    return b.cfar_desc(alpha=q.alpha, gd=q.gd, gr=q.gr, td=q.td, tr=q.tr, min_train=q.min_train, max_det=q.max_det)


def _bd(b, q, keep=True):
    return b.bearing_desc(q.mx, q.my, q.d, q.ncx, q.ncy, q.mode, q.loading, q.levels, b.BEARING_KEEP_SPECTRUM if keep else 0)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same_bits(a, c):
    return a.shape == c.shape and np.array_equal(_bits(a), _bits(c))


def _hold(got, spec, chi, det, count, ref, guard, prm, q, tag):
    """a line's dir (and spec) against the model on the same chi, det and count; returns the model's result"""
    want = BM.bearing(chi, det, count, ref, guard, prm, q)
    assert want["ambiguous"] == 0, f"{tag}: the model finds {want['ambiguous']} ambiguous point(s)"
    assert np.all(np.isfinite(got)), tag
    live = min(int(count), prm.max_det)
    assert np.array_equal(got[:, [0, 1, 3, 4, 7]].astype(np.float64), want["dir"][:, [0, 1, 3, 4, 7]]), (tag, got[:live], want["dir"][:live])
    err = np.abs(got.astype(np.float64) - want["dir"])
    assert np.all(err <= want["bar"]), (tag, got[:live], want["dir"][:live], want["bar"][:live])
    assert not got[live:].any(), tag
    if spec is not None:
        assert np.all(np.isfinite(spec)) and spec.min() >= 0.0 and spec.max() <= 1.0, tag
        serr = np.abs(spec.astype(np.float64) - want["spec"])
        assert np.all(serr <= want["sbar"][:, None, None] + U * want["spec"]), (tag, float(np.max(serr)), want["sbar"])
        assert not spec[live:].any(), tag
    return want


def _per_op(b, chi, det, count, ref, guard, prm, q, tag):
    got, spec = b.bearing(chi, det, count, ref, guard, _cfd(b, prm), _bd(b, q))
    want = _hold(got, spec, chi, det, count, ref, guard, prm, q, tag)
    live = min(int(count), prm.max_det)
    print(f"{tag}: {chi.shape} K {prm.max_det} count {count}: N {want['N'][:live]}, dir {got[:min(live, 3), :5]}, T bar {want['sbar'][:1]}")
    return got, spec, want


# (tag, mx, my, (ncx, ncy), ref, nd, R, guard, cfar half-widths, K, mode, loading, levels, [((d, tau), (x, y))], count or None)
# Line arrays: a 1 x 2's map does not depend on x, a 2 x 1's target sits where sin(beta) = 0, so that their maxima are bit-for-bit
# ties on both sides and the first index decides; a 2 x 1's other maxima would be mirror pairs (beta, pi - beta) that no bar can call.
HAND = [
    ("1x2 on 5x7, K 1, a detection at lag 0", 1, 2, (5, 7), 0, 8, 6, 0, dict(gd=1, gr=1, td=2, tr=3), 1, BM.CONVENTIONAL, 1e-2, 1, [((3, 0), (0, 2))], None),
    ("2x1 on 5x7, the peak in the grid's corner: the zoom clamps", 2, 1, (5, 7), 2, 8, 6, 1, dict(gd=1, gr=1, td=2, tr=3), 1, BM.ADAPTIVE, 1.0, 5,
     [((7, 5), (0, 0))], None),
    ("3x2 on 16x16, K 64: lag 0, lag R - 1, beside the guard, across the wrap; loading 1e-6", 3, 2, (16, 16), 1, 8, 12, 1, dict(gd=1, gr=1, td=2, tr=3), 64,
     BM.ADAPTIVE, 1e-6, 0, [((1, 0), (3, 4)), ((7, 11), (12, 9)), ((1, 6), (5, 13)), ((7, 3), (9, 2)), ((4, 5), (15, 8))], None),
    ("3x2 on 16x16, conventional, levels 8", 3, 2, (16, 16), 6, 8, 12, 1, dict(gd=1, gr=1, td=2, tr=3), 4, BM.CONVENTIONAL, 1e-2, 8,
     [((2, 3), (6, 5)), ((6, 8), (11, 10))], None),
    ("7x3 on 100x100, off the grid, count > K", 7, 3, (100, 100), 0, 16, 10, 2, dict(gd=1, gr=1, td=3, tr=4), 2, BM.ADAPTIVE, 1e-2, 3,
     [((5, 4), (31.37, 61.71)), ((12, 9), (70.5, 22.5))], 9),
    ("7x3 on 100x100, the peak on the grid's border", 7, 3, (100, 100), 21, 16, 10, 2, dict(gd=1, gr=1, td=3, tr=4), 4, BM.CONVENTIONAL, 1e-2, 5,
     [((2, 0), (40.0, 0.0)), ((14, 9), (55.0, 99.0))], None),
    ("8x8 on 16x16, conventional, levels 8", 8, 8, (16, 16), 0, 8, 8, 1, dict(gd=1, gr=1, td=2, tr=3), 3, BM.CONVENTIONAL, 1e-2, 8, [((3, 4), (10, 5))], None),
    ("8x8 on 16x16, adaptive with N < m", 8, 8, (16, 16), 64, 8, 8, 1, dict(gd=0, gr=0, td=1, tr=2), 3, BM.ADAPTIVE, 1e-2, 1,
     [((3, 4), (10, 5)), ((1, 0), (4, 12))], None),
    ("8x8 on 100x100, adaptive", 8, 8, (100, 100), 3, 8, 8, 1, dict(gd=1, gr=1, td=2, tr=3), 1, BM.ADAPTIVE, 1e-2, 1, [((5, 2), (62, 35))], None),
]


def _hand_line(c, seed):
    tag, mx, my, nc, ref, nd, R, guard, cf, K, mode, loading, levels, targets, count = c
    q = BM.Desc(mx, my, 0.5, nc[0], nc[1], mode, loading, levels)
    floor = np.insert(BM.steer(q, [nc[0] / 2], [nc[1] / 2])[0], ref, 1.0)
    chi = BM.noise_chi(1 + q.m, nd, R, seed, floor)
    for (d, tau), (x, y) in targets:
        BM.plant(chi, ref, q, d, tau, x, y)
    det = BM.hand_det([cell for cell, _ in targets], nd, K)
    return chi, det, len(targets) if count is None else count, ref, guard, C.Params(1.0, max_det=K, **cf), q


@pytest.mark.parametrize("case", HAND, ids=[c[0] for c in HAND])
def test_hand_made_lines_per_op(b, case):
    chi, det, count, ref, guard, prm, q = _hand_line(case, 500 + len(case[0]))
    got, spec, want = _per_op(b, chi, det, count, ref, guard, prm, q, case[0])
    live = min(count, prm.max_det)
    for k, (_, (x, y)) in enumerate(case[13][:live]):
        if q.mx > 1 and q.my > 1 and y != 0:                                     # (at beta = 0 every x is the same direction)
            # the planted direction is found: the grid point next to it, and with the zoom the direction itself
            assert abs(got[k][0] - x) <= 0.5 and abs(got[k][1] - y) <= 0.5, (case[0], k, got[k])
            if q.levels >= 5:
                assert abs(got[k][0] + got[k][3] - x) <= 0.02 and abs(got[k][1] + got[k][4] - y) <= 0.02, (case[0], k, got[k])
    if q.mode == BM.ADAPTIVE:
        nd, R = chi.shape[1:]
        for k in range(live):
            d, tau = BM.cell_of(det[k], nd)
            assert want["N"][k] == C.train_cell(np.zeros((nd, R)), guard, prm, d, tau)[1] > 0
    if "N < m" in case[0]:
        assert np.all(want["N"][:live] < q.m)


def test_empty_lists_zero_snapshots_and_nothing_to_train_on(b):
    chi, det, count, ref, guard, prm, q = _hand_line(HAND[2], 77)
    got, spec, _ = _per_op(b, chi, det, 0, ref, guard, prm, q, "count 0")
    assert not got.any() and not spec.any()
    dead = chi.copy()
    d, tau = BM.cell_of(det[1], chi.shape[1])
    dead[:, d, tau] = 0                                                          # an all-zero snapshot in slot 1 alone
    got, spec, _ = _per_op(b, dead, det, count, ref, guard, prm, q, "a zero snapshot")
    assert list(got[1]) == [0, 0, 0, 0, 0, 0, 0, BM.STATUS_ZERO] and not spec[1].any() and got[0][7] == 0 and got[2][2] > 0.9
    quiet = np.zeros_like(chi)                                                   # nothing around the cell: trace(Q) = 0, W = I
    quiet[:, d, tau] = chi[:, d, tau]
    got, spec, want = _per_op(b, quiet, det[1:], 1, ref, guard, C.Params(1.0, gd=prm.gd, gr=prm.gr, td=prm.td, tr=prm.tr, max_det=63), q, "trace(Q) = 0")
    assert got[0][7] == BM.STATUS_IDENTITY and want["N"][0] > 0 and got[0][2] > 0.9
    # guard = nd / 2 leaves one Doppler bin; with training over Doppler only nothing trains it: N = 0
    q0 = BM.Desc(3, 2, 0.5, 16, 16, BM.ADAPTIVE, 1e-2, 2)
    prm0 = C.Params(1.0, gd=0, gr=0, td=1, tr=0, max_det=2)
    chi0 = BM.plant(BM.noise_chi(7, 8, 6, 5), 0, q0, 4, 3, 6, 9)
    got, spec, want = _per_op(b, chi0, BM.hand_det([(4, 3)], 8, 2), 1, 0, 4, prm0, q0, "N = 0")
    assert want["N"][0] == 0 and got[0][7] == BM.STATUS_IDENTITY and (got[0][0], got[0][1]) == (6, 9)
    # a hand-made list that names no cell of the map: status bit 2, zeros, and the slots beside it untouched
    wild = det.copy()
    wild[1, 0] = chi.shape[2]
    got, spec = b.bearing(chi, wild, count, ref, guard, _cfd(b, prm), _bd(b, q))
    assert list(got[1]) == [0, 0, 0, 0, 0, 0, 0, BM.STATUS_CELL] and not spec[1].any() and got[0][2] > 0.9 and got[2][2] > 0.9


def test_refusals(b, torch):
    good = dict(mx=3, my=2, d=0.5, ncx=16, ncy=16, mode=b.BEARING_ADAPTIVE, loading=1e-2, levels=3, flags=0)
    bad = [dict(mx=0), dict(my=-1), dict(mx=2), dict(mx=7), dict(ncx=1), dict(ncy=513), dict(d=0.0), dict(d=float("nan")), dict(mode=0), dict(mode=3), dict(loading=0.0),
           dict(loading=1.5), dict(levels=-1), dict(levels=9), dict(flags=2)]
    cf = b.Caf(7, 2048, 64, 16, max_batch=2)
    with pytest.raises(b.CrsdrError) as e:
        cf.set_bearing(b.bearing_desc(**good))                                   # the detector is off
    assert e.value.code == ESTATE
    cf.set_cfar(b.cfar_desc(8.0, max_det=4))
    for over in bad:
        with pytest.raises(b.CrsdrError) as e:
            cf.set_bearing(b.bearing_desc(**{**good, **over}))
        assert e.value.code == EINVAL, over
    with pytest.raises(b.CrsdrError) as e:
        cf.fetch_bearing()                                                       # no bearings set
    assert e.value.code == ESTATE
    cf.set_bearing(b.bearing_desc(**good))
    with pytest.raises(b.CrsdrError) as e:
        cf.fetch_bearing()                                                       # nothing submitted since
    assert e.value.code == ESTATE
    with pytest.raises(b.CrsdrError) as e:
        cf.set_cfar(b.cfar_desc(8.0, max_det=8))                                 # the buffers are sized by its K
    assert e.value.code == ESTATE
    with pytest.raises(b.CrsdrError) as e:
        cf.set_cfar(None)
    assert e.value.code == ESTATE
    assert cf.bearing_device_buffers()["dir"] and not cf.bearing_device_buffers()["spec"]
    cf.set_bearing(None)
    cf.set_cfar(b.cfar_desc(8.0, max_det=8))                                     # off: the detector may change again
    with pytest.raises(b.CrsdrError) as e:
        cf.bearing_device_buffers()
    assert e.value.code == ESTATE
    cf.close()


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


KEYS = ("chi", "map", "peak", "det", "count", "snap")


def _run(b, torch, blocks, seg, nlags, guard, frames, prm, q, pad=0, max_batch=None, cancel=None, nblocks=None):
    """the lines of `blocks` [T][nrows][B] (row 0 the reference, Hann) through the engine with detector and bearings on"""
    T, nrows, B = blocks.shape
    pk = Packets(torch, blocks, pad)
    cf = b.Caf(nrows, B, seg, nlags, 0, HANN, guard, max_batch=max_batch or T, frames=frames)
    if cancel:
        cf.set_cancel(*cancel)
    cf.set_cfar(_cfd(b, prm))
    cf.set_bearing(_bd(b, q))
    cf.submit(pk.ptr, pk.stride, pk.offset, nblocks or T)
    assert cf._last() == ((nblocks or T) // frames, 8 + (4 if cancel else 0))
    out = {**cf.fetch(), **cf.fetch_cfar(), **cf.fetch_bearing()}
    cf.close()
    return out


def _echo(out, e, sc):
    """the slot of the echo's detection in line e's array-map list"""
    nrows = out["chi"].shape[1]
    det = out["det"][e][nrows]
    hit = [k for k in range(min(int(out["count"][e][nrows]), det.shape[0])) if (det[k][0], det[k][1]) == (sc[9], sc[10])]
    assert len(hit) == 1, (det[:4], sc[9], sc[10])
    return hit[0]


@pytest.mark.parametrize("mode", [BM.CONVENTIONAL, BM.ADAPTIVE], ids=["conventional", "adaptive"])
@pytest.mark.parametrize("sc", BM.SCENES, ids=[BM.scene_id(s) for s in BM.SCENES])
def test_scenes_through_the_engine(b, torch, sc, mode):
    """the echo's bearing is its cell in both modes, the direct path's leaks at Doppler +-1, lag 0 point at broadside; the engine, the
    per-op call on the fetched arrays and the model agree"""
    line, q, _ = BM.scene_line(sc)
    q.mode = mode
    prm = C.Params(BM.ALPHA, max_det=8, **BM.CFAR)
    out = _run(b, torch, np.stack(line), sc[6], sc[7], 1, sc[5], prm, q)
    nrows = 1 + q.m
    det, count = out["det"][0][nrows], int(out["count"][0][nrows])
    want = _hold(out["dir"][0], out["spec"][0], out["chi"][0], det, count, 0, 1, prm, q, f"scene {BM.scene_id(sc)} mode {mode}")
    k = _echo(out, 0, sc)
    print(f"scene {BM.scene_id(sc)} mode {mode}: count {count}, echo {out['dir'][0][k][:3]}, N {want['N'][:count]}")
    assert (out["dir"][0][k][0], out["dir"][0][k][1]) == sc[8]
    leaks = [j for j in range(min(count, 8)) if det[j][0] == 0 and abs(det[j][1]) == 1]
    assert len(leaks) == 2 and all((out["dir"][0][j][0], out["dir"][0][j][1]) == (q.ncx // 2, q.ncy // 2) for j in leaks), out["dir"][0][:count]
    got, spec = b.bearing(out["chi"][0], det, count, 0, 1, _cfd(b, prm), _bd(b, q))
    assert _same_bits(got, out["dir"][0]) and _same_bits(spec, out["spec"][0])


@pytest.mark.parametrize("off", BM.OFFSETS, ids=[f"{o[0]:+.2f}{o[1]:+.2f}" for o in BM.OFFSETS])
@pytest.mark.parametrize("sc", BM.OFF_SCENES, ids=[BM.scene_id(s) for s in BM.OFF_SCENES])
def test_scenes_off_the_grid(b, torch, sc, off):
    """guard 2, levels 5: the refined position within 0.15 cell of the truth conventional, within 0.02 adaptive at loading 1e-2"""
    line, q, (x, y) = BM.scene_line(sc, off)
    q.levels = 5
    prm = C.Params(BM.ALPHA, max_det=8, **BM.CFAR)
    for mode, bound in ((BM.CONVENTIONAL, 0.15), (BM.ADAPTIVE, 0.02)):
        q.mode = mode
        out = _run(b, torch, np.stack(line), sc[6], sc[7], 2, sc[5], prm, q)
        f = out["dir"][0][_echo(out, 0, sc)]
        ex, ey = f[0] + f[3] - x, f[1] + f[4] - y
        print(f"scene {BM.scene_id(sc)} off {off} mode {mode}: {f[:5]} error ({ex:+.4f}, {ey:+.4f})")
        assert max(abs(ex), abs(ey)) <= bound, (mode, f, (x, y))
        assert abs(f[5] - (f[0] + f[3]) * np.pi / q.ncx) <= 4 * U * np.pi and abs(f[6] - (f[1] + f[4]) * np.pi / q.ncy) <= 4 * U * np.pi


@pytest.mark.parametrize("seed", BM.WEAK["seeds"])
def test_the_weak_echo(b, torch, seed):
    """24 dB under the direct path: adaptive is on the true cell with T >= 0.99, conventional has T <= 0.9"""
    w = BM.WEAK
    sc = BM.SCENES[w["scene"]]
    line, q, _ = BM.scene_line(sc, amp=w["amp"], seed=seed)
    q.loading = float(np.float32(w["loading"]))
    prm = C.Params(w["alpha"], max_det=8, **w["cfar"])
    fits = {}
    for mode in (BM.CONVENTIONAL, BM.ADAPTIVE):
        q.mode = mode
        out = _run(b, torch, np.stack(line), sc[6], sc[7], w["guard"], sc[5], prm, q)
        fits[mode] = out["dir"][0][_echo(out, 0, sc)]
    print(f"weak echo seed {seed}: conventional {fits[BM.CONVENTIONAL][:3]}, adaptive {fits[BM.ADAPTIVE][:3]}")
    assert (fits[BM.ADAPTIVE][0], fits[BM.ADAPTIVE][1]) == sc[8] and fits[BM.ADAPTIVE][2] >= 0.99
    assert fits[BM.CONVENTIONAL][2] <= 0.9


def _same_line(x, e, y, f, keys):
    v = lambda a: a.view(np.float32) if np.iscomplexobj(a) else a
    return all(_same_bits(v(x[k][e]), v(y[k][f])) for k in keys)


def test_a_line_has_its_bits_anywhere_and_the_launch_count_is_fixed(b, torch):
    sc = BM.SCENES[0]
    frames = sc[5]
    q = BM.Desc(sc[0], sc[1], sc[2], sc[3], sc[3], BM.ADAPTIVE, 1e-2, 3)
    prm = C.Params(BM.ALPHA, max_det=5, **BM.CFAR)
    lines = [BM.scene_line(sc, seed=40 + e)[0] for e in range(4)]
    lines[3] = lines[0]
    blocks = np.stack([m for line in lines for m in line])                       # 8 blocks, 4 lines
    alone = _run(b, torch, blocks, sc[6], sc[7], 1, frames, prm, q, max_batch=8, nblocks=frames)      # nblocks = frames: 8 launches (asserted in _run)
    batch = _run(b, torch, blocks, sc[6], sc[7], 1, frames, prm, q, pad=40)                           # nblocks = max_batch: 8 as well
    keys = KEYS + ("dir", "spec")
    assert int(alone["count"][0][-1]) >= 3 and alone["dir"][0][:3, 2].min() > 0.5
    assert _same_line(alone, 0, batch, 0, keys) and _same_line(alone, 0, batch, 3, keys) and not _same_line(alone, 0, batch, 1, keys)
    for e in range(4):
        nrows = 1 + q.m
        _hold(batch["dir"][e], batch["spec"][e], batch["chi"][e], batch["det"][e][nrows], int(batch["count"][e][nrows]), 0, 1, prm, q, f"line {e} of 4")
    # the per-op call on device memory
    dev = torch.device("cuda", 0)
    nd = frames * (sc[4] // (2 * sc[6]))
    chi = torch.from_numpy(alone["chi"][0].copy()).to(dev)
    det = torch.from_numpy(alone["det"][0][-1].copy()).to(dev)
    cnt = torch.from_numpy(alone["count"][0][-1:].copy()).to(dev)
    dd, ds = torch.zeros(prm.max_det * 8, device=dev), torch.zeros(prm.max_det * q.ncx * q.ncy, device=dev)
    b.bearing_device(dd.data_ptr(), ds.data_ptr(), chi.data_ptr(), 1 + q.m, nd, sc[7], 0, 1, det.data_ptr(), cnt.data_ptr(), _cfd(b, prm), _bd(b, q))
    assert _same_bits(dd.cpu().numpy().reshape(prm.max_det, 8), alone["dir"][0]) and _same_bits(ds.cpu().numpy().reshape(prm.max_det, q.ncx, q.ncy), alone["spec"][0])


def test_behind_a_plan_with_the_canceller_and_off_again(b, torch):
    """behind a plan's batch on the plan's stream, with the canceller on and off; set_bearing(NULL) restores the launches and leaves
    every other result as those of a Caf that never had bearings"""
    sc = BM.SCENES[0]
    frames, nblocks = sc[5], 8
    q = BM.Desc(sc[0], sc[1], sc[2], sc[3], sc[3], BM.ADAPTIVE, 1e-2, 2)
    prm = C.Params(BM.ALPHA, max_det=4, **BM.CFAR)
    nrows, B = 1 + q.m, sc[4]
    rows = np.stack([m for e in range(nblocks // frames) for m in BM.scene_line(sc, seed=60 + e)[0]])
    plan = b.Plan(nrows, B, b.MODE_DIGITAL, max_batch=8)
    cf = b.Caf(nrows, B, sc[6], sc[7], 0, HANN, 1, max_batch=8, frames=frames)
    never = b.Caf(nrows, B, sc[6], sc[7], 0, HANN, 1, max_batch=8, frames=frames)
    for c in (cf, never):
        c.set_cfar(_cfd(b, prm))
    plan.submit(rows, seq=0)
    cf.set_bearing(_bd(b, q))
    cf.submit_plan(plan)
    assert cf._last() == (nblocks // frames, 8) and cf.last_launches() == 8
    out = {**cf.fetch(), **cf.fetch_cfar(), **cf.fetch_bearing()}
    for e in range(nblocks // frames):
        _hold(out["dir"][e], out["spec"][e], out["chi"][e], out["det"][e][nrows], int(out["count"][e][nrows]), 0, 1, prm, q, f"behind a plan, line {e}")
        got, spec = b.bearing(out["chi"][e], out["det"][e][nrows], int(out["count"][e][nrows]), 0, 1, _cfd(b, prm), _bd(b, q))
        assert _same_bits(got, out["dir"][e]) and _same_bits(spec, out["spec"][e])
    assert set(cf.fetch_bearing(spec=False)) == {"dir"} and all(cf.bearing_device_buffers().values())
    cf.set_cancel(2, 0)
    cf.submit_plan(plan)
    assert cf._last() == (nblocks // frames, 12)
    can = {**cf.fetch(), **cf.fetch_cfar(), **cf.fetch_bearing()}
    for e in range(nblocks // frames):
        _hold(can["dir"][e], can["spec"][e], can["chi"][e], can["det"][e][nrows], int(can["count"][e][nrows]), 0, 1, prm, q, f"with the canceller, line {e}")
    cf.set_cancel(None)
    cf.set_bearing(None)
    cf.submit_plan(plan)
    never.submit_plan(plan)
    assert cf._last() == never._last() == (nblocks // frames, 5)
    off, base = {**cf.fetch(), **cf.fetch_cfar()}, {**never.fetch(), **never.fetch_cfar()}
    for e in range(nblocks // frames):
        assert _same_line(off, e, base, e, KEYS) and _same_line(off, e, out, e, KEYS)
    with pytest.raises(b.CrsdrError) as err:
        cf.fetch_bearing()
    assert err.value.code == ESTATE
    for c in (cf, never, plan):
        c.close()


def test_one_emitter_through_doa_and_caf(b, torch):
    """one emitter and no direct path on the same device packets: crsdr_doa's MUSIC peak (k = 1) and the bearing of the echo's detection
    are the same cell"""
    for sc in BM.SCENES[:2]:
        line, q, _ = BM.scene_line(sc, amp=0.5, direct=0.0)
        prm = C.Params(BM.ALPHA, max_det=4, **BM.CFAR)
        blocks = np.stack(line)
        pk = Packets(torch, blocks)
        T, nrows, B = blocks.shape
        cf = b.Caf(nrows, B, sc[6], sc[7], 0, HANN, 1, max_batch=T, frames=T)
        cf.set_cfar(_cfd(b, prm))
        cf.set_bearing(_bd(b, q, keep=False))
        cf.submit(pk.ptr, pk.stride, pk.offset, T)
        doa = b.Doa(nrows, B, 1, q.d, q.mx, q.my, q.ncx, q.ncy, max_batch=T, frames=T)
        doa.submit(pk.ptr, pk.stride, pk.offset, T)
        out = {**cf.fetch_cfar(), **cf.fetch_bearing()}
        k = _echo({"chi": np.zeros((1, nrows)), **out}, 0, sc)
        peak = doa.fetch_peaks()
        print(f"scene {BM.scene_id(sc)}: doa peak {peak.reshape(-1)[:2]}, bearing {out['dir'][0][k][:3]}")
        assert tuple(int(v) for v in peak.reshape(-1)[:2]) == (int(out["dir"][0][k][0]), int(out["dir"][0][k][1])) == sc[8]
        cf.close()
        doa.close()
