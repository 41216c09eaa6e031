"""GPU checks of crsdr_caf's coherent beam maps (crsdr_caf_set_beams, crsdr_beam_maps, crsdr_beam_fuse) against the fp64 numpy model in
tests/caf_beams_model.py, whose docstring derives the bars used here.  The model is always run on the arrays the device itself was
given or published.  Every comparison of detections first asserts that the detector's model finds NO ambiguous cell; then

    bmap                                       within the bars
    bcount, the cells and order of bdet        equal; its figures within the detector's bars
    fused, nfused                              equal to the model's fusion of the device's own bdet, bit for bit
    engine, per-op calls, batch positions      bit for bit"""
import importlib

import numpy as np
import pytest

import caf_beams_model as B
import caf_bearing_model as BM
import caf_cfar_model as C
import caf_model as M

pytestmark = pytest.mark.gpu
EINVAL, ESTATE = -1, -5
HANN = M.WINDOW_HANN


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


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same_bits(a, c):
    return a.shape == c.shape and np.array_equal(_bits(a), _bits(c))


def _chi(nrows, nd, R, seed):
    rng = np.random.default_rng(seed)
    return ((rng.standard_normal((nrows, nd, R)) + 1j * rng.standard_normal((nrows, nd, R))) * 1e-3).astype(np.complex64)


def _w(nb, m, seed):
    rng = np.random.default_rng(seed)
    return ((rng.standard_normal((nb, m)) + 1j * rng.standard_normal((nb, m))) / np.sqrt(2 * m)).astype(np.complex64)


# (m, nbeams, ref, (nd, R)): m in {1, 2, 21, 33, 64}; nbeams in {1, 31, 32, 33, 64}; 8, 31, 32, 33 and 40 cells (31 and 33 as hand-shaped
# lines of one lag) and lines of more than one workgroup (128 cells each); ref first, middle and last
MAPS = [(1, 1, 0, (8, 1)), (2, 31, 2, (8, 4)), (21, 32, 10, (8, 5)), (21, 33, 0, (31, 1)), (33, 64, 33, (33, 1)), (64, 64, 0, (8, 5)), (64, 33, 32, (8, 4)),
        (33, 1, 5, (8, 1)), (21, 64, 21, (16, 24)), (2, 32, 1, (64, 5))]


def _maps_case(c, seed):
    m, nb, ref, (nd, R) = c
    chi, W = _chi(m + 1, nd, R, seed), _w(nb, m, seed + 1)
    chi[:, 0, 0] = 0                                                             # a cell of zeros
    chi[:, nd - 1, R - 1] *= np.float32(1e-36)                                   # fp32 subnormals
    chi[m // 2, 2, 0] = np.float32(1e-42)
    W[nb - 1] = 0                                                                # a weight row of zeros
    return chi, W, ref


@pytest.mark.parametrize("case", MAPS, ids=[f"m{c[0]}-nb{c[1]}-ref{c[2]}-{c[3][0]}x{c[3][1]}" for c in MAPS])
def test_beam_maps_per_op_against_the_model(b, torch, case):
    chi, W, ref = _maps_case(case, 300 + case[0] + case[1])
    got = b.beam_maps(chi, W, ref)
    P, bar = B.bmap(chi, ref, W)
    assert np.all(np.isfinite(got))
    err = np.abs(got.astype(np.float64) - P)
    print(f"{case}: worst error / bar {float(np.max(err / bar)):.3f}")
    assert np.all(err <= bar), (case, float(np.max(err / bar)))
    assert not got[-1].any() and not got[:, 0, 0].any()
    # device memory: the same bits
    dev = torch.device("cuda", 0)
    dc = torch.from_numpy(chi.view(np.float32).copy()).to(dev)
    dm = torch.full((got.size + 64,), -1.0, device=dev)
    b.beam_maps_device(dm.data_ptr(), dc.data_ptr(), chi.shape[0], chi.shape[1], chi.shape[2], ref, W)
    back = dm.cpu().numpy()
    assert _same_bits(back[:got.size].reshape(got.shape), got) and np.all(back[got.size:] == -1.0)      # nothing past the end


def _more_than_k():
    return [(bm, 2 * bm, tau, 20.0 - tau - bm) for bm in range(3) for tau in (0, 2, 4)]


FUSE = {**{k: (v[0], 4, 4) for k, v in B.HAND_FUSE.items()}, "more survivors than K": (_more_than_k(), 3, 5), "all counts zero": ([], 5, 3)}


@pytest.mark.parametrize("name", list(FUSE), ids=list(FUSE))
def test_beam_fuse_per_op_on_hand_made_lists(b, torch, name):
    entries, nb, K = FUSE[name]
    bdet, bcount = B.hand_lists(entries, nb, K, B.HAND_ND)
    got, nf = b.beam_fuse(bdet, bcount, B.HAND_ND, B.HAND_R)
    want, wnf = B.fuse(bdet, bcount, B.HAND_ND, B.HAND_R)
    assert nf == wnf and _same_bits(got, want.astype(np.float32)), (name, got, want)
    if name in B.HAND_FUSE:
        s = M.signed_bins(B.HAND_ND)
        assert [(int(r[7]), int(r[1]), int(r[0])) for r in got[:nf]] == [(bm, s[d], tau) for bm, d, tau in B.HAND_FUSE[name][1]]
    if name == "more survivors than K":
        assert nf == 9 > K and got[:, 2].min() > 0
    if name == "all counts zero":
        assert nf == 0 and not got.any()
    dev = torch.device("cuda", 0)
    dt, dn = torch.from_numpy(bdet).to(dev), torch.from_numpy(bcount).to(dev)
    df, dk = torch.full((K * 8 + 8,), -1.0, device=dev), torch.full((2,), -1, device=dev, dtype=torch.int32)
    b.beam_fuse_device(df.data_ptr(), dk.data_ptr(), dt.data_ptr(), dn.data_ptr(), nb, K, B.HAND_ND, B.HAND_R)
    back = df.cpu().numpy()
    assert _same_bits(back[:K * 8].reshape(K, 8), got) and np.all(back[K * 8:] == -1.0) and list(dk.cpu().numpy()) == [nf, -1]


def test_a_full_house_of_candidates_fuses_as_the_model_says(b):
    """64 beams x 64 slots: every place of the kernel's list is taken"""
    rng = np.random.default_rng(9)
    full = []
    for bm in range(64):
        cells = rng.choice(64 * 24, size=64, replace=False)
        full += [(bm, int(c) // 24, int(c) % 24, float(p)) for c, p in zip(cells, np.sort(rng.integers(1, 50, size=64))[::-1])]
    bdet, bcount = B.hand_lists(full, 64, 64, 64)
    bcount[5] = 900                                                              # a count above K reads K slots
    bcount[6] = -3                                                               # and a negative one none
    got, nf = b.beam_fuse(bdet, bcount, 64, 24)
    want, wnf = B.fuse(bdet, bcount, 64, 24)
    assert nf == wnf > 64 and _same_bits(got, want.astype(np.float32))


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


OLD = ("chi", "map", "peak", "det", "count", "snap")
NEW = ("bmap", "bdet", "bcount", "fused", "nfused")


def _same_line(x, e, y, f, keys):
    v = lambda a: a.view(np.float32) if np.iscomplexobj(a) else a
    return all(_same_bits(np.atleast_1d(v(x[k][e])), np.atleast_1d(v(y[k][f]))) for k in keys)


def _hold_line(b, out, e, W, guard, prm, tag):
    """line e of an engine result: against the model on the device's own arrays, and against the per-op calls bit for bit"""
    chi, bmap = out["chi"][e], out["bmap"][e]
    P, bar = B.bmap(chi, 0, W)
    err = np.abs(bmap.astype(np.float64) - P)
    assert np.all(np.isfinite(bmap)) and np.all(err <= bar), (tag, float(np.max(err / bar)))
    assert _same_bits(b.beam_maps(chi, W, 0), bmap), tag
    want = B.detect_beams(bmap, guard, prm)
    assert want["ambiguous"] == 0, f"{tag}: the model finds {want['ambiguous']} ambiguous cell(s)"
    assert np.array_equal(out["bcount"][e], want["bcount"]), (tag, out["bcount"][e], want["bcount"])
    assert np.array_equal(out["bdet"][e][:, :, [0, 1, 7]].astype(np.float64), want["bdet"][:, :, [0, 1, 7]]), tag
    assert np.all(np.abs(out["bdet"][e].astype(np.float64) - want["bdet"]) <= want["bar"]), tag
    for bm in range(len(W)):
        det, count = b.cfar(bmap[bm], guard, _cfd(b, prm))
        assert _same_bits(det, out["bdet"][e][bm]) and count == out["bcount"][e][bm], (tag, bm)
    nd, R = bmap.shape[1:]
    fused, nf = B.fuse(out["bdet"][e], out["bcount"][e], nd, R)
    assert nf == out["nfused"][e] and _same_bits(out["fused"][e], fused), (tag, out["fused"][e], fused)
    got, gnf = b.beam_fuse(out["bdet"][e], out["bcount"][e], nd, R)
    assert gnf == nf and _same_bits(got, out["fused"][e]), tag
    return nf


def _scene0(seeds):
    sc = BM.SCENES[0]
    lines = [BM.scene_line(sc, seed=s)[0] for s in seeds]
    q = BM.Desc(sc[0], sc[1], sc[2], sc[3], sc[3])
    return sc, np.stack([m for line in lines for m in line]), q, B.steer_weights(q, B.lattice(4, 4, sc[3]))


def test_a_line_has_its_bits_anywhere_equals_the_per_op_calls_and_the_launch_count_is_fixed(b, torch):
    sc, blocks, q, W = _scene0((40, 41, 42, 40))                                 # 8 blocks, 4 lines; the last is the first again
    frames, guard = sc[5], 1
    prm = C.Params(BM.ALPHA, max_det=5, **BM.CFAR)
    res = {}
    for tag, pad, nblocks in (("alone", 0, frames), ("batch", 40, 8)):
        pk = Packets(torch, blocks, pad)
        cf = b.Caf(blocks.shape[1], blocks.shape[2], sc[6], sc[7], 0, HANN, guard, max_batch=8, frames=frames)
        cf.set_cfar(_cfd(b, prm))
        cf.set_beams(W)
        cf.submit(pk.ptr, pk.stride, pk.offset, nblocks)
        assert cf._last() == (nblocks // frames, 5 + 4)
        res[tag] = {**cf.fetch(), **cf.fetch_cfar(), **cf.fetch_beams()}
        assert all(cf.beams_device_buffers().values())
        cf.close()
    alone, batch = res["alone"], res["batch"]
    assert _same_line(alone, 0, batch, 0, OLD + NEW) and _same_line(alone, 0, batch, 3, OLD + NEW) and not _same_line(alone, 0, batch, 1, ("bmap",))
    found = [_hold_line(b, batch, e, W, guard, prm, f"line {e} of 4") for e in range(2)]
    print(f"fused detections of the first two lines: {found}; {batch['fused'][0][:found[0], [0, 1, 2, 7]]}")
    assert min(found) >= 1
    # the echo is in the fused list once, whatever the number of beams that saw it
    assert [tuple(r[[0, 1]]) for r in batch["fused"][0][:found[0]]].count((sc[9], sc[10])) == 1


def test_behind_a_plan_with_the_canceller_beside_the_bearings_and_off_again(b, torch):
    """behind a plan's batch on the plan's stream; with the canceller; with bearings beside the beams; with the detector off; and with
    beams off again every combination has the launches and the bits of a Caf that never had beams"""
    sc, _, q, W = _scene0((60,))
    frames, nblocks, guard = sc[5], 8, 1
    q.mode, q.levels = BM.ADAPTIVE, 2
    prm = C.Params(BM.ALPHA, max_det=4, **BM.CFAR)
    nrows, Bk = 1 + q.m, sc[4]
    rows = np.stack([m for e in range(nblocks // frames) for m in BM.scene_line(sc, seed=60 + e)[0]])
    plan = b.Plan(nrows, Bk, b.MODE_DIGITAL, max_batch=8)
    plan.submit(rows, seq=0)
    cf = b.Caf(nrows, Bk, sc[6], sc[7], 0, HANN, guard, max_batch=8, frames=frames)
    never = b.Caf(nrows, Bk, sc[6], sc[7], 0, HANN, guard, max_batch=8, frames=frames)
    bd = b.bearing_desc(q.mx, q.my, q.d, q.ncx, q.ncy, q.mode, q.loading, q.levels, 0)
    lines = nblocks // frames

    def both(cancel, cfar, bearing):
        """(cf with beams, never without) in one combination of the other stages, submitted behind the plan"""
        outs = []
        for c, beams in ((cf, True), (never, False)):
            if beams:
                c.set_beams(None)                                                # (first: while beams are on the detector stays as it is)
            c.set_bearing(None)
            c.set_cfar(_cfd(b, prm) if cfar else None)
            c.set_cancel(*(cancel or (None,)))
            if bearing:
                c.set_bearing(bd)
            if beams:
                c.set_beams(W)
            c.submit_plan(plan)
            o = {**c.fetch(), **(c.fetch_cfar() if cfar else {}), **(c.fetch_cancel() if cancel else {}), **(c.fetch_bearing() if bearing else {}),
                 **(c.fetch_beams() if beams else {})}
            outs.append((o, c._last()))
        return outs

    for cancel, cfar, bearing in ((None, True, False), ((2, 0), True, False), (None, True, True), ((2, 0), True, True), (None, False, False), ((2, 0), False, False)):
        (on, (n1, l1)), (base, (n0, l0)) = both(cancel, cfar, bearing)
        tag = f"cancel {cancel} cfar {cfar} bearing {bearing}"
        assert n1 == n0 == lines and l0 == 3 + (4 if cancel else 0) + (2 if cfar else 0) + (3 if bearing else 0) and l1 == l0 + (4 if cfar else 1), (tag, l0, l1)
        keys = tuple(k for k in base)
        for e in range(lines):
            assert _same_line(on, e, base, e, keys), (tag, e)                   # (dir, coef and cinfo among them where their stages are on)
        if cfar:
            for e in range(2):
                _hold_line(b, on, e, W, guard, prm, f"{tag}, line {e}")
        else:
            assert set(on) & set(NEW) == {"bmap"}
            for e in range(lines):
                P, bar = B.bmap(on["chi"][e], 0, W)
                assert np.all(np.abs(on["bmap"][e].astype(np.float64) - P) <= bar), tag
            with pytest.raises(b.CrsdrError) as err:
                cf.fetch_beams(lists=True)                                       # no lists without the detector
            assert err.value.code == ESTATE
    # off again: the launches and the bits of a Caf that never had beams, and the state rules
    cf.set_beams(None)
    cf.set_cancel(None)
    never.set_cancel(None)
    for c in (cf, never):
        c.set_cfar(_cfd(b, prm))
        c.submit_plan(plan)
    assert cf._last() == never._last() == (lines, 5)
    off, base = {**cf.fetch(), **cf.fetch_cfar()}, {**never.fetch(), **never.fetch_cfar()}
    assert all(_same_line(off, e, base, e, OLD) for e in range(lines))
    for call in (cf.fetch_beams, cf.beams_device_buffers):
        with pytest.raises(b.CrsdrError) as err:
            call()
        assert err.value.code == ESTATE
    cf.set_beams(W)
    with pytest.raises(b.CrsdrError) as err:
        cf.fetch_beams()                                                         # nothing submitted since
    assert err.value.code == ESTATE
    for desc in (_cfd(b, prm), None):
        with pytest.raises(b.CrsdrError) as err:
            cf.set_cfar(desc)                                                    # beams on: the detector stays as it is
        assert err.value.code == ESTATE
    for bad in (np.zeros((65, q.m), dtype=np.complex64), np.full((2, q.m), np.nan, dtype=np.complex64), np.full((2, q.m), np.inf, dtype=np.complex64)):
        with pytest.raises(b.CrsdrError) as err:
            cf.set_beams(bad)
        assert err.value.code == EINVAL
    with pytest.raises(b.CrsdrError) as err:
        cf.set_beams(W, flags=1)
    assert err.value.code == EINVAL
    for c in (cf, never, plan):
        c.close()


def test_the_weak_echo_end_to_end(b, torch):
    """caf_beams_model.WEAK, seed 0: the device's fused list at alpha 16 is the one record (lag 7, Doppler 5, beam 20); the array map's
    detections at alpha 4 do not hold the cell"""
    w = B.WEAK
    sc = BM.SCENES[w["scene"]]
    blocks, q, _ = BM.scene_line(sc, amp=w["amp"], seed=0)
    blocks = np.stack(blocks)
    W = b.beam_steer(q.mx, q.my, q.d, B.lattice(8, 8, sc[3]), q.ncx, q.ncy)
    pk = Packets(torch, blocks)
    cf = b.Caf(blocks.shape[1], blocks.shape[2], sc[6], sc[7], 0, HANN, w["guard"], max_batch=sc[5], frames=sc[5])
    prm = C.Params(w["alpha"], max_det=w["max_det"], **w["cfar"])
    cf.set_cfar(_cfd(b, prm))
    cf.set_beams(W)
    cf.submit(pk.ptr, pk.stride, pk.offset, sc[5])
    out = {**cf.fetch(), **cf.fetch_beams()}
    nf = _hold_line(b, out, 0, W, w["guard"], prm, "the weak echo")
    hits = [bm for bm in range(64) for r in out["bdet"][0][bm][:min(int(out["bcount"][0][bm]), prm.max_det)] if (r[0], r[1]) == (sc[9], sc[10])]
    print(f"the weak echo: fused {out['fused'][0][:nf]}, its cell in beams {hits}")
    assert nf == 1 and tuple(out["fused"][0][0][[0, 1, 7]]) == (sc[9], sc[10], w["beam"]) and not out["fused"][0][1:].any()
    cf.set_beams(None)
    low = C.Params(w["map_alphas"][0], max_det=64, **w["cfar"])
    cf.set_cfar(_cfd(b, low))
    cf.submit(pk.ptr, pk.stride, pk.offset, sc[5])
    got = cf.fetch_cfar()
    nrows = blocks.shape[1]
    count, det = int(got["count"][0][nrows]), got["det"][0][nrows]
    assert count <= 64 and (sc[9], sc[10]) not in [(r[0], r[1]) for r in det[:count]], det[:count]
    cf.close()
