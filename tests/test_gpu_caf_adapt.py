"""The adaptive beams on the device (crsdr_caf_set_beam_adapt, crsdr_caf_fetch_beam_adapt, crsdr_beam_adapt; include/crsdr.h (w),
"Adaptive beams"): the per-op call against tests/caf_adapt_model.py within the bars its docstring derives, at the edges of the 16-blocks
of the covariance kernel and of its tiles; the regions; the fallbacks; the chain into the beam maps; the engine byte for byte against
the per-op chain with the other stages on; the launch counts; and the scene that the model fixes on the CPU."""
import importlib

import numpy as np
import pytest

import caf_adapt_model as A
import caf_beams_model as B
import caf_bearing_model as BM
import caf_cfar_model as C
import caf_model as M
import caf_track_model as T

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


def _ad(b, q):
    return b.beam_adapt_desc(q.loading, q.d_lo, q.d_n, q.r_lo, q.r_n)


def _bits(a):
    a = np.ascontiguousarray(a)
    return (a.view(np.float32) if np.iscomplexobj(a) else a).view(np.uint32)


def _same_bits(a, c):
    return a.shape == c.shape and np.array_equal(_bits(a), _bits(c))


def _chi(nrows, nd, R, seed):
    rng = np.random.default_rng(seed)
    return BM.noise_chi(nrows, nd, R, seed, floor=np.exp(2j * np.pi * rng.random(nrows)))


def _w(nb, m, seed):
    rng = np.random.default_rng(seed)
    return ((rng.standard_normal((nb, m)) + 1j * rng.standard_normal((nb, m))) / np.sqrt(2 * m)).astype(np.complex64)


def _hold(b, chi, ref, V, q, tag):
    """the per-op call against the model's bars; returns (aw, ainfo, the model's dict)"""
    aw, info, stat = b.beam_adapt(chi, V, _ad(b, q), ref)
    r = A.adapt(chi, ref, V, q)
    assert stat == r["status"] == 0, (tag, stat)
    assert np.all(np.isfinite(aw.view(np.float32))) and np.all(np.isfinite(info))
    ew = np.maximum(np.abs(aw.real - r["w"].real), np.abs(aw.imag - r["w"].imag))
    ei = np.abs(info - r["info"])
    print(f"{tag}: tiles {A.tiles_of(q.N)} worst weight error / bar {float(np.max(ew / np.maximum(r['wbar'], 1e-300))):.3g}, figure {float(np.max(ei / np.maximum(r['ibar'], 1e-300))):.3g}")
    assert np.all(ew <= r["wbar"]) and np.all(ei <= r["ibar"]), tag
    return aw, info, r


# (m, nbeams, ref, (nd, R)): every edge of the 16-blocks, nbeams at the edges of the passes and of the beam groups, ref first, middle, last
BLOCKS = [(1, 1, 0, (5, 7)), (2, 32, 2, (5, 7)), (15, 33, 7, (8, 33)), (16, 64, 0, (8, 33)), (17, 1, 17, (8, 33)), (32, 32, 16, (5, 7)), (33, 33, 0, (8, 33)),
          (48, 64, 48, (5, 7)), (49, 1, 24, (8, 33)), (64, 64, 64, (8, 33))]


@pytest.mark.parametrize("case", BLOCKS, ids=[f"m{c[0]}-nb{c[1]}-ref{c[2]}-{c[3][0]}x{c[3][1]}" for c in BLOCKS])
def test_per_op_against_the_model_at_the_edges_of_the_blocks(b, torch, case):
    m, nb, ref, (nd, R) = case
    chi, V = _chi(m + 1, nd, R, 500 + m), _w(nb, m, 600 + m)
    V[nb - 1] = 0                                                                # a beam that is all zero keeps it
    q = A.whole(nd, R)
    aw, info, r = _hold(b, chi, ref, V, q, str(case))
    assert not aw[-1].any() and not info[-1].any()
    if nb > 1 and m > 1:
        assert np.any(info[:-1, 0] < info[:-1, 1])                               # the floor is taken out
    # the mistakes would not pass
    for which in A.MUTATIONS:
        if m > 2 and nb > 1 and (which != "ref_counts" or ref != m) and which not in ("doppler_nowrap", "last_tile_dropped"):
            bad = A.adapt(chi, ref, V, q, which)
            assert np.any(np.abs(aw.real - bad["w"].real) > r["wbar"]) or np.any(np.abs(aw.imag - bad["w"].imag) > r["wbar"]), (which, case)
    # device memory: the same bits, and nothing past the end
    dev = torch.device("cuda", 0)
    dc = torch.from_numpy(chi.view(np.float32).copy()).to(dev)
    dw, di, ds = torch.full((aw.size * 2 + 64,), -1.0, device=dev), torch.full((info.size + 64,), -1.0, device=dev), torch.full((17,), -1, device=dev, dtype=torch.int32)
    b.beam_adapt_device(dw.data_ptr(), di.data_ptr(), ds.data_ptr(), dc.data_ptr(), m + 1, nd, R, ref, V, _ad(b, q))
    bw, bi, bs = dw.cpu().numpy(), di.cpu().numpy(), ds.cpu().numpy()
    assert _same_bits(bw[:aw.size * 2].view(np.complex64).reshape(aw.shape), aw) and np.all(bw[aw.size * 2:] == -1.0)
    assert _same_bits(bi[:info.size].reshape(info.shape), info) and np.all(bi[info.size:] == -1.0)
    assert bs[0] == 0 and np.all(bs[1:] == -1)


# (m, ref, (nd, R), Desc): one cell, N = 1 < m; a Doppler range that wraps through nd - 1 -> 0; a range ending at lag R - 1; N at
# tile - 1, tile, tile + 1 and 2 tile + 1 of the 64-cell tile; more than 64 chunks, so that a tile is two chunks (40 tiles of 128)
REGIONS = [(5, 2, (8, 33), A.Desc(1e-6, 3, 1, 32, 1)), (5, 0, (8, 33), A.Desc(1e-2, 6, 4, 0, 33)), (17, 9, (8, 33), A.Desc(1e-2, 2, 3, 20, 13)),
           (5, 5, (8, 33), A.Desc(1e-2, 7, 3, 5, 21)), (20, 3, (8, 33), A.Desc(1e-3, 7, 2, 1, 32)), (5, 1, (8, 33), A.Desc(1.0, 4, 5, 20, 13)),
           (33, 0, (5, 43), A.Desc(1e-2, 3, 3, 0, 43)), (3, 1, (128, 40), A.Desc(1e-2, 100, 128, 0, 40))]


@pytest.mark.parametrize("case", REGIONS, ids=[f"m{c[0]}-{c[2][0]}x{c[2][1]}-d{c[3].d_lo}+{c[3].d_n}-r{c[3].r_lo}+{c[3].r_n}" for c in REGIONS])
def test_the_regions(b, case):
    m, ref, (nd, R), q = case
    chi, V = _chi(m + 1, nd, R, 700 + q.N), _w(5, m, 800 + q.N)
    aw, _, r = _hold(b, chi, ref, V, q, f"N {q.N}")
    for which in ("doppler_nowrap", "lag_short", "last_tile_dropped"):
        bad = A.adapt(chi, ref, V, q, which)
        differs = len(A.train_cells(q, nd, R, which)) != q.N and q.N > 1
        if differs and bad["status"] == 0:
            assert np.any(np.abs(aw.real - bad["w"].real) > r["wbar"]) or np.any(np.abs(aw.imag - bad["w"].imag) > r["wbar"]), (which, case)
    # the cells outside the region do not count: their values changed, the same bits
    other = chi.copy()
    inside = np.zeros((nd, R), dtype=bool)
    for d, tau in A.train_cells(q, nd, R):
        inside[d, tau] = True
    other[:, ~inside] *= np.float32(3.0)
    other[ref] = 7.0
    assert _same_bits(b.beam_adapt(other, V, _ad(b, q), ref)[0], aw)


def test_the_fallbacks(b):
    m, ref, nd, R, q = 17, 9, 8, 33, A.Desc(1e-2, 6, 5, 1, 32)
    chi, V = _chi(m + 1, nd, R, 31), _w(33, m, 32)
    V[4, 3] = np.complex64(complex(-0.0, 0.0))                                   # (bit for bit: a negative zero stays one)
    d = _ad(b, q)
    clean = b.beam_adapt(chi, V, d, ref)
    assert clean[2] == 0 and not _same_bits(clean[0], V)
    zero = chi.copy()
    for dd, tau in A.train_cells(q, nd, R):
        zero[:, dd, tau] = 0
    aw, info, stat = b.beam_adapt(zero, V, d, ref)
    assert stat == A.STATUS_ZERO == 1 and _same_bits(aw, V) and not info.any()
    for bad in (np.nan, np.inf):
        inside = chi.copy()
        inside[3, 7, 5] = bad                                                    # planted as data inside the region
        aw, info, stat = b.beam_adapt(inside, V, d, ref)
        assert stat & A.STATUS_SOLVE and _same_bits(aw, V) and not info.any(), bad
        outside = chi.copy()
        outside[3, 4, 5] = bad                                                   # the same outside it: Doppler 4, lag 0, the reference row
        outside[5, 7, 0] = bad
        outside[ref, 7, 5] = bad
        aw, info, stat = b.beam_adapt(outside, V, d, ref)
        assert stat == 0 and _same_bits(aw, clean[0]) and _same_bits(info, clean[1]), bad


def test_the_chain_into_the_beam_maps(b):
    """crsdr_beam_maps(aw): the maps against caf_beams_model's bar with the published aw, and their mean over the training cells
    against ainfo[b][0] within the model's fp32 bar"""
    m, ref, nd, R, q = 21, 10, 16, 24, A.Desc(1e-2, 3, 11, 0, 24)
    chi, V = _chi(m + 1, nd, R, 41), _w(33, m, 42)
    aw, info, r = _hold(b, chi, ref, V, q, "the chain")
    bmap = b.beam_maps(chi, aw, ref)
    P, bar = B.bmap(chi, ref, aw)
    assert np.all(np.abs(bmap.astype(np.float64) - P) <= bar)
    for bm in range(len(V)):
        mean, mb = A.beam_mean(bmap[bm], q), A.mean_bar(chi, ref, r, bm, q)
        assert abs(mean - float(info[bm, 0])) <= mb and mb < 1e-3 * info[bm, 0], (bm, mean, info[bm], mb)
    conv = b.beam_maps(chi, V, ref)
    assert np.allclose([A.beam_mean(conv[bm], q) for bm in range(len(V))], info[:, 1], rtol=1e-5)


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


def _scene0(seeds):
    sc = BM.SCENES[0]
    lines = [BM.scene_line(sc, seed=s)[0] for s in seeds]
    q = BM.Desc(sc[0], sc[1], sc[2], sc[3], sc[3])
    return sc, np.stack([m for line in lines for m in line]), q, B.steer_weights(q, B.lattice(4, 4, sc[3]))


TRACKER = T.Desc(8, source=1)


def _per_op_chain(b, out, W, qa, guard, prm, idesc, tdesc, tag, first=None):
    """every line of an engine result against (crsdr_ambiguity[_cancel] ->) crsdr_beam_adapt -> crsdr_beam_maps -> (crsdr_map_integrate)
    -> crsdr_cfar -> crsdr_beam_fuse -> (crsdr_track), byte for byte.  first(e): the per-op chi of line e from its packet (lines of one
    packet); without it the chain starts at the engine's own chi"""
    lines = len(out["chi"])
    for e in range(lines):
        if first is not None:
            assert _same_bits(first(e), out["chi"][e]), (tag, e)                 # the stage leaves chi as the per-op call makes it
        aw, info, stat = b.beam_adapt(out["chi"][e], W, _ad(b, qa), 0)
        assert _same_bits(aw, out["aw"][e]) and _same_bits(info, out["ainfo"][e]) and stat == out["astat"][e] == 0, (tag, e)
        assert _same_bits(b.beam_maps(out["chi"][e], aw, 0), out["bmap"][e]), (tag, e)
        assert not _same_bits(b.beam_maps(out["chi"][e], W, 0), out["bmap"][e]), (tag, e)
    maps = out["bmap"]
    if idesc is not None:
        maps, _ = b.map_integrate(out["bmap"], idesc)
        assert _same_bits(maps, out["ibmap"]), tag
    if prm is None:
        return
    nd, R = maps.shape[2:]
    for e in range(lines):
        for bm in range(len(W)):
            det, count = b.cfar(maps[e][bm], guard, _cfd(b, prm))
            assert _same_bits(det, out["bdet"][e][bm]) and count == out["bcount"][e][bm], (tag, e, bm)
        fused, nf = b.beam_fuse(out["bdet"][e], out["bcount"][e], nd, R)
        assert nf == out["nfused"][e] and _same_bits(fused, out["fused"][e]), (tag, e)
    if tdesc is not None:
        aux = np.stack([out["fused"][..., 7], np.full(out["fused"].shape[:2], -1.0, dtype=np.float32)], axis=-1)
        trk, ntrk, _ = b.track(out["fused"], out["nfused"], nd, R, tdesc, aux)
        assert trk.tobytes() == out["trk"].tobytes() and ntrk.tobytes() == out["ntrk"].tobytes(), tag


def test_a_line_has_its_bits_anywhere_and_the_launches_are_two_more(b, torch):
    sc, blocks, q, W = _scene0((40, 41, 40, 40))                                 # 8 blocks, 4 lines: the first again at the third and the fourth place
    frames, guard = sc[5], 1
    prm = C.Params(BM.ALPHA, max_det=5, **BM.CFAR)
    qa = A.whole(sc[4] // (2 * sc[6]) * frames, sc[7], 1e-2, guard)
    res = {}
    for tag, pad, nblocks in (("alone", 0, frames), ("batch", 40, 8)):
        pk = Packets(torch, blocks, pad)
        cf = b.Caf(blocks.shape[1], blocks.shape[2], sc[6], sc[7], 0, HANN, guard, max_batch=8, frames=frames)
        cf.set_cfar(_cfd(b, prm))
        cf.set_beams(W)
        cf.submit(pk.ptr, pk.stride, pk.offset, nblocks)
        assert cf._last() == (nblocks // frames, 5 + 4)
        plain = cf.fetch_beams()
        cf.set_beam_adapt(_ad(b, qa))
        with pytest.raises(b.CrsdrError) as err:
            cf.fetch_beam_adapt()                                                # nothing submitted since
        assert err.value.code == ESTATE
        cf.submit(pk.ptr, pk.stride, pk.offset, nblocks)
        assert cf._last() == (nblocks // frames, 5 + 4 + 2)                      # TWO launches more, whatever the batch
        res[tag] = {**cf.fetch(), **cf.fetch_beams(), **cf.fetch_beam_adapt()}
        assert all(cf.beam_adapt_device_buffers().values())
        assert not _same_bits(res[tag]["bmap"], plain["bmap"])
        cf.set_beam_adapt(None)                                                  # off again: the launches and the bits of before
        cf.submit(pk.ptr, pk.stride, pk.offset, nblocks)
        assert cf._last() == (nblocks // frames, 5 + 4)
        again = cf.fetch_beams()
        assert all(_same_bits(again[k], plain[k]) for k in plain)
        for call in (cf.fetch_beam_adapt, cf.beam_adapt_device_buffers):
            with pytest.raises(b.CrsdrError) as err:
                call()
            assert err.value.code == ESTATE
        cf.close()
    alone, batch = res["alone"], res["batch"]
    keys = ("chi", "aw", "ainfo", "astat", "bmap", "bdet", "bcount", "fused", "nfused")
    for k in keys:
        for e in (0, 2, 3):
            assert _same_bits(np.atleast_1d(alone[k][0]), np.atleast_1d(batch[k][e])), (k, e)
    assert not _same_bits(batch["aw"][0], batch["aw"][1])
    _per_op_chain(b, batch, W, qa, guard, prm, None, None, "batch")
    r = A.adapt(batch["chi"][1], 0, W, qa)
    assert np.all(np.abs(batch["aw"][1].real - r["w"].real) <= r["wbar"]) and np.all(np.abs(batch["aw"][1].imag - r["w"].imag) <= r["wbar"])


def test_the_engine_equals_the_per_op_chain_with_the_other_stages_on_and_behind_a_plan(b, torch):
    """the detector off and on, the canceller on, CRSDR_INTEGRATE_BEAMS on, the tracker on the fused list; behind a plan's batch; the
    state rules; set_beams turns the adaptation off"""
    sc, _, q, W = _scene0((60,))
    frames, nblocks, guard = sc[5], 8, 1
    lines = nblocks // frames
    prm = C.Params(BM.ALPHA, max_det=4, **BM.CFAR)
    nrows, Bk = 1 + q.m, sc[4]
    rows = np.stack([m for e in range(lines) for m in BM.scene_line(sc, seed=60 + e)[0]])
    plan = b.Plan(nrows, Bk, b.MODE_DIGITAL, max_batch=8)
    plan.submit(rows, seq=0)
    cf = b.Caf(nrows, Bk, sc[6], sc[7], 0, HANN, guard, max_batch=8, frames=frames)
    qa = A.Desc(1e-2, cf.nd - 5, 11, 2, sc[7] - 2)                               # wrapped, and ending at the last lag
    idesc, tdesc = b.integrate_desc(0.5, 0.25, what=b.INTEGRATE_BEAMS), b.TrackDesc(*TRACKER.fields())
    for cancel, cfar, integ, track in ((None, False, False, False), (None, True, False, False), ((2, 0), True, False, False), (None, True, True, False),
                                       ((2, 0), False, True, False), (None, True, False, True), ((2, 0), True, True, True)):
        tag = f"cancel {cancel} cfar {cfar} integrate {integ} track {track}"
        cf.set_track(None)
        cf.set_integrate(None)
        cf.set_beams(None)
        cf.set_cfar(_cfd(b, prm) if cfar else None)
        cf.set_cancel(*(cancel or (None,)))
        cf.set_beams(W)
        cf.set_beam_adapt(_ad(b, qa))
        if integ:
            cf.set_integrate(idesc)
        if track:
            cf.set_track(tdesc)
        cf.submit_plan(plan)
        base = 3 + (4 if cancel else 0) + (2 if cfar else 0) + (4 if cfar else 1) + (1 if integ else 0) + (1 if track else 0)
        assert cf._last() == (lines, base + 2), (tag, cf._last())
        out = {**cf.fetch(), **cf.fetch_beams(), **cf.fetch_beam_adapt(), **(cf.fetch_integrate() if integ else {}), **(cf.fetch_track() if track else {})}
        _per_op_chain(b, out, W, qa, guard, prm if cfar else None, idesc if integ else None, tdesc if track else None, tag)
    # lines of ONE packet, so that the chain starts at the packets: crsdr_ambiguity[_cancel] -> ... with every later stage on
    one = b.Caf(nrows, Bk, sc[6], sc[7], 0, HANN, guard, max_batch=8, frames=1)
    pk = Packets(torch, rows, 24)
    q1 = A.Desc(1e-2, one.nd - 3, 7, 1, sc[7] - 1)
    for cancel in (None, (2, 0)):
        tag = f"one packet a line, cancel {cancel}"
        one.set_track(None)
        one.set_integrate(None)
        one.set_beams(None)
        one.set_cfar(_cfd(b, prm))
        one.set_cancel(*(cancel or (None,)))
        one.set_beams(W)
        one.set_beam_adapt(_ad(b, q1))
        one.set_integrate(idesc)
        one.set_track(tdesc)
        one.submit(pk.ptr, pk.stride, pk.offset, nblocks)
        assert one._last() == (nblocks, 3 + (4 if cancel else 0) + 2 + 4 + 1 + 1 + 2), (tag, one._last())
        out = {**one.fetch(), **one.fetch_beams(), **one.fetch_beam_adapt(), **one.fetch_integrate(), **one.fetch_track()}
        first = (lambda e: b.ambiguity_cancel(rows[e], sc[6], sc[7], cancel[0], cancel[1], 0, HANN, guard)[0]) if cancel else \
                (lambda e: b.ambiguity(rows[e], sc[6], sc[7], 0, HANN, guard)[0])
        _per_op_chain(b, out, W, q1, guard, prm, idesc, tdesc, tag, first)
    one.close()
    # the state rules: the order is beams, adapt, integrate, track
    for desc in (_ad(b, qa), None):
        with pytest.raises(b.CrsdrError) as err:
            cf.set_beam_adapt(desc)                                              # the tracker and the integration are on
        assert err.value.code == ESTATE
    cf.set_track(None)
    with pytest.raises(b.CrsdrError) as err:
        cf.set_beam_adapt(None)                                                  # the integration still is
    assert err.value.code == ESTATE
    cf.set_integrate(None)
    cf.set_beam_adapt(_ad(b, A.whole(cf.nd, sc[7])))
    cf.set_beams(W)                                                              # every set_beams turns the adaptation off
    cf.submit_plan(plan)
    assert cf._last() == (lines, 3 + 4 + 2 + 4)
    with pytest.raises(b.CrsdrError) as err:
        cf.fetch_beam_adapt()
    assert err.value.code == ESTATE
    cf.set_beams(None)
    with pytest.raises(b.CrsdrError) as err:
        cf.set_beam_adapt(_ad(b, qa))                                            # no beams set
    assert err.value.code == ESTATE
    cf.set_beam_adapt(None)
    cf.set_beams(W)
    for bad in (dict(d_lo=-1), dict(d_lo=cf.nd), dict(d_n=0), dict(d_n=cf.nd + 1), dict(r_lo=-1), dict(r_n=0), dict(r_lo=1, r_n=sc[7]), dict(loading=0.0),
                dict(loading=1.5), dict(loading=float("nan")), dict(flags=1)):
        a = dict(loading=1e-2, d_lo=0, d_n=cf.nd, r_lo=0, r_n=sc[7], flags=0)
        a.update(bad)
        with pytest.raises(b.CrsdrError) as err:
            cf.set_beam_adapt(b.beam_adapt_desc(**a))
        assert err.value.code == EINVAL, bad
    for c in (cf, plan):
        c.close()


def test_the_scene_end_to_end(b, torch):
    """caf_adapt_model.SCENE: with the caller's steered lattice the fused list holds no record within one cell of the echo; with
    adaptation on it is exactly one record, at the echo's cell, in the beam steered nearest to it"""
    s = A.SCENE
    sc = BM.SCENES[s["scene"]]
    line, chi32, qarr, _, (lag, dop) = A.scene_line()
    blocks = np.stack(line)
    W = b.beam_steer(qarr.mx, qarr.my, qarr.d, B.lattice(8, 8, sc[3]), qarr.ncx, qarr.ncy)
    pk = Packets(torch, blocks)
    cf = b.Caf(blocks.shape[1], blocks.shape[2], sc[6], sc[7], 0, HANN, s["guard"], max_batch=sc[5], frames=sc[5])
    prm = A.scene_params()
    cf.set_cfar(_cfd(b, prm))
    cf.set_beams(W)
    cf.submit(pk.ptr, pk.stride, pk.offset, sc[5])
    out = cf.fetch_beams()
    nf = int(out["nfused"][0])
    near = [r for r in out["fused"][0][:min(nf, prm.max_det)] if abs(r[0] - lag) <= 1 and abs(r[1] - dop) <= 1]
    print(f"the caller's lattice: {nf} fused, near the echo {near}")
    assert C.AMBIGUOUS and B.detect_beams(out["bmap"][0], s["guard"], prm)["ambiguous"] == 0
    assert not near
    qa = A.whole(cf.nd, sc[7], s["loading"], s["guard"])
    cf.set_beam_adapt(_ad(b, qa))
    cf.submit(pk.ptr, pk.stride, pk.offset, sc[5])
    out = {**cf.fetch(chi=True, map=False, peak=False), **cf.fetch_beams(), **cf.fetch_beam_adapt()}
    want = B.detect_beams(out["bmap"][0], s["guard"], prm)
    assert want["ambiguous"] == 0 and np.array_equal(out["bcount"][0], want["bcount"])
    r = A.adapt(out["chi"][0], 0, W, qa)
    assert out["astat"][0] == 0 and np.all(np.abs(out["aw"][0].real - r["w"].real) <= r["wbar"]) and np.all(np.abs(out["aw"][0].imag - r["w"].imag) <= r["wbar"])
    gain = 10.0 * np.log10(out["ainfo"][0][:, 0] / out["ainfo"][0][:, 1])
    print(f"adaptation on: fused {out['fused'][0][:int(out['nfused'][0])]}, mean gain {float(np.mean(gain)):.1f} dB")
    assert int(out["nfused"][0]) == 1 and tuple(out["fused"][0][0][[0, 1, 7]]) == (lag, dop, s["beam"]) and not out["fused"][0][1:].any()
    cf.close()
