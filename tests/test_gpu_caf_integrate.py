"""GPU checks of crsdr_caf's integration across lines (crsdr_caf_set_integrate, crsdr_map_integrate) against the fp64 numpy model in
tests/caf_integrate_model.py.  The definition pins every rounding, so there is no bar: per op imap AND the final state are the model's
bytes, at every shape at which the kernel packs its workgroups differently (R = 1: 256 bins a workgroup; 63 / 64 / 65: four, four and
two; 1024: one bin, four cells a thread; nd = 4096: many workgroups), for shifts in both directions, none, and past the whole row.  Cuts
through the state buffer and host against device memory byte for byte.  Through the engine on the smallest objects: imap is the per-op
call on the fetched map, the detector's array-map entry is crsdr_cfar on the fetched imap, everything else keeps its bits, the launch
counts, the beam maps' chain, the tracker behind it, a plan in front of it, the carry-over, the reset, off again, and the state rules."""
import importlib

import numpy as np
import pytest

import caf_integrate_model as IM

pytestmark = pytest.mark.gpu
ESTATE = -5


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


def _maps(seed, L, nmaps, nd, R):
    """random positive fp32 with exact zeros and a few extreme magnitudes"""
    rng = np.random.default_rng(seed)
    m = rng.exponential(1.0, size=(L, nmaps, nd, R)).astype(np.float32)
    m[rng.random(m.shape) < 0.05] = 0.0
    flat = m.reshape(-1)
    flat[rng.integers(0, flat.size, 6)] = np.array([3e38, 1e-40, 1e30, 1e-30, 2.0 ** -126, 65504.0], dtype=np.float32)
    return m


COUPLINGS, FORGETS = [0.0, 0.5, -0.5, 2.75], [1.0, 0.5, 1.0 / 8.0, 2.0 ** -20]
# (nd, R, nmaps, nlines, coupling, forget)
CASES = ([(8, 1, 1, 3, 0.0, 1.0), (8, 1, 1, 3, 2.75, 0.125), (8, 1024, 1, 4, 2.75, 0.5), (8, 1024, 1, 4, -0.5, 2.0 ** -20)]
         + [(16, R, 2, 5, c, a) for R in (63, 64, 65) for c, a in ((0.5, 0.125), (-0.5, 0.5), (2.75, 1.0), (0.0, 2.0 ** -20))]
         + [(4096, 2, 1, 2, 0.5, 0.5), (4096, 2, 1, 2, -0.5, 1.0), (4096, 2, 1, 2, 0.0, 0.125)]
         + [(64, 48, 3, 12, c, a) for c in COUPLINGS for a in FORGETS]
         + [(8, 4, 1, 6, 3.0, 0.125), (8, 4, 1, 6, -3.0, 0.5)])          # |D| >= R: every cell clamps to one end


@pytest.mark.parametrize("nd,R,nmaps,L,c,a", CASES, ids=[f"{nd}x{R}x{n}x{L}-c{c}-a{a:.3g}" for nd, R, n, L, c, a in CASES])
def test_per_op_against_the_model(b, nd, R, nmaps, L, c, a):
    maps = _maps(nd * 131 + R, L, nmaps, nd, R)
    want, wstate = IM.run(maps, a, c)
    got, state = b.map_integrate(maps, b.integrate_desc(a, c))
    differ = int((got.view(np.uint32) != want.view(np.uint32)).sum())
    print(f"nd {nd} R {R} maps {nmaps} lines {L} coupling {c} forget {a}: cells that differ {differ} of {got.size}, header {state[:16].view('<i8').tolist()}")
    assert got.tobytes() == want.tobytes()
    assert state.tobytes() == wstate.tobytes()


def test_a_state_far_from_the_reset(b):
    """a hand-made header: line 12345 and on, where m * delta is large and the offsets' differences are still whole cells"""
    nd, R, L = 64, 48, 4
    maps = _maps(9, L, 2, nd, R)
    state = np.zeros(16 + 8 * 2 * nd * R, dtype=np.uint8)
    state[:8] = np.array([12345], dtype="<i8").view(np.uint8)
    state[16:] = np.random.default_rng(10).exponential(1.0, size=2 * nd * R).view(np.uint8)
    want, wstate = IM.run(maps, 0.125, 0.05, state=state)
    got, after = b.map_integrate(maps, b.integrate_desc(0.125, 0.05), state)
    assert got.tobytes() == want.tobytes() and after.tobytes() == wstate.tobytes() and after[:16].view("<i8").tolist() == [12349, 0]


def test_cuts_through_the_state_are_byte_equal(b):
    nd, R, nmaps = 64, 48, 3
    maps = _maps(11, 12, nmaps, nd, R)
    d = b.integrate_desc(0.125, 0.5)
    whole, wstate = b.map_integrate(maps, d)
    for cut in ([12], [1] * 12, [5, 7], [1, 11], [4, 4, 4]):
        state, parts, lo = None, [], 0
        for n in cut:
            out, state = b.map_integrate(maps[lo:lo + n], d, state)          # (the state goes through the host between the calls)
            parts.append(out)
            lo += n
        assert np.concatenate(parts).tobytes() == whole.tobytes() and state.tobytes() == wstate.tobytes(), cut


@pytest.mark.parametrize("nd,R,nmaps,L", [(16, 65, 2, 5), (8, 1024, 1, 4), (8, 1, 1, 3)])
def test_device_memory_gives_the_bytes_of_host_memory(b, torch, nd, R, nmaps, L):
    maps = _maps(12, L, nmaps, nd, R)
    d = b.integrate_desc(0.25, 2.75)
    got, state = b.map_integrate(maps, d)
    dev = torch.device("cuda", 0)
    n = maps.size
    dm = torch.from_numpy(maps.copy()).to(dev)
    di = torch.full((n + 16,), -1.0, device=dev)
    ds = torch.zeros(2 + nmaps * nd * R + 4, device=dev, dtype=torch.float64)
    ds[2 + nmaps * nd * R:] = -1.0
    b.map_integrate_device(di.data_ptr(), ds.data_ptr(), dm.data_ptr(), L, nmaps, nd, R, d)
    i, s = di.cpu().numpy(), ds.cpu().numpy()
    assert i[:n].tobytes() == got.tobytes() and np.all(i[n:] == -1.0)                                # nothing past the end
    assert s[:2 + nmaps * nd * R].tobytes() == state.tobytes() and np.all(s[2 + nmaps * nd * R:] == -1.0)
    assert dm.cpu().numpy().tobytes() == maps.tobytes()


# ---- through the engine: the smallest objects ----
NROWS, B, SEG, NLAGS, T = 4, 256, 16, 4, 8
OFFSET = 16 + 4 * NROWS
STRIDE = OFFSET + NROWS * B + 24
FORGET, COUPLING = 0.25, 0.5
WEIGHTS = np.array([[1, 1, 1], [1, 1j, -1]], dtype=np.complex64) / np.float32(np.sqrt(3.0))


def _blocks():
    return np.random.default_rng(20250301).integers(-128, 128, size=(T, NROWS, B), dtype=np.int8)


@pytest.fixture(scope="module")
def packets(torch):
    host = np.full((T, STRIDE), 0x55, dtype=np.int8)
    host[:, OFFSET:OFFSET + NROWS * B] = _blocks().reshape(T, -1)
    return torch.from_numpy(host).to(torch.device("cuda", 0))


def _cfar(b):
    return b.cfar_desc(1.5, gd=0, gr=0, td=1, tr=1, min_train=1, max_det=4)


def _engine(b, frames, beams=False):
    cf = b.Caf(NROWS, B, SEG, NLAGS, 0, 0, 0, max_batch=T, frames=frames)
    cf.set_cfar(_cfar(b))
    if beams:
        cf.set_beams(WEIGHTS)
    return cf


def _submit(cf, packets, lo=0, n=T):
    cf.submit(packets.data_ptr() + lo * STRIDE, STRIDE, OFFSET, n)


def _same(a, c, keys, tag):
    for k in keys:
        assert np.ascontiguousarray(a[k]).tobytes() == np.ascontiguousarray(c[k]).tobytes(), (tag, k)


def _hold_array(b, cf, out, imap, tag):
    """imap against the per-op call on the fetched map; the array map's lists against crsdr_cfar on the fetched imap"""
    d = b.integrate_desc(FORGET, COUPLING)
    want, _ = b.map_integrate(out["map"], d)
    assert imap.tobytes() == want.reshape(imap.shape).tobytes(), tag
    assert imap[0].tobytes() == out["map"][0].tobytes() and imap[1:].tobytes() != out["map"][1:].tobytes(), tag
    for l in range(len(imap)):
        det, count = b.cfar(imap[l], 0, _cfar(b))
        assert det.tobytes() == out["det"][l, NROWS].tobytes() and count == out["count"][l, NROWS], (tag, l)


@pytest.mark.parametrize("frames", [1, 2])
def test_through_the_engine(b, packets, frames):
    never, cf = _engine(b, frames), _engine(b, frames)
    _submit(never, packets)
    base, l0 = {**never.fetch(), **never.fetch_cfar()}, never.last_launches()
    lines = T // frames
    assert l0 == 5 and base["map"].shape == (lines, 8 * frames, NLAGS)
    d = b.integrate_desc(FORGET, COUPLING)
    cf.set_integrate(d)
    _submit(cf, packets)
    out, imap = {**cf.fetch(), **cf.fetch_cfar()}, cf.fetch_integrate()["imap"]
    assert cf.last_launches() == l0 + 1
    _hold_array(b, cf, out, imap, "one submit")
    _same(out, base, ("chi", "map", "peak"), "on")
    for l in range(lines):                                                           # snap: the current line's chi at the integrated map's detections
        for k in range(min(int(out["count"][l, NROWS]), 4)):
            cell = int(out["det"][l, NROWS, k, 1]) % (8 * frames) * NLAGS + int(out["det"][l, NROWS, k, 0])
            assert out["snap"][l, k].tobytes() == out["chi"][l].reshape(NROWS, -1)[:, cell].tobytes(), (l, k)
    assert out["det"][:, :NROWS].tobytes() == base["det"][:, :NROWS].tobytes() and out["count"][:, :NROWS].tobytes() == base["count"][:, :NROWS].tobytes()
    # the state carries over two submits: against ONE per-op run over both submits' maps
    cf.integrate_reset()
    half = frames * (lines // 2)
    parts = []
    for lo in (0, half):
        _submit(cf, packets, lo, half)
        parts.append((cf.fetch()["map"], cf.fetch_integrate()["imap"]))
    both = np.concatenate([p[1] for p in parts])
    assert both.tobytes() == imap.tobytes()
    assert both.tobytes() == b.map_integrate(np.concatenate([p[0] for p in parts]), d)[0].reshape(both.shape).tobytes()
    # without a reset the counter goes on: the first line is no longer the map; with it the result is a fresh object's
    _submit(cf, packets)
    assert cf.fetch_integrate()["imap"].tobytes() != imap.tobytes()
    cf.integrate_reset()
    _submit(cf, packets)
    assert cf.fetch_integrate()["imap"].tobytes() == imap.tobytes()
    # the tracker behind it follows the integrated map's lists
    td = b.TrackDesc(4, b.TRACK_SRC_ARRAY, 0.5, 0.5, 9.0, 1.0, 1e-3, 1e-3, 1e-4, COUPLING, 1, 1, 2, 4)
    cf.set_track(td)
    cf.integrate_reset()
    _submit(cf, packets)
    assert cf.last_launches() == l0 + 2
    lists, t = cf.fetch_cfar(snap=False), cf.fetch_track()
    assert lists["det"].tobytes() == out["det"].tobytes()
    trk, ntrk, _ = b.track(lists["det"][:, NROWS], lists["count"][:, NROWS], 8 * frames, NLAGS, td)
    assert trk.tobytes() == t["trk"].tobytes() and ntrk.tobytes() == t["ntrk"].tobytes()
    for call in (lambda: cf.set_integrate(None), lambda: cf.set_integrate(d)):
        with pytest.raises(b.CrsdrError) as err:
            call()                                                                   # the tracker is on: its lists are the integration's
        assert err.value.code == ESTATE
    cf.set_track(None)
    # off again: today's bits and launches
    cf.set_integrate(None)
    _submit(cf, packets)
    off = {**cf.fetch(), **cf.fetch_cfar()}
    assert cf.last_launches() == l0
    _same(off, base, base.keys(), "off")
    for call in (cf.fetch_integrate, cf.integrate_reset, cf.integrate_device_buffers):
        with pytest.raises(b.CrsdrError) as err:
            call()
        assert err.value.code == ESTATE
    cf.close()
    never.close()


@pytest.mark.parametrize("frames", [1, 2])
def test_the_beam_maps_through_the_engine(b, packets, frames):
    never, cf = _engine(b, frames, beams=True), _engine(b, frames, beams=True)
    _submit(never, packets)
    base, l0 = {**never.fetch(), **never.fetch_cfar(), **never.fetch_beams()}, never.last_launches()
    assert l0 == 5 + 4
    d = b.integrate_desc(FORGET, COUPLING, what=b.INTEGRATE_ARRAY | b.INTEGRATE_BEAMS)
    cf.set_integrate(d)
    _submit(cf, packets)
    assert cf.last_launches() == l0 + 2
    out, maps = {**cf.fetch(), **cf.fetch_cfar(), **cf.fetch_beams()}, cf.fetch_integrate()
    _hold_array(b, cf, out, maps["imap"], "array + beams")
    _same(out, base, ("chi", "map", "peak", "bmap"), "beams on")
    ibmap = maps["ibmap"]
    assert ibmap.tobytes() == b.map_integrate(out["bmap"], d)[0].tobytes()            # every (line, beam) map on its own
    nd = 8 * frames
    for l in range(len(ibmap)):
        for k in range(2):
            det, count = b.cfar(ibmap[l, k], 0, _cfar(b))
            assert det.tobytes() == out["bdet"][l, k].tobytes() and count == out["bcount"][l, k], (l, k)
        fused, nfused = b.beam_fuse(out["bdet"][l], out["bcount"][l], nd, NLAGS)
        assert fused.tobytes() == out["fused"][l].tobytes() and nfused == out["nfused"][l], l
    # the beams alone: one launch, the array map's lists as ever
    cf.set_integrate(b.integrate_desc(FORGET, COUPLING, what=b.INTEGRATE_BEAMS))
    _submit(cf, packets)
    assert cf.last_launches() == l0 + 1
    alone = {**cf.fetch_cfar(), **cf.fetch_beams()}
    _same(alone, base, ("det", "count", "snap"), "beams alone")
    _same(alone, out, ("bdet", "bcount", "fused", "nfused"), "beams alone")
    assert cf.fetch_integrate()["ibmap"].tobytes() == ibmap.tobytes()
    with pytest.raises(b.CrsdrError) as err:
        cf.fetch_integrate(imap=True)
    assert err.value.code == ESTATE
    # while integration is on the beams stay as they are; the detector may change
    for call in (lambda: cf.set_beams(None), lambda: cf.set_beams(WEIGHTS)):
        with pytest.raises(b.CrsdrError) as err:
            call()
        assert err.value.code == ESTATE
    cf.set_integrate(None)
    _submit(cf, packets)
    assert cf.last_launches() == l0
    _same({**cf.fetch(), **cf.fetch_cfar(), **cf.fetch_beams()}, base, base.keys(), "off")
    cf.close()
    never.close()


def test_behind_a_plan(b):
    blocks = _blocks()
    plan = b.Plan(NROWS, B, b.MODE_DIGITAL, max_batch=T)
    cf = _engine(b, 1)
    d = b.integrate_desc(FORGET, COUPLING)
    cf.set_integrate(d)
    got = []
    for lo in (0, 4):
        plan.submit(blocks[lo:lo + 4], seq=lo)
        cf.submit_plan(plan)
        got.append((cf.fetch()["map"], cf.fetch_integrate()["imap"], cf.fetch_cfar()))
    assert cf.last_launches() == 6
    maps, imap = np.concatenate([g[0] for g in got]), np.concatenate([g[1] for g in got])
    assert imap.tobytes() == b.map_integrate(maps, d)[0].reshape(imap.shape).tobytes()
    for l in range(4):
        det, count = b.cfar(got[1][1][l], 0, _cfar(b))
        assert det.tobytes() == got[1][2]["det"][l, NROWS].tobytes() and count == got[1][2]["count"][l, NROWS]
    cf.close()
    plan.close()


def test_the_state_rules(b, packets):
    cf = b.Caf(NROWS, B, SEG, NLAGS, 0, 0, 0, max_batch=T, frames=1)
    d = b.integrate_desc(FORGET, COUPLING)

    def refused(call):
        with pytest.raises(b.CrsdrError) as err:
            call()
        assert err.value.code == ESTATE, err.value

    refused(lambda: cf.set_integrate(b.integrate_desc(FORGET, COUPLING, what=b.INTEGRATE_BEAMS)))          # no beams
    refused(lambda: cf.set_integrate(b.integrate_desc(FORGET, COUPLING, what=3)))
    cf.set_integrate(d)                                                              # no detector: the integrated map alone
    _submit(cf, packets)
    assert cf.last_launches() == 4 and cf.fetch_integrate()["imap"][0].tobytes() == cf.fetch()["map"][0].tobytes()
    cf.set_cfar(_cfar(b))                                                            # the detector stays allowed ...
    cf.set_cfar_estimator(b.CfarEstDesc(1, 0, 0))                                    # ... and so does its estimator
    cf.set_cfar(_cfar(b))
    refused(lambda: cf.set_beams(WEIGHTS))
    refused(lambda: cf.set_beams(None))
    bd = b.bearing_desc(3, 1, 0.5, 8, 8)
    cf.set_bearing(bd)                                                               # cfar -> integrate -> bearing
    refused(lambda: cf.set_integrate(None))
    refused(lambda: cf.set_integrate(d))
    _submit(cf, packets)
    assert cf.last_launches() == 3 + 1 + 2 + 3
    cf.set_bearing(None)
    td = b.TrackDesc(4, b.TRACK_SRC_ARRAY, 0.5, 0.5, 9.0, 1.0, 1e-3, 1e-3, 1e-4, COUPLING, 1, 1, 2, 4)
    cf.set_track(td)
    refused(lambda: cf.set_integrate(None))
    refused(lambda: cf.set_integrate(d))
    cf.integrate_reset()                                                             # (the reset is no setter)
    cf.set_track(None)
    cf.set_integrate(None)
    cf.set_beams(WEIGHTS)
    cf.set_integrate(b.integrate_desc(FORGET, COUPLING, what=3))
    bufs = cf.integrate_device_buffers()
    assert bufs["imap"] and bufs["ibmap"] and bufs["state"]
    refused(cf.fetch_integrate)                                                      # nothing submitted since
    # the limits come before the state
    with pytest.raises(b.CrsdrError) as err:
        cf.set_integrate(b.integrate_desc(0.0, COUPLING))
    assert err.value.code == -1
    cf.close()
