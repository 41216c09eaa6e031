"""GPU checks of crsdr_caf's tracker (crsdr_caf_set_track, crsdr_track) against the fp64 numpy model in tests/caf_track_model.py, whose
docstring fixes the bar used here.  Per op on the model's own scenes, each of which test_caf_track_model.py holds to the margin the bar
needs: ids, statuses, ages, hits, misses, slots and counts equal, the figures within the bar plus half an fp32 ulp.  Cuts through the
state buffer and host against device memory byte for byte.  Through the engine on a planted echo whose Doppler moves a bin a line: the
engine's table equals crsdr_track on its own fetched lists byte for byte (and the model on them), in every configuration of the chain."""
import importlib

import numpy as np
import pytest

import caf_cfar_model as C
import caf_model as CM
import caf_track_model as M

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


def _desc(b, q):
    return b.TrackDesc(*q.fields())


SIZE_SCENES = [f"size_{T}_{K}" for T, K in M.SIZES]
HAND_SCENES = ["empty", "fill", "tie", "wrap", "exit", "outside", "notfinite", "constant", "crossing", "coast", "full", "gate_s", "history", "clutter", "cuts"]


@pytest.mark.parametrize("name", SIZE_SCENES + HAND_SCENES)
def test_per_op_against_the_model(b, name):
    q, det, count, aux = M.scene(name)
    want, wn, margin = M.expected(name)
    got, ngot, state = b.track(det, count, M.ND, M.R, _desc(b, q), aux)
    worst = M.hold(got, ngot, want, wn, name)
    print(f"{name}: T {q.T} K {det.shape[1]} lines {len(det)}: worst error / allowance {worst:.3f}, margin {float(np.min(margin)):.3g}, counts {wn.sum(axis=0).tolist()}")
    tr = M.run(q, det, count, aux)[3]
    mine = tr.state()
    assert int(state[:4].view("<i4")[0]) == tr.counter
    for k in ("id", "status", "age", "hits", "misses", "hist"):
        assert np.array_equal(state[16:].view(M.SLOT)[k], mine[16:].view(M.SLOT)[k]), (name, k)


def test_the_id_counter_wraps_to_1(b):
    """a state buffer whose header says that all but two ids are out: the next three tracks are 2^24 - 2, 2^24 - 1 and 1"""
    q, det, count, aux = M.scene(M.WRAP_SCENE)
    state = M.Tracker(q).state()
    state[:4] = np.array([M.WRAP_COUNTER], dtype="<i4").view(np.uint8)
    got, ngot, after = b.track(det, count, M.ND, M.R, _desc(b, q), aux, state)
    want, wn, _, tr = M.run(q, det, count, aux, counter=M.WRAP_COUNTER)
    M.hold(got, ngot, want, wn, "the counter's wrap")
    assert [int(v) for v in got[2, :, 0]] == [(1 << 24) - 2, (1 << 24) - 1, 1] and int(after[:4].view("<i4")[0]) == tr.counter == 1


def test_cuts_through_the_state_are_byte_equal(b):
    q, det, count, aux = M.scene("size_65_64")
    d = _desc(b, q)
    whole = b.track(det, count, M.ND, M.R, d, aux)
    for cut in ([(k, k + 1) for k in range(8)], [(0, 3), (3, 8)]):
        state, parts = None, []
        for lo, hi in cut:
            t, n, state = b.track(det[lo:hi], count[lo:hi], M.ND, M.R, d, aux[lo:hi], state)
            parts.append((t, n))
        assert np.concatenate([p[0] for p in parts]).tobytes() == whole[0].tobytes() and np.concatenate([p[1] for p in parts]).tobytes() == whole[1].tobytes(), cut
        assert state.tobytes() == whole[2].tobytes(), cut


@pytest.mark.parametrize("name", ["size_128_64", "size_2_3", "tie"])
def test_device_memory_gives_the_bytes_of_host_memory(b, torch, name):
    q, det, count, aux = M.scene(name)
    d = _desc(b, q)
    got, ngot, state = b.track(det, count, M.ND, M.R, d, aux)
    dev = torch.device("cuda", 0)
    L, K, T = det.shape[0], det.shape[1], q.T
    dd, dc, da = torch.from_numpy(det.copy()).to(dev), torch.from_numpy(count.copy()).to(dev), torch.from_numpy(aux.copy()).to(dev)
    ds = torch.zeros(2 + 16 * T + 4, device=dev, dtype=torch.float64)
    ds[2 + 16 * T:] = -1.0
    dt, dn = torch.full((L * T * 16 + 16,), -1.0, device=dev), torch.full((L * 4 + 4,), -1, device=dev, dtype=torch.int32)
    b.track_device(dt.data_ptr(), dn.data_ptr(), ds.data_ptr(), dd.data_ptr(), dc.data_ptr(), da.data_ptr(), L, K, M.ND, M.R, d)
    t, n, s = dt.cpu().numpy(), dn.cpu().numpy(), ds.cpu().numpy()
    assert t[:got.size].tobytes() == got.tobytes() and np.all(t[got.size:] == -1.0)                  # nothing past the end
    assert n[:ngot.size].tobytes() == ngot.tobytes() and np.all(n[ngot.size:] == -1)
    assert s[:2 + 16 * T].tobytes() == state.tobytes() and np.all(s[2 + 16 * T:] == -1.0)


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


BLOCK, SEG, NLAGS, GUARD, LAG = 2048, 64, 16, 1, 5
DOPPLER = [-6 + e for e in range(8)]            # a bin a line; line 6 lies on the ridge that the guard cuts out and is coasted through
PRM = C.Params(12.0, max_det=4)
TRACKER = M.Desc(8)


def _blocks(nrows):
    """8 packets, one line each: the echo of the reference at lag 5 on every other row, its Doppler a bin further every line"""
    return np.stack([CM.echo_scene(BLOCK, 1, [(c, LAG, d0, 0.5) for c in range(1, nrows)], nrows=nrows, seed=500 + e)[0] for e, d0 in enumerate(DOPPLER)])


def _engine(b, nrows):
    cf = b.Caf(nrows, BLOCK, SEG, NLAGS, 0, CM.WINDOW_RECT, GUARD, max_batch=8, frames=1)
    cf.set_cfar(b.cfar_desc(alpha=PRM.alpha, gd=PRM.gd, gr=PRM.gr, td=PRM.td, tr=PRM.tr, min_train=PRM.min_train, max_det=PRM.max_det))
    return cf


def _lists(cf, out, source):
    """the lists the tracker read, and the auxiliary pairs as it forms them"""
    if source == "fused":
        return out["fused"], out["nfused"], np.stack([out["fused"][..., 7], np.full(out["fused"].shape[:2], -1.0, dtype=np.float32)], axis=-1)
    det, count = out["det"][:, cf.nrows], out["count"][:, cf.nrows]
    if "dir" not in out:
        return det, count, None
    d = out["dir"].astype(np.float64)
    return det, count, np.stack([d[..., 0] + d[..., 3], d[..., 1] + d[..., 4]], axis=-1).astype(np.float32)


def _hold_engine(b, cf, submit, fetch, source, tag, restart=lambda: None):
    """8 lines in one submit and as 4 + 4; against crsdr_track and the model on the fetched lists; the echo's track; reset.  restart:
    called in front of every pass over the packets (a plan carries its last lag and phasor from batch to batch: crsdr_plan_reset puts
    it where it was before the first, so that every pass sees the same packets)"""
    d = _desc(b, TRACKER) if source != "fused" else b.TrackDesc(*M.Desc(8, source=1).fields())
    cf.set_track(d)
    restart()
    submit(0, 8)
    out = fetch()
    trk, ntrk = out["trk"], out["ntrk"]
    det, count, aux = _lists(cf, out, source)
    got, ngot, _ = b.track(det, count, M.ND, NLAGS, d, aux)
    assert got.tobytes() == trk.tobytes() and ngot.tobytes() == ntrk.tobytes(), tag                   # the per-op call: the same kernel, the same bytes
    want, wn, margin, _ = M.run(TRACKER, det, count, aux, M.ND, NLAGS)
    assert np.all(margin >= 1000 * M.BAR), (tag, margin)
    M.hold(trk, ntrk, want, wn, tag)
    last = trk[-1]
    near = [t for t in last if t[1] == M.CONFIRMED and abs(t[2] - LAG) <= 1.0 and abs(t[3] - DOPPLER[-1]) <= 1.0]
    print(f"{tag}: counts {ntrk.tolist()}, the echo's track {near[0][[0, 2, 3, 4, 7, 8]] if near else None}, list sizes {count.tolist()}")
    assert len(near) == 1 and near[0][8] >= 6, (tag, last)                                            # one id since the first lines
    if aux is not None:
        j = int(near[0][10])
        assert j >= 0 and tuple(near[0][14:16]) == tuple(aux[-1, j]), tag
    # the same packets as two submits of four: the state carries over
    cf.track_reset()
    restart()
    halves = []
    for lo in (0, 4):
        submit(lo, 4)
        halves.append(fetch())
    cut_trk, cut_ntrk = np.concatenate([h["trk"] for h in halves]), np.concatenate([h["ntrk"] for h in halves])
    assert cut_trk.tobytes() == trk.tobytes() and cut_ntrk.tobytes() == ntrk.tobytes(), tag
    parts = [_lists(cf, h, source) for h in halves]
    both = [np.concatenate([p[k] for p in parts]) if parts[0][k] is not None else None for k in range(3)]
    got, ngot, _ = b.track(both[0], both[1], M.ND, NLAGS, d, both[2])
    assert got.tobytes() == cut_trk.tobytes() and ngot.tobytes() == cut_ntrk.tobytes(), tag          # and one per-op call over the halves' own lists
    # without a reset the ids go on; with it they start again at 1
    restart()
    submit(0, 4)
    on = fetch()["trk"]
    assert on[..., 0].max() > trk[..., 0].max(), tag
    cf.track_reset()
    restart()
    submit(0, 4)
    again = fetch()
    assert again["trk"].tobytes() == trk[:4].tobytes() and again["trk"][again["trk"][..., 1] > 0][:, 0].min() == 1, tag


@pytest.mark.parametrize("config", ["plain", "canceller", "bearings", "fused", "plan"])
def test_through_the_engine(b, torch, config):
    nrows = 4 if config == "fused" else 3
    blocks = _blocks(nrows)
    cf = _engine(b, nrows)
    plan = None
    extra = 0
    if config == "canceller":
        cf.set_cancel(2, 0)
        extra = 4
    if config == "bearings":
        cf.set_bearing(b.bearing_desc(2, 1, 0.5, 16, 16, b.BEARING_CONVENTIONAL, 1e-2, 2, 0))
        extra = 3
    if config == "fused":
        W = b.beam_steer(3, 1, 0.5, [[8.0, 8.0], [4.0, 8.0], [12.0, 8.0]], 16, 16)                    # the echo is broadside: beam 0
        cf.set_beams(W)
        extra = 4
    if config == "plan":
        plan = b.Plan(nrows, BLOCK, b.MODE_DIGITAL, max_batch=8)

        def submit(lo, n):
            plan.submit(blocks[lo:lo + n], seq=lo)
            cf.submit_plan(plan)
    else:
        pk = Packets(torch, blocks, pad=24)

        def submit(lo, n):
            cf.submit(pk.ptr + lo * pk.stride, pk.stride, pk.offset, n)

    def fetch():
        return {**cf.fetch_cfar(snap=False), **(cf.fetch_bearing() if config == "bearings" else {}), **(cf.fetch_beams(bmap=False) if config == "fused" else {}),
                **cf.fetch_track()}

    _hold_engine(b, cf, submit, fetch, "fused" if config == "fused" else "array", config, plan.reset if plan is not None else lambda: None)
    assert cf.last_launches() == 3 + 2 + extra + 1
    if config == "fused":
        t = cf.fetch_track()["trk"]
        assert np.all(t[..., 14][t[..., 1] > 0] >= 0) and np.all(t[..., 15][t[..., 1] > 0] == -1)    # (beam, -1)
    cf.close()
    if plan is not None:
        plan.close()


def test_off_is_the_engine_that_never_had_a_tracker(b, torch):
    """with the tracker off chi, det, dir, fused and the launch count are those of a Caf whose tracker was never set; on, one launch more;
    while it is on the detector, the bearings and the beams stay as they are"""
    nrows = 4
    blocks = _blocks(nrows)
    pk = Packets(torch, blocks)
    W = b.beam_steer(3, 1, 0.5, [[8.0, 8.0], [4.0, 8.0]], 16, 16)
    bd = b.bearing_desc(3, 1, 0.5, 16, 16, b.BEARING_CONVENTIONAL, 1e-2, 1, 0)

    def make():
        cf = _engine(b, nrows)
        cf.set_cancel(2, 0)
        cf.set_bearing(bd)
        cf.set_beams(W)
        return cf

    def results(cf):
        cf.submit(pk.ptr, pk.stride, pk.offset, 8)
        return {**cf.fetch(), **cf.fetch_cfar(), **cf.fetch_bearing(), **cf.fetch_beams(), **cf.fetch_cancel()}, cf.last_launches()

    never, cf = make(), make()
    base, l0 = results(never)
    assert l0 == 3 + 4 + 2 + 3 + 4
    for source in (b.TRACK_SRC_ARRAY, b.TRACK_SRC_FUSED):
        cf.set_track(b.TrackDesc(*M.Desc(8, source=source).fields()))
        on, l1 = results(cf)
        assert l1 == l0 + 1
        for k in base:
            assert np.ascontiguousarray(on[k]).tobytes() == np.ascontiguousarray(base[k]).tobytes(), (source, k)    # on: nothing else moves either
        t = cf.fetch_track()
        assert t["ntrk"][-1, 1] >= 1
        for call in (lambda: cf.set_cfar(None), lambda: cf.set_cfar(b.cfar_desc(8.0)), lambda: cf.set_bearing(None), lambda: cf.set_bearing(bd),
                     lambda: cf.set_beams(None), lambda: cf.set_beams(W)):
            with pytest.raises(b.CrsdrError) as err:
                call()
            assert err.value.code == ESTATE
        cf.set_track(None)
        off, l2 = results(cf)
        assert l2 == l0
        for k in base:
            assert np.ascontiguousarray(off[k]).tobytes() == np.ascontiguousarray(base[k]).tobytes(), (source, k)
        for call in (cf.fetch_track, cf.track_reset, cf.track_device_buffers):
            with pytest.raises(b.CrsdrError) as err:
                call()
            assert err.value.code == ESTATE
    # the fused source needs beams with detection
    cf.set_beams(None)
    with pytest.raises(b.CrsdrError) as err:
        cf.set_track(b.TrackDesc(*M.Desc(8, source=1).fields()))
    assert err.value.code == ESTATE
    cf.close()
    never.close()
