"""crsdr_caf's canceller on the device (crsdr_caf_set_cancel, crsdr_ambiguity_cancel; csrc/caf_cancel.hpp, the k_caf variants of
csrc/caf.hpp) against tests/caf_cancel_model.py: chi, coef, cinfo, map and peak within the bars the model derives, at the shapes where
the kernels can go wrong; the bits of a line wherever it sits, per op and behind a plan; a singular line; the two scenes of the change
end to end with the detector; and the launch count."""
import importlib

import numpy as np
import pytest

import caf_cancel_model as X
import caf_cfar_model as C
import caf_model as M

pytestmark = pytest.mark.gpu
EINVAL, ESTATE = -1, -5
RECT, HANN = M.WINDOW_RECT, M.WINDOW_HANN
ON, ON_CFAR, OFF = 7, 9, 3                                                       # launches of a submit


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


KEYS = ("chi", "map", "peak", "coef", "cinfo")


def _bits(a):
    a = np.ascontiguousarray(a)
    return (a.view(np.float32) if np.iscomplexobj(a) else a).view(np.uint32)


def _same_line(x, e, y, f, keys=KEYS):
    return all(np.array_equal(_bits(x[k][e]), _bits(y[k][f])) for k in keys)


def _engine(b, torch, blocks, seg, R, ref, kind, guard, frames, K, P, pad=0, max_batch=None, cfar=None):
    """every line of blocks [T][nrows][B] through the engine with the canceller on"""
    T, nrows, B = blocks.shape
    pk = Packets(torch, blocks, pad)
    cf = b.Caf(nrows, B, seg, R, ref, kind, guard, max_batch=max_batch or T, frames=frames)
    cf.set_cancel(K, P)
    if cfar is not None:
        cf.set_cfar(cfar)
    cf.submit(pk.ptr, pk.stride, pk.offset, T)
    assert cf._last() == (T // frames, ON if cfar is None else ON_CFAR)
    out = {**cf.fetch(), **cf.fetch_cancel(), **({} if cfar is None else cf.fetch_cfar())}
    cf.close()
    assert out["coef"].shape == (T // frames, nrows, X.basis(K, P)) and out["cinfo"].shape == (T // frames, nrows, 2)
    return out


def _hold(got, line, seg, R, ref, kind, guard, K, P, tag, cond_max=16.0):
    """one line's chi, coef, cinfo against the model of `line`, map and peak against the model on the device's own chi"""
    chi, mp, peak, coef, cinfo = got
    r = X.cancel(line, seg, R, ref, kind, K, P)
    assert r["cond"] <= cond_max, (tag, r["cond"])                               # the bars of h stay tight
    assert all(np.all(np.isfinite(a)) for a in got), tag
    rc = M.worst_ratio(chi, r["chi"], r["bar"])
    eh = np.maximum(np.abs(coef.real - r["h"].real), np.abs(coef.imag - r["h"].imag))
    rh = float(np.max(eh / np.maximum(r["hbar"], 1e-300)))
    rs = float(np.max(np.abs(cinfo[:, 0] - r["share"]) / np.maximum(r["sbar"], 1e-300)))
    wm, bm = M.array_map(chi, ref)
    rm = M.worst_ratio(mp.astype(np.float64), wm, bm)
    wp, bp = M.all_peaks(chi, mp, guard)
    ep = np.abs(peak.astype(np.float64) - wp)
    print(f"{tag}: cond {r['cond']:.2f}; largest error / bar: chi {rc:.4f} coef {rh:.4f} share {rs:.4f} map {rm:.4f}; share {np.round(r['share'], 4)}")
    assert rc <= 1.0 and rh <= 1.0 and rs <= 1.0 and rm <= 1.0, (tag, rc, rh, rs, rm)
    assert np.array_equal(cinfo[:, 1], r["status"]) and not coef[ref].any() and tuple(cinfo[ref]) == (1.0, 0.0), tag
    assert np.all(ep <= bp), (tag, peak, wp, bp)
    return r


# (name, nrows, B, frames, seg, R, ref, window, guard, K, P)
CASES = [
    ("smallest K 1", 3, 256, 1, 16, 16, 0, HANN, 0, 1, 0), ("smallest K 2", 3, 256, 1, 16, 16, 2, RECT, 1, 2, 0), ("smallest K 16", 3, 256, 1, 16, 16, 1, HANN, 0, 16, 0),
    ("smallest K 1 P 2", 3, 256, 1, 16, 16, 0, RECT, 0, 1, 2), ("smallest K 2 P 2", 3, 256, 1, 16, 16, 1, HANN, 2, 2, 2),      # (K 16 with P 2 is 80 members: refused)
    ("tile crossing", 3, 1024, 1, 32, 20, 2, HANN, 1, 17, 0), ("K 32", 2, 4096, 1, 64, 32, 0, HANN, 0, 32, 0), ("K 16 P 1", 3, 4096, 1, 64, 32, 1, RECT, 2, 16, 1),
    ("one-lag tiles", 2, 8192, 16, 16, 5, 1, HANN, 2, 3, 1), ("packet fronts", 3, 128, 4, 16, 16, 2, HANN, 0, 5, 1), ("odd rows", 4, 512, 2, 32, 7, 3, RECT, 0, 7, 2),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_against_the_model(b, torch, case):
    name, nrows, B, frames, seg, R, ref, kind, guard, K, P = case
    line = M.echo_scene(B, frames, [(c, 3 % R, 2, 0.2) for c in range(nrows) if c != ref], nrows=nrows, ref=ref, seed=len(name))
    if frames == 1:
        got = b.ambiguity_cancel(line[0], seg, R, K, P, ref, kind, guard)
    else:
        out = _engine(b, torch, np.stack(line), seg, R, ref, kind, guard, frames, K, P)
        got = tuple(out[k][0] for k in KEYS)
    r = _hold(got, line, seg, R, ref, kind, guard, K, P, name)
    others = [c for c in range(nrows) if c != ref]
    assert np.all(r["share"][others] < 0.5)                                      # the direct path went, so the check is of a cancelled row
    # row r is bit for bit the canceller-off path's
    off = b.ambiguity(line[0], seg, R, ref, kind, guard)[0] if frames == 1 else None
    if off is not None:
        assert np.array_equal(_bits(off[ref]), _bits(got[0][ref])) and not np.array_equal(_bits(off[others[0]]), _bits(got[0][others[0]]))


def test_a_line_has_its_bits_anywhere_per_op_and_behind_a_plan(b, torch):
    nrows, B, seg, R, ref, kind, guard, K, P = 3, 2048, 64, 17, 2, HANN, 1, 5, 1
    blocks = np.stack([M.echo_scene(B, 1, [(0, 6, 3, 0.2)], nrows=nrows, ref=ref, seed=700 + t)[0] for t in range(8)])
    blocks[7] = blocks[0]
    alone = _engine(b, torch, blocks[:1], seg, R, ref, kind, guard, 1, K, P, max_batch=8)
    batch = _engine(b, torch, blocks, seg, R, ref, kind, guard, 1, K, P, pad=40)
    assert _same_line(alone, 0, batch, 0) and _same_line(alone, 0, batch, 7) and not _same_line(alone, 0, batch, 1)
    _hold(tuple(batch[k][3] for k in KEYS), [blocks[3]], seg, R, ref, kind, guard, K, P, "line 3 of 8")
    host = dict(zip(KEYS, [a[None] for a in b.ambiguity_cancel(blocks[0], seg, R, K, P, ref, kind, guard)]))
    assert _same_line(alone, 0, host, 0)
    dev = torch.device("cuda", 0)
    nd, n = B // (2 * seg), X.basis(K, P)
    m = torch.from_numpy(blocks[0].copy()).to(dev)
    bufs = [torch.zeros(s, dtype=torch.float32, device=dev) for s in (nrows * nd * R * 2, nd * R, (nrows + 1) * 6, nrows * n * 2, nrows * 2)]
    b.ambiguity_cancel_device(bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(), m.data_ptr(), nrows, B, seg, R, ref, kind, guard, K, P, bufs[3].data_ptr(),
                              bufs[4].data_ptr())
    for k, t in zip(KEYS, bufs):
        assert np.array_equal(t.cpu().numpy().view(np.uint32).ravel(), _bits(alone[k][0]).ravel()), k
    # row r's chi is the canceller-off submit's, every other row's is not
    pk = Packets(torch, blocks)
    cf = b.Caf(nrows, B, seg, R, ref, kind, guard, max_batch=8)
    cf.submit(pk.ptr, pk.stride, pk.offset, 8)
    assert cf._last() == (8, OFF)
    off = cf.fetch()
    assert np.array_equal(_bits(off["chi"][:, ref]), _bits(batch["chi"][:, ref])) and not np.array_equal(_bits(off["chi"][:, 0]), _bits(batch["chi"][:, 0]))
    # behind a plan, on the plan's stream, against a submit on the packets it published
    plan = b.Plan(nrows, B, b.MODE_DIGITAL, max_batch=8)
    plan.submit(blocks, seq=0)
    cf.set_cancel(K, P)
    cf.submit_plan(plan)
    assert cf._last() == (8, ON)
    behind = {**cf.fetch(), **cf.fetch_cancel()}
    pub = Packets(torch, np.stack([plan.fetch(block=t)["matrix"].copy() for t in range(8)]))
    cf.submit(pub.ptr, pub.stride, pub.offset, 8)
    again = {**cf.fetch(), **cf.fetch_cancel()}
    assert all(_same_line(behind, e, again, e) for e in range(8))
    # off again: the off path's launches and bits
    cf.set_cancel(None)
    cf.submit(pk.ptr, pk.stride, pk.offset, 8)
    assert cf._last() == (8, OFF)
    back = cf.fetch()
    assert all(_same_line(back, e, off, e, ("chi", "map", "peak")) for e in range(8))
    with pytest.raises(b.CrsdrError) as e:
        cf.fetch_cancel()
    assert e.value.code == ESTATE
    cf.close()
    plan.close()


def test_a_singular_line_in_a_batch(b, torch):
    nrows, B, seg, R, ref, kind, guard, K, P = 3, 512, 16, 16, 1, HANN, 1, 4, 1
    blocks = np.stack([M.echo_scene(B, 1, [], nrows=nrows, ref=ref, seed=800 + t)[0] for t in range(4)])
    blocks[2, ref] = 0                                                           # line 2: an all-zero reference
    blocks[3, 0] = 0                                                             # line 3: an all-zero row
    out = _engine(b, torch, blocks, seg, R, ref, kind, guard, 1, K, P)
    pk = Packets(torch, blocks)
    cf = b.Caf(nrows, B, seg, R, ref, kind, guard, max_batch=4)
    cf.submit(pk.ptr, pk.stride, pk.offset, 4)
    off = cf.fetch()
    cf.close()
    assert _same_line(out, 2, off, 2, ("chi", "map", "peak")) and not out["coef"][2].any()
    assert out["cinfo"][2].tolist() == [[1.0, 1.0], [1.0, 0.0], [1.0, 1.0]]
    for e in (0, 1, 3):                                                          # its neighbours as if it were not there
        _hold(tuple(out[k][e] for k in KEYS), [blocks[e]], seg, R, ref, kind, guard, K, P, f"beside a singular line, line {e}")
        alone = dict(zip(KEYS, [a[None] for a in b.ambiguity_cancel(blocks[e], seg, R, K, P, ref, kind, guard)]))
        assert _same_line(out, e, alone, 0), e
    assert not out["coef"][3][0].any() and tuple(out["cinfo"][3][0]) == (1.0, 0.0) and not out["chi"][3][0].any()


# the detector of tests/test_caf_cancel_model.py: the full training set of 90 cells, 10^-6 per cell
def _detector(b):
    return b.cfar_desc(alpha=b.cfar_alpha(1e-6, 90), gd=1, gr=1, td=3, tr=4, min_train=90, max_det=8)


@pytest.mark.parametrize("seed", range(4))
def test_the_scenes_end_to_end(b, torch, seed):
    """the device's peak and its only detection sit on the echo (lag 20, Doppler 5) with the canceller on, and not with it off"""
    static, doppler = X.clutter_scene(seed), X.clutter_scene(seed, paths=X.DOPPLER_PATHS)
    blocks = np.stack([static[0], doppler[0]])
    pk = Packets(torch, blocks)
    cf = b.Caf(2, blocks.shape[2], 64, 32, 0, HANN, 0, max_batch=2)
    cf.set_cfar(_detector(b))
    cf.submit(pk.ptr, pk.stride, pk.offset, 2)
    off = {**cf.fetch(), **cf.fetch_cfar()}
    got = {}
    for P in (0, 1):
        cf.set_cancel(8, P)
        cf.submit(pk.ptr, pk.stride, pk.offset, 2)
        assert cf._last() == (2, ON_CFAR)
        got[P] = {**cf.fetch(), **cf.fetch_cfar(), **cf.fetch_cancel()}
    cf.close()
    echo = lambda o, e: (o["peak"][e][1][0], o["peak"][e][1][1]) == (20, 5)
    only = lambda o, e: o["count"][e][1] == 1 and (o["det"][e][1][0][0], o["det"][e][1][0][1]) == (20, 5)
    print(f"seed {seed}: shares static {got[0]['cinfo'][0][1][0]:.4f}; doppler P 0 {got[0]['cinfo'][1][1][0]:.4f}, P 1 {got[1]['cinfo'][1][1][0]:.4f}")
    assert not echo(off, 0) and not echo(off, 1) and not only(off, 0) and not only(off, 1)
    assert echo(got[0], 0) and only(got[0], 0)
    assert (got[0]["peak"][1][1][0], got[0]["peak"][1][1][1]) == (2, 1) and not only(got[0], 1)
    assert echo(got[1], 0) and only(got[1], 0) and echo(got[1], 1) and only(got[1], 1)
    assert 0.004 < got[0]["cinfo"][0][1][0] < 0.009 and 0.15 < got[0]["cinfo"][1][1][0] < 0.2 and 0.004 < got[1]["cinfo"][1][1][0] < 0.009


def test_the_launch_count_does_not_depend_on_the_batch(b, torch):
    nrows, B, seg, R = 3, 512, 16, 8
    blocks = np.stack([M.random_matrix(nrows, B, 60 + t) for t in range(8)])
    pk = Packets(torch, blocks)
    cf = b.Caf(nrows, B, seg, R, 0, RECT, 0, max_batch=8)
    cf.set_cancel(3, 1)
    for nblocks in (1, 8):
        cf.submit(pk.ptr, pk.stride, pk.offset, nblocks)
        assert cf._last() == (nblocks, ON) and cf.fetch_cancel()["coef"].shape == (nblocks, nrows, 9)
    cf.set_cfar(_detector(b))
    for nblocks in (8, 1):
        cf.submit(pk.ptr, pk.stride, pk.offset, nblocks)
        assert cf._last() == (nblocks, ON_CFAR)
    cf.close()
