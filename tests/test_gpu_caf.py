"""GPU checks of crsdr_caf and its per-op form crsdr_ambiguity against the fp64 numpy model in tests/caf_model.py, whose docstring derives
the bars used here:

    chi     |dev - model| <= 2^-24 (7 log2 nd + 2) scale ||w o y_c[:, tau]||_2 on the real and on the imaginary part of a cell
    map     the model on the device's own published fp32 chi: map (u + nrows e)
    peak    the model on the device's own published chi and map: lag and doppler exactly, the rest within the fp64 bars

Everything else is equality of bits and derived, not measured: the range stage is integers, nothing in a line depends on another line
or on nblocks, and the per-op call launches the same kernels on the same arguments."""
import importlib

import numpy as np
import pytest

import caf_model as M

pytestmark = pytest.mark.gpu
EINVAL, ESTATE = -1, -5
RECT, HANN = M.WINDOW_RECT, M.WINDOW_HANN


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
    """T packet-shaped slots on the device, as a plan lays them out: packet t at base + t * stride, its matrix [nrows][B] at
    + 16 + 4 * nrows (4-byte aligned only when nrows is odd); pad: bytes between one packet's end and the next one's start."""

    def __init__(self, torch, blocks, pad=0):
        blocks = np.ascontiguousarray(blocks)
        self.T, self.nrows, self.B = blocks.shape
        self.offset = 16 + 4 * self.nrows
        self.stride = self.offset + self.nrows * self.B + pad
        host = np.full((self.T, self.stride), 0x55, dtype=np.int8)
        host[:, self.offset:self.offset + self.nrows * self.B] = blocks.reshape(self.T, -1)
        self.buf = torch.from_numpy(host).to(torch.device("cuda", 0))
        self.ptr = self.buf.data_ptr()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same_bits(a, c):
    return a.shape == c.shape and np.array_equal(_bits(a), _bits(c))


def _same_line(x, e, y, f):
    return all(_same_bits(x[k][e].view(np.float32) if k == "chi" else x[k][e], y[k][f].view(np.float32) if k == "chi" else y[k][f]) for k in ("chi", "map", "peak"))


def _run(b, torch, blocks, seg, nlags, ref, kind, guard, frames, pad=0, max_batch=None):
    """every line of `blocks` [T][nrows][B] through the engine -> {chi, map, peak}"""
    T, nrows, B = blocks.shape
    pk = Packets(torch, blocks, pad)
    cf = b.Caf(nrows, B, seg, nlags, ref, kind, guard, max_batch=max_batch or T, frames=frames)
    cf.submit(pk.ptr, pk.stride, pk.offset, T)
    assert cf._last() == (T // frames, 3)
    out = cf.fetch()
    cf.close()
    assert out["chi"].shape == (T // frames, nrows, frames * B // (2 * seg), nlags)
    return out


def _check_line(chi, mp, peak, want, bar, ref, guard, tag):
    """one line of the device against the model: chi within its bar; map and peak against the model on the device's own arrays"""
    assert np.all(np.isfinite(chi.view(np.float32))) and np.all(np.isfinite(mp)) and np.all(np.isfinite(peak)), tag
    r = M.worst_ratio(chi.astype(np.complex128), want, bar)
    wm, bm = M.array_map(chi, ref)
    rm = M.worst_ratio(mp.astype(np.float64), wm, bm)
    wp, bp = M.all_peaks(chi, mp, guard)
    ep = np.abs(peak.astype(np.float64) - wp)
    print(f"{tag}: largest error / bar: chi {r:.4f} map {rm:.4f}; peak rows within bars {int(np.all(ep <= bp, axis=1).sum())} of {len(ep)}")
    assert r <= 1.0, (tag, r)
    assert rm <= 1.0, (tag, rm)
    assert np.all(ep <= bp), (tag, peak, wp, bp)
    return r


# (nrows, B, seg, frames, nlags, ref, pad): the smallest everything; nlags = seg with the last row as reference; an odd lag count with a
# lag-tile tail, two packets' zero prefixes and the reference in the middle; even nrows (the matrix only 4-byte aligned) at two strides;
# nd = 4096 (one lag a tile); nd = 8 with seg at its maximum; the workload's shape, one line; nd = 2048 (two lags a tile, the last tile one)
CASES = [(2, 512, 16, 1, 1, 0, 0), (2, 512, 16, 1, 16, 1, 0), (3, 2048, 64, 2, 17, 1, 0), (4, 2048, 64, 2, 16, 0, 4), (4, 2048, 64, 2, 16, 0, 0),
         (2, 16384, 16, 8, 5, 0, 0), (2, 8192, 4096, 8, 33, 0, 0), (22, 16384, 128, 4, 64, 0, 0), (2, 8192, 16, 8, 5, 1, 0)]
_Y = {}


def _model(case, line, kind):
    """the model of a case's line; the exact range stage is computed once per case and shared by the windows"""
    nrows, B, seg, frames, nlags, ref, pad = case
    if case not in _Y:
        _Y[case] = M.range_stage(line, seg, nlags, ref)
    return M.caf_from_y(*_Y[case], seg, kind)


@pytest.mark.parametrize("kind", [RECT, HANN])
@pytest.mark.parametrize("case", CASES)
def test_chi_map_and_peaks_against_the_model(b, torch, case, kind):
    nrows, B, seg, frames, nlags, ref, pad = case
    line = [M.random_matrix(nrows, B, 7 * B + seg + t) for t in range(frames)]
    want, bar = _model(case, line, kind)
    nd = frames * B // (2 * seg)
    guard = min(2, nd // 2)
    out = _run(b, torch, np.stack(line), seg, nlags, ref, kind, guard, frames, pad)
    _check_line(out["chi"][0], out["map"][0], out["peak"][0], want, bar, ref, guard, f"case {case} window {kind}")


def test_exact_cells_at_zero_doppler(b, torch):
    """rect, bin d = 0, rows of small integers: sum_k y fits fp32 exactly and the transform's DC path is additions only, so chi[0][tau] is
    the exact integer sum times the fp32 scale: two roundings (the scale's own and the product's).  This pins the range stage's integers."""
    nrows, B, seg, frames, nlags, ref = 3, 2048, 64, 2, 17, 1
    rng = np.random.default_rng(5)
    line = [rng.integers(-3, 4, size=(nrows, B)).astype(np.int8) for _ in range(frames)]
    yr, yi = M.range_stage(line, seg, nlags, ref)
    sr, si = yr.sum(axis=1), yi.sum(axis=1)                                       # [nrows][R], exact
    assert max(np.abs(sr).max(), np.abs(si).max()) < 2 ** 24 and np.abs(si).max() > 0
    out = _run(b, torch, np.stack(line), seg, nlags, ref, RECT, 0, frames)
    nd = frames * B // (2 * seg)
    sc = M.scale_of(seg, nd, RECT)
    got = out["chi"][0][:, 0, :].astype(np.complex128)
    for g, s in ((got.real, sr), (got.imag, si)):
        exact = s.astype(np.float64) * sc
        assert np.all(np.abs(g - exact) <= 2.0 * M.U * (1.0 + M.U) * np.abs(exact)), np.max(np.abs(g - exact) / np.maximum(np.abs(exact), 1e-300))


def test_full_scale_and_all_zero(b, torch):
    nrows, B, seg, frames, nlags = 2, 8192, 4096, 8, 33
    full = [np.full((nrows, B), -128, dtype=np.int8)] * frames                    # |y| = 2^27 at lag 0
    want, bar = M.caf(full, seg, nlags, 0, HANN)
    out = _run(b, torch, np.stack(full), seg, nlags, 0, HANN, 1, frames)
    _check_line(out["chi"][0], out["map"][0], out["peak"][0], want, bar, 0, 1, "every byte -128, seg 4096")
    assert abs(out["chi"][0][1, 0, 0].real - 2 ** 27 / (127.0 ** 2 * seg)) <= bar[1, 0, 0]
    for guard in (0, 2):
        z = _run(b, torch, np.zeros((frames, nrows, B), dtype=np.int8), seg, nlags, 1, HANN, guard, frames)
        assert not z["chi"].view(np.float32).any() and not z["map"].any() and not z["peak"].any()
        assert all(np.all(np.isfinite(v.view(np.float32) if np.iscomplexobj(v) else v)) for v in z.values())


# (B, seg, frames, nlags, t0, d0, a): tests/test_caf_model.py runs the same four on the CPU
SCENES = [(2048, 64, 2, 16, 5, 3, 0.3), (2048, 64, 2, 16, 11, -7, 0.3), (1024, 16, 1, 8, 3, 5, 0.3), (4096, 128, 4, 32, 20, -9, 0.1)]


@pytest.mark.parametrize("kind", [RECT, HANN])
@pytest.mark.parametrize("scene", SCENES)
def test_echo_scenes(b, torch, scene, kind):
    B, seg, frames, nlags, t0, d0, a = scene
    line = M.echo_scene(B, frames, [(1, t0, d0, a)], seed=B + t0)
    want, bar = M.caf(line, seg, nlags, 0, kind)
    out = _run(b, torch, np.stack(line), seg, nlags, 0, kind, 2, frames)
    _check_line(out["chi"][0], out["map"][0], out["peak"][0], want, bar, 0, 2, f"scene {scene} window {kind}")
    pk = out["peak"][0]
    assert (pk[1, 0], pk[1, 1]) == (t0, d0) and (pk[2, 0], pk[2, 1]) == (t0, d0), pk      # the surveillance row, and the map (one row but r)
    print(f"scene {scene} window {kind}: row 1 peak {pk[1]}")


def test_two_echoes_in_different_rows(b, torch):
    """the map's peak is the stronger echo's, not every row's own"""
    B, seg, frames, nlags = 2048, 64, 2, 16
    line = M.echo_scene(B, frames, [(0, 4, 6, 0.2), (2, 9, -5, 0.4)], nrows=3, ref=1, seed=77)
    want, bar = M.caf(line, seg, nlags, 1, HANN)
    out = _run(b, torch, np.stack(line), seg, nlags, 1, HANN, 2, frames)
    _check_line(out["chi"][0], out["map"][0], out["peak"][0], want, bar, 1, 2, "two echoes")
    pk = out["peak"][0]
    assert (pk[0, 0], pk[0, 1]) == (4, 6) and (pk[2, 0], pk[2, 1]) == (9, -5) and (pk[3, 0], pk[3, 1]) == (9, -5), pk


def test_guard_sweep(b, torch):
    B, seg, frames, nlags, t0, d0, a = SCENES[0]
    line = M.echo_scene(B, frames, [(1, t0, d0, a)], seed=B + t0)
    nd = frames * B // (2 * seg)
    want, bar = M.caf(line, seg, nlags, 0, RECT)
    where = {}
    for guard in (0, 1, 2, nd // 2):
        out = _run(b, torch, np.stack(line), seg, nlags, 0, RECT, guard, frames)
        _check_line(out["chi"][0], out["map"][0], out["peak"][0], want, bar, 0, guard, f"guard {guard}")
        where[guard] = tuple(out["peak"][0][1, :2])
    assert where[0] == (0, 0) and where[1] == (t0, d0) and where[2] == (t0, d0) and where[nd // 2][1] == -nd // 2, where


def test_a_line_has_its_bits_anywhere_and_from_the_per_op_call(b, torch):
    nrows, B, seg, nlags, ref, kind, guard = 3, 2048, 64, 17, 2, HANN, 2
    blocks = np.stack([M.random_matrix(nrows, B, 900 + t) for t in range(8)])
    blocks[7] = blocks[0]
    alone = _run(b, torch, blocks[:1], seg, nlags, ref, kind, guard, 1, max_batch=8)
    batch = _run(b, torch, blocks, seg, nlags, ref, kind, guard, 1, pad=40)
    assert _same_line(alone, 0, batch, 0) and _same_line(alone, 0, batch, 7)
    assert not _same_line(alone, 0, batch, 1)
    chi, mp, pk = b.ambiguity(blocks[0], seg, nlags, ref, kind, guard)
    assert _same_bits(chi.view(np.float32), alone["chi"][0].view(np.float32)) and _same_bits(mp, alone["map"][0]) and _same_bits(pk, alone["peak"][0])
    dev = torch.device("cuda", 0)
    nd = B // (2 * seg)
    m = torch.zeros(4 + nrows * B, dtype=torch.int8, device=dev)                 # the matrix 4 bytes into an allocation: 4-byte aligned only
    m[4:] = torch.from_numpy(blocks[0].reshape(-1)).to(dev)
    dc, dm, dp = torch.zeros(nrows * nd * nlags * 2, device=dev), torch.zeros(nd * nlags, device=dev), torch.zeros((nrows + 1) * 6, device=dev)
    b.ambiguity_device(dc.data_ptr(), dm.data_ptr(), dp.data_ptr(), m.data_ptr() + 4, nrows, B, seg, nlags, ref, kind, guard)
    assert _same_bits(dc.cpu().numpy().reshape(nrows, nd, nlags, 2), chi.view(np.float32).reshape(nrows, nd, nlags, 2))
    assert _same_bits(dm.cpu().numpy().reshape(nd, nlags), mp) and _same_bits(dp.cpu().numpy().reshape(nrows + 1, 6), pk)
    dp.zero_()
    b.ambiguity_device(0, 0, dp.data_ptr(), m.data_ptr() + 4, nrows, B, seg, nlags, ref, kind, guard)      # only the peaks asked for
    assert _same_bits(dp.cpu().numpy().reshape(nrows + 1, 6), pk)
    with pytest.raises(b.CrsdrError) as e:
        b.ambiguity_device(dc.data_ptr() + 4, dm.data_ptr(), dp.data_ptr(), m.data_ptr() + 4, nrows, B, seg, nlags, ref, kind, guard)      # chi 8-byte aligned
    assert e.value.code == EINVAL


@pytest.mark.parametrize("nblocks", [1, 8])
def test_behind_a_plan_on_the_packets_as_published(b, torch, nblocks):
    """a plan's batch, the maps behind it on the plan's stream with no host wait in between; the same bits as a submit on the fetched
    packets, and as many launches for one block as for eight"""
    nrows, B, seg, nlags, frames = 3, 2048, 64, 16, 1 if nblocks == 1 else 2
    rows = np.stack([M.echo_scene(B, 1, [(1, 5, 0, 0.3)], nrows=nrows, seed=300 + t)[0] for t in range(nblocks)])
    plan = b.Plan(nrows, B, b.MODE_DIGITAL, max_batch=8)
    cf = b.Caf(nrows, B, seg, nlags, 0, HANN, 2, max_batch=8, frames=frames)
    with pytest.raises(b.CrsdrError) as e:
        cf.fetch()
    assert e.value.code == ESTATE
    plan.submit(rows, seq=0)
    cf.submit_plan(plan)
    assert cf._last() == (nblocks // frames, 3)
    out = cf.fetch()
    pub = np.stack([plan.fetch(block=t)["matrix"].copy() for t in range(nblocks)])
    pk = Packets(torch, pub)
    cf.submit(pk.ptr, pk.stride, pk.offset, nblocks)
    assert cf._last() == (nblocks // frames, 3)
    again = cf.fetch()
    for e_ in range(nblocks // frames):
        assert _same_line(out, e_, again, e_), e_
        want, bar = M.caf(list(pub[e_ * frames:(e_ + 1) * frames]), seg, nlags, 0, HANN)
        _check_line(out["chi"][e_], out["map"][e_], out["peak"][e_], want, bar, 0, 2, f"plan nblocks {nblocks} line {e_}")
    assert set(cf.fetch(chi=False, map=False)) == {"peak"} and all(cf.device_buffers().values())
    cf.close()
    plan.close()


def test_refusals(b, torch):
    nrows, B = 5, 1024
    cf = b.Caf(nrows, B, 16, 8, 0, RECT, 0, max_batch=8, frames=2)
    fresh = b.Plan(nrows, B, b.MODE_FAITHFUL, max_batch=8)
    with pytest.raises(b.CrsdrError) as e:
        cf.submit_plan(fresh)                                                # nothing submitted
    assert e.value.code == ESTATE
    with pytest.raises(b.CrsdrError) as e:
        cf._last()                                                           # ... and nothing of its own
    assert e.value.code == ESTATE
    rows = np.stack([M.random_matrix(nrows, B, 40 + t) for t in range(3)])
    fresh.submit(rows, seq=0)
    with pytest.raises(b.CrsdrError) as e:
        cf.submit_plan(fresh)                                                # a batch of 3 is not a multiple of frames = 2
    assert e.value.code == EINVAL
    fresh.sync()
    slab = torch.zeros(8 * (nrows - 1) * B, dtype=torch.int8, device=torch.device("cuda", 0))
    fresh.bind_slab(slab.data_ptr(), (nrows - 1) * B, 0, 8)
    with pytest.raises(b.CrsdrError) as e:
        cf.submit_plan(fresh)                                                # slab output: the matrix is not in the packet
    assert e.value.code == ESTATE
    fresh.close()
    other = b.Plan(nrows - 1, B, b.MODE_FAITHFUL, max_batch=8)
    with pytest.raises(b.CrsdrError) as e:
        cf.submit_plan(other)                                                # another nrows
    assert e.value.code == EINVAL
    other.close()
    pk = Packets(torch, rows[:2])
    for args in ((pk.ptr, pk.stride, pk.offset, 3), (pk.ptr, pk.stride, pk.offset, 10), (pk.ptr, pk.stride, pk.offset + 2, 2),
                 (pk.ptr, pk.stride + 2, pk.offset, 2), (0, pk.stride, pk.offset, 2)):
        with pytest.raises(b.CrsdrError) as e:
            cf.submit(*args)                                                 # nblocks % frames, > max_batch, alignment, NULL
        assert e.value.code == EINVAL
    cf.close()
