"""GPU checks of the beams of crsdr_doa (crsdr_doa_set_beams / crsdr_doa_fetch_beams / crsdr_beamform): the device's weights, power and
beams against the fp64 restatement (tests/doa_beams_model.py) fed with what the device published -- fetch_subspace, sv, peak or
peaks / found, and the packets.

Bars, derived, not measured:
  weights  |u_dev - u_model|_inf <= 2^-22 |u_model|_inf per beam: fp64 arithmetic (relative error <= sqrt(m) (1 + 1 / loading) 1e-16 <= 1e-9
           for loading >= 1e-6) and one rounding to fp32 (2^-24 per component); power to 2^-22 relative.  Empty slots exactly 0 / -1.
  beams    with the model using the device's fp32 weights, per sample and component
           |y_dev - y_model| <= (4 m + 4) 2^-24 sum_c (|Re u_c| + |Im u_c|) (|I_c[n]| + |Q_c[n]|) / 127: the bound for a sum of 2 m products in
           any order, doubled to cover the 1 / 127 wherever it is applied and fused or unfused multiply-adds.  Every entry.  Empty slots 0.
  crsdr_beamform on the same matrix and the fetched weights: the batched beams bit for bit.
The separation scenes are those of tests/test_doa_beams_abi.py (same seed), where the fp64 pipeline meets the same conditions."""
import importlib

import numpy as np
import pytest

import doa_beams_model as model
import ura

pytestmark = pytest.mark.gpu
EINVAL, ESTATE = -1, -5
P = np.pi
REL = 2.0 ** -22


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
    + 16 + 4 * nrows."""

    def __init__(self, torch, blocks):
        blocks = np.ascontiguousarray(blocks)
        self.T, self.nrows, self.B = blocks.shape
        self.offset = 16 + 4 * self.nrows
        self.stride = self.offset + self.nrows * self.B
        host = np.full((self.T, self.stride), 0x55, dtype=np.int8)
        host[:, self.offset:] = blocks.reshape(self.T, -1)
        self.buf = torch.from_numpy(host).to(torch.device("cuda", 0))
        self.ptr = self.buf.data_ptr()


def _blocks(T, L, mx, my, seed, nsrc=2):
    """T blocks, each with nsrc sources of its own; full-scale samples included (the quantiser clips at +-127 / -128)."""
    rng = np.random.default_rng(seed)
    return np.stack([ura.scene(L, [(0.4 + 2.3 * rng.random(), 0.4 + 2.3 * rng.random(), 1.0 / (1 + j)) for j in range(nsrc)], rng, mx=mx, my=my,
                               sigma_s=30.0) for _ in range(T)])


def _slots(doa, e, dirs, peak, fixed):
    """the model's slots of estimate e: fixed angles, the estimate's peaks, or its one peak"""
    if fixed is not None:
        return [tuple(float(x) for x in np.asarray(ang, dtype=np.float32)) for ang in fixed]
    if dirs is not None:
        return model.following_slots(int(dirs["found"][e]), dirs["peaks"][e], doa.ncx, doa.ncy)
    return [model.grid_angles(int(peak[e][0]), int(peak[e][1]), doa.ncx, doa.ncy)]


def _check_against_model(b, doa, blocks, n, mode, loading, mx, my, fixed=None, beamform_blocks=(0,), what=""):
    """Everything the device published for the last submit of n blocks against the model; returns the fetched beams dict."""
    F, m = doa.frames, doa.m
    out, vec = doa.fetch(), doa.fetch_subspace()
    dirs = doa.fetch_directions() if doa.npeaks else None
    got = doa.fetch_beams()
    nb = doa.nbeams
    assert got["weights"].shape == (n // F, nb, m) and got["power"].shape == (n // F, nb) and got["beams"].shape == (n, nb, doa.B // 2)
    worst_w = worst_p = worst_y = 0.0
    for e in range(n // F):
        slots = _slots(doa, e, dirs, out["peak"], fixed)
        assert len(slots) == nb
        w, p = model.slot_weights(vec[e], out["sv"][e], slots, mode, loading, ura.D, mx, my)
        for s_, ang in enumerate(slots):
            if ang is None:
                assert not got["weights"][e, s_].view(np.float32).any() and got["power"][e, s_] == -1.0, (what, e, s_)
                assert not got["beams"][e * F:(e + 1) * F, s_].view(np.float32).any(), (what, e, s_)
                continue
            dw, ref = np.abs(got["weights"][e, s_].astype(np.complex128) - w[s_].astype(np.complex128)).max(), np.abs(w[s_]).max()
            worst_w = max(worst_w, dw / ref)
            assert dw <= REL * ref, (what, "weights", e, s_, dw, ref)
            dp = abs(float(got["power"][e, s_]) - float(p[s_]))
            worst_p = max(worst_p, dp / max(abs(float(p[s_])), 1e-300))
            assert dp <= REL * abs(float(p[s_])), (what, "power", e, s_, got["power"][e, s_], p[s_])
        assert np.isfinite(got["weights"][e].view(np.float32)).all()
        for t in range(e * F, (e + 1) * F):
            y = model.beams(blocks[t], got["weights"][e])
            bound = model.beam_bound(blocks[t], got["weights"][e])
            d = got["beams"][t].astype(np.complex128) - y
            over = (np.abs(d.real) > bound) | (np.abs(d.imag) > bound)
            live = bound > 0
            if live.any():
                worst_y = max(worst_y, float((np.maximum(np.abs(d.real), np.abs(d.imag))[live] / bound[live]).max()))
            assert not over.any(), (what, "beams", t, int(over.sum()), np.argwhere(over)[:4].tolist())
    for t in beamform_blocks:
        if t < n:
            per_op = b.beamform(blocks[t], got["weights"][t // F])
            assert np.array_equal(per_op.view(np.uint32), got["beams"][t].view(np.uint32)), (what, "crsdr_beamform", t)
    print(f"{what}: n {n} slots {nb}: worst weights {worst_w / REL:.3f} and power {worst_p / REL:.3f} of the 2^-22 bar, beams {worst_y:.3f} of theirs")
    return got


SHAPES = [(mx, my, B) for mx, my in ((2, 1), (7, 3), (11, 3), (8, 8)) for B in (64, 16384, 131072)]


@pytest.mark.parametrize("mx,my,B", SHAPES)
def test_shapes_against_the_model(b, torch, mx, my, B):
    # set_peaks(4, 2) with MVDR beams at nblocks 1 and max_batch, then (beams off, peaks off, beams on) one conventional beam
    m = mx * my
    T = 2 if B > 16384 else 64                   # the beams of 64 blocks x 16 slots of 131072 would be 537 MB
    blocks = _blocks(T, B // 2, mx, my, 7000 + 100 * m + (B % 97))
    pk = Packets(torch, blocks)
    doa = b.Doa(m + 1, B, 1, ura.D, mx, my, max_batch=T)
    doa.set_peaks(4, 2)
    doa.set_beams(b.BEAM_MVDR, 1e-2)
    assert doa.nbeams == 4
    for n in (1, T):
        doa.submit(pk.ptr, pk.stride, pk.offset, n)
        assert doa.last_launches() == 9
        _check_against_model(b, doa, blocks, n, model.MVDR, 1e-2, mx, my, beamform_blocks=(0, n - 1), what=f"{mx}x{my} B {B} mvdr")
    doa.set_beams(b.BEAM_OFF)
    doa.set_peaks(0)
    doa.set_beams(b.BEAM_CONVENTIONAL)
    assert doa.nbeams == 1
    doa.submit(pk.ptr, pk.stride, pk.offset, T)
    assert doa.last_launches() == 7
    _check_against_model(b, doa, blocks, T, model.CONVENTIONAL, 0.0, mx, my, beamform_blocks=(T - 1,), what=f"{mx}x{my} B {B} conventional")
    doa.close()


@pytest.mark.parametrize("mode,loading", [(1, 0.0), (2, 1e-6), (2, 1e-2), (2, 1.0)])
def test_sixteen_slots_with_empty_ones_and_fixed_directions(b, torch, mode, loading):
    mx, my, B, T = 7, 3, 2048, 8
    blocks = _blocks(T, B // 2, mx, my, 99)
    pk = Packets(torch, blocks)
    # a coarse grid: fewer than 16 local peaks at radius 3, so the last slots are empty
    doa = b.Doa(22, B, 2, ura.D, mx, my, 24, 24, max_batch=T)
    doa.set_peaks(16, 3)
    doa.set_beams(mode, loading if mode == 2 else 0.5)
    assert doa.nbeams == 16
    doa.submit(pk.ptr, pk.stride, pk.offset, T)
    found = doa.fetch_directions()["found"]
    assert (found >= 1).all() and (found < 16).any(), found
    _check_against_model(b, doa, blocks, T, mode, loading, mx, my, what=f"16 slots mode {mode} loading {loading}")
    # three fixed directions, the same for every estimate; the peaks stay on and do not matter
    fixed = np.array([[0.5 * P, 0.5 * P], [0.3 * P, 0.61 * P], [2.0, 1.0]], dtype=np.float32)
    doa.set_beams(mode, loading if mode == 2 else 0.5, fixed_angles=fixed)
    assert doa.nbeams == 3
    doa.set_peaks(2, 1)                                                  # allowed: fixed beams are not sized by the count
    doa.submit(pk.ptr, pk.stride, pk.offset, T)
    assert doa.last_launches() == 9
    _check_against_model(b, doa, blocks, T, mode, loading, mx, my, fixed=fixed, what=f"3 fixed mode {mode} loading {loading}")
    doa.close()


def test_stacked_frames_share_one_weight_set(b, torch):
    mx, my, B, T, F = 7, 3, 4096, 16, 4
    blocks = _blocks(T, B // 2, mx, my, 4)
    pk = Packets(torch, blocks)
    doa = b.Doa(22, B, 2, ura.D, mx, my, max_batch=T, frames=F)
    doa.set_peaks(4, 2)
    doa.set_beams(b.BEAM_MVDR, 1e-2)
    for n in (4, 16):
        doa.submit(pk.ptr, pk.stride, pk.offset, n)
        got = _check_against_model(b, doa, blocks, n, model.MVDR, 1e-2, mx, my, beamform_blocks=(0, n - 1), what="F = 4")
        assert got["weights"].shape[0] == n // F and got["beams"].shape[0] == n
    doa.close()


def test_an_all_zero_packet_gets_the_conventional_beam(b, torch):
    mx, my, B, T = 7, 3, 1024, 4
    blocks = _blocks(T, B // 2, mx, my, 8)
    blocks[2] = 0
    pk = Packets(torch, blocks)
    for peaks in (0, 4):
        doa = b.Doa(22, B, 1, ura.D, mx, my, max_batch=T)
        if peaks:
            doa.set_peaks(peaks, 2)
        doa.set_beams(b.BEAM_MVDR, 1e-2)
        doa.submit(pk.ptr, pk.stride, pk.offset, T)
        sv = doa.fetch()["sv"]
        assert not sv[2].any(), sv[2]
        got = _check_against_model(b, doa, blocks, T, model.MVDR, 1e-2, mx, my, what=f"zero packet, peaks {peaks}")
        assert np.isfinite(got["weights"].view(np.float32)).all() and not got["beams"][2].view(np.float32).any()
        live = got["power"][2] != -1.0
        assert live[0] and (got["power"][2][live] == 0.0).all()
        assert np.allclose(np.abs(got["weights"][2][live]), 1.0 / 21, rtol=1e-6)       # a / m
        doa.close()


@pytest.mark.parametrize("name,grid_pts", [("on grid", model.ON_GRID), ("off grid", model.OFF_GRID)])
def test_mvdr_separates_a_weak_source_from_a_strong_one(b, torch, name, grid_pts):
    blk, sig = model.separation_block(grid_pts)
    pk = Packets(torch, blk[None])
    doa = b.Doa(22, 2 * model.L, model.K, ura.D, ura.MX, ura.MY, max_batch=1)
    doa.set_peaks(4, 2)
    doa.set_beams(b.BEAM_MVDR, model.LOADING)
    doa.submit(pk.ptr, pk.stride, pk.offset, 1)
    mv = _check_against_model(b, doa, blk[None], 1, model.MVDR, model.LOADING, ura.MX, ura.MY, what=name + " mvdr")
    dirs = doa.fetch_directions()
    doa.set_beams(b.BEAM_OFF)
    doa.set_beams(b.BEAM_CONVENTIONAL)
    doa.submit(pk.ptr, pk.stride, pk.offset, 1)
    cv = _check_against_model(b, doa, blk[None], 1, model.CONVENTIONAL, 0.0, ura.MX, ura.MY, what=name + " conventional")
    found = int(dirs["found"][0])
    if name == "off grid":
        assert found == 4
    print("conventional power", cv["power"][0].tolist())
    model.check_separation(sig, mv["beams"][0], cv["beams"][0], mv["power"][0], dirs["peaks"][0], found, grid_pts, name + " (device)")
    doa.close()


def test_through_a_plan_with_no_host_in_between(b, torch):
    # calibrate, freeze, a batch of k = 2 scenes: plan.submit then doa.submit_plan, fetched at the end; the plan's own packets, then
    # packets bound to a caller's buffer
    rng = np.random.default_rng(41)
    L, M, T, k = 4096, 21, 4, 2
    sources = [(0.35 * P, 0.40 * P, 1.0), (0.65 * P, 0.62 * P, 0.8)]
    phi = rng.uniform(-np.pi, np.pi, M)
    plan = b.Plan(M + 1, 2 * L, b.MODE_FAITHFUL, max_batch=T)
    doa = b.Doa(M + 1, 2 * L, k, ura.D, ura.MX, ura.MY, max_batch=T)
    doa.set_peaks(k, 1)
    doa.set_beams(b.BEAM_MVDR, 1e-2)
    for t in range(16):
        plan.block(ura.calibration_block(L, phi, rng), seq=t)
    rows = np.stack([ura.scene(L, sources, rng, phi=phi) for _ in range(T)])
    plan.submit(rows, seq=16, flags=0)
    doa.submit_plan(plan)                                                    # no sync, no fetch in between
    assert doa.last_launches() == 9
    mats = np.stack([plan.fetch(block=t)["matrix"] for t in range(T)])
    _check_against_model(b, doa, mats, T, model.MVDR, 1e-2, ura.MX, ura.MY, beamform_blocks=(0, T - 1), what="plan, own packets")
    stride = (plan.packet_bytes + 255) // 256 * 256
    bound = torch.zeros(T * stride, dtype=torch.int8, device=torch.device("cuda", 0))
    plan.bind_packet(bound.data_ptr(), stride)
    plan.submit(rows, seq=20, flags=0)
    doa.submit_plan(plan)
    got = doa.fetch_beams(weights=False, power=False)                         # waits for the stream
    host = bound.cpu().numpy().reshape(T, stride)
    mats2 = host[:, plan.matrix_offset:plan.packet_bytes].reshape(T, M + 1, 2 * L)
    _check_against_model(b, doa, mats2, T, model.MVDR, 1e-2, ura.MX, ura.MY, beamform_blocks=(1,), what="plan, bound packets")
    assert got["beams"].shape == (T, k, L)
    plan.bind_packet(None)
    plan.sync()
    doa.close()
    plan.close()


def test_switching_off_restores_the_object_and_launches_are_constant(b, torch):
    M, L, T = 21, 512, 64
    blocks = _blocks(T, L, 7, 3, 5, nsrc=1)
    pk = Packets(torch, blocks)
    doa = b.Doa(M + 1, 2 * L, 1, ura.D, ura.MX, ura.MY, 40, 40, max_batch=T, flags=b.DOA_KEEP_SPECTRUM)
    never = b.Doa(M + 1, 2 * L, 1, ura.D, ura.MX, ura.MY, 40, 40, max_batch=T, flags=b.DOA_KEEP_SPECTRUM)
    for with_peaks, base in ((False, 5), (True, 7)):
        if with_peaks:
            doa.set_peaks(4, 2)
            never.set_peaks(4, 2)
        doa.set_beams(b.BEAM_MVDR, 1e-3)
        assert all(doa.beam_buffers()[k] for k in ("weights", "power", "beams"))
        counts = {}
        for n in (1, 64):
            doa.submit(pk.ptr, pk.stride, pk.offset, n)
            counts[n] = doa.last_launches()
            assert doa.fetch_beams()["beams"].shape == (n, 4 if with_peaks else 1, L)
        assert counts[1] == counts[64] == base + 2, counts
        doa.set_beams(b.BEAM_OFF)
        bufs = doa.beam_buffers()
        assert bufs["nbeams"] == 0 and all(bufs[k] is None for k in ("weights", "power", "beams"))
        doa.submit(pk.ptr, pk.stride, pk.offset, 64)
        never.submit(pk.ptr, pk.stride, pk.offset, 64)
        assert doa.last_launches() == never.last_launches() == base
        assert doa._last() == never._last()
        a, c = doa.fetch(), never.fetch()
        for key in ("peak", "peak_value", "sv", "status", "pm"):
            assert np.array_equal(a[key].view(np.uint32), c[key].view(np.uint32)), key
        if with_peaks:
            x, y = doa.fetch_directions(), never.fetch_directions()
            for key in ("found", "peaks", "values"):
                assert np.array_equal(x[key].view(np.uint32), y[key].view(np.uint32)), key
        with pytest.raises(b.CrsdrError) as e:
            doa.fetch_beams()
        assert e.value.code == ESTATE
    doa.close()
    never.close()


def test_refusals(b, torch):
    doa = b.Doa(22, 1024, 1, ura.D, ura.MX, ura.MY, max_batch=2)
    lib = b.lib()
    ang = np.zeros((17, 2), dtype=np.float32)
    for mode, loading, fixed in ((3, 1e-2, None), (-1, 1e-2, None), (b.BEAM_MVDR, 0.0, None), (b.BEAM_MVDR, 5e-7, None), (b.BEAM_MVDR, 1.5, None),
                                 (b.BEAM_MVDR, float("nan"), None), (b.BEAM_CONVENTIONAL, 0.0, ang), (b.BEAM_MVDR, 1e-2, ang)):
        with pytest.raises(b.CrsdrError) as e:
            doa.set_beams(mode, loading, fixed_angles=fixed)
        assert e.value.code == EINVAL, (mode, loading)
    assert lib.crsdr_doa_set_beams(doa._h, b.BEAM_MVDR, 1e-2, -1, None) == EINVAL
    assert lib.crsdr_doa_set_beams(doa._h, b.BEAM_MVDR, 1e-2, 2, None) == EINVAL          # fixed directions and no angles
    doa.set_beams(b.BEAM_CONVENTIONAL, 123.0)                                            # the loading is ignored there
    with pytest.raises(b.CrsdrError) as e:
        doa.fetch_beams()                                                                # before a submit
    assert e.value.code == ESTATE
    with pytest.raises(b.CrsdrError) as e:
        doa.fetch_subspace()
    assert e.value.code == ESTATE
    for count in (4, 0):
        with pytest.raises(b.CrsdrError) as e:
            doa.set_peaks(count, 1)                                                      # following beams are sized by the count
        assert e.value.code == ESTATE
    doa.set_beams(b.BEAM_OFF)
    with pytest.raises(b.CrsdrError) as e:
        doa.fetch_beams()                                                                # beams off
    assert e.value.code == ESTATE
    doa.set_peaks(4, 1)
    doa.set_peaks(0)
    # crsdr_beamform
    mat, w = np.zeros((22, 64), dtype=np.int8), np.zeros((1, 21), dtype=np.complex64)
    out = np.zeros((1, 32), dtype=np.complex64)
    f32, i8 = b.C.POINTER(b.C.c_float), b.C.POINTER(b.C.c_int8)
    args = lambda nrows, B, nb, kind: (out.ctypes.data_as(f32), mat.ctypes.data_as(i8), nrows, B, w.ctypes.data_as(f32), nb, kind)
    assert lib.crsdr_beamform(*args(22, 64, 1, b.MEM_HOST)) == 0
    for bad in ((1, 64, 1, b.MEM_HOST), (66, 64, 1, b.MEM_HOST), (22, 48, 1, b.MEM_HOST), (22, 64, 0, b.MEM_HOST), (22, 64, 17, b.MEM_HOST), (22, 64, 1, 7)):
        assert lib.crsdr_beamform(*args(*bad)) == EINVAL, bad
    doa.close()


def test_cpp_engine_prints_a_power_per_direction():
    # coherent_demo --bench --music --peaks 2 --beams mvdr: cbeamformer::batch with set_peaks and set_beams; the synthetic channels all
    # carry the reference noise, so the strongest direction of every aligned block is broadside, grid point (50, 50), with the most power
    import os
    import re
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    host = os.path.join(root, "coherent-rtlsdr_amd", "host")
    importlib.import_module("coherent-rtlsdr_amd.binding").build()
    subprocess.run(["make", "-C", host, "all"], check=True, stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(host, "coherent_demo"), "--bench", "--music", "--peaks", "2", "--beams", "mvdr", "--nsig", "21", "--batch", "8",
                        "--blocks", "32"], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "DEMO OK" in r.stdout, r.stdout + r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("doa: batch")]
    assert len(lines) == 4, lines
    for ln in lines:
        assert "8 estimates, peaks of the first:" in ln, ln
        dirs = re.findall(r"\((-?\d+), (-?\d+)\) power ([-+0-9.eE]+)", ln.split("peaks of the first:")[1])
        assert len(dirs) == 2 and dirs[0][:2] == ("50", "50"), ln
        power = [float(d[2]) for d in dirs]
        assert power[0] > 0 and power[0] > power[1] >= 0, ln
