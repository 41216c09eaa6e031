"""GPU checks of the batched direction-of-arrival engine (crsdr_doa): one submit for a batch of device-resident packets gives, per
estimate, exactly what crsdr_covariance -> crsdr_noisesubspace -> crsdr_pmusic2d -> argmax give for that packet's matrix.

Bars.  Equality with the per-op chain is bit for bit (np.array_equal) and derived, not measured: the covariance sums are exact
integers whatever the K split and go through the same fp64 epilogue; the subspace and every grid point run the same device function
as the per-op kernels (music::herm_subspace, music::pmusic2d_point, compiled without contraction).  Against the independent fp64
model the bars are the existing ones of tests/test_gpu_music.py: pm rtol 1e-2, peak within 1.5 grid points of the mirrored
direction."""
import importlib

import numpy as np
import pytest

import ura

pytestmark = pytest.mark.gpu


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
    + 16 + 4 * nrows.  The base is 256-byte aligned, so the matrix is 4- but (for nrows = 22: offset 104) not 16-byte aligned."""

    def __init__(self, torch, blocks, extra_stride=0):
        blocks = np.ascontiguousarray(blocks)
        self.T, self.nrows, self.B = blocks.shape
        self.offset = 16 + 4 * self.nrows
        self.stride = self.offset + self.nrows * self.B + extra_stride
        assert self.stride % 4 == 0
        host = np.full((self.T, self.stride), 0x55, dtype=np.int8)            # the headers / gaps hold something that is not zero
        host[:, self.offset: self.offset + self.nrows * self.B] = blocks.reshape(self.T, -1)
        self.buf = torch.from_numpy(host).to(torch.device("cuda", 0))
        self.ptr = self.buf.data_ptr()
        assert self.ptr % 256 == 0


def _per_op(b, matrix, k, d, mx, my, ncx, ncy):
    rxx = b.covariance(matrix)
    vec, sv = b.noisesubspace(rxx)
    pm = b.pmusic2d(vec, k, d, mx, my, ncx, ncy)
    return rxx, sv, pm


def _assert_equals_per_op(b, out, e, matrix, k, d, mx, my, ncx, ncy):
    rxx, sv, pm = _per_op(b, matrix, k, d, mx, my, ncx, ncy)
    assert np.array_equal(out["rxx"][e], rxx), f"estimate {e}: rxx differs in {np.count_nonzero(out['rxx'][e] != rxx)} entries"
    assert np.array_equal(out["sv"][e], sv), f"estimate {e}: sv {np.abs(out['sv'][e] - sv).max()}"
    assert np.array_equal(out["pm"][e], pm), f"estimate {e}: pm differs in {np.count_nonzero(out['pm'][e] != pm)} points"
    assert tuple(out["peak"][e]) == np.unravel_index(np.argmax(out["pm"][e]), (ncx, ncy))
    assert out["peak_value"][e] == out["pm"][e].max()
    assert out["status"][e] == 0


def _mirrored(alpha, beta, nc=100):
    # Rxx = X^H X of heatmap2d2.cpp:197 has conj(a) as its principal vector: the peak sits at (pi - alpha, pi - beta)
    return (np.pi - alpha) * nc / np.pi, (np.pi - beta) * nc / np.pi


def test_batch_equals_the_per_op_chain_bit_for_bit(b, torch):
    rng = np.random.default_rng(17)
    T, L, M = 16, 8192, 21
    dirs = [(0.5 + 0.13 * t, 2.4 - 0.11 * t) for t in range(T)]
    blocks = np.stack([ura.scene(L, [(al, be, 1.0)], rng) for al, be in dirs])
    pk = Packets(torch, blocks)
    assert (pk.ptr + pk.offset) % 16 != 0
    doa = b.Doa(M + 1, 2 * L, 1, ura.D, ura.MX, ura.MY, 100, 100, max_batch=T, frames=1, flags=b.DOA_KEEP_SPECTRUM | b.DOA_KEEP_RXX)
    doa.submit(pk.ptr, pk.stride, pk.offset, T)
    out = doa.fetch()
    assert out["rxx"].shape == (T, M, M) and out["pm"].shape == (T, 100, 100) and out["sv"].shape == (T, M)
    for t in range(T):
        _assert_equals_per_op(b, out, t, blocks[t], 1, ura.D, ura.MX, ura.MY, 100, 100)
    assert len({tuple(p) for p in out["peak"]}) == T                         # a different direction per block, a different peak
    assert np.array_equal(doa.fetch_peaks(), out["peak"])
    doa.close()


@pytest.mark.parametrize("B,max_batch", [(64, 5), (16384, 5), (131072, 2)])
@pytest.mark.parametrize("mx,my", [(2, 1), (4, 2), (11, 3), (8, 8)])
def test_other_sizes(b, torch, mx, my, B, max_batch):
    # one and two 32-row operand blocks (m = 33: one live row in the second), one MFMA step per wave at most (B = 64: two of the four
    # waves idle), K slices at the int32 bound (B = 131072), fewer blocks than the engine was made for, a non-square scan grid
    M, L, ncx, ncy = mx * my, B // 2, 20, 30
    nblocks = max_batch - 1 if max_batch > 2 else 2
    rng = np.random.default_rng(1000 * M + B % 997)
    blocks = np.stack([ura.scene(L, [(0.8 + 0.3 * t, 1.9 - 0.2 * t, 1.0)], rng, mx=mx, my=my) for t in range(nblocks)])
    blocks[0, 1] = -128                                                      # a full-scale DC row: the largest sums a slice has to hold
    pk = Packets(torch, blocks)
    doa = b.Doa(M + 1, B, 1, ura.D, mx, my, ncx, ncy, max_batch=max_batch, flags=b.DOA_KEEP_SPECTRUM | b.DOA_KEEP_RXX)
    doa.submit(pk.ptr, pk.stride, pk.offset, nblocks)
    out = doa.fetch()
    assert out["peak"].shape == (nblocks, 2)
    for t in range(nblocks):
        _assert_equals_per_op(b, out, t, blocks[t], 1, ura.D, mx, my, ncx, ncy)
    doa.close()


def test_stacked_frames(b, torch):
    # measurement_script.m: Nframes blocks stacked, X = [X; Xc] -- one estimate over four consecutive packets equals the per-op chain
    # on the four matrices concatenated along the row
    rng = np.random.default_rng(23)
    F, T, L, M = 4, 8, 8192, 21
    dirs = [(0.9, 2.0), (2.1, 1.2)]
    blocks = np.stack([ura.scene(L, [(*dirs[t // F], 1.0)], rng) for t in range(T)])
    pk = Packets(torch, blocks, extra_stride=64)
    doa = b.Doa(M + 1, 2 * L, 1, ura.D, ura.MX, ura.MY, max_batch=T, frames=F, flags=b.DOA_KEEP_SPECTRUM | b.DOA_KEEP_RXX)
    doa.submit(pk.ptr, pk.stride, pk.offset, T)
    out = doa.fetch()
    assert out["peak"].shape == (T // F, 2)
    for e in range(T // F):
        stacked = np.concatenate(list(blocks[e * F: (e + 1) * F]), axis=1)   # [nrows][F * B]
        assert stacked.shape == (M + 1, F * 2 * L)
        _assert_equals_per_op(b, out, e, stacked, 1, ura.D, ura.MX, ura.MY, 100, 100)
        cx, cy = _mirrored(*dirs[e])
        assert abs(out["peak"][e, 0] - cx) <= 1.5 and abs(out["peak"][e, 1] - cy) <= 1.5
    doa.close()


def test_against_the_independent_fp64_model(b, torch):
    rng = np.random.default_rng(29)
    L, M = 8192, 21
    dirs = [(0.7 + 0.2 * t, 2.2 - 0.15 * t) for t in range(8)]
    blocks = np.stack([ura.scene(L, [(al, be, 1.0)], rng) for al, be in dirs])
    pk = Packets(torch, blocks)
    doa = b.Doa(M + 1, 2 * L, 1, ura.D, ura.MX, ura.MY, max_batch=8, flags=b.DOA_KEEP_SPECTRUM)
    doa.submit(pk.ptr, pk.stride, pk.offset, 8)
    out = doa.fetch()
    assert "rxx" not in out
    for t, (al, be) in enumerate(dirs):
        cx, cy = _mirrored(al, be)
        print(f"direction {t}: peak {tuple(out['peak'][t])} expected ({cx:.2f}, {cy:.2f})")
        assert abs(out["peak"][t, 0] - cx) <= 1.5 and abs(out["peak"][t, 1] - cy) <= 1.5
        _, _, s64, pm64 = ura.music_fp64(blocks[t], 1)
        print(f"direction {t}: pm max rel err {np.abs(out['pm'][t] / pm64 - 1).max():.3e}")
        assert np.allclose(out["sv"][t], s64, rtol=1e-5)
        assert np.allclose(out["pm"][t], pm64, rtol=1e-2)
        assert out["status"][t] == 0
    doa.close()


@pytest.mark.parametrize("bound", [False, True])
def test_through_a_plan_with_no_host_in_between(b, torch, bound):
    # calibrate (reference noise on), freeze, then batches of 8 scene blocks with a moving source: plan.submit_batch and doa.submit_plan
    # back to back, one fetch.  Twice with different scenes: nothing is left over from the first batch.  bound: the plan writes its
    # packets into a caller's buffer (crsdr_plan_bind_packet) and the engine follows it there.
    rng = np.random.default_rng(31)
    L, M, T = 8192, 21, 8
    phi = rng.uniform(-np.pi, np.pi, M)
    plan = b.Plan(M + 1, 2 * L, b.MODE_FAITHFUL, max_batch=T)
    doa = b.Doa(M + 1, 2 * L, 1, ura.D, ura.MX, ura.MY, max_batch=T)
    if bound:
        stride = plan.packet_bytes + 8 + (-(plan.packet_bytes + 8)) % 4
        mine = torch.zeros(T * stride + 256, dtype=torch.int8, device=torch.device("cuda", 0))
        plan.bind_packet(mine.data_ptr(), stride)
    for t in range(16):
        plan.block(ura.calibration_block(L, phi, rng), seq=t)
    seq = 16
    peaks = []
    for rnd in range(2):
        dirs = [(0.8 + 0.6 * rnd + 0.1 * t, 2.3 - 0.5 * rnd - 0.08 * t) for t in range(T)]
        rows = np.stack([ura.scene(L, [(al, be, 1.0)], rng, phi=phi) for al, be in dirs])
        plan.submit(rows, seq=seq, flags=0)
        doa.submit_plan(plan)                                                # no sync, no fetch in between
        out = doa.fetch(spectrum=False, rxx=False)
        assert doa.last_launches() == 5
        seq += T
        assert out["peak"].shape == (T, 2) and not out["status"].any()
        for t, (al, be) in enumerate(dirs):
            cx, cy = _mirrored(al, be)
            assert abs(out["peak"][t, 0] - cx) <= 1.5 and abs(out["peak"][t, 1] - cy) <= 1.5, (rnd, t, out["peak"][t], cx, cy)
            m = plan.fetch(block=t)["matrix"]
            _, sv, pm = _per_op(b, m, 1, ura.D, ura.MX, ura.MY, 100, 100)
            assert tuple(out["peak"][t]) == np.unravel_index(np.argmax(pm), pm.shape)
            assert out["peak_value"][t] == pm.max() and np.array_equal(out["sv"][t], sv)
        peaks.append(out["peak"].copy())
        plan.sync()
    assert not np.array_equal(peaks[0], peaks[1])
    doa.close()
    plan.close()


def test_refusals(b, torch):
    L, M = 1024, 21
    doa = b.Doa(M + 1, 2 * L, 1, ura.D, ura.MX, ura.MY, max_batch=8, frames=2)
    with pytest.raises(b.CrsdrError) as e:
        doa.fetch()                                                          # before any submit
    assert e.value.code == -5
    fresh = b.Plan(M + 1, 2 * L, b.MODE_FAITHFUL, max_batch=8)
    with pytest.raises(b.CrsdrError) as e:
        doa.submit_plan(fresh)                                               # nothing submitted
    assert e.value.code == -5
    rng = np.random.default_rng(2)
    rows = np.stack([ura.scene(L, [(1.0, 1.5, 1.0)], rng) for _ in range(3)])
    fresh.submit(rows, seq=0)
    with pytest.raises(b.CrsdrError) as e:
        doa.submit_plan(fresh)                                               # a batch of 3 is not a multiple of frames = 2
    assert e.value.code == -1
    fresh.sync()
    slab = torch.zeros(8 * M * 2 * L, dtype=torch.int8, device=torch.device("cuda", 0))
    fresh.bind_slab(slab.data_ptr(), M * 2 * L, 0, 8)
    with pytest.raises(b.CrsdrError) as e:
        doa.submit_plan(fresh)                                               # slab output: the matrix is not in the packet
    assert e.value.code == -5
    fresh.close()
    other = b.Plan(M, 2 * L, b.MODE_FAITHFUL, max_batch=8)
    with pytest.raises(b.CrsdrError) as e:
        doa.submit_plan(other)                                               # another nrows
    assert e.value.code == -1
    other.close()
    pk = Packets(torch, rows[:2])
    for args in ((pk.ptr, pk.stride, pk.offset, 3), (pk.ptr, pk.stride, pk.offset, 10), (pk.ptr, pk.stride, pk.offset + 2, 2),
                 (pk.ptr, pk.stride + 2, pk.offset, 2), (0, pk.stride, pk.offset, 2)):
        with pytest.raises(b.CrsdrError) as e:
            doa.submit(*args)                                                # nblocks % frames, > max_batch, alignment, NULL
        assert e.value.code == -1
    doa.submit(pk.ptr, pk.stride, pk.offset, 2)
    for kw in (dict(spectrum=True), dict(rxx=True)):
        with pytest.raises(b.CrsdrError) as e:
            doa.fetch(**kw)                                                  # created without KEEP_SPECTRUM / KEEP_RXX
        assert e.value.code == -1
    out = doa.fetch()
    assert out["peak"].shape == (1, 2) and "pm" not in out and out["status"][0] == 0
    assert doa.device_buffers()["pm"] is None and doa.device_buffers()["peak"]
    doa.close()


def test_launches_do_not_depend_on_the_batch(b, torch):
    rng = np.random.default_rng(5)
    L, M, T = 512, 21, 64
    blocks = np.stack([ura.scene(L, [(0.6 + 0.03 * t, 1.4, 1.0)], rng) for t in range(T)])
    pk = Packets(torch, blocks)
    doa = b.Doa(M + 1, 2 * L, 1, ura.D, ura.MX, ura.MY, 40, 40, max_batch=T)
    counts = {}
    for n in (1, 64):
        doa.submit(pk.ptr, pk.stride, pk.offset, n)
        counts[n] = doa.last_launches()
        out = doa.fetch()
        assert out["peak"].shape == (n, 2) and not out["status"].any()
    assert counts[1] == counts[64] == 5, counts
    bufs = doa.device_buffers()
    assert bufs["peak"] and bufs["peak_value"] and bufs["sv"] and bufs["vec"] and bufs["pm"] is None
    doa.close()


def test_cpp_engine_prints_a_direction_per_block():
    # cbeamformer::batch behind ccoherent's pipelined batches (coherent_demo --bench --music): the 21 synthetic channels all carry the
    # reference noise, so every aligned block is one source at broadside
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    host = os.path.join(root, "coherent-rtlsdr_amd", "host")
    importlib.import_module("coherent-rtlsdr_amd.binding").build()
    subprocess.run(["make", "-C", host, "all"], check=True, stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(host, "coherent_demo"), "--bench", "--music", "--nsig", "21", "--batch", "8", "--blocks", "32"],
                       capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "DEMO OK" in r.stdout, r.stdout + r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("doa: batch")]
    assert len(lines) == 4 and all("8 directions" in ln for ln in lines), lines
    assert all("first (50, 50), last (50, 50), 8 at broadside" in ln for ln in lines), lines
