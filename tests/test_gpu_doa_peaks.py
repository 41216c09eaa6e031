"""GPU checks of several directions per estimate (crsdr_doa_set_peaks / crsdr_doa_fetch_directions): the device's found, peaks and
values equal the numpy restatement of the definition (tests/doa_peaks_model.py) applied to the fetched spectrum.

Bars.  Equality with the restatement is exact (np.array_equal, values compared as bit patterns) and derived, not measured: the pass
only compares the bits the scan wrote, and the scan's arithmetic is unchanged (test_slot_zero_is_the_existing_peak, and the existing
tests/test_gpu_doa.py pin it against the per-op chain).  The physical test uses the existing bar of tests/test_gpu_doa.py against the
fp64 model: a source's mirrored direction within 1.5 grid points."""
import importlib
import itertools

import numpy as np
import pytest

import doa_peaks_model as model
import ura

pytestmark = pytest.mark.gpu
EINVAL, ESTATE = -1, -5
P = np.pi


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


def _blocks(T, L, mx, my, seed):
    rng = np.random.default_rng(seed)
    return np.stack([ura.scene(L, [(0.4 + 2.3 * rng.random(), 0.4 + 2.3 * rng.random(), 1.0)], rng, mx=mx, my=my) for _ in range(T)])


def _assert_same(got, exp, what=""):
    assert np.array_equal(got["found"], exp["found"]), (what, got["found"], exp["found"])
    assert np.array_equal(got["peaks"], exp["peaks"]), (what, np.argwhere(got["peaks"] != exp["peaks"])[:8])
    assert np.array_equal(got["values"].view(np.uint32), exp["values"].view(np.uint32)), what


def _mirrored(alpha, beta, nc=100):
    return (P - alpha) * nc / P, (P - beta) * nc / P


def _resolves(peaks, sources):
    """every source's mirrored direction within 1.5 grid points (both coordinates) of a distinct reported peak"""
    want = [_mirrored(a, be) for a, be, _ in sources]
    return any(all(abs(peaks[j][0] - w[0]) <= 1.5 and abs(peaks[j][1] - w[1]) <= 1.5 for j, w in zip(perm, want))
               for perm in itertools.permutations(range(len(peaks)), len(want)))


CASES = [  # (mx, my, ncx, ncy, count, radius)
    (7, 3, 100, 100, 4, 1),
    (7, 3, 100, 100, 16, 3),
    (8, 8, 37, 129, 16, 2),
    (2, 1, 1, 200, 5, 1),
    (3, 1, 3, 3, 16, 1),              # found < count
    (7, 3, 257, 65, 8, 16),           # ragged tiles, the largest radius
]


@pytest.mark.parametrize("mx,my,ncx,ncy,count,radius", CASES)
def test_exact_against_the_restatement(b, torch, mx, my, ncx, ncy, count, radius):
    # the same packets through an object that keeps the spectrum and one that does not (the workspace path): the same bits
    M, L, T = mx * my, 1024, 64
    blocks = _blocks(T, L, mx, my, 1000 * M + ncx)
    pk = Packets(torch, blocks)
    keep = b.Doa(M + 1, 2 * L, 1, ura.D, mx, my, ncx, ncy, max_batch=T, flags=b.DOA_KEEP_SPECTRUM)
    ws = b.Doa(M + 1, 2 * L, 1, ura.D, mx, my, ncx, ncy, max_batch=T)
    keep.set_peaks(count, radius)
    ws.set_peaks(count, radius)
    for n in (1, 64):
        keep.submit(pk.ptr, pk.stride, pk.offset, n)
        out = keep.fetch()
        got = keep.fetch_directions()
        assert got["peaks"].shape == (n, count, 2) and got["values"].shape == (n, count)
        exp = model.batch_directions(out["pm"], count, radius)
        print(f"{mx}x{my} {ncx}x{ncy} count {count} r {radius} n {n}: found {np.unique(got['found']).tolist()}")
        _assert_same(got, exp, "kept spectrum")
        # slot 0 is crsdr_doa_fetch's peak, bit for bit
        assert (got["found"] >= 1).all()
        assert np.array_equal(got["peaks"][:, 0], out["peak"])
        assert np.array_equal(got["values"][:, 0].view(np.uint32), out["peak_value"].view(np.uint32))
        ws.submit(pk.ptr, pk.stride, pk.offset, n)
        _assert_same(ws.fetch_directions(), got, "workspace")
        assert np.array_equal(ws.fetch()["peak"], out["peak"])
    assert ws.device_buffers()["pm"] is None and all(ws.direction_buffers().values())
    with pytest.raises(b.CrsdrError) as e:
        ws.fetch(spectrum=True)
    assert e.value.code == EINVAL
    keep.close()
    ws.close()


def test_stacked_frames(b, torch):
    M, L, T, F = 21, 1024, 64, 4
    blocks = _blocks(T, L, 7, 3, 44)
    pk = Packets(torch, blocks)
    doa = b.Doa(M + 1, 2 * L, 1, ura.D, 7, 3, max_batch=T, frames=F, flags=b.DOA_KEEP_SPECTRUM)
    doa.set_peaks(6, 2)
    for n in (4, 64):
        doa.submit(pk.ptr, pk.stride, pk.offset, n)
        out = doa.fetch()
        got = doa.fetch_directions()
        assert got["found"].shape == (n // F,)
        _assert_same(got, model.batch_directions(out["pm"], 6, 2))
        assert np.array_equal(got["peaks"][:, 0], out["peak"])
    doa.close()


SCENES = [  # k uncorrelated far-field sources (alpha, beta, amplitude) on the 7 x 3 URA
    [(0.35 * P, 0.40 * P, 1.0), (0.65 * P, 0.62 * P, 0.8)],
    [(0.30 * P, 0.55 * P, 1.0), (0.55 * P, 0.35 * P, 1.0)],
    [(0.30 * P, 0.40 * P, 1.0), (0.65 * P, 0.62 * P, 0.9), (0.45 * P, 0.70 * P, 0.8)],
]


def test_several_sources_are_resolved(b, torch):
    # count = k: the fp64 model finds 14-21 local maxima per spectrum at r = 1, so asking for more than k would test side lobes.
    # The inputs are ones for which the fp64 model (ura.music_fp64 + the restatement) meets the same bar; that is asserted here first,
    # on the CPU, for the very block the device gets.  One default_rng(7), a fresh block per scene and radius, in this order.
    rng = np.random.default_rng(7)
    L, M = 8192, 21
    for sources in SCENES:
        k = len(sources)
        for r in (1, 3):
            blk = ura.scene(L, sources, rng)
            _, _, _, pm64 = ura.music_fp64(blk, k)
            n64, p64, _ = model.directions(pm64.astype(np.float32), k, r)
            assert n64 == k and _resolves(p64, sources), ("fp64 model", k, r, p64)
            pk = Packets(torch, blk[None])
            doa = b.Doa(M + 1, 2 * L, k, ura.D, ura.MX, ura.MY, max_batch=1)
            doa.set_peaks(k, r)
            doa.submit(pk.ptr, pk.stride, pk.offset, 1)
            got = doa.fetch_directions()
            print(f"k {k} r {r}: device {got['peaks'][0].tolist()} fp64 {p64.tolist()} "
                  f"expected {[tuple(round(x, 2) for x in _mirrored(a, be)) for a, be, _ in sources]}")
            assert got["found"][0] == k and _resolves(got["peaks"][0], sources), (k, r, got["peaks"][0])
            doa.close()


def test_through_a_plan_with_no_host_in_between(b, torch):
    # calibrate (reference noise on), freeze, a batch of k = 2 scenes: plan.submit then doa.submit_plan, one fetch at the end
    rng = np.random.default_rng(37)
    L, M, T, k = 8192, 21, 4, 2
    sources = SCENES[0]
    phi = rng.uniform(-np.pi, np.pi, M)
    plan = b.Plan(M + 1, 2 * L, b.MODE_FAITHFUL, max_batch=T)
    doa = b.Doa(M + 1, 2 * L, k, ura.D, ura.MX, ura.MY, max_batch=T, flags=b.DOA_KEEP_SPECTRUM)
    doa.set_peaks(k, 1)
    for t in range(16):
        plan.block(ura.calibration_block(L, phi, rng), seq=t)
    rows = np.stack([ura.scene(L, sources, rng, phi=phi) for _ in range(T)])
    plan.submit(rows, seq=16, flags=0)
    doa.submit_plan(plan)                                                    # no sync, no fetch in between
    got = doa.fetch_directions()
    out = doa.fetch()
    assert doa.last_launches() == 7
    _assert_same(got, model.batch_directions(out["pm"], k, 1))
    for t in range(T):
        m = plan.fetch(block=t)["matrix"]
        _, _, _, pm64 = ura.music_fp64(m, k)
        assert _resolves(model.directions(pm64.astype(np.float32), k, 1)[1], sources), ("fp64 model", t)
        print(f"block {t}: device {got['peaks'][t].tolist()}")
        assert got["found"][t] == k and _resolves(got["peaks"][t], sources), (t, got["peaks"][t])
    plan.sync()
    doa.close()
    plan.close()


def test_launches_and_switching(b, torch):
    M, L, T = 21, 512, 64
    blocks = _blocks(T, L, 7, 3, 5)
    pk = Packets(torch, blocks)
    doa = b.Doa(M + 1, 2 * L, 1, ura.D, ura.MX, ura.MY, 40, 40, max_batch=T, flags=b.DOA_KEEP_SPECTRUM)
    never = b.Doa(M + 1, 2 * L, 1, ura.D, ura.MX, ura.MY, 40, 40, max_batch=T, flags=b.DOA_KEEP_SPECTRUM)
    doa.set_peaks(4, 2)
    counts = {}
    for n in (1, 64):
        doa.submit(pk.ptr, pk.stride, pk.offset, n)
        counts[n] = doa.last_launches()
        assert doa.fetch_directions()["peaks"].shape == (n, 4, 2)
    assert counts[1] == counts[64] == 7, counts
    # a new shape between submits
    doa.set_peaks(8, 1)
    with pytest.raises(b.CrsdrError) as e:
        doa.fetch_directions()                                               # nothing submitted since set_peaks
    assert e.value.code == ESTATE
    doa.submit(pk.ptr, pk.stride, pk.offset, 64)
    got = doa.fetch_directions()
    assert got["peaks"].shape == (64, 8, 2) and got["values"].shape == (64, 8)
    _assert_same(got, model.batch_directions(doa.fetch()["pm"], 8, 1))
    # off again: five launches, and what an object that never had peaks gives
    doa.set_peaks(0)
    assert all(v is None for v in doa.direction_buffers().values())
    doa.submit(pk.ptr, pk.stride, pk.offset, 64)
    assert doa.last_launches() == 5
    with pytest.raises(b.CrsdrError) as e:
        doa.fetch_directions()
    assert e.value.code == ESTATE
    never.submit(pk.ptr, pk.stride, pk.offset, 64)
    assert never.last_launches() == 5
    a, c = doa.fetch(), never.fetch()
    for key in ("peak", "peak_value", "sv", "status", "pm"):
        assert np.array_equal(a[key], c[key]), key
    doa.close()
    never.close()


def test_refusals(b, torch):
    doa = b.Doa(22, 1024, 1, ura.D, ura.MX, ura.MY, max_batch=2)
    for count, radius in ((-1, 1), (17, 1), (4, 0), (4, 17)):
        with pytest.raises(b.CrsdrError) as e:
            doa.set_peaks(count, radius)
        assert e.value.code == EINVAL, (count, radius)
    with pytest.raises(b.CrsdrError) as e:
        doa.fetch_directions()                                               # before set_peaks
    assert e.value.code == ESTATE
    doa.set_peaks(4, 2)
    with pytest.raises(b.CrsdrError) as e:
        doa.fetch_directions()                                               # before a submit
    assert e.value.code == ESTATE
    doa.close()


def test_cpp_engine_prints_several_directions_per_batch():
    # coherent_demo --bench --music --peaks 3: cbeamformer::batch with set_peaks; the synthetic channels all carry the reference noise,
    # so the strongest direction of every aligned block is broadside, grid point (50, 50)
    import os
    import re
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    host = os.path.join(root, "coherent-rtlsdr_amd", "host")
    importlib.import_module("coherent-rtlsdr_amd.binding").build()
    subprocess.run(["make", "-C", host, "all"], check=True, stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(host, "coherent_demo"), "--bench", "--music", "--peaks", "3", "--nsig", "21", "--batch", "8",
                        "--blocks", "32"], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "DEMO OK" in r.stdout, r.stdout + r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("doa: batch")]
    assert len(lines) == 4, lines
    for ln in lines:
        assert "8 estimates, peaks of the first:" in ln, ln
        dirs = re.findall(r"\((-?\d+), (-?\d+)\)", ln.split("peaks of the first:")[1])
        assert len(dirs) == 3 and dirs[0] == ("50", "50"), ln
