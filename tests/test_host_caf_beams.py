"""The beams' decisions on the host, and the demo.

csrc/caf_beams.hpp -- the limits, which row is which element, a beam sum in the kernel's order and its power, the steering weights, the
candidates, their order, "within one cell", suppression and the survivor's record, the functions the kernels of
csrc/caf_beams_kernels.hpp call -- as a stand-alone program (tools/caf_beams_cpu.cc) under AddressSanitizer + UBSan, on inputs the numpy
model wrote: every index of the product's own functions checked without a GPU, the maps held against tests/caf_beams_model.py within the
bars its docstring derives, the fused lists equal to the model's, the weights within the steering allowance.  The sanitizers report on
stderr and through the exit status; both must stay clean.  Nothing is loaded into Python under a sanitizer."""
import importlib
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import caf_beams_model as B
import caf_bearing_model as BM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "caf_beams_cpu.cc")
HOST = os.path.join(ROOT, "coherent-rtlsdr_amd", "host")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed for the host build of the beams' decisions")
    out = tmp_path_factory.mktemp("asan") / "caf_beams_cpu"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off", "-o", str(out), SRC], check=True)
    return str(out)


def run(exe, tmp_path, items):
    """items: ("maps", chi, ref, W) -> bmap | ("fuse", bdet, bcount, nd, R) -> (fused, nfused) | ("steer", Desc, xy) -> w"""
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        f.write(np.int32(len(items)).tobytes())
        for it in items:
            if it[0] == "maps":
                _, chi, ref, W = it
                nrows, nd, R = chi.shape
                f.write(np.array([0, nrows, nd, R, ref, len(W)], dtype=np.int32).tobytes())
                f.write(np.ascontiguousarray(chi, dtype=np.complex64).tobytes())
                f.write(np.ascontiguousarray(W, dtype=np.complex64).tobytes())
            elif it[0] == "fuse":
                _, bdet, bcount, nd, R = it
                f.write(np.array([1, bdet.shape[0], bdet.shape[1], nd, R], dtype=np.int32).tobytes())
                f.write(np.ascontiguousarray(bdet, dtype=np.float32).tobytes())
                f.write(np.ascontiguousarray(bcount, dtype=np.int32).tobytes())
            else:
                _, q, xy = it
                f.write(np.array([2, q.mx, q.my, q.ncx, q.ncy, len(xy)], dtype=np.int32).tobytes())
                f.write(np.float32(q.d).tobytes())
                f.write(np.ascontiguousarray(xy, dtype=np.float64).tobytes())
    r = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-3000:])
    raw = open(dst, "rb").read()
    out, at = [], 0
    for it in items:
        if it[0] == "maps":
            shape = (len(it[3]),) + it[1].shape[1:]
            out.append(np.frombuffer(raw, np.float32, int(np.prod(shape)), at).reshape(shape))
            at += 4 * out[-1].size
        elif it[0] == "fuse":
            K = it[1].shape[1]
            nf = int(np.frombuffer(raw, np.int32, 1, at)[0])
            out.append((np.frombuffer(raw, np.float32, K * 8, at + 4).reshape(K, 8), nf))
            at += 4 + 32 * K
        else:
            n = len(it[2]) * it[1].m
            out.append(np.frombuffer(raw, np.float32, 2 * n, at).view(np.complex64).reshape(len(it[2]), it[1].m))
            at += 8 * n
    assert at == len(raw)
    return out


def _chi(nrows, nd, R, seed):
    rng = np.random.default_rng(seed)
    return ((rng.standard_normal((nrows, nd, R)) + 1j * rng.standard_normal((nrows, nd, R))) * 1e-3).astype(np.complex64)


def _w(nb, m, seed):
    rng = np.random.default_rng(seed)
    return ((rng.standard_normal((nb, m)) + 1j * rng.standard_normal((nb, m))) / np.sqrt(2 * m)).astype(np.complex64)


# (m, nbeams, ref, nd, R): one element; ref first, middle and last; 64 x 64
MAPS = [(1, 1, 0, 8, 1), (2, 31, 2, 8, 4), (21, 33, 10, 8, 5), (33, 32, 0, 16, 3), (64, 64, 64, 8, 4)]


def test_the_maps_on_the_host_against_the_model(exe, tmp_path):
    items = []
    for k, (m, nb, ref, nd, R) in enumerate(MAPS):
        chi, W = _chi(m + 1, nd, R, 100 + k), _w(nb, m, 200 + k)
        chi[:, 0, 0] = 0
        chi[:, 1, R - 1] *= np.float32(1e-36)                                    # fp32 subnormals
        W[nb - 1] = 0
        items.append(("maps", chi, ref, W))
    for (_, chi, ref, W), got in zip(items, run(exe, tmp_path, items)):
        P, bar = B.bmap(chi, ref, W)
        assert np.all(np.isfinite(got))
        err = np.abs(got.astype(np.float64) - P)
        assert np.all(err <= bar), (chi.shape, len(W), float(np.max(err / bar)))
        assert not got[-1].any() and not got[:, 0, 0].any()
        # the mistakes about the elements and the weights' layout would not pass
        for which in B.MUTATIONS:
            if chi.shape[0] > 2 and len(W) > 1 and (which != "ref_counts" or ref != chi.shape[0] - 1):
                assert np.any(np.abs(got.astype(np.float64) - B.bmap(chi, ref, W, which)[0]) > bar), (which, chi.shape)


def test_the_fusion_on_the_host_equals_the_model(exe, tmp_path):
    items = [("fuse",) + B.hand_lists(entries, 4, 4, B.HAND_ND) + (B.HAND_ND, B.HAND_R) for entries, _ in B.HAND_FUSE.values()]
    # more survivors than K, counts above K, all counts zero, and 64 x 64 candidates
    spread = [(b, 2 * b, tau, 20.0 - tau - b) for b in range(3) for tau in (0, 2, 4)]      # nine cells, no two within one cell
    items.append(("fuse",) + B.hand_lists(spread, 3, 5, 8) + (8, 6))
    items.append(("fuse", np.zeros((5, 3, 8), dtype=np.float32), np.zeros(5, dtype=np.int32), 8, 6))
    rng = np.random.default_rng(9)
    full = []
    for b in range(64):
        cells = rng.choice(64 * 24, size=64, replace=False)
        full += [(b, int(c) // 24, int(c) % 24, float(p)) for c, p in zip(cells, np.sort(rng.integers(1, 50, size=64))[::-1])]
    items.append(("fuse",) + B.hand_lists(full, 64, 64, 64) + (64, 24))
    for (_, bdet, bcount, nd, R), (fused, nf) in zip(items, run(exe, tmp_path, items)):
        want, wnf = B.fuse(bdet, bcount, nd, R)
        assert nf == wnf and np.array_equal(fused.view(np.uint32), want.astype(np.float32).view(np.uint32)), (bdet.shape, nf, wnf)
    assert run(exe, tmp_path, items[-3:-2])[0][1] > 5                           # (more survivors than K = 5)


def test_the_steering_weights_on_the_host(exe, tmp_path):
    items = [("steer", BM.Desc(7, 3, BM.SCENES[1][2], 100, 100), B.lattice(8, 8, 100)), ("steer", BM.Desc(1, 1, 0.5, 2, 2), np.array([[0.0, 2.0]])),
             ("steer", BM.Desc(8, 8, 0.5, 512, 512), np.array([[0.0, 0.0], [511.5, 17.25], [256.0, 256.0]]))]
    for (_, q, xy), got in zip(items, run(exe, tmp_path, items)):
        want = B.steer_weights(q, xy).astype(np.complex128)
        dw = got.astype(np.complex128) - want
        assert np.all(np.abs(dw.real) <= B.steer_bar(q)[None]) and np.all(np.abs(dw.imag) <= B.steer_bar(q)[None])
        assert np.allclose(np.sum(np.abs(got.astype(np.complex128)) ** 2, axis=1), 1.0, atol=1e-6)


@pytest.mark.gpu
def test_the_device_has_the_bits_of_the_host_chain(exe, tmp_path):
    """the accumulators of k_caf_beams are the k-ordered fmaf chain that bm::beam_sum states: crsdr_beam_maps equals the host program
    bit for bit, at one and two beam groups, whole chunks of eight elements and a tail, zeros and fp32 subnormals among the inputs"""
    b = importlib.import_module("coherent-rtlsdr_amd.binding")
    if b.device_count() < 1:
        pytest.fail("no HIP device: the product path has no CPU fallback")
    items = []
    for k, (m, nb, ref, nd, R) in enumerate([(21, 33, 10, 8, 5), (64, 64, 64, 8, 4), (8, 32, 0, 16, 3), (3, 5, 1, 8, 1)]):
        chi, W = _chi(m + 1, nd, R, 400 + k), _w(nb, m, 500 + k)
        chi[:, 0, 0] = 0
        chi[:, 1, R - 1] *= np.float32(1e-36)
        W[nb - 1] = 0
        items.append(("maps", chi, ref, W))
    for (_, chi, ref, W), host in zip(items, run(exe, tmp_path, items)):
        dev = b.beam_maps(chi, W, ref)
        assert dev.shape == host.shape and np.array_equal(dev.view(np.uint32), host.view(np.uint32)), (chi.shape, len(W), int((dev != host).sum()))


@pytest.fixture(scope="module")
def host_build():
    importlib.import_module("coherent-rtlsdr_amd.binding").build()
    subprocess.run(["make", "-C", HOST, "all", "libcsynth.so"], check=True, stdout=subprocess.DEVNULL)
    return HOST


FUSED = re.compile(r"beams: batch (\d+) line (\d+) fused (\d+) of (\d+): lag (\S+) doppler (\S+) power (\S+) snr (\S+) dB beam (\d+) alpha (\S+) deg beta (\S+) deg")


@pytest.mark.gpu
def test_host_demo_prints_the_fused_detections(host_build):
    """coherent_demo --bench --caf ... --cfar ... --caf-beams MXxMY:NXxNY (ccaf::batch over crsdr_caf_set_beams): fused lines with their
    beam's angles; shapes that do not match --nsig and lattices of more than 64 beams are refused; without --cfar the maps alone."""
    base = [os.path.join(host_build, "coherent_demo"), "--bench", "--caf", "64:16", "--nsig", "3", "--batch", "8", "--blocks", "16"]
    on = subprocess.run(base + ["--cfar", "12", "--max-det", "4", "--caf-beams", "3x1:4x2"], capture_output=True, text=True, timeout=300)
    print("\n".join([l for l in on.stdout.splitlines() if l.startswith(("beams:", "cfar:"))][:12]), on.stdout[-300:], on.stderr)
    assert on.returncode == 0 and "DEMO OK" in on.stdout, on.stdout + on.stderr
    rows = FUSED.findall(on.stdout)
    assert rows and all(int(r[8]) < 8 and 0.0 <= float(r[9]) <= 180.0 and 0.0 <= float(r[10]) <= 180.0 and float(r[6]) > 0.0 for r in rows), rows
    assert all(int(r[2]) < min(int(r[3]), 4) for r in rows)
    maps = subprocess.run(base + ["--caf-beams", "3x1:4x2"], capture_output=True, text=True, timeout=300)
    assert maps.returncode == 0 and "DEMO OK" in maps.stdout and "beams: 8 maps per line" in maps.stdout and not FUSED.findall(maps.stdout), maps.stdout + maps.stderr
    tall = subprocess.run(base + ["--cfar", "12", "--max-det", "4", "--caf-beams", "3x1:1x64"], capture_output=True, text=True, timeout=300)
    rows = FUSED.findall(tall.stdout)                                            # 64 beams along y: every direction inside the grid
    assert tall.returncode == 0 and rows and all(int(r[8]) < 64 and 0.0 <= float(r[9]) <= 180.0 and 0.0 <= float(r[10]) <= 180.0 for r in rows), tall.stdout[-2000:]
    for bad in (["--caf-beams", "2x2:4x2"], ["--caf-beams", "3x1:9x8"], ["--caf-beams", "3x1"]):
        r = subprocess.run(base + ["--cfar", "12"] + bad, capture_output=True, text=True, timeout=300)
        assert r.returncode != 0 and "--caf-beams MXxMY:NXxNY refused" in r.stdout + r.stderr, (bad, r.stdout[-500:], r.stderr[-500:])
