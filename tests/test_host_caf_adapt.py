"""The adaptive beams' decisions on the host.

csrc/caf_adapt.hpp -- the limits, the enumeration of the training cells and of their tiles, the order of the partial sums, the line's
solve on the bearings' Cholesky pieces, the figures and the fallback, the functions the kernels of csrc/caf_adapt_kernels.hpp call -- as
a stand-alone program (tools/caf_adapt_cpu.cc) under AddressSanitizer + UBSan, on inputs the numpy model wrote: every index of the
product's own functions checked without a GPU, the sums, the weights and the figures held against tests/caf_adapt_model.py within the
bars its docstring derives.  The sanitizers report on stderr and through the exit status; both must stay clean.  Nothing is loaded into
Python under a sanitizer."""
import importlib
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import caf_adapt_model as A
import caf_bearing_model as BM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "caf_adapt_cpu.cc")
HOST = os.path.join(ROOT, "coherent-rtlsdr_amd", "host")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed for the host build of the adaptive beams' decisions")
    out = tmp_path_factory.mktemp("asan") / "caf_adapt_cpu"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off", "-o", str(out), SRC], check=True)
    return str(out)


def run(exe, tmp_path, items):
    """items: (chi [nrows][nd][R], ref, V [nb][m], Desc) -> (status, tiles, aw [nb][m] complex64, ainfo [nb][2], Qs packed [pairs] complex128)"""
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        f.write(np.int32(len(items)).tobytes())
        for chi, ref, V, q in items:
            nrows, nd, R = chi.shape
            f.write(np.array([nrows, nd, R, ref, len(V), q.d_lo, q.d_n, q.r_lo, q.r_n], dtype=np.int32).tobytes())
            f.write(np.float32(q.loading).tobytes())
            f.write(np.ascontiguousarray(chi, dtype=np.complex64).tobytes())
            f.write(np.ascontiguousarray(V, dtype=np.complex64).tobytes())
    r = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-3000:])
    raw = open(dst, "rb").read()
    out, at = [], 0
    for chi, ref, V, q in items:
        nb, m = V.shape
        pairs = m * (m + 1) // 2
        status, tiles = (int(x) for x in np.frombuffer(raw, np.int32, 2, at))
        aw = np.frombuffer(raw, np.float32, 2 * nb * m, at + 8).view(np.complex64).reshape(nb, m)
        info = np.frombuffer(raw, np.float32, 2 * nb, at + 8 + 8 * nb * m).reshape(nb, 2)
        Qs = np.frombuffer(raw, np.float64, 2 * pairs, at + 8 + 8 * nb * m + 8 * nb).view(np.complex128)
        out.append((status, tiles, aw, info, Qs))
        at += 8 + 8 * nb * m + 8 * nb + 16 * pairs
    assert at == len(raw)
    return out


def _chi(nrows, nd, R, seed):
    rng = np.random.default_rng(seed)
    return BM.noise_chi(nrows, nd, R, seed, floor=np.exp(2j * np.pi * rng.random(nrows)))


def _w(nb, m, seed):
    rng = np.random.default_rng(seed)
    return ((rng.standard_normal((nb, m)) + 1j * rng.standard_normal((nb, m))) / np.sqrt(2 * m)).astype(np.complex64)


def check(item, got):
    chi, ref, V, q = item
    status, tiles, aw, info, Qs = got
    m = V.shape[1]
    r = A.adapt(chi, ref, V, q)
    assert status == r["status"] and tiles == A.tiles_of(q.N)
    if status:
        assert np.array_equal(aw.view(np.uint32), V.view(np.uint32)) and not info.any()
        return
    Q = np.array([[Qs[i * (i + 1) // 2 + k] if k <= i else np.conj(Qs[k * (k + 1) // 2 + i]) for k in range(m)] for i in range(m)]) / q.N
    assert np.all(np.abs(Q - r["Q"]) <= 2.0 * r["qbar"]), chi.shape
    assert np.all(np.isfinite(aw.view(np.float32)))
    assert np.all(np.abs(aw.real - r["w"].real) <= r["wbar"]) and np.all(np.abs(aw.imag - r["w"].imag) <= r["wbar"]), (chi.shape, float(np.max(np.abs(aw - r["w"]) / r["wbar"])))
    assert np.all(np.abs(info - r["info"]) <= r["ibar"]), (chi.shape, float(np.max(np.abs(info - r["info"]) / np.maximum(r["ibar"], 1e-300))))


# (m, nbeams, ref, nd, R, Desc): one element; 17 with the reference in the middle, a wrapped region of three tiles; 64 x 64 with the
# reference last, a region of more than 64 chunks (tiles of two chunks), N = 1 < m
CASES = [(1, 1, 0, 5, 7, A.Desc(1e-2, 0, 5, 0, 7)), (17, 33, 9, 8, 33, A.Desc(1e-2, 6, 5, 1, 32)), (64, 64, 64, 8, 33, A.Desc(1e-6, 0, 8, 0, 33)),
         (3, 2, 1, 128, 40, A.Desc(1.0, 100, 128, 0, 40)), (17, 4, 0, 5, 7, A.Desc(1e-3, 4, 1, 6, 1))]


def test_the_host_program_against_the_model(exe, tmp_path):
    items = []
    for k, (m, nb, ref, nd, R, q) in enumerate(CASES):
        chi, V = _chi(m + 1, nd, R, 300 + k), _w(nb, m, 400 + k)
        V[nb - 1] = 0
        items.append((chi, ref, V, q))
    got = run(exe, tmp_path, items)
    assert [g[1] for g in got] == [1, 3, 5, 40, 1]
    for item, g in zip(items, got):
        check(item, g)
        assert not g[2][-1].any() and not g[3][-1].any()                       # the all-zero beam keeps its zeros
    # the mistakes would not pass (the second case: wrapped, the reference in the middle, three tiles)
    chi, ref, V, q = items[1]
    r = A.adapt(chi, ref, V, q)
    for which in A.MUTATIONS:
        bad = A.adapt(chi, ref, V, q, which)
        assert np.any(np.abs(got[1][2].real - bad["w"].real) > r["wbar"]) or np.any(np.abs(got[1][2].imag - bad["w"].imag) > r["wbar"]), which


def test_the_tiles_are_the_edges_they_are_said_to_be(exe, tmp_path):
    """the library's own tiling (ad::tiles_of, as the program reports it) at tile - 1, tile, tile + 1 and 2 tile + 1 cells of the 64-cell
    tile, at the last N with one chunk a tile, the first with two, and the GPU test's largest region"""
    shapes = {63: (3, 21), 64: (2, 32), 65: (5, 13), 129: (3, 43), 4096: (64, 64), 4097: (17, 241), 5120: (128, 40)}
    items = []
    for k, (N, (d_n, r_n)) in enumerate(shapes.items()):
        nd, R = d_n + 1, r_n + 1
        items.append((_chi(3, nd, R, 900 + k), 1, _w(1, 2, 950 + k), A.Desc(1e-2, nd - 1, d_n, 1, r_n)))
        assert items[-1][3].N == N
    got = run(exe, tmp_path, items)
    assert [g[1] for g in got] == [1, 1, 2, 3, 64, 33, 40] == [A.tiles_of(n) for n in shapes] and A.tile_cells(5120) == 128
    for item, g in zip(items, got):
        check(item, g)


def test_the_fallbacks_on_the_host(exe, tmp_path):
    m, nb, ref, nd, R, q = CASES[1]
    chi, V = _chi(m + 1, nd, R, 7), _w(nb, m, 8)
    zero, nan_in, nan_out, inf_in = chi.copy(), chi.copy(), chi.copy(), chi.copy()
    for d, tau in A.train_cells(q, nd, R):
        zero[:, d, tau] = 0
    nan_in[3, 7, 5] = np.nan
    inf_in[3, 0, 32] = np.inf
    nan_out[3, 4, 5] = np.nan
    nan_out[5, 7, 0] = np.nan
    items = [(x, ref, V, q) for x in (zero, nan_in, nan_out, inf_in)]
    got = run(exe, tmp_path, items)
    assert [g[0] for g in got] == [A.STATUS_ZERO, A.STATUS_SOLVE, 0, A.STATUS_SOLVE]
    for item, g in zip(items, got):
        check(item, g)
    clean = run(exe, tmp_path, [(chi, ref, V, q)])[0]
    assert np.array_equal(got[2][2].view(np.uint32), clean[2].view(np.uint32))       # a NaN outside the region: no effect


@pytest.fixture(scope="module")
def host_build():
    importlib.import_module("coherent-rtlsdr_amd.binding").build()
    subprocess.run(["make", "-C", HOST, "all", "libcsynth.so"], check=True, stdout=subprocess.DEVNULL)
    return HOST


GAIN = re.compile(r"adapt: batch (\d+) line (\d+) status (\d+) mean gain (\S+) dB over (\d+) beams")


@pytest.mark.gpu
def test_host_demo_prints_the_mean_gain(host_build):
    """coherent_demo --bench --caf ... --caf-beams MXxMY:NXxNY --caf-adapt LOADING[:D_LO:D_N:R_LO:R_N] (ccaf::batch over
    crsdr_caf_set_beam_adapt): per line the status and the mean of 10 log10(ainfo[b][0] / ainfo[b][1]), never above 0 dB; without
    --caf-beams, and with a loading or a region outside the limits, it is refused."""
    base = [os.path.join(host_build, "coherent_demo"), "--bench", "--caf", "64:16", "--nsig", "3", "--batch", "8", "--blocks", "16"]
    for extra in (["--cfar", "12", "--max-det", "4", "--caf-adapt", "0.01"], ["--caf-adapt", "0.01:7:3:2:14"]):
        on = subprocess.run(base + ["--caf-beams", "3x1:4x2"] + extra, capture_output=True, text=True, timeout=300)
        print("\n".join([l for l in on.stdout.splitlines() if l.startswith("adapt:")][:6]), on.stdout[-300:], on.stderr)
        assert on.returncode == 0 and "DEMO OK" in on.stdout, on.stdout + on.stderr
        rows = GAIN.findall(on.stdout)
        assert rows and all(int(r[2]) == 0 and int(r[4]) == 8 and -60.0 < float(r[3]) <= 0.005 for r in rows), rows
    for bad in (["--caf-adapt", "0.01"], ["--caf-beams", "3x1:4x2", "--caf-adapt", "2"], ["--caf-beams", "3x1:4x2", "--caf-adapt", "0.01:0:8:10:14"],
                ["--caf-beams", "3x1:4x2", "--caf-adapt", "0.01:3"]):
        r = subprocess.run(base + bad, capture_output=True, text=True, timeout=300)
        assert r.returncode != 0 and "--caf-adapt LOADING[:D_LO:D_N:R_LO:R_N] refused" in r.stdout + r.stderr, (bad, r.stdout[-500:], r.stderr[-500:])
