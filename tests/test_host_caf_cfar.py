"""The CFAR detector's decision arithmetic and the C++ host layer over it.

CPU: csrc/caf_cfar.hpp -- the training set and its count, the threshold test, the neighbourhood test, the order of the detections and
the eight figures that the kernels of csrc/caf_cfar_kernels.hpp call -- as a stand-alone program (tools/caf_cfar_cpu.cc) under
AddressSanitizer + UBSan, on maps the numpy model wrote: every index of the product's own functions checked without a GPU, and the
detections held against tests/caf_cfar_model.py within the bars its docstring derives.  The sanitizers report on stderr and through
the exit status; both must stay clean.  Nothing is loaded into Python under a sanitizer.

GPU: coherent_demo --bench --caf ... --cfar (ccaf::batch over crsdr_caf_set_cfar) prints a line per batch, line and detection of the
array map."""
import importlib
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import caf_cfar_model as C
import caf_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "caf_cfar_cpu.cc")
HOST = os.path.join(ROOT, "coherent-rtlsdr_amd", "host")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed for the host build of the detector")
    out = tmp_path_factory.mktemp("asan") / "caf_cfar_cpu"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off", "-o", str(out), SRC], check=True)
    return str(out)


def run(exe, tmp_path, items):
    """items: (src [nd][R] float32 or complex64, guard, Params, parts) -> (count, det [K][8] float32) each"""
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        f.write(np.int32(len(items)).tobytes())
        for a, guard, q, parts in items:
            nd, R = a.shape
            f.write(np.array([nd, R, guard, 2 if np.iscomplexobj(a) else 1, q.gd, q.gr, q.td, q.tr, q.min_train, q.max_det, parts], dtype=np.int32).tobytes())
            f.write(np.float32(q.alpha).tobytes())
            f.write(np.ascontiguousarray(a).tobytes())
    r = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-3000:])
    raw = open(dst, "rb").read()
    out, at = [], 0
    for a, guard, q, parts in items:
        out.append((int(np.frombuffer(raw, np.int32, 1, at)[0]), np.frombuffer(raw, np.float32, q.max_det * 8, at + 4).reshape(q.max_det, 8)))
        at += 4 + 32 * q.max_det
    assert at == len(raw)
    return out


def _want(a, guard, q):
    return C.detect(M.power(a) if np.iscomplexobj(a) else a.astype(np.float64), guard, q)


def _hold(got, items, ambiguous=0):
    """every case against the model: no ambiguous cell (but the ones put at the threshold on purpose), the same count, the same cells in
    the same order, every figure within its bar"""
    for (count, det), (a, guard, q, parts) in zip(got, items):
        want = _want(a, guard, q)
        assert want["ambiguous"] == ambiguous, (a.shape, guard, want["ambiguous"])
        assert np.all(np.isfinite(det)) and count == want["count"], (a.shape, guard, parts, count, want["count"])
        assert np.array_equal(det[:, [0, 1, 7]].astype(np.float64), want["det"][:, [0, 1, 7]]), (a.shape, guard, parts, det, want["det"])
        assert np.all(np.abs(det.astype(np.float64) - want["det"]) <= want["bar"]), (a.shape, guard, parts, det, want["det"], want["bar"])
        assert not det[min(count, q.max_det):].any()


def _floor(nd, R, seed, complex_):
    rng = np.random.default_rng(seed)
    if complex_:
        return (np.sqrt(0.5) * (rng.standard_normal((nd, R)) + 1j * rng.standard_normal((nd, R)))).astype(np.complex64)
    return rng.exponential(1.0, size=(nd, R)).astype(np.float32)


def test_the_kernels_decisions_on_the_host(exe, tmp_path):
    """a target at every corner of the map, at both guard edges and on either side of the cyclic wrap, over a noise floor"""
    items, planted = [], []
    for nd, R, q in ((8, 1, C.Params(6.0, 0, 0, 3, 0, max_det=4)), (8, 5, C.Params(6.0, 1, 1, 2, 15, max_det=4)), (32, 16, C.Params(8.0, 1, 1, 3, 4, max_det=8)),
                     (16, 70, C.Params(8.0, 1, 2, 0, 14, max_det=8)), (4096, 3, C.Params(8.0, 1, 1, 7, 1, max_det=4))):
        for guard in (0, 1, 2, nd // 2):
            edge = [g for g in (guard, nd - guard) if 0 <= g < nd] if guard else [0]
            spots = [(d, t) for d in sorted({0, nd - 1, nd // 2, nd // 2 - 1, *edge}) for t in sorted({0, R - 1, R // 2})]
            for i, (d, t) in enumerate(spots):
                complex_ = bool(i % 2)
                a = _floor(nd, R, 1000 * nd + 10 * i + guard, complex_)
                a[d, t] = 30.0 + (20.0j if complex_ else 0.0)
                a[(d + 1) % nd, t] = 3.0                                         # uneven neighbours: offsets that are not zero
                if t + 1 < R:
                    a[d, t + 1] = 2.5
                items.append((a, guard, q, 1 if i % 2 else 7))
                planted.append((d, t))
    got = run(exe, tmp_path, items)
    _hold(got, items)
    seen = 0
    for (count, det), (a, guard, q, parts), (d, t) in zip(got, items, planted):
        if abs(M.signed_bins(a.shape[0])[d]) >= guard and C.train_sums(np.zeros(a.shape), guard, q)[1][d, t] >= 1:
            assert count >= 1 and (det[0, 0], det[0, 1]) == (t, M.signed_bins(a.shape[0])[d]), (a.shape, guard, d, t, det[0])
            seen += 1
    assert seen > len(items) // 2


def test_plateaus_exact_thresholds_and_zeros_on_the_host(exe, tmp_path):
    four = C.Params(4.0, 1, 1, 3, 4, max_det=4)
    flat = np.ones((16, 24), dtype=np.float32)
    plateau = flat.copy()
    plateau[5, 6] = plateau[5, 7] = plateau[6, 6] = plateau[6, 7] = 9.0          # its first cell
    wrapped = flat.copy()
    wrapped[15, 3] = wrapped[0, 3] = 9.0                                         # a plateau across the cyclic wrap: (0, 3) has the smaller index
    at = flat.copy()
    at[5, 6], at[11, 17] = 4.0, 5.0                                              # noise = 1 and t = 4 exactly: P = 4 is not a detection
    cat = np.ones((16, 24), dtype=np.complex64)
    cat[5, 6], cat[11, 17] = 2.0 + 0j, 1.0 + 2.0j                                # |.|^2 = 4 and 5
    many = flat.copy()
    many[::4, ::4] = 9.0 + np.arange(6)[None, :]                                 # 24 detections, six powers four times each: ties by index
    zero, czero = np.zeros((4096, 3), dtype=np.float32), np.zeros((8, 1), dtype=np.complex64)
    items = [(plateau, 0, four, 1), (plateau, 0, four, 5), (wrapped, 0, four, 3), (many, 0, C.Params(4.0, 0, 0, 1, 1, max_det=5), 1),
             (many, 0, C.Params(4.0, 0, 0, 1, 1, max_det=64), 9)]
    got = run(exe, tmp_path, items)
    _hold(got, items)
    assert got[0][0] == 1 and (got[0][1][0, 0], got[0][1][0, 1]) == (6, 5) and list(got[1][1][0]) == list(got[0][1][0])
    assert got[2][0] == 1 and (got[2][1][0, 0], got[2][1][0, 1]) == (3, 0)
    assert got[3][0] == 24 and list(got[3][1][:, 2]) == [14, 14, 14, 14, 13] and list(got[3][1][:4, 1]) == [0, 4, -8, -4] and np.all(got[3][1][:4, 0] == 20)
    assert got[4][0] == 24 and np.all(np.diff(got[4][1][:24, 2]) <= 0) and not got[4][1][24:].any()
    exact = [(at, 0, four, 1), (cat, 0, four, 4)]
    got = run(exe, tmp_path, exact)
    _hold(got, exact, ambiguous=1)                                               # (the cell AT the threshold, and the model calls it as the device must)
    for count, det in got:
        assert count == 1 and list(det[0]) == [17, -5, 5, 5, 1, 0, 0, 90]
    zeros = [(zero, 0, four, 2), (zero, 2048, four, 1), (czero, 4, C.Params(4.0, 0, 0, 3, 0, max_det=64), 1), (czero, 0, C.Params(4.0, 0, 0, 3, 0), 3)]
    for count, det in run(exe, tmp_path, zeros):
        assert count == 0 and not det.any() and np.all(np.isfinite(det))


@pytest.fixture(scope="module")
def host_build():
    importlib.import_module("coherent-rtlsdr_amd.binding").build()
    subprocess.run(["make", "-C", HOST, "all", "libcsynth.so"], check=True, stdout=subprocess.DEVNULL)
    return HOST


LINE = re.compile(r"cfar: batch (\d+) line (\d+) det (\d+) of (\d+): lag (\d+)([+-]\S+) doppler (-?\d+)([+-]\S+) snr (\S+) dB")


@pytest.mark.gpu
def test_host_demo_prints_the_detections_of_the_array_map(host_build):
    nsig, batch, blocks, seg, lags = 3, 8, 16, 64, 16
    r = subprocess.run([os.path.join(host_build, "coherent_demo"), "--bench", "--caf", f"{seg}:{lags}", "--cfar", "12", "--max-det", "4", "--nsig", str(nsig),
                        "--batch", str(batch), "--blocks", str(blocks)], capture_output=True, text=True, timeout=300)
    print(r.stdout[-6000:], r.stderr)
    assert r.returncode == 0 and "DEMO OK" in r.stdout, r.stdout + r.stderr
    first = {}
    for bt, line, k, count, lag, dlag, dop, ddop, snr in LINE.findall(r.stdout):
        assert int(count) >= 1 and int(k) < min(int(count), 4)
        assert all(np.isfinite(float(v)) for v in (dlag, ddop, snr)) and abs(float(dlag)) <= 0.5 and abs(float(ddop)) <= 0.5
        if int(k) == 0:
            first[(int(bt), int(line))] = (int(lag), int(dop), float(snr))
    nb = max(3, blocks // batch)                                                 # (the bench times at least three batches)
    assert sorted(first) == [(bt, line) for bt in range(nb) for line in range(batch)], sorted(first)
    # guard 0: every line's strongest detection is the direct path, and it stands above the threshold it passed
    assert all(v[:2] == (0, 0) and v[2] > 12.0 for v in first.values()), first
