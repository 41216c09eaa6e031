"""The bearings' arithmetic on the host, and the demo.

csrc/caf_bearing_solve.hpp -- which row is which element, the training walk, the covariance and its loading, the Cholesky factor and
its inverse, the co-array coefficients, the statistic, the first maximum and the zoom step, the functions the kernels of
csrc/caf_bearing.hpp call -- as a stand-alone program (tools/caf_bearing_cpu.cc) under AddressSanitizer + UBSan, on inputs the numpy
model wrote: every index of the product's own functions checked without a GPU, and T, the position and the figures held against
tests/caf_bearing_model.py within the bars its docstring derives.  The sanitizers report on stderr and through the exit status; both
must stay clean.  Nothing is loaded into Python under a sanitizer."""
import importlib
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import caf_bearing_model as BM
import caf_cfar_model as CF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "caf_bearing_cpu.cc")
HOST = os.path.join(ROOT, "coherent-rtlsdr_amd", "host")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed for the host build of the bearings' arithmetic")
    out = tmp_path_factory.mktemp("asan") / "caf_bearing_cpu"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off", "-o", str(out), SRC], check=True)
    return str(out)


def run(exe, tmp_path, items):
    """items: (chi [nrows][nd][R] complex64, ref, guard, CF.Params, BM.Desc, d, tau) -> (N, status, T [ncx][ncy], dir [8]) each"""
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        f.write(np.int32(len(items)).tobytes())
        for chi, ref, guard, prm, q, d, tau in items:
            nrows, nd, R = chi.shape
            f.write(np.array([nrows, nd, R, ref, guard, prm.gd, prm.gr, prm.td, prm.tr, q.mx, q.my, q.ncx, q.ncy, q.mode, q.levels, d, tau], dtype=np.int32).tobytes())
            f.write(np.array([q.d, q.loading], dtype=np.float32).tobytes())
            f.write(np.ascontiguousarray(chi, dtype=np.complex64).tobytes())
    r = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-3000:])
    raw = open(dst, "rb").read()
    out, at = [], 0
    for chi, ref, guard, prm, q, d, tau in items:
        n, status = (int(v) for v in np.frombuffer(raw, np.int32, 2, at))
        at += 8
        T = np.frombuffer(raw, np.float64, q.ncx * q.ncy, at).reshape(q.ncx, q.ncy)
        at += 8 * T.size
        fig = np.frombuffer(raw, np.float32, 8, at)
        at += 32
        out.append((n, status, T, fig))
    assert at == len(raw)
    return out


# (mx, my, nc, ref, nd, R, guard, cfar, mode, loading, levels, (d, tau)): m = 2, 6, 21, 64 in both modes; N < m; N = 0; a cell at lag 0
# and at lag R - 1; across the Doppler wrap
CASES = [
    (1, 2, (5, 7), 0, 8, 4, 0, dict(gd=0, gr=0, td=1, tr=1), BM.CONVENTIONAL, 1e-2, 3, (1, 2)),
    (1, 2, (5, 7), 2, 8, 4, 0, dict(gd=0, gr=0, td=1, tr=1), BM.ADAPTIVE, 1.0, 3, (0, 0)),
    (3, 2, (16, 16), 3, 16, 8, 1, dict(gd=1, gr=1, td=2, tr=3), BM.ADAPTIVE, 1e-2, 5, (15, 7)),
    (7, 3, (20, 24), 0, 16, 12, 2, dict(gd=1, gr=1, td=3, tr=4), BM.ADAPTIVE, 1e-2, 2, (2, 5)),
    (7, 3, (20, 24), 21, 16, 12, 2, dict(gd=1, gr=1, td=3, tr=4), BM.CONVENTIONAL, 1e-2, 8, (14, 11)),
    (8, 8, (12, 10), 0, 8, 6, 1, dict(gd=1, gr=1, td=2, tr=3), BM.ADAPTIVE, 1e-2, 1, (6, 3)),
    (8, 8, (12, 10), 5, 8, 6, 1, dict(gd=0, gr=0, td=0, tr=1), BM.ADAPTIVE, 1e-2, 0, (3, 3)),          # N = 2 < m = 64
    (3, 2, (16, 16), 0, 8, 6, 4, dict(gd=0, gr=0, td=1, tr=0), BM.ADAPTIVE, 1e-2, 2, (4, 3)),          # N = 0: W = I, status bit 1
]


def _item(c, seed):
    mx, my, nc, ref, nd, R, guard, cf, mode, loading, levels, (d, tau) = c
    q = BM.Desc(mx, my, 0.5, nc[0], nc[1], mode, loading, levels)
    floor = BM.steer(q, [nc[0] / 2], [nc[1] / 2])[0]
    chi = BM.noise_chi(1 + q.m, nd, R, seed, np.insert(floor, ref, 1.0))
    return chi, ref, guard, CF.Params(1.0, **cf), q, d, tau


def test_the_arithmetic_on_the_host_against_the_model(exe, tmp_path):
    items = [_item(c, 70 + i) for i, c in enumerate(CASES)]
    got = run(exe, tmp_path, items)
    seen = set()
    for (chi, ref, guard, prm, q, d, tau), (n, status, T, fig) in zip(items, got):
        want = BM.one(chi, ref, guard, prm, q, d, tau)
        assert want["ambiguous"] == 0, (q.mx, q.my)                              # a case the model cannot call is replaced, never skipped
        assert n == want["N"] and status == int(want["dir"][7]), (q.mx, q.my, n, status)
        if q.mode == BM.ADAPTIVE:
            assert n == CF.train_cell(np.zeros(chi.shape[1:]), guard, prm, d, tau)[1]
        assert np.all(np.isfinite(T)) and T.min() >= 0.0 and T.max() <= 1.0 + want["tbar"]
        assert np.max(np.abs(T - want["spec"])) <= want["tbar"], (q.mx, q.my, np.max(np.abs(T - want["spec"])) / want["tbar"])
        assert np.all(np.abs(fig - want["dir"]) <= want["bar"]), (q.mx, q.my, fig, want["dir"])
        seen.add((q.m, n < q.m if q.mode == BM.ADAPTIVE else None, status))
    assert {2, 6, 21, 64} == {m for m, _, _ in seen} and (64, True, 0) in seen and (6, True, BM.STATUS_IDENTITY) in seen


def test_zero_snapshots_and_zero_training_on_the_host(exe, tmp_path):
    chi, ref, guard, prm, q, d, tau = _item(CASES[2], 90)
    dead = chi.copy()
    dead[:, d, tau] = 0                                                          # an all-zero snapshot: zeros and status bit 0, never a NaN
    quiet = np.zeros_like(chi)
    quiet[:, d, tau] = chi[:, d, tau]                                            # nothing around the cell: trace(Q) = 0, W = I, status bit 1
    got = run(exe, tmp_path, [(dead, ref, guard, prm, q, d, tau), (quiet, ref, guard, prm, q, d, tau)])
    n, status, T, fig = got[0]
    assert status == BM.STATUS_ZERO and not T.any() and not fig[:7].any() and fig[7] == BM.STATUS_ZERO
    n, status, T, fig = got[1]
    want = BM.one(quiet, ref, guard, prm, q, d, tau)
    assert status == BM.STATUS_IDENTITY == int(want["dir"][7]) and n == want["N"] > 0
    conv = BM.Desc(q.mx, q.my, q.d, q.ncx, q.ncy, BM.CONVENTIONAL, levels=q.levels)
    assert np.max(np.abs(T - BM.one(quiet, ref, guard, prm, conv, d, tau)["spec"])) <= want["tbar"]
    assert np.all(np.abs(fig - want["dir"]) <= want["bar"]) and np.all(np.isfinite(T))


@pytest.fixture(scope="module")
def host_build():
    importlib.import_module("coherent-rtlsdr_amd.binding").build()
    subprocess.run(["make", "-C", HOST, "all", "libcsynth.so"], check=True, stdout=subprocess.DEVNULL)
    return HOST


DET = re.compile(r"cfar: batch (\d+) line (\d+) det (\d+) of \d+:")
BRG = re.compile(r"bearing: batch (\d+) line (\d+) det (\d+): cell \((\d+), (\d+)\) alpha (\S+) deg beta (\S+) deg fit (\S+)")


@pytest.mark.gpu
def test_host_demo_prints_a_bearing_per_detection(host_build):
    """coherent_demo --bench --caf ... --cfar ... --bearing MXxMY (ccaf::batch over crsdr_caf_set_bearing): one bearing line per
    detection line, fits in [0, 1]; shapes that do not match --nsig, and --bearing without --cfar, are refused."""
    base = [os.path.join(host_build, "coherent_demo"), "--bench", "--caf", "64:16", "--nsig", "3", "--batch", "8", "--blocks", "16"]
    on = subprocess.run(base + ["--cfar", "12", "--max-det", "4", "--bearing", "3x1"], capture_output=True, text=True, timeout=300)
    print(on.stdout[-3000:], on.stderr)
    assert on.returncode == 0 and "DEMO OK" in on.stdout, on.stdout + on.stderr
    dets = [tuple(int(v) for v in t) for t in DET.findall(on.stdout)]
    brgs = {(int(bt), int(e), int(k)): (int(cx), int(cy), float(al), float(be), float(fit)) for bt, e, k, cx, cy, al, be, fit in BRG.findall(on.stdout)}
    assert sorted(dets) == sorted(brgs), (dets, sorted(brgs))
    assert all(0.0 <= v[4] <= 1.0 and 0.0 <= v[2] <= 180.0 and 0.0 <= v[3] <= 180.0 for v in brgs.values()), brgs
    ad = subprocess.run(base + ["--cfar", "12", "--max-det", "4", "--bearing", "3x1:32", "--adaptive", "0.01", "--bearing-levels", "3"], capture_output=True, text=True,
                        timeout=300)
    assert ad.returncode == 0 and "DEMO OK" in ad.stdout and len(BRG.findall(ad.stdout)) == len(DET.findall(ad.stdout)), ad.stdout + ad.stderr
    for bad, why in ((["--bearing", "3x1"], "needs --cfar"), (["--cfar", "12", "--bearing", "2x2"], "--bearing MXxMY[:NC] [--adaptive LOADING] [--bearing-levels L] refused"),
                     (["--cfar", "12", "--bearing", "3x1:1000"], "--bearing MXxMY[:NC] [--adaptive LOADING] [--bearing-levels L] refused")):
        r = subprocess.run(base + bad, capture_output=True, text=True, timeout=300)
        assert r.returncode != 0 and why in r.stdout + r.stderr, (bad, r.stdout[-500:], r.stderr[-500:])
