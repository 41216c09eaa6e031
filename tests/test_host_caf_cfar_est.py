"""The CFAR estimators' decision arithmetic on the host, and the demo's flags for them.

csrc/caf_cfar.hpp's estimator functions -- the half an offset belongs to, the closed-form half counts, the half means and their choice,
os_rank, the selection by the letter -- as a stand-alone program (tools/caf_cfar_est_cpu.cc) under AddressSanitizer + UBSan, on maps
the numpy model wrote: every index checked without a GPU, the closed forms against a count cell by cell and the kernel's counting rule
against the sorted selection inside the program (exit status 3, 4), and the detections held against tests/caf_cfar_est_model.py
within the bars its docstring derives.  The sanitizers report on stderr and through the exit status; both must stay clean.  Nothing
is loaded into Python under a sanitizer."""
import importlib
import os
import shutil
import subprocess

import numpy as np
import pytest

import caf_cfar_est_model as E
import caf_cfar_model as C
import caf_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "caf_cfar_est_cpu.cc")
HOST = os.path.join(ROOT, "coherent-rtlsdr_amd", "host")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed for the host build of the estimators")
    out = tmp_path_factory.mktemp("asan") / "caf_cfar_est_cpu"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off", "-o", str(out), SRC], check=True)
    return str(out)


def run(exe, tmp_path, items):
    """items: (src [nd][R] float32 or complex64, guard, Params, Est, parts) -> (count, det [K][8] float32) each"""
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        f.write(np.int32(len(items)).tobytes())
        for a, guard, q, est, parts in items:
            nd, R = a.shape
            f.write(np.array([nd, R, guard, 2 if np.iscomplexobj(a) else 1, q.gd, q.gr, q.td, q.tr, q.min_train, q.max_det, parts, est.est, est.axis, est.rank],
                             dtype=np.int32).tobytes())
            f.write(np.float32(q.alpha).tobytes())
            f.write(np.ascontiguousarray(a).tobytes())
    r = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-3000:])
    raw = open(dst, "rb").read()
    out, at = [], 0
    for a, guard, q, est, parts in items:
        out.append((int(np.frombuffer(raw, np.int32, 1, at)[0]), np.frombuffer(raw, np.float32, q.max_det * 8, at + 4).reshape(q.max_det, 8)))
        at += 4 + 32 * q.max_det
    assert at == len(raw)
    return out


def _hold(got, items):
    """every case against the model: no ambiguous and no half-ambiguous cell, the same count, the same cells in the same order, every
    figure within its bar, and for OS power, snr and noise the model's own rounded once"""
    for (count, det), (a, guard, q, est, parts) in zip(got, items):
        want = E.detect(M.power(a) if np.iscomplexobj(a) else a.astype(np.float64), guard, q, est)
        assert want["ambiguous"] == 0 and want["half_ambiguous"] == 0, (a.shape, guard, est.est, want["ambiguous"], want["half_ambiguous"])
        assert np.all(np.isfinite(det)) and count == want["count"], (a.shape, guard, est.est, est.axis, est.rank, count, want["count"])
        assert np.array_equal(det[:, [0, 1, 7]].astype(np.float64), want["det"][:, [0, 1, 7]]), (a.shape, guard, est.est, det, want["det"])
        assert np.all(np.abs(det.astype(np.float64) - want["det"]) <= want["bar"]), (a.shape, guard, est.est, det, want["det"], want["bar"])
        if est.est == E.OS:
            assert np.array_equal(det[:, [2, 3, 4]], want["det"][:, [2, 3, 4]].astype(np.float32))
        assert not det[min(count, q.max_det):].any()


def _floor(nd, R, seed, complex_):
    rng = np.random.default_rng(seed)
    if complex_:
        return (np.sqrt(0.5) * (rng.standard_normal((nd, R)) + 1j * rng.standard_normal((nd, R)))).astype(np.complex64)
    return rng.exponential(1.0, size=(nd, R)).astype(np.float32)


def _ests(q):
    Nfull = E.full_count(q)
    return [E.Est(E.GO, E.LAG), E.Est(E.GO, E.DOPPLER), E.Est(E.SO, E.LAG), E.Est(E.SO, E.DOPPLER), E.Est(E.OS, 0, 1), E.Est(E.OS, 0, max(1, Nfull // 2)),
            E.Est(E.OS, 0, Nfull)]


def test_the_estimators_decisions_on_the_host(exe, tmp_path):
    """a target at every corner of the map, at both guard edges and on either side of the cyclic wrap, over a noise floor; rank 1, the
    middle and Nfull"""
    items = []
    for nd, R, q in ((8, 1, C.Params(5.0, 0, 0, 3, 0, max_det=4)), (8, 5, C.Params(5.0, 1, 1, 2, 15, max_det=4)), (32, 16, C.Params(6.0, 1, 1, 3, 4, max_det=8)),
                     (16, 70, C.Params(6.0, 1, 2, 0, 14, max_det=8)), (64, 3, C.Params(6.0, 1, 1, 7, 1, max_det=4))):
        for guard in (0, 2, nd // 2):
            edge = [g for g in (guard, nd - guard) if 0 <= g < nd] if guard else [0]
            spots = [(d, t) for d in sorted({0, nd - 1, nd // 2 - 1, *edge}) for t in sorted({0, R - 1, R // 2})]
            ests = _ests(q)
            for i, (d, t) in enumerate(spots):
                complex_ = bool(i % 2)
                a = _floor(nd, R, 1000 * nd + 10 * i + guard, complex_)
                a[d, t] = 30.0 + (20.0j if complex_ else 0.0)
                a[(d + 1) % nd, t] = 3.0
                if t + 1 < R:
                    a[d, t + 1] = 2.5
                items.append((a, guard, q, ests[i % len(ests)], 1 if i % 2 else 7))
                items.append((a, guard, q, ests[(i + 3) % len(ests)], 5))
    got = run(exe, tmp_path, items)
    _hold(got, items)
    assert sum(1 for count, det in got if count >= 1) > len(items) // 3


def test_plateaus_ties_zeros_and_absent_cells_on_the_host(exe, tmp_path):
    four = C.Params(3.0, 1, 1, 3, 4, max_det=8)
    # (over a drawn floor: on a constant one every pair of unequal halves has equal means, which the model calls half-ambiguous)
    flat = _floor(16, 24, 77, False)
    plateau = flat.copy()
    plateau[5, 6] = plateau[5, 7] = plateau[6, 6] = plateau[6, 7] = 9.0          # its first cell; the others tie inside each other's windows
    ties = np.tile(np.array([1.0, 2.0, 3.0], dtype=np.float32), (16, 8))         # three values, each many times in every window
    ties[4, 4], ties[12, 20], ties[0, 0], ties[15, 23] = 40.0, 40.0, 50.0, 50.0
    zedge = _floor(16, 24, 5, False)
    zedge[:, 0], zedge[:, 23], zedge[3, :] = 0.0, 0.0, 0.0                       # true zeros on the lag edges, beside absent cells, and on the ridge's rim
    zedge[2, 1], zedge[9, 22], zedge[4, 12] = 30.0, 30.0, 30.0
    half0 = flat.copy()
    half0[:, :10] = 0.0                                                          # an all-zero lower half beside cells of lag 10 and 11
    half0[6, 10], half0[9, 15] = 20.0, 20.0
    zero, czero = np.zeros((64, 3), dtype=np.float32), np.zeros((8, 1), dtype=np.complex64)
    items = []
    for a, guard in ((plateau, 0), (ties, 0), (zedge, 0), (zedge, 3), (half0, 0)):
        for est in _ests(four) + [E.Est(E.OS, 0, 67)]:
            if a is not ties or est.est == E.OS:                                 # (integers: the ordered statistic's ties)
                items.append((a, guard, four, est, 3))
    got = run(exe, tmp_path, items)
    _hold(got, items)
    by = {(id(a), guard, est.est, est.axis, est.rank): (count, det) for (count, det), (a, guard, q, est, parts) in zip(got, items)}
    count, det = by[(id(plateau), 0, E.OS, 0, 67)]
    assert count >= 1 and (det[0, 0], det[0, 1]) == (6, 5) and np.sum(det[:, 2] == 9.0) == 1          # the plateau's first cell, and it alone
    # smallest-of beside an all-zero half detects nothing there; greatest-of takes the other half
    count, det = by[(id(half0), 0, E.SO, E.LAG, 0)]
    assert (10.0, 6.0) not in {(float(x[0]), float(x[1])) for x in det[:count]}
    count, det = by[(id(half0), 0, E.GO, E.LAG, 0)]
    assert (10.0, 6.0) in {(float(x[0]), float(x[1])) for x in det[:count]}
    # rank 1 over zeros: the order statistic is 0, no noise estimate, no detection
    count, det = by[(id(half0), 0, E.OS, 0, 1)]
    assert (10.0, 6.0) not in {(float(x[0]), float(x[1])) for x in det[:count]}
    zeros = [(zero, 0, four, est, 2) for est in _ests(four)] + [(zero, 32, four, E.Est(E.OS, 0, 90), 1), (czero, 4, C.Params(4.0, 0, 0, 3, 0, max_det=64), E.Est(E.OS, 0, 6), 1),
                                                                (czero, 0, C.Params(4.0, 0, 0, 3, 0), E.Est(E.GO, E.DOPPLER), 3)]
    for count, det in run(exe, tmp_path, zeros):
        assert count == 0 and not det.any() and np.all(np.isfinite(det))


def test_cell_averaging_through_the_program_is_the_detectors(exe, tmp_path):
    a = _floor(32, 40, 9, False)
    a[7, 7], a[20, 39] = 60.0, 50.0
    q = C.Params(8.0, 1, 1, 3, 4, max_det=8)
    (count, det), = run(exe, tmp_path, [(a, 2, q, E.Est(E.CA), 4)])
    want = C.detect(a.astype(np.float64), 2, q)
    assert count == want["count"] and np.all(np.abs(det.astype(np.float64) - want["det"]) <= want["bar"]) and count >= 2


@pytest.fixture(scope="module")
def host_build():
    importlib.import_module("coherent-rtlsdr_amd.binding").build()
    subprocess.run(["make", "-C", HOST, "all", "libcsynth.so"], check=True, stdout=subprocess.DEVNULL)
    return HOST


def _demo(host_build, *args):
    return subprocess.run([os.path.join(host_build, "coherent_demo"), *args], capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("args,line", [(("--cfar-est", "go"), "estimator go axis lag rank 0"), (("--cfar-est", "so", "--cfar-axis", "doppler"), "estimator so axis doppler rank 0"),
                                       (("--cfar-est", "os:67"), "estimator os axis - rank 67"), (("--cfar-est", "os"), "estimator os axis - rank 67")])
def test_the_demo_parses_the_estimator(host_build, args, line):
    # the flags are read and judged before any device is asked for: the line stands whether or not the run goes on
    r = _demo(host_build, "--bench", "--caf", "64:16", "--cfar", "12", *args)
    assert "cfar: " + line in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize("args", [("--cfar-est", "go"), ("--cfar-axis", "lag"), ("--cfar", "12", "--cfar-est", "ca"), ("--cfar", "12", "--cfar-est", "os:0"),
                                  ("--cfar", "12", "--cfar-est", "os:x"), ("--cfar", "12", "--cfar-est", "go", "--cfar-axis", "range"),
                                  ("--cfar", "12", "--cfar-est", "os:5", "--cfar-axis", "lag"), ("--cfar", "12", "--cfar-axis", "lag")])
def test_the_demo_refuses_bad_estimator_flags(host_build, args):
    r = _demo(host_build, "--bench", "--caf", "64:16", *args)
    assert r.returncode == 1 and "DEMO FAILED" in r.stdout and "cfar: --cfar-est" in r.stdout, r.stdout + r.stderr
    assert "estimator " not in r.stdout
