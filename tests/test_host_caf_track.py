"""The tracker's decisions on the host, and the demo.

csrc/caf_track.hpp -- the limits, what a measurement is, the wrap, predict, the gate, update and coast, the status rules, the strict order,
initiation and the record, the functions the kernel of csrc/caf_track_kernels.hpp calls -- as a stand-alone program
(tools/caf_track_cpu.cc) under AddressSanitizer + UBSan, on inputs the numpy model wrote: every index of the product's own functions
checked without a GPU, ids, statuses, slots and counts equal to tests/caf_track_model.py, the figures within the bar its docstring fixes
plus the record's one fp32 rounding.  The sanitizers report on stderr and through the exit status; both must stay clean.  Nothing is
loaded into Python under a sanitizer."""
import importlib
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import caf_track_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "caf_track_cpu.cc")
HOST = os.path.join(ROOT, "coherent-rtlsdr_amd", "host")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed for the host build of the tracker's decisions")
    out = tmp_path_factory.mktemp("asan") / "caf_track_cpu"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off", "-o", str(out), SRC], check=True)
    return str(out)


def run(exe, tmp_path, items):
    """items: (q, det, count, aux, cut[, counter]) with cut the lines of each submit -> [(trk, ntrk, state)]"""
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        f.write(np.int32(len(items)).tobytes())
        for q, det, count, aux, cut, *rest in items:
            L, K, _ = det.shape
            fl = q.fields()
            f.write(np.array([L, K, M.ND, M.R, aux is not None, len(cut), rest[0] if rest else 0], dtype=np.int32).tobytes())
            f.write(np.array(fl[:2], dtype=np.int32).tobytes() + np.array(fl[2:10], dtype=np.float64).tobytes() + np.array(fl[10:], dtype=np.int32).tobytes())
            f.write(np.array(cut, dtype=np.int32).tobytes() + det.tobytes() + count.tobytes() + (b"" if aux is None else aux.tobytes()))
    r = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-3000:])
    raw, out, at = open(dst, "rb").read(), [], 0
    for q, det, count, aux, cut, *rest in items:
        L, T = len(det), q.T
        trk = np.frombuffer(raw, np.float32, L * T * 16, at).reshape(L, T, 16)
        ntrk = np.frombuffer(raw, np.int32, L * 4, at + trk.nbytes).reshape(L, 4)
        at += trk.nbytes + ntrk.nbytes
        out.append((trk, ntrk, np.frombuffer(raw, np.uint8, 16 + 128 * T, at)))
        at += 16 + 128 * T
    assert at == len(raw)
    return out


def held(got, ngot, name):
    want, wn, _ = M.expected(name)
    return M.hold(got, ngot, want, wn, name)


def test_every_scene_on_the_host_against_the_model(exe, tmp_path):
    items = [M.scene(name) + ([len(M.scene(name)[1])],) for name in M.SCENE_NAMES]
    for name, (trk, ntrk, state) in zip(M.SCENE_NAMES, run(exe, tmp_path, items)):
        held(trk, ntrk, name)
        q, det, count, aux = M.scene(name)
        tr = M.run(q, det, count, aux)[3]
        mine = tr.state()
        assert int(state[:4].view("<i4")[0]) == tr.counter
        a, b = state[16:].view(M.SLOT), mine[16:].view(M.SLOT)
        assert all(np.array_equal(a[k], b[k]) for k in ("id", "status", "age", "hits", "misses", "hist")), name


def test_the_id_counter_wraps_to_1(exe, tmp_path):
    q, det, count, aux = M.scene(M.WRAP_SCENE)
    (trk, ntrk, state), = run(exe, tmp_path, [(q, det, count, aux, [len(det)], M.WRAP_COUNTER)])
    want, wn, _, tr = M.run(q, det, count, aux, counter=M.WRAP_COUNTER)
    M.hold(trk, ntrk, want, wn, "the counter's wrap")
    assert sorted(set(trk[trk[..., 1] > 0][:, 0].astype(int))) == [1, (1 << 24) - 2, (1 << 24) - 1] and int(state[:4].view("<i4")[0]) == tr.counter == 1


def test_cuts_through_the_state_buffer_give_the_same_bytes(exe, tmp_path):
    q, det, count, aux = M.scene("cuts")
    cuts = [[12], [1] * 12, [3, 5, 4], [11, 1], [1, 11], [6, 6]]
    out = run(exe, tmp_path, [(q, det, count, aux, cut) for cut in cuts])
    for trk, ntrk, state in out[1:]:
        assert trk.tobytes() == out[0][0].tobytes() and ntrk.tobytes() == out[0][1].tobytes() and state.tobytes() == out[0][2].tobytes()


@pytest.fixture(scope="module")
def host_build():
    importlib.import_module("coherent-rtlsdr_amd.binding").build()
    subprocess.run(["make", "-C", HOST, "all", "libcsynth.so"], check=True, stdout=subprocess.DEVNULL)
    return HOST


def test_the_demo_parses_track_and_refuses_it_without_cfar(host_build):
    """numbers only: the demo checks --track against the library's limits before it looks for a device"""
    base = [os.path.join(host_build, "coherent_demo"), "--bench", "--caf", "64:16", "--nsig", "3", "--batch", "8", "--blocks", "16"]
    r = subprocess.run(base + ["--cfar", "12", "--track", "2:4:7.5", "--track-max", "8", "--track-sigma", "0.25:0.75", "--track-q", "0.5:0.25:0.125", "--coupling", "-0.5"],
                       capture_output=True, text=True, timeout=300)
    assert "track: 2 of 4 gate 7.5 slots 8 sigma 0.25:0.75 q 0.5:0.25:0.125 coupling -0.5 source array" in r.stdout, r.stdout[-500:] + r.stderr[-500:]
    r = subprocess.run(base + ["--cfar", "12", "--track", "3:5", "--caf-beams", "3x1:4x2"], capture_output=True, text=True, timeout=300)
    assert "track: 3 of 5 gate 9 slots 16 sigma 0.5:0.5 q 0.001:0.001:0.0001 coupling 0 source fused" in r.stdout, r.stdout[-500:] + r.stderr[-500:]
    r = subprocess.run(base + ["--track", "3:5"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--track needs --caf and --cfar" in r.stdout and "DEMO FAILED" in r.stdout
    for bad in (["--track", "6:5"], ["--track", "3"], ["--track", "3:33"], ["--track", "3:5:0"], ["--track", "3:5", "--track-max", "129"], ["--track", "3:5", "--track-sigma", "1"],
                ["--track", "3:5", "--track-sigma", "0:1"], ["--track", "3:5", "--track-q", "1:1"], ["--track", "3:5", "--coupling", "inf"]):
        r = subprocess.run(base + ["--cfar", "12"] + bad, capture_output=True, text=True, timeout=300)
        assert r.returncode != 0 and "--track M:N[:GATE]" in r.stdout and "refused" in r.stdout, (bad, r.stdout[-500:])


TRACK = re.compile(r"track: batch (\d+) line (\d+) id (\d+): lag (\S+) doppler (\S+) rate (\S+) age (\d+) hits (\d+) live (\d+)(.*)")


@pytest.mark.gpu
def test_host_demo_prints_the_tracks(host_build):
    """coherent_demo --bench --caf ... --cfar ... --track M:N (ccaf::batch over crsdr_caf_set_track): the confirmed tracks of every
    line; with --caf-beams their beam, with --bearing their angles"""
    base = [os.path.join(host_build, "coherent_demo"), "--bench", "--caf", "64:16", "--cfar", "12", "--max-det", "4", "--track", "3:5", "--nsig", "3", "--batch", "8",
            "--blocks", "16"]
    on = subprocess.run(base, capture_output=True, text=True, timeout=300)
    print("\n".join([l for l in on.stdout.splitlines() if l.startswith("track:")][:12]), on.stdout[-300:], on.stderr)
    assert on.returncode == 0 and "DEMO OK" in on.stdout, on.stdout + on.stderr
    rows = TRACK.findall(on.stdout)
    assert rows and all(int(r[2]) >= 1 and 0.0 <= float(r[3]) <= 16.0 and -8.0 <= float(r[4]) <= 8.0 and int(r[6]) >= 2 for r in rows), rows[:5]
    fused = subprocess.run(base + ["--caf-beams", "3x1:4x2"], capture_output=True, text=True, timeout=300)
    rows = TRACK.findall(fused.stdout)
    assert fused.returncode == 0 and rows and all(re.fullmatch(r" beam [0-7]", r[9]) for r in rows), fused.stdout[-2000:]
    angles = subprocess.run(base + ["--bearing", "3x1:32"], capture_output=True, text=True, timeout=300)
    rows = TRACK.findall(angles.stdout)
    assert angles.returncode == 0 and rows and all(" alpha " in r[9] and " beta " in r[9] for r in rows), angles.stdout[-2000:]
