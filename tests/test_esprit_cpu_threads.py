"""csrc/esprit.hpp's device function on the CPU (tools/esprit_cpu.cc: 64 host threads as the wave's lanes, a pthread barrier as
__syncthreads), built as a stand-alone program with AddressSanitizer + UBSan and again with ThreadSanitizer: every index of the
kernel's arithmetic and every barrier checked without a GPU, and its results held against the numpy model within the device's bar.
The sanitizers report on stderr and through the exit status; both must stay clean."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import doa_esprit_model as em

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "esprit_cpu.cc")
BUILDS = {"asan": "-fsanitize=address,undefined", "tsan": "-fsanitize=thread"}


@pytest.fixture(scope="module", params=sorted(BUILDS))
def exe(request, tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed for the host build of the kernel's device function")
    out = tmp_path_factory.mktemp(request.param) / "esprit_cpu"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", BUILDS[request.param], "-fno-sanitize-recover=all", "-ffp-contract=off", "-o", str(out), SRC, "-lpthread"],
                   check=True)
    return str(out)


def run(exe, tmp_path, vec, sv, k, d, sx, sy, slots):
    M = sx * sy
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        f.write(np.array([M, k, sx, sy, slots], dtype=np.int32).tobytes())
        f.write(np.float32(d).tobytes())
        f.write(np.ascontiguousarray(vec, dtype=np.complex64).tobytes())
        f.write(np.ascontiguousarray(sv, dtype=np.float32).tobytes())
    r = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-3000:])
    raw, o = open(dst, "rb").read(), 8
    out = {"found": int(np.frombuffer(raw, np.int32, 1, 0)[0]), "status": int(np.frombuffer(raw, np.int32, 1, 4)[0])}
    for key, dt, n in (("phases", np.float64, 2), ("angles", np.float32, 2), ("modulus", np.float32, 2), ("power", np.float32, 1), ("flags", np.int32, 1)):
        a = np.frombuffer(raw, dt, n * slots, o)
        out[key] = a.reshape(slots, 2) if n == 2 else a
        o += a.nbytes
    assert o == len(raw)
    return out


@pytest.mark.parametrize("shape", em.SHAPES, ids=[f"{s[0]}x{s[1]}-k{s[2]}" for s in em.SHAPES])
def test_the_kernels_arithmetic_on_host_threads(exe, tmp_path, shape):
    sx, sy, k = shape
    slots = min(k + 1, em.MAX_K)                                  # an empty slot behind the directions where there is room
    block, _ = em.shape_scene(sx, sy, k)
    vec, sv = em.fp64_subspace(block)
    d = em.shape_d(sx, sy)
    got, model = run(exe, tmp_path, vec, sv, k, d, sx, sy, slots), em.esprit(vec, sv, k, d, sx, sy, slots=slots)
    assert got["found"] == k and got["status"] == 0
    worst = max(model["cond_gx"], model["cond_gy"], model["cond_v"])
    bar = em.BAR if em.well_conditioned(model) else min(em.BAR * max(1.0, worst / 4.0), 1e-9)
    err = em.phase_error(got["phases"], model["phases"])
    print(f"{sx}x{sy} k={k}: {err:.2e} rad (bar {bar:.1e})")
    assert err <= bar
    for key in ("angles", "modulus", "power"):
        assert np.all(np.abs(got[key].astype(np.float64) - model[key].astype(np.float64)) <= 4 * np.spacing(np.abs(model[key])).astype(np.float64)), key
    assert np.array_equal(got["flags"], model["flags"])


def test_the_empty_results_on_host_threads(exe, tmp_path):
    for vec, sv, k, status in ((np.zeros((6, 6)), np.zeros(6), 2, 0), (np.eye(6), np.ones(6), 3, 2), (np.eye(6), np.ones(6), 0, 0), (np.eye(6), np.ones(6), 4, 0)):
        got = run(exe, tmp_path, vec, sv, k, 0.5, 3, 2, 3)          # k = 0 and k above the slots: nothing found, nothing written out of place
        assert got["found"] == 0 and got["status"] == status, (k, got)
        assert not got["phases"].any() and np.all(got["angles"] == -1) and np.all(got["modulus"] == -1) and np.all(got["power"] == -1) and not got["flags"].any()
