"""The integration's host arithmetic, and the demo.

csrc/caf_integrate_solve.hpp -- the limits, the offsets of the range walk, lambda, the clamped source cell and the three-operation update,
the functions the kernel of csrc/caf_integrate.hpp calls -- as a stand-alone program (tools/caf_integrate_cpu.cc) under AddressSanitizer
+ UBSan and without contraction, on inputs the numpy model wrote: every index of the product's own functions checked without a GPU, the
offsets and lambda equal to tests/caf_integrate_model.py, imap and the final state equal to it BYTE FOR BYTE.  The sanitizers report on
stderr and through the exit status; both must stay clean.  Nothing is loaded into Python under a sanitizer."""
import importlib
import os
import shutil
import subprocess

import numpy as np
import pytest

import caf_integrate_model as IM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "caf_integrate_cpu.cc")
HOST = os.path.join(ROOT, "coherent-rtlsdr_amd", "host")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed for the host build of the integration's arithmetic")
    out = tmp_path_factory.mktemp("asan") / "caf_integrate_cpu"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off", "-o", str(out), SRC], check=True)
    return str(out)


def run(exe, tmp_path, items):
    """items: (maps [L][nmaps][nd][R], forget, coupling, cut[, m0]) -> [(imap, state, D [L][nd], lambda [L])]"""
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        f.write(np.int32(len(items)).tobytes())
        for maps, forget, coupling, cut, *rest in items:
            L, nmaps, nd, R = maps.shape
            f.write(np.array([L, nmaps, nd, R, len(cut)], dtype=np.int32).tobytes() + np.int64(rest[0] if rest else 0).tobytes())
            f.write(np.array([forget, coupling], dtype=np.float64).tobytes() + np.array(cut, dtype=np.int32).tobytes() + maps.astype(np.float32).tobytes())
    r = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-3000:])
    raw, out, at = open(dst, "rb").read(), [], 0
    for maps, *_ in items:
        L, nmaps, nd, R = maps.shape
        imap = np.frombuffer(raw, np.float32, maps.size, at).reshape(maps.shape)
        at += imap.nbytes
        state = np.frombuffer(raw, np.uint8, 16 + 8 * nmaps * nd * R, at)
        at += state.nbytes
        D = np.frombuffer(raw, np.int64, L * nd, at).reshape(L, nd)
        at += D.nbytes
        lam = np.frombuffer(raw, np.float64, L, at)
        at += lam.nbytes
        out.append((imap, state, D, lam))
    assert at == len(raw)
    return out


def _maps(seed, L, nmaps, nd, R):
    rng = np.random.default_rng(seed)
    m = rng.exponential(1.0, size=(L, nmaps, nd, R)).astype(np.float32)
    m[rng.random(m.shape) < 0.05] = 0.0
    m.reshape(-1)[:3] = [3e38, 1e-40, 1e30]
    return m


def test_offsets_and_lambda_against_the_model(exe, tmp_path):
    items = []
    for nd, c in ((8, 0.0), (8, 256.0), (16, 0.5), (16, -0.5), (64, 0.05), (64, 2.75), (4096, 0.5), (4096, -0.013)):
        for m0 in (0, 1, 7, 12345, 2 ** 31 + 5):
            items.append((_maps(nd, 3, 1, nd, 1), 0.125, c, [3], m0))
    for (maps, a, c, _, m0), (_, state, D, lam) in zip(items, run(exe, tmp_path, items)):
        nd = maps.shape[2]
        for l in range(3):
            assert np.array_equal(D[l], IM.steps(m0 + l, c, nd)), (nd, c, m0, l)
            assert lam[l].tobytes() == np.float64(IM.lam(m0 + l, a)).tobytes()
        assert state[:16].view("<i8").tolist() == [m0 + 3, 0]


def test_whole_sequences_byte_for_byte(exe, tmp_path):
    items = [(_maps(1, 12, 3, 64, 48), 0.125, 0.05, [12]), (_maps(2, 5, 2, 16, 65), 0.5, 2.75, [5]), (_maps(3, 4, 1, 8, 4), 1.0, 3.0, [4]),
             (_maps(4, 6, 1, 16, 1), 2.0 ** -20, -0.5, [6]), (_maps(5, 9, 2, 8, 7), 0.3, -2.75, [9])]
    for (maps, a, c, _), (imap, state, _, _) in zip(items, run(exe, tmp_path, items)):
        want, wstate = IM.run(maps, a, c)
        assert imap.tobytes() == want.tobytes() and state.tobytes() == wstate.tobytes(), (maps.shape, a, c)


def test_cuts_through_the_state_buffer_give_the_same_bytes(exe, tmp_path):
    maps = _maps(6, 12, 2, 16, 9)
    cuts = [[12], [1] * 12, [5, 7], [1, 11], [4, 4, 4]]
    out = run(exe, tmp_path, [(maps, 0.25, 0.5, cut) for cut in cuts])
    for imap, state, _, _ in out[1:]:
        assert imap.tobytes() == out[0][0].tobytes() and state.tobytes() == out[0][1].tobytes()


@pytest.fixture(scope="module")
def host_build():
    importlib.import_module("coherent-rtlsdr_amd.binding").build()
    subprocess.run(["make", "-C", HOST, "all", "libcsynth.so"], check=True, stdout=subprocess.DEVNULL)
    return HOST


def test_the_demo_parses_integrate_and_refuses_bad_ones(host_build):
    """numbers only: the demo checks --integrate before it looks for a device"""
    base = [os.path.join(host_build, "coherent_demo"), "--bench", "--nsig", "3", "--batch", "8", "--blocks", "16"]
    caf = ["--caf", "64:16"]
    r = subprocess.run(base + caf + ["--cfar", "12", "--integrate", "8:0.05"], capture_output=True, text=True, timeout=300)
    assert "integrate: window 8 forget 0.125 coupling 0.05 maps array\n" in r.stdout, r.stdout[-500:] + r.stderr[-500:]
    r = subprocess.run(base + caf + ["--cfar", "12", "--integrate", "4", "--caf-beams", "3x1:4x2"], capture_output=True, text=True, timeout=300)
    assert "integrate: window 4 forget 0.25 coupling 0 maps array+beams\n" in r.stdout, r.stdout[-500:] + r.stderr[-500:]
    r = subprocess.run(base + ["--integrate", "8"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--integrate needs --caf" in r.stdout and "DEMO FAILED" in r.stdout
    for bad in ("0", "0.5", "-3", "x", "nan", "inf", "8:inf", "8:nan"):
        r = subprocess.run(base + caf + ["--integrate", bad], capture_output=True, text=True, timeout=300)
        assert r.returncode != 0 and "--integrate W[:COUPLING] refused" in r.stdout and "DEMO FAILED" in r.stdout, (bad, r.stdout[-500:])
