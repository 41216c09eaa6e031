"""The canceller's solve on the host.

csrc/caf_cancel_solve.hpp -- where an entry of the normal matrix sits, the Cholesky factor with its pivot rule, the solve of a row's
equations and the residual share, the functions the kernels of csrc/caf_cancel.hpp call -- as a stand-alone program
(tools/caf_cancel_cpu.cc) under AddressSanitizer + UBSan, on the sums the numpy model wrote: every index of the product's own functions
checked without a GPU, and h and the share held against tests/caf_cancel_model.py within the bars its docstring derives.  The
sanitizers report on stderr and through the exit status; both must stay clean.  Nothing is loaded into Python under a sanitizer."""
import importlib
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import caf_cancel_model as X
import caf_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "caf_cancel_cpu.cc")
HOST = os.path.join(ROOT, "coherent-rtlsdr_amd", "host")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed for the host build of the canceller's solve")
    out = tmp_path_factory.mktemp("asan") / "caf_cancel_cpu"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off", "-o", str(out), SRC], check=True)
    return str(out)


def run(exe, tmp_path, items):
    """items: (K, P, S [4 P + 1][K][K] complex128, E [nrows], c [nrows][n] complex128) -> (status, h [nrows][n], share [nrows]) each"""
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        f.write(np.int32(len(items)).tobytes())
        for K, P, S, E, c in items:
            f.write(np.array([K, P, len(E)], dtype=np.int32).tobytes())
            f.write(np.ascontiguousarray(S, dtype=np.complex128).tobytes())
            for e, row in zip(E, c):
                f.write(np.float64(e).tobytes())
                f.write(np.ascontiguousarray(row, dtype=np.complex128).tobytes())
    r = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-3000:])
    raw = open(dst, "rb").read()
    out, at = [], 0
    for K, P, S, E, c in items:
        n, nrows = X.basis(K, P), len(E)
        status = int(np.frombuffer(raw, np.int32, 1, at)[0])
        at += 4
        rows = np.frombuffer(raw, np.float64, nrows * (2 * n + 1), at).reshape(nrows, 2 * n + 1)
        at += 8 * rows.size
        out.append((status, rows[:, 0:2 * n:2] + 1j * rows[:, 1:2 * n:2], rows[:, 2 * n]))
    assert at == len(raw)
    return out


def _case(shape, seed):
    nrows, B, frames, seg, R, ref, K, P = shape
    line = M.echo_scene(B, frames, [], nrows=nrows, ref=ref, seed=seed)
    r = X.cancel(line, seg, R, ref, M.WINDOW_HANN, K, P)
    assert r["cond"] <= 16.0
    return r, (K, P, X.s_sums(r["G"], P), r["E"], r["c"])


# (nrows, B, frames, seg, R, ref, K, P): the smallest basis, both Doppler extents, the largest bases (n = 32 and n = 48)
SHAPES = [(3, 256, 1, 16, 16, 0, 1, 0), (3, 256, 1, 16, 16, 1, 2, 2), (3, 512, 2, 16, 20, 2, 17, 0), (2, 4096, 1, 64, 32, 0, 32, 0), (3, 4096, 2, 64, 32, 1, 16, 1)]


def test_the_solve_on_the_host_against_the_model(exe, tmp_path):
    cases = [_case(s, 40 + i) for i, s in enumerate(SHAPES)]
    got = run(exe, tmp_path, [c[1] for c in cases])
    for (r, item), (status, h, share), shape in zip(cases, got, SHAPES):
        ref = shape[5]
        others = [c for c in range(shape[0]) if c != ref]                        # (the program solves row r's equations as well: the kernel skips them)
        assert status == 0 and np.all(np.isfinite(h)), shape
        err = np.maximum(np.abs(h.real - r["h"].real), np.abs(h.imag - r["h"].imag))
        assert np.all(err[others] <= r["hbar"][others]), (shape, np.max(err[others] / r["hbar"][others]))
        assert np.all(np.abs(share - r["share"])[others] <= r["sbar"][others]), shape
        # row r against itself: the first basis member of p = 0, exactly to the bar of a solve of that size
        want = np.zeros(h.shape[1])
        want[shape[7] * shape[6]] = 1.0
        assert np.all(np.abs(h[ref] - want) <= np.max(r["hbar"][others])) and share[ref] <= 1e-9, shape


def test_singular_lines_zero_rows_and_clamps_on_the_host(exe, tmp_path):
    r, (K, P, S, E, c) = _case(SHAPES[1], 50)
    zero = np.zeros_like(S)
    dup = S.copy()                                                               # a reference that repeats: delays 0 and 1 alike, rank deficient
    dup[:] = S[:, :1, :1]
    E2 = np.array([0.0, E[0], 1e-300])                                           # the good matrix, with rows at the edges of the share
    c2 = np.stack([np.zeros_like(c[0]), c[0], c[0]])
    got = run(exe, tmp_path, [(K, P, zero, E, c), (K, P, dup, E, c), (K, P, S, E2, c2)])
    for status, h, share in got[:2]:
        assert status == X.STATUS_SINGULAR and not h.any() and np.all(share == 1.0)
    status, h, share = got[2]
    assert status == 0 and not h[0].any() and share[0] == 1.0                    # E = 0: all of it stays, and no NaN
    assert 0.0 <= share[1] <= 1.0 and share[2] == 0.0 and np.all(np.isfinite(h))  # more taken out than there is: clamped


@pytest.fixture(scope="module")
def host_build():
    importlib.import_module("coherent-rtlsdr_amd.binding").build()
    subprocess.run(["make", "-C", HOST, "all", "libcsynth.so"], check=True, stdout=subprocess.DEVNULL)
    return HOST


LINE = re.compile(r"cancel: batch (\d+) line (\d+): taps (\d+) dopp (\d+) residual (\S+) dB")
PEAK = re.compile(r"caf: batch (\d+) line (\d+) row (\d+): lag (\d+)\S+ doppler (-?\d+)\S+ power (\S+) dB")


@pytest.mark.gpu
def test_host_demo_prints_the_residual_of_every_line(host_build):
    """coherent_demo --bench --caf ... --cancel K:P (ccaf::batch over crsdr_caf_set_cancel): a line per batch and line.  The synthetic
    channels are the reference noise with noise of their own, so the canceller takes power out of every one: the residual is below 0 dB,
    and every cancelled row's peak is lower than without it."""
    nsig, batch, blocks, seg, lags = 3, 8, 16, 64, 16
    base = [os.path.join(host_build, "coherent_demo"), "--bench", "--caf", f"{seg}:{lags}", "--nsig", str(nsig), "--batch", str(batch), "--blocks", str(blocks)]
    off = subprocess.run(base, capture_output=True, text=True, timeout=300)
    on = subprocess.run(base + ["--cancel", "4:1"], capture_output=True, text=True, timeout=300)
    print(on.stdout[-3000:], on.stderr)
    assert off.returncode == 0 and on.returncode == 0 and "DEMO OK" in on.stdout, on.stdout + on.stderr
    seen = {(int(bt), int(e)): float(db) for bt, e, taps, dopp, db in LINE.findall(on.stdout) if (taps, dopp) == ("4", "1")}
    nb = max(3, blocks // batch)                                                 # (the bench times at least three batches)
    assert sorted(seen) == [(bt, e) for bt in range(nb) for e in range(batch)], sorted(seen)
    assert all(v < 0.0 for v in seen.values()), seen
    power = lambda out: {(int(bt), int(e), int(c)): float(p) for bt, e, c, lag, dop, p in PEAK.findall(out)}
    p_off, p_on = power(off.stdout), power(on.stdout)
    assert p_off.keys() == p_on.keys() and len(p_on) == nb * batch * (nsig + 1)
    assert all(p_on[k] == p_off[k] if k[2] == 0 else p_on[k] < p_off[k] for k in p_on), (p_on, p_off)
    bad = subprocess.run(base + ["--cancel", "17"], capture_output=True, text=True, timeout=300)      # more taps than lags
    assert bad.returncode != 0 and "--cancel K[:P] refused" in bad.stdout
