"""csrc/refcancel_solve.hpp -- the Gram indexing, the fp64 Cholesky factor, the solve and the residual that the canceller's kernels call
-- as a stand-alone CPU program (tools/refcancel_cpu.cc) under AddressSanitizer + UBSan, on cases written here: every index of the
product's own functions checked without a GPU, and the coefficients held against numpy's solve.  The sanitizers report on stderr and
through the exit status; both must stay clean."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import refcancel_cases as cases
import refcancel_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "refcancel_cpu.cc")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed for the host build of the canceller's solve")
    out = tmp_path_factory.mktemp("asan") / "refcancel_cpu"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off", "-o", str(out), SRC], check=True)
    return str(out)


def pack_gram(G9):
    """the 9 x 9 Gram -> the 90 integers of the kernels' layout: (re, im) of the entries on and above the diagonal, row-major"""
    out = []
    for i in range(9):
        for j in range(i, 9):
            out += [int(G9[i, j].real), int(G9[i, j].imag)]
    return np.array(out, dtype=np.int32)


def sums_of(block, row, d, taps):
    """(gram [90], c [taps], E, G [taps][taps]) of one row"""
    K = (taps - 1) // 2
    y, R9 = M.row_parts(block, row, d, 4)
    c9, G9, E = M.sums(y, R9)
    return pack_gram(G9), c9[4 - K:5 + K], E, G9[4 - K:5 + K, 4 - K:5 + K]


def run(exe, tmp_path, items):
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        f.write(np.int32(len(items)).tobytes())
        for taps, gram, c, E in items:
            f.write(np.int32(taps).tobytes() + gram.tobytes() + np.ascontiguousarray(c, dtype=np.complex128).tobytes() + np.float64(E).tobytes())
    r = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-3000:])
    raw, o, out = open(dst, "rb").read(), 0, []
    for taps, _, _, _ in items:
        status = int(np.frombuffer(raw, np.int32, 1, o)[0])
        g = np.frombuffer(raw, np.complex128, taps, o + 4)
        res = float(np.frombuffer(raw, np.float64, 1, o + 4 + 16 * taps)[0])
        out.append((status, g, res))
        o += 4 + 16 * taps + 8
    assert o == len(raw)
    return out


def test_the_kernels_solve_on_the_host(exe, tmp_path):
    block, lag, ph = cases.perop_case(256)
    items, want = [], []
    for taps in (1, 3, 9):
        for row in (3, 5, 6, 8, 9):
            gram, c, E, G = sums_of(block, row, int(lag[row]), taps)
            items.append((taps, gram, c, E))
            want.append((G, c, E))
    for (status, g, res), (G, c, E) in zip(run(exe, tmp_path, items), want):
        ref = np.linalg.solve(G, c)
        cond = np.linalg.cond(G)
        assert status == 0
        assert np.abs(g - ref).max() <= 1e-10 * cond * max(np.abs(ref).max(), 1e-300), (G.shape, np.abs(g - ref).max(), cond)
        assert abs(res - M.residual_share(E, ref, c)) <= 1e-12 * max(cond, 1.0)
        mg, mres, mst = M.solve(G, c, E)
        assert mst == 0 and np.abs(g - mg).max() <= 1e-10 * cond * np.abs(ref).max() and abs(res - mres) <= 1e-12 * max(cond, 1.0)


def test_deficient_reference_rows_on_the_host(exe, tmp_path):
    items, expect = [], []
    for kind, taps in (("zero", 1), ("zero", 9), ("single", 3), ("single", 9), ("constant", 3), ("constant", 9)):
        block, lag, ph = cases.failure_case(kind)
        gram, c, E, G = sums_of(block, 5, int(lag[5]), taps)
        items.append((taps, gram, c, E))
        expect.append((kind, G, c, E))
    # a Gram written by hand: every entry the same, rank one (a constant row without its edge terms)
    items.append((3, pack_gram(np.full((9, 9), 1000.0 + 0j)), np.full(3, 500.0 + 20j), 4000.0))
    expect.append(("rank one", None, None, None))
    # and an empty row under a sound reference row: g = 0, residual 1, no failure
    block, lag, ph = cases.perop_case(256)
    gram, c, E, G = sums_of(block, 1, int(lag[1]), 9)
    assert E == 0 and not c.any()
    items.append((9, gram, c, E))
    expect.append(("empty row", G, c, E))
    for (status, g, res), (kind, G, c, E) in zip(run(exe, tmp_path, items), expect):
        if kind in ("zero", "single", "rank one"):
            assert status == M.STATUS_SINGULAR and not g.any() and res == 1.0, (kind, status, g, res)
        elif kind == "empty row":
            assert status == 0 and not g.any() and res == 1.0
        else:                                                   # constant: full rank through its edge terms, badly conditioned
            ref, cond = np.linalg.solve(G, c), np.linalg.cond(G)
            assert status == 0 and np.abs(g - ref).max() <= 1e-10 * cond * np.abs(ref).max(), (kind, cond)
