"""The alignment figures' arithmetic and the C++ host layer of the spectra engine.

CPU: csrc/spectra_align.hpp -- the sums, the delay, the phase, the gain and the coherence that the kernel of csrc/spectra.hpp calls -- as a
stand-alone program (tools/spectra_align_cpu.cc) under AddressSanitizer + UBSan, on vectors the numpy model wrote: every index of the
product's own functions checked without a GPU, and the figures held against tests/spectra_model.py within the fp64 bar its docstring
derives.  The sanitizers report on stderr and through the exit status; both must stay clean.

GPU: coherent_demo --bench --spectra (cspectra::batch over crsdr_spectra) prints a line per batch, packet and row."""
import importlib
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import peak_cases
import spectra_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "spectra_align_cpu.cc")
HOST = os.path.join(ROOT, "coherent-rtlsdr_amd", "host")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed for the host build of the alignment figures")
    out = tmp_path_factory.mktemp("asan") / "spectra_align_cpu"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off", "-o", str(out), SRC], check=True)
    return str(out)


def run(exe, tmp_path, items):
    """items: (psd [nrows][N] float32, cross [nrows][N] complex64, lo, hi, step) -> align [nrows][4] float32 each"""
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        f.write(np.int32(len(items)).tobytes())
        for psd, cross, lo, hi, step in items:
            nrows, N = psd.shape
            f.write(np.array([nrows, N, lo, hi, step], dtype=np.int32).tobytes())
            f.write(np.ascontiguousarray(psd, dtype=np.float32).tobytes() + np.ascontiguousarray(cross, dtype=np.complex64).tobytes())
    r = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-3000:])
    raw, o, out = open(dst, "rb").read(), 0, []
    for psd, _, _, _, _ in items:
        nrows = psd.shape[0]
        out.append(np.frombuffer(raw, np.float32, 4 * nrows, o).reshape(nrows, 4))
        o += 16 * nrows
    assert o == len(raw)
    return out


def _spectra32(rows, N, overlap=1, kind=M.WINDOW_HANN):
    psd, cross = M.welch([rows], N, overlap, kind)
    return psd.astype(np.float32), cross.astype(np.complex64)


def test_the_kernels_figures_on_the_host(exe, tmp_path):
    items = []
    for N, L in ((16, 256), (64, 2048), (256, 4096)):
        rows = peak_cases._bandlimited_rows(L, (0.3, -0.4, 0.0, 2.25, -1.5, 0.05), (0.4, -1.1, 2.5, 0.0, 1.9, -2.7))
        psd, cross = _spectra32(rows, N)
        # the estimator's band, the widest band there is (every bin, the wrap at -N/2 included) and the narrowest (two bins), as one sum
        # and as the kernel's 64 interleaved parts
        for lo, hi in ((-max(N // 10, 1), max(N // 10, 1)), (-N // 2, N // 2 - 1), (-1, 0), (N // 2 - 2, N // 2 - 1), (-N // 2, -N // 2 + 1)):
            for step in (1, 64):
                items.append((psd, cross, lo, hi, step))
    g = M.gaussian_matrix(5, 1024, 9)
    items.append((*_spectra32(g, 64, 0, M.WINDOW_RECT), -16, 15, 64))
    for got, (psd, cross, lo, hi, step) in zip(run(exe, tmp_path, items), items):
        want, bar = M.align(psd, cross, lo, hi)
        err = M.align_errors(got, want)
        live = bar[:, 0] > 0
        assert live.all() and np.all(np.isfinite(got))
        assert np.all(err <= bar), (psd.shape, lo, hi, step, (err / bar).max())
        assert np.array_equal(got[0], np.array([0, 0, 1, 1], dtype=np.float32))


def test_degenerate_spectra_on_the_host(exe, tmp_path):
    N = 16
    zero = (np.zeros((3, N), dtype=np.float32), np.zeros((3, N), dtype=np.complex64))
    # one live bin: A = 0 (no two neighbours), so delay 0; the figures come from that bin alone
    one_p, one_c = np.zeros((2, N), dtype=np.float32), np.zeros((2, N), dtype=np.complex64)
    one_p[:, 3], one_c[0, 3], one_c[1, 3] = (4.0, 1.0), 4.0, 2.0 * np.exp(0.5j)
    # a reference without power under a live row: gain and coherence 0, never a division by zero
    dead_p, dead_c = np.zeros((2, N), dtype=np.float32), np.zeros((2, N), dtype=np.complex64)
    dead_p[1] = 1.0
    out = run(exe, tmp_path, [(*zero, -4, 4, 64), (one_p, one_c, -8, 7, 1), (dead_p, dead_c, -8, 7, 64)])
    assert not out[0].any()
    assert np.array_equal(out[1][0], np.array([0, 0, 1, 1], dtype=np.float32))
    assert out[1][1][0] == 0 and abs(out[1][1][1] - 0.5) < 1e-6 and abs(out[1][1][2] - 0.5) < 1e-6 and abs(out[1][1][3] - 1.0) < 1e-6
    assert not out[2].any()
    for o in out:
        assert np.all(np.isfinite(o))


@pytest.fixture(scope="module")
def host_build():
    importlib.import_module("coherent-rtlsdr_amd.binding").build()
    subprocess.run(["make", "-C", HOST, "all", "libcsynth.so"], check=True, stdout=subprocess.DEVNULL)
    return HOST


LINE = re.compile(r"spectra: batch (\d+) line (\d+) row (\d+): delay (\S+) phase (\S+) gain (\S+) coherence (\S+) peak bin (\d+) power (\S+) dB")


@pytest.mark.gpu
def test_host_demo_prints_the_alignment_of_every_row(host_build):
    nsig, batch, blocks = 3, 8, 32
    r = subprocess.run([os.path.join(host_build, "coherent_demo"), "--bench", "--spectra", "256:half", "--window", "hann", "--nsig", str(nsig), "--batch", str(batch),
                        "--blocks", str(blocks)], capture_output=True, text=True, timeout=300)
    print(r.stdout[-6000:], r.stderr)
    assert r.returncode == 0 and "DEMO OK" in r.stdout, r.stdout + r.stderr
    lines = LINE.findall(r.stdout)
    assert len(lines) == (blocks // batch) * batch * (1 + nsig), len(lines)      # batches x lines (a packet each) x rows
    near = 0
    for _, _, row, delay, phase, gain, coh, bin_, db in lines:
        assert 0.0 <= float(coh) <= 1.0 and 0 <= int(bin_) < 256 and np.isfinite(float(db))
        if int(row) == 0:
            assert (float(delay), float(phase), float(gain), float(coh)) == (0.0, 0.0, 1.0, 1.0)
        else:
            near += abs(float(delay)) <= 1.0
    # the integer lag has been removed and the synthetic channels carry the aligned reference noise
    assert 2 * near >= (blocks // batch) * batch * nsig, near


@pytest.mark.gpu
def test_host_demo_refuses_a_bad_transform(host_build):
    r = subprocess.run([os.path.join(host_build, "coherent_demo"), "--bench", "--spectra", "100", "--batch", "8", "--blocks", "32"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 1 and "DEMO FAILED" in r.stdout and "--spectra" in r.stdout, r.stdout + r.stderr
