"""The peak figures' arithmetic and the C++ host layer of the range-Doppler engine.

CPU: csrc/caf_peak.hpp -- the searched set, the first maximum, the mean and the two parabolas that the kernel of csrc/caf.hpp calls --
as a stand-alone program (tools/caf_peak_cpu.cc) under AddressSanitizer + UBSan, on maps the numpy model wrote: every index of the
product's own functions checked without a GPU, and the figures held against tests/caf_model.py within the bar its docstring derives.
The sanitizers report on stderr and through the exit status; both must stay clean.  Nothing is loaded into Python under a sanitizer.

GPU: coherent_demo --bench --caf (ccaf::batch over crsdr_caf) prints a line per batch, line and row."""
import importlib
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import caf_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "caf_peak_cpu.cc")
HOST = os.path.join(ROOT, "coherent-rtlsdr_amd", "host")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed for the host build of the peak figures")
    out = tmp_path_factory.mktemp("asan") / "caf_peak_cpu"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off", "-o", str(out), SRC], check=True)
    return str(out)


def run(exe, tmp_path, items):
    """items: (src [nd][R] float32 or complex64, guard, step) -> peak [6] float32 each"""
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        f.write(np.int32(len(items)).tobytes())
        for a, guard, step in items:
            nd, R = a.shape
            f.write(np.array([nd, R, guard, 2 if np.iscomplexobj(a) else 1, step], dtype=np.int32).tobytes())
            f.write(np.ascontiguousarray(a).tobytes())
    r = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-3000:])
    raw = open(dst, "rb").read()
    assert len(raw) == 24 * len(items)
    return np.frombuffer(raw, np.float32).reshape(len(items), 6)


def _want(a, guard):
    return M.peaks(M.power(a) if np.iscomplexobj(a) else a.astype(np.float64), guard)


def _floor(nd, R, seed, complex_):
    rng = np.random.default_rng(seed)
    if complex_:
        return (0.1 * (rng.standard_normal((nd, R)) + 1j * rng.standard_normal((nd, R)))).astype(np.complex64)
    return (0.01 * rng.random((nd, R))).astype(np.float32)


def test_the_kernels_figures_on_the_host(exe, tmp_path):
    items = []
    for nd, R in ((8, 1), (4096, 3), (32, 16)):
        for guard in (0, 1, 2, nd // 2):
            edge = [g for g in (guard, nd - guard) if 0 <= g < nd] if guard else [0]     # both guard edges (s = +guard, s = -guard)
            # every corner of the map, both edges of the guard, and the bins on either side of the cyclic wrap
            spots = [(d, t) for d in sorted({0, nd - 1, nd // 2, nd // 2 - 1, *edge}) for t in sorted({0, R - 1, R // 2})]
            for i, (d, t) in enumerate(spots):
                for complex_ in (False, True):
                    a = _floor(nd, R, 1000 * nd + 10 * i + guard, complex_)
                    a[d, t] = 3.0 + (2.0j if complex_ else 0.0)
                    a[(d + 1) % nd, t] = 2.0                                      # uneven neighbours: offsets that are not zero
                    if t + 1 < R:
                        a[d, t + 1] = 1.5
                    items.append((a, guard, 1 if i % 2 else 256))
    got = run(exe, tmp_path, items)
    live = 0
    for g, (a, guard, step) in zip(got, items):
        want, bar = _want(a, guard)
        assert np.all(np.isfinite(g)) and abs(g[4]) <= 0.5 and abs(g[5]) <= 0.5
        assert np.all(np.abs(g.astype(np.float64) - want) <= bar), (a.shape, guard, step, g, want, bar)
        live += (g[4] != 0) + (g[5] != 0)
    assert live > len(items) // 4                                                # (the offsets were exercised, not all guarded to zero)


def test_plateaus_ties_and_zeros_on_the_host(exe, tmp_path):
    tie = np.zeros((8, 4), dtype=np.float32)
    tie[5, 2] = tie[3, 1] = tie[3, 3] = 7.0
    flat = np.full((16, 5), 2.0, dtype=np.float32)
    ctie = np.zeros((8, 3), dtype=np.complex64)
    ctie[6, 1], ctie[2, 2] = 3 + 4j, 5 + 0j                                      # |.|^2 = 25 both: the first index wins, whichever part holds it
    zero, czero = np.zeros((4096, 3), dtype=np.float32), np.zeros((8, 1), dtype=np.complex64)
    items = [(tie, 0, 1), (tie, 0, 256), (tie, 4, 256), (flat, 0, 256), (flat, 3, 1), (flat, 8, 256), (ctie, 0, 256), (ctie, 0, 2), (zero, 0, 256), (zero, 2048, 1),
             (czero, 4, 256), (czero, 0, 1)]
    got = run(exe, tmp_path, items)
    for g, (a, guard, step) in zip(got, items):
        want, bar = _want(a, guard)
        assert np.all(np.isfinite(g)) and np.all(np.abs(g.astype(np.float64) - want) <= bar), (a.shape, guard, step, g, want)
    assert list(got[0]) == [1, 3, 7, 7 / (21 / 32), 0, 0] and list(got[1]) == list(got[0])
    assert not got[2].any()                                                      # only d = 4 is searched, and it is zero
    assert list(got[3]) == [0, 0, 2, 1, 0, 0] and list(got[4]) == [0, 3, 2, 1, 0, 0] and list(got[5]) == [0, -8, 2, 1, 0, 0]
    assert (got[6][0], got[6][1]) == (2, 2) and list(got[7]) == list(got[6])
    assert not got[8:].any()


@pytest.fixture(scope="module")
def host_build():
    importlib.import_module("coherent-rtlsdr_amd.binding").build()
    subprocess.run(["make", "-C", HOST, "all", "libcsynth.so"], check=True, stdout=subprocess.DEVNULL)
    return HOST


LINE = re.compile(r"caf: batch (\d+) line (\d+) (row \d+|map): lag (\d+)([+-]\S+) doppler (-?\d+)([+-]\S+) power (\S+) dB ratio (\S+) dB")


@pytest.mark.gpu
def test_host_demo_prints_the_peak_of_every_row(host_build):
    nsig, batch, blocks, seg, lags, L = 3, 8, 16, 64, 16, 8192
    r = subprocess.run([os.path.join(host_build, "coherent_demo"), "--bench", "--caf", f"{seg}:{lags}", "--nsig", str(nsig), "--batch", str(batch), "--blocks", str(blocks)],
                       capture_output=True, text=True, timeout=300)
    print(r.stdout[-6000:], r.stderr)
    assert r.returncode == 0 and "DEMO OK" in r.stdout, r.stdout + r.stderr
    lines = LINE.findall(r.stdout)
    nb = max(3, blocks // batch)                                                 # (the bench times at least three batches)
    assert len(lines) == nb * batch * (1 + nsig + 1), len(lines)                 # batches x lines (a packet each) x (rows + the map)
    # The scene's own ratio, by the model on the demo's seed: block 0 of the synthetic source, every signal row moved back by its own
    # integer delay (a rotation within the block: at worst the plan's alignment keeps as many samples of the copy), against row 0.
    # The demo's lines are other blocks of the same source: the searched cells' mean (over nd R - 1 >= 2047 noise cells) and the peak
    # (N = 8192 samples) each move by about 2 % from block to block, 0.2 dB together; 0.5 dB is allowed below the model's figure.
    synth = importlib.import_module("coherent-rtlsdr_amd.synth")
    rows, prm = synth.make_block(nsig, L, synth.config_seed(1), 0)
    for k in range(nsig):
        rows[1 + k] = np.roll(rows[1 + k], -2 * int(prm.d[k]))
    chi, _ = M.caf([rows], seg, lags, 0, M.WINDOW_RECT)
    chi32 = chi.astype(np.complex64)
    want, _ = M.all_peaks(chi32, M.array_map(chi32, 0)[0], 0)
    want_db = 10 * np.log10(want[:, 3])
    print("the model's ratios for the scene (rows, then the map), dB:", np.round(want_db, 2))
    assert np.all(want[:, :2] == 0)
    for _, _, who, lag, dlag, dop, ddop, power, ratio in lines:
        entry = nsig + 1 if who == "map" else int(who.split()[1])
        assert (int(lag), int(dop)) == (0, 0), (who, lag, dop)
        assert abs(float(dlag)) <= 0.5 and abs(float(ddop)) <= 0.5 and np.isfinite(float(power))
        assert float(ratio) > want_db[entry] - 0.5, (who, ratio, want_db[entry])


@pytest.mark.gpu
def test_host_demo_refuses_a_bad_segment(host_build):
    r = subprocess.run([os.path.join(host_build, "coherent_demo"), "--bench", "--caf", "100:16", "--batch", "8", "--blocks", "16"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 1 and "DEMO FAILED" in r.stdout and "--caf" in r.stdout, r.stdout + r.stderr
