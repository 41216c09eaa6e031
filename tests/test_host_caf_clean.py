"""The second cancellation stage's arithmetic on the host.

csrc/caf_clean_solve.hpp -- the limits, the walk that picks the targets from a detection list, the member table, where an entry of the
joint normal matrix sits, the joint Cholesky factor with its pivot rule and the solve on it, the functions the kernels of
csrc/caf_clean.hpp call -- as a stand-alone program (tools/caf_clean_cpu.cc) under AddressSanitizer + UBSan, on the lists and sums the
numpy model wrote: every index of the product's own functions checked without a GPU; the picks, the table and the status equal to
tests/caf_clean_model.py's, h and the share within the bars its docstring derives, and the leading block of the factor equal to the
canceller's own factor bit for bit.  The sanitizers report on stderr and through the exit status; both must stay clean.  Nothing is
loaded into Python under a sanitizer."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import caf_cancel_model as X
import caf_clean_model as Z
import caf_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "caf_clean_cpu.cc")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed for the host build of the second stage's arithmetic")
    out = tmp_path_factory.mktemp("asan") / "caf_clean_cpu"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off", "-o", str(out), SRC], check=True)
    return str(out)


def run(exe, tmp_path, items):
    """items: dict(nd, R, nrows, K, P, prm, det [Kdet][8], count, and, where the limits hold, S, A2 [n2max][nmax], E [nrows], c [nrows][nmax])
    -> per item dict(limit, and then picked, slot_lag, members [(lag, slot, owner, pos, g, phi)], status, L (packed), h [nrows][n], share)"""
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        f.write(np.int32(len(items)).tobytes())
        for it in items:
            p = it["prm"]
            det = np.ascontiguousarray(it["det"], dtype=np.float32)
            f.write(np.array([it["nd"], it["R"], it["nrows"], it["K"], it["P"], p.T, p.wl, p.wq, det.shape[0], it["count"]], dtype=np.int32).tobytes())
            f.write(np.float32(p.min_snr).tobytes())
            f.write(det.tobytes())
            if "S" not in it:
                continue
            f.write(np.ascontiguousarray(it["S"], dtype=np.complex128).tobytes())
            f.write(np.ascontiguousarray(it["A2"], dtype=np.complex128).tobytes())
            for e, row in zip(it["E"], it["c"]):
                f.write(np.float64(e).tobytes())
                f.write(np.ascontiguousarray(row, dtype=np.complex128).tobytes())
    r = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-3000:])
    raw = open(dst, "rb").read()
    out, at = [], 0

    def take(dtype, count):
        nonlocal at
        a = np.frombuffer(raw, dtype, count, at)
        at += a.nbytes
        return a

    for it in items:
        o = dict(limit=int(take(np.int32, 1)[0]))
        out.append(o)
        if o["limit"]:
            continue
        nt = int(take(np.int32, 1)[0])
        o["picked"] = take(np.int32, it["prm"].T)[:nt].tolist()
        nmem, nslot = (int(v) for v in take(np.int32, 2))
        o["slot_lag"] = take(np.int32, nslot).tolist()
        o["members"] = []
        for _ in range(nmem):
            lag, slot, owner, pos = (int(v) for v in take(np.int32, 4))
            g, fr, fi = take(np.float64, 3)
            o["members"].append((lag, slot, owner, pos, float(g), complex(fr, fi)))
        n = X.basis(it["K"], it["P"]) + nmem
        o["status"] = int(take(np.int32, 1)[0])
        o["L"] = take(np.complex128, n * (n + 1) // 2)
        rows = take(np.float64, it["nrows"] * (2 * n + 1)).reshape(it["nrows"], 2 * n + 1)
        o["h"], o["share"] = rows[:, 0:2 * n:2] + 1j * rows[:, 1:2 * n:2], rows[:, 2 * n]
    assert at == len(raw)
    return out


def _item(r, nd, R, nrows, K, P, prm, det, count):
    """the program's input from the model's dict r of a line"""
    n1, n2max = r["n1"], prm.T * prm.per
    n, nmax = r["A"].shape[0], r["n1"] + prm.T * prm.per
    A2 = np.zeros((n2max, nmax), dtype=np.complex128)
    A2[:n - n1, :n] = np.tril(r["A"])[n1:]
    c = np.zeros((nrows, nmax), dtype=np.complex128)
    c[:, :n] = r["c"]
    return dict(nd=nd, R=R, nrows=nrows, K=K, P=P, prm=prm, det=det, count=count, S=X.s_sums(r["stage1"]["G"], P), A2=A2, E=r["stage1"]["E"], c=c)


def _rec(lag, dop, snr, ddop=0.0, power=1.0):
    return [lag, dop, power, snr, power / snr, 0.0, ddop, 40]


def _packed(L):
    """the program's packed lower triangle: the diagonal holds (L_kk, 1 / L_kk)"""
    n = L.shape[0]
    return np.array([L[i, k] if k < i else complex(L[i, i].real, 1.0 / L[i, i].real) for i in range(n) for k in range(i + 1)])


def test_the_masking_scene_on_the_host_against_the_model(exe, tmp_path):
    mk = Z.MASK
    line = Z.masking_scene(0)
    s1 = X.cancel(line, mk["seg"], mk["R"], mk["ref"], M.WINDOW_HANN, mk["taps"], mk["dopp"])
    _, d1 = Z.array_list(s1["chi"], mk["ref"], 0, Z.masking_detector())
    det = d1["det"].astype(np.float32)
    items, models = [], []
    for wl, wq, T in ((1, 1, 2), (2, 2, 1), (0, 0, 8), (2, 1, 4)):
        prm = Z.Params(T, 100.0, wl, wq)
        r = Z.clean(line, mk["seg"], mk["R"], mk["ref"], M.WINDOW_HANN, mk["taps"], mk["dopp"], det, d1["count"], prm)
        assert r["cond"] <= Z.COND_MAX and r["picked"] == [0]
        models.append(r)
        items.append(_item(r, mk["nd"], mk["R"], mk["nrows"], mk["taps"], mk["dopp"], prm, det, d1["count"]))
    for r, it, o in zip(models, items, run(exe, tmp_path, items)):
        assert o["limit"] == 0 and o["picked"] == r["picked"] and o["status"] == 0
        assert [(m[0], m[2], m[3]) for m in o["members"]] == [(m[0], m[2], m[3]) for m in r["members"]]
        assert [m[4] for m in o["members"]] == [m[1] for m in r["members"]]      # g: exact
        assert all(o["slot_lag"][m[1]] == m[0] for m in o["members"]) and len(set(o["slot_lag"])) == len(o["slot_lag"])
        assert all(abs(m[5] - Z.phase(m[4], it["nd"])[-1]) <= 8 * 2.0 ** -53 for m in o["members"])
        others = [c for c in range(it["nrows"]) if c != mk["ref"]]
        err = np.maximum(np.abs(o["h"].real - r["h"].real), np.abs(o["h"].imag - r["h"].imag))
        # (the program solves row r's equations as well; the model zeroes them)
        assert np.all(err[others] <= r["hbar"][others]), np.max(err[others] / r["hbar"][others])
        assert np.all(np.abs(o["share"] - r["share"])[others] <= r["sbar"][others])
        # the leading block is the canceller's own factor, bit for bit: the same program on the same S without picks
        n1 = r["n1"]
        alone = run(exe, tmp_path, [dict(it, count=0)])[0]
        assert alone["picked"] == [] and np.array_equal(alone["L"].view(np.uint64), o["L"][:n1 * (n1 + 1) // 2].view(np.uint64))
        assert np.allclose(o["L"], _packed(r["L"]), rtol=1e-9, atol=1e-9 * np.abs(r["L"]).max())


def test_the_walk_and_the_table_at_their_edges_on_the_host(exe, tmp_path):
    """hand-made lists at nd 32, R 16, K 2, P 1: the picks and the table against the model, the clipped clusters and the wrap included"""
    nd, R, K, P = 32, 16, 2, 1
    lists = [
        [_rec(0, 9, 500.0), _rec(15, -12, 400.0), _rec(7, 3, 50.0)],                              # lag 0 and R - 1: clipped; the third under min_snr
        [_rec(5, -16, 900.0, ddop=0.25), _rec(6, 15, 800.0, ddop=0.3), _rec(9, 15, 700.0)],       # across the wrap: the second touches the first
        [_rec(2, 2, 900.0, ddop=0.4), _rec(2, 3, 800.0), _rec(3, -2, 700.0, ddop=-0.6)],          # the first touches the clutter basis at wq 2, the third is clear of it by its lag
        [_rec(4 + 3 * i, 8, 900.0 - i) for i in range(4)],                                        # more candidates than T
        [],
    ]
    items, want = [], []
    for wl, wq, T in ((1, 1, 2), (2, 2, 1), (0, 0, 3), (1, 2, 2)):
        prm = Z.Params(T, 100.0, wl, wq)
        for recs in lists:
            det = np.zeros((4, 8), dtype=np.float32)
            det[:len(recs)] = np.array(recs, dtype=np.float32).reshape(-1, 8)
            if Z.bad_limit(nd, R, 1, 3, K, P, prm):
                items.append(dict(nd=nd, R=R, nrows=3, K=K, P=P, prm=prm, det=det, count=len(recs)))
                want.append(None)
                continue
            picked = Z.pick_walk(det, len(recs), nd, K, P, prm)
            tm = Z.target_members(det, picked, R, prm)
            n1, n2max = X.basis(K, P), prm.T * prm.per
            n = n1 + len(tm)
            rng = np.random.default_rng(len(items))
            Bm = rng.standard_normal((n, n + 4)) + 1j * rng.standard_normal((n, n + 4))
            A = Bm @ Bm.conj().T                                                  # any positive definite matrix: the table and the indices are the subject
            S = np.zeros((4 * P + 1, K, K), dtype=np.complex128)
            for i in range(n1):
                for j in range(n1):
                    S[j // K - i // K + 2 * P, j % K, i % K] = A[i, j]           # gram_entry's place; entries it reads twice must agree
            for i in range(n1):
                for j in range(n1):
                    A[i, j] = S[j // K - i // K + 2 * P, j % K, i % K]
            A = np.tril(A) + np.tril(A, -1).conj().T
            A += np.eye(n) * (np.abs(A).sum() + 1.0)                              # the block structure made it indefinite: dominant diagonal
            for i in range(n1):
                S[2 * P, i % K, i % K] = A[i, i]
            A2 = np.zeros((n2max, n1 + n2max), dtype=np.complex128)
            A2[:n - n1, :n] = np.tril(A)[n1:]
            c = np.zeros((3, n1 + n2max), dtype=np.complex128)
            c[:, :n] = rng.standard_normal((3, n)) + 1j * rng.standard_normal((3, n))
            items.append(dict(nd=nd, R=R, nrows=3, K=K, P=P, prm=prm, det=det, count=len(recs), S=S, A2=A2, E=np.ones(3), c=c))
            want.append((picked, tm, A, c[:, :n]))
    assert sum(w is not None for w in want) >= 15
    for it, w, o in zip(items, want, run(exe, tmp_path, items)):
        if w is None:
            assert o["limit"] != 0
            continue
        picked, tm, A, c = w
        assert o["limit"] == 0 and o["picked"] == picked, (it["prm"].__dict__, it["det"][:, :2], o["picked"], picked)
        assert [(m[0], m[2], m[3], m[4]) for m in o["members"]] == [(m[0], m[2], m[3], m[1]) for m in tm]
        assert all(0 <= m[0] < R for m in o["members"])
        assert o["status"] == 0
        # the diagonal of S is shared by the Doppler blocks: solve the matrix the program saw
        n1 = X.basis(K, P)
        for i in range(n1):
            A[i, i] = it["S"][2 * P, i % K, i % K]
        h = np.linalg.solve(A, c.T).T
        assert np.allclose(o["h"], h, rtol=1e-9, atol=1e-12)
    # the walk's decisions at these lists, spelt out once: clipped clusters, the wrap, the clutter basis, T reached
    prm = Z.Params(2, 100.0, 1, 1)
    d = lambda recs: np.array(recs + [[0] * 8] * (4 - len(recs)), dtype=np.float32)
    assert Z.pick_walk(d(lists[0]), 3, nd, K, P, prm) == [0, 1] and len(Z.target_members(d(lists[0]), [0, 1], R, prm)) == 12
    assert Z.pick_walk(d(lists[1]), 3, nd, K, P, prm) == [0, 2]
    assert Z.pick_walk(d(lists[2]), 3, nd, K, P, Z.Params(2, 100.0, 1, 2)) == [1, 2]
    assert Z.pick_walk(d(lists[3]), 4, nd, K, P, prm) == [0, 1]


def test_failed_pivots_on_the_host(exe, tmp_path):
    """status 1 for an all-zero S, status 2 for a target column that repeats another: h stays zero, the share 1, and no NaN"""
    mk = Z.MASK
    line = Z.masking_scene(1)
    s1 = X.cancel(line, mk["seg"], mk["R"], mk["ref"], M.WINDOW_HANN, mk["taps"], mk["dopp"])
    _, d1 = Z.array_list(s1["chi"], mk["ref"], 0, Z.masking_detector())
    prm = Z.Params(1, 100.0, 1, 0)
    det = d1["det"].astype(np.float32)
    r = Z.clean(line, mk["seg"], mk["R"], mk["ref"], M.WINDOW_HANN, mk["taps"], mk["dopp"], det, d1["count"], prm)
    good = _item(r, mk["nd"], mk["R"], mk["nrows"], mk["taps"], mk["dopp"], prm, det, d1["count"])
    zero = dict(good, S=np.zeros_like(good["S"]))
    dup = dict(good, A2=good["A2"].copy())
    n1 = r["n1"]
    dup["A2"][1, :n1 + 1] = dup["A2"][0, :n1 + 1]                                 # the second target member equal to the first: its pivot is 0
    dup["A2"][1, n1 + 1] = dup["A2"][0, n1].real
    got = run(exe, tmp_path, [good, zero, dup])
    assert [o["status"] for o in got] == [0, Z.STATUS_SINGULAR, Z.STATUS_TARGET]
    for o in got[1:]:
        assert not o["h"].any() and np.all(o["share"] == 1.0)


HOST = os.path.join(ROOT, "coherent-rtlsdr_amd", "host")


@pytest.fixture(scope="module")
def host_build():
    import importlib
    importlib.import_module("coherent-rtlsdr_amd.binding").build()
    subprocess.run(["make", "-C", HOST, "all", "libcsynth.so"], check=True, stdout=subprocess.DEVNULL)
    return HOST


@pytest.mark.gpu
def test_host_demo_prints_the_picks_and_the_residual_list_of_every_line(host_build):
    """coherent_demo --bench --caf ... --cancel K:P --cfar DB --clean T (ccaf::batch over crsdr_caf_set_clean): a summary line per batch
    and line, the picks in front of it and the residual's detections behind it; refused without the canceller."""
    import re
    nsig, batch, blocks, seg, lags = 3, 8, 16, 64, 16
    base = [os.path.join(host_build, "coherent_demo"), "--bench", "--caf", f"{seg}:{lags}", "--nsig", str(nsig), "--batch", str(batch), "--blocks", str(blocks), "--guard", "2",
            "--cfar", "12", "--max-det", "4"]
    on = subprocess.run(base + ["--cancel", "4:1", "--clean", "2:15:1:1"], capture_output=True, text=True, timeout=300)
    print(on.stdout[-3000:], on.stderr)
    assert on.returncode == 0 and "DEMO OK" in on.stdout, on.stdout + on.stderr
    lines = {(int(bt), int(e)): (int(n), int(st), int(rc)) for bt, e, n, st, rc in re.findall(r"clean: batch (\d+) line (\d+): (\d+) picks status (\d+) residual list (\d+)", on.stdout)}
    nb = max(3, blocks // batch)
    assert sorted(lines) == [(bt, e) for bt in range(nb) for e in range(batch)], sorted(lines)
    picks = re.findall(r"clean: batch (\d+) line (\d+) pick (\d+) of (\d+):", on.stdout)
    assert len(picks) == sum(n for n, _, _ in lines.values()) and all(st in (0, 2) for _, st, _ in lines.values())
    bad = subprocess.run(base + ["--clean", "2"], capture_output=True, text=True, timeout=300)       # no canceller
    assert bad.returncode != 0 and "--clean T[:MIN_SNR_DB[:WL:WQ]] refused" in bad.stdout
