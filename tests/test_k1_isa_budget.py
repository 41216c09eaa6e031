"""The two-row K1's row loop stays inside its static instruction budget (CPU only: one compile of crsdr.hip).

k_xcorr_lag14q is issue-bound: the pair period is the sum of both rows' issued instructions, so a vector
instruction or a wait state that creeps back into the row loop is time.  The budget is set against the table of the commit
before the address / max-tree change, profiles/k1_wait/isa_new.txt (tools/k1_isa_count.py --loops, then whole kernels):
that row loop held 3 859 vector instructions, 2 768 of them packed, and 217 wait states.  The change takes the LDS literal
adds (about 124) and the regrouped lane maximum (about 31) out; 150 is the floor those two alone must clear.  The packed
count is the arithmetic itself and must not move.  Registers: 256 at the most, nothing spilled, no scratch.

k_xcorr_lag14p is the bit-for-bit yardstick of the two-row kernel (tests/test_gpu_k1_twshare.py, test_k1_variants_agree):
the change must not reach it, so its rows must equal the recorded ones in every column, inside loops and whole."""
import importlib.util
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARENT_TABLE = os.path.join(ROOT, "profiles", "k1_wait", "isa_new.txt")
FLOOR = 150


def _tool():
    spec = importlib.util.spec_from_file_location("k1_isa_count", os.path.join(ROOT, "tools", "k1_isa_count.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _parent_rows(t):
    """[loops table, whole-kernel table] of the recorded file, each {kernel: {column: int}} (first row of a name wins:
    template instantiations share a short name, the two kernels asked for here have one row each)."""
    tables = []
    for line in open(PARENT_TABLE):
        f = line.split()
        if not f or f[0].startswith("#"):
            continue
        if f[0] == "kernel":
            assert tuple(f[1:]) == t.COLUMNS, f
            tables.append({})
            continue
        tables[-1].setdefault(f[0], dict(zip(t.COLUMNS, map(int, f[1:]))))
    assert len(tables) == 2
    return tables


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    t = _tool()
    path = str(tmp_path_factory.mktemp("k1_isa") / "crsdr.s")
    t.compile_asm(path)
    txt = open(path).read()
    out = []
    for loops in (True, False):
        rows = {}
        for r in t.table(txt, r"k_xcorr_lag14[pq]E", loops):
            rows.setdefault(r["kernel"], {c: int(r[c]) for c in t.COLUMNS})
        out.append(rows)
    return t, out


def test_the_recorded_parent_table_is_the_one_the_budget_names():
    loops, whole = _parent_rows(_tool())
    q = loops["k_xcorr_lag14q"]
    assert (q["VALU"], q["packed"], q["wait"]) == (3859, 2768, 217)
    assert whole["k_xcorr_lag14q"]["VALU"] == 4014


def test_two_row_kernel_row_loop_budget(tables):
    t, (loops, _) = tables
    parent = _parent_rows(t)[0]["k_xcorr_lag14q"]
    q = loops["k_xcorr_lag14q"]
    print("k_xcorr_lag14q row loop:", q, "parent:", parent)
    assert q["packed"] == parent["packed"] == 2768
    assert q["VALU"] <= parent["VALU"] - FLOOR
    assert q["VGPR"] <= 256
    assert q["vspill"] == 0
    assert q["scratch"] == 0
    assert q["wait"] <= parent["wait"] == 217


def test_one_row_kernel_is_untouched(tables):
    t, (loops, whole) = tables
    p_loops, p_whole = _parent_rows(t)
    assert loops["k_xcorr_lag14p"] == p_loops["k_xcorr_lag14p"]
    assert whole["k_xcorr_lag14p"] == p_whole["k_xcorr_lag14p"]
