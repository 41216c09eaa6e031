"""The carried-chain two-row K1 (k_xcorr_lag14r) against the two-row kernel it was split from (k_xcorr_lag14q), statically
(CPU only: one compile of crsdr.hip, tools/k1_isa_count.py --loops).

Both kernels are one body (csrc/xcorr14q.hpp, q_xcorr_lag14_body).  k_xcorr_lag14q builds the two column twiddle chains
W_16384^(vt k), k = 1 .. 31, in a row's first pass and again in its last one: four builds of 52 packed instructions per row.
k_xcorr_lag14r builds both once before the row loop and carries them over the back edge, so its row loop holds two builds:
104 packed instructions fewer.  Both chains are carried here, so the floor is 100 (it would be 50 for one carried chain); the
vector instructions as a whole must drop by the same floor.  The carried chains are 124 registers that live from a row's last
pass to the next row's first: the kernel may use all 256 VGPRs (one workgroup per CU, two waves per SIMD: no occupancy is lost)
but spills nothing and has no scratch.  Wait states: no more than the row loop had before the address / max-tree change (217).

tests/test_k1_isa_budget.py pins k_xcorr_lag14q itself; tests/test_k1_isa_hazards.py walks every kernel, this one included."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PACKED_Q = 2768      # the row loop of k_xcorr_lag14q (tests/test_k1_isa_budget.py)
FLOOR = 100          # both chains carried


def _tool():
    spec = importlib.util.spec_from_file_location("k1_isa_count", os.path.join(ROOT, "tools", "k1_isa_count.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def loops(tmp_path_factory):
    t = _tool()
    path = str(tmp_path_factory.mktemp("k1_carry_isa") / "crsdr.s")
    t.compile_asm(path)
    rows = {}
    for r in t.table(open(path).read(), r"k_xcorr_lag14[qr]E", True):
        rows.setdefault(r["kernel"], {c: int(r[c]) for c in t.COLUMNS})
    return rows


def test_both_kernels_are_found_by_name(loops):
    assert set(loops) == {"k_xcorr_lag14q", "k_xcorr_lag14r"}


def test_carried_chain_kernel_row_loop(loops):
    q, r = loops["k_xcorr_lag14q"], loops["k_xcorr_lag14r"]
    print("k_xcorr_lag14r row loop:", r, "k_xcorr_lag14q:", q)
    assert q["packed"] == PACKED_Q
    assert r["packed"] <= PACKED_Q - FLOOR
    assert r["VALU"] <= q["VALU"] - FLOOR
    assert r["wait"] <= 217
    assert r["VGPR"] <= 256
    assert r["vspill"] == 0
    assert r["scratch"] == 0
