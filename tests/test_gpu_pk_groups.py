"""cpk.hpp's grouped forms (several independent values per asm statement, first halves before second halves) against the
single forms they replace, bit for bit: tools/pk_check.hip compares every grouped primitive (cmul_g2/3/4 and head_g2 in
both conjugations, q_first4) and every place that uses one (tw_chain, tw_apply, tw_stage1s_inv, dft4_inv_mul) with the
single forms run one after the other, on 65536 threads x 128 values drawn from random numbers in K1's range, random
numbers of any exponent, +-0, +-inf, NaN, denormals and the largest finite values.  Only the order of instructions differs
between the two, so every bit must agree, NaN payloads included."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_grouped_primitives_give_the_bits_of_the_single_forms(tmp_path):
    exe = str(tmp_path / "pk_check")
    subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-slp-vectorize",
                    "-w", "-o", exe, os.path.join(ROOT, "tools", "pk_check.hip")], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "grouped forms:" in r.stdout and "mismatches 0" in r.stdout.split("grouped forms:")[1].splitlines()[0], r.stdout
    assert r.stdout.rstrip().endswith("mismatches 0"), r.stdout
