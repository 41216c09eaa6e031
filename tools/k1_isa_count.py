#!/usr/bin/env python3
"""Static instruction table of the K1 kernels (CPU only, no GPU needed).

    python3 tools/k1_isa_count.py [--asm FILE.s] [--pattern REGEX]

Compiles coherent-rtlsdr_amd/csrc/crsdr.hip to device assembly with the Makefile's flags (or reads FILE.s) and prints,
per kernel whose name matches REGEX (default: K0 and the two B = 16384 K1 kernels), the number of vector ALU
instructions in its body, how many of them are packed fp32 (v_pk_add / v_pk_mul / v_pk_fma), and the VGPR / SGPR /
scratch figures of the code object's metadata.  The counts are static (instructions in the code, not executed ones):
k_xcorr_lag14q holds one row pair's worth of straight-line code, so its count is per row pair.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "coherent-rtlsdr_amd", "csrc")
FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-slp-vectorize"]


def compile_asm(out):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, *FLAGS, "--cuda-device-only", "-S", "-o", out, "crsdr.hip"], cwd=CSRC, check=True,
                   stderr=subprocess.DEVNULL)


def kernel_bodies(txt, loops_only=False):
    """{mangled name: list of instruction mnemonics} for every kernel symbol in the assembly.

    loops_only: only the instructions of basic blocks that the assembly's block comments place in a loop (for
    k_xcorr_lag14q: the row loop, without what a workgroup does once before and after it)."""
    out = {}
    for m in re.finditer(r"^(_Z\S+):\s*;\s*@\1\n(.*?)^\.Lfunc_end", txt, re.S | re.M):
        mn = []
        in_loop = False
        for line in m.group(2).splitlines():
            s = line.strip()
            if re.match(r"(\.LBB\d+_\d+:|; %bb\.\d+:)", s):        # a new block: its comment (and the lines below it) say whether it is in a loop
                in_loop = "Loop" in s
                continue
            if s.startswith(";") and "Loop" in s and ("Header" in s or "Parent" in s):
                in_loop = True
                continue
            if not s or s.startswith((";", ".", "_")) or s.endswith(":"):
                continue
            if in_loop or not loops_only:
                mn.append(s.split()[0])
        out[m.group(1)] = mn
    return out


def metadata(txt):
    meta = txt[txt.rfind("amdhsa.kernels:"):]
    res = {}
    for blk in meta.split("\n  - ")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk)
        if not name:
            continue
        g = lambda k: (re.search(r"\." + k + r":\s+(\d+)", blk) or [None, "?"])[1]
        res[name.group(1)] = {k: g(k) for k in ("vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count",
                                                   "private_segment_fixed_size")}
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--asm", help="read this device assembly instead of compiling")
    ap.add_argument("--pattern", default=r"k_xcorr_lag14[pq]|k_ref_spectrum14p")
    ap.add_argument("--loops", action="store_true",
                    help="count only instructions inside loops (k_xcorr_lag14q: per row pair, without the workgroup's one-off prologue)")
    args = ap.parse_args()
    if args.asm:
        txt = open(args.asm).read()
    else:
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "crsdr.s")
            compile_asm(path)
            txt = open(path).read()
    bodies, meta = kernel_bodies(txt, args.loops), metadata(txt)
    pat = re.compile(args.pattern)
    print(f"{'kernel':22s} {'VALU':>6s} {'packed':>6s} {'pk_add':>6s} {'pk_mul':>6s} {'pk_fma':>6s} {'SALU':>5s} "
          f"{'VGPR':>4s} {'SGPR':>4s} {'vspill':>6s} {'sspill':>6s} {'scratch':>7s}")
    for name, mn in sorted(bodies.items()):
        if not pat.search(name):
            continue
        short = re.search(r"\d+(k_\w+?)E", name)
        short = short.group(1) if short else name[:22]
        valu = sum(1 for x in mn if x.startswith("v_"))
        pk = {k: sum(1 for x in mn if x.startswith("v_pk_" + k + "_f32")) for k in ("add", "mul", "fma")}
        salu = sum(1 for x in mn if x.startswith("s_") and not x.startswith(("s_waitcnt", "s_nop", "s_barrier",
                                                                             "s_cbranch", "s_branch", "s_setprio",
                                                                             "s_sleep", "s_endpgm")))
        md = meta.get(name, {})
        print(f"{short:22s} {valu:6d} {sum(pk.values()):6d} {pk['add']:6d} {pk['mul']:6d} {pk['fma']:6d} {salu:5d} "
              f"{md.get('vgpr_count', '?'):>4s} {md.get('sgpr_count', '?'):>4s} {md.get('vgpr_spill_count', '?'):>6s} "
              f"{md.get('sgpr_spill_count', '?'):>6s} {md.get('private_segment_fixed_size', '?'):>7s}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
