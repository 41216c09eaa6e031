#!/usr/bin/env python3
"""Static instruction table of the K1 kernels (CPU only, no GPU needed).

    python3 tools/k1_isa_count.py [--asm FILE.s] [--pattern REGEX] [--loops] [--hazards]

Compiles coherent-rtlsdr_amd/csrc/crsdr.hip to device assembly with the Makefile's flags (or reads FILE.s) and prints,
per kernel whose name matches REGEX (default: K0 and the three B = 16384 K1 kernels), the number of vector ALU
instructions in its body, how many of them are packed fp32 (v_pk_add / v_pk_mul / v_pk_fma), and the VGPR / SGPR /
scratch figures of the code object's metadata.  The counts are static (instructions in the code, not executed ones):
k_xcorr_lag14q holds one row pair's worth of straight-line code, so its count is per row pair.
nop / wait: the s_nop instructions in the body and the wait states they stand for (s_nop N = N + 1): issue slots of the
wave's stream that no VALU count shows.

--hazards lists, for EVERY kernel of the file, the two read-after-write distances that gfx950 wants padded and that the
row loop is full of: a packed fp32 instruction (v_pk_add / mul / fma_f32) whose destination the very next instruction
reads, and a v_cmp whose mask a VALU instruction reads less than two wait states later.  The compiler pads both outside
inline asm, so a hit can only sit inside a hand-written multi-instruction asm block (cpk.hpp's grouped primitives), whose
author owns the hazard.  Exit status 1 if there is any.
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
                mn.append(s.split()[0] if not s.startswith("s_nop") else "s_nop:" + s.split()[1])
        out[m.group(1)] = mn
    return out


_MODS = re.compile(r"\b(?:op_sel|op_sel_hi|neg_lo|neg_hi|bitop3|row_\w+|bank_mask|row_mask|quad_perm|offset\d?|dst_sel|src\d_sel)\s*:\s*(?:\[[^\]]*\]|\S+)")


def _regs(tok):
    """Register names an operand touches: every VGPR / SGPR of a range, vcc, exec."""
    out = set()
    for m in re.finditer(r"\b([vsa])\[(\d+):(\d+)\]|\b([vsa])(\d+)\b|\b(vcc|exec)(?:_lo|_hi)?\b", tok):
        if m.group(1):
            out |= {m.group(1) + str(i) for i in range(int(m.group(2)), int(m.group(3)) + 1)}
        elif m.group(4):
            out.add(m.group(4) + m.group(5))
        else:
            out.add(m.group(6))
    return out


def _split(line):
    """(mnemonic, destination registers, source registers) of one instruction line."""
    line = line.split(";")[0].strip()
    parts = line.split(None, 1)
    mn = parts[0]
    ops = [o.strip() for o in _MODS.sub("", parts[1]).split(",")] if len(parts) > 1 else []
    ndst = 0 if not mn.startswith("v_") else 2 if "_co_" in mn or mn.startswith("v_div_scale") else 1
    dst, src = set(), set()
    for i, o in enumerate(ops):
        (dst if i < ndst else src).update(_regs(o))
    return mn, dst, src


def kernel_lines(txt):
    """{mangled name: [(instruction line, inside an inline-asm statement)] in program order}, block labels dropped."""
    out = {}
    for m in re.finditer(r"^(_Z\S+):\s*;\s*@\1\n(.*?)^\.Lfunc_end", txt, re.S | re.M):
        body, in_asm = [], False
        for line in m.group(2).splitlines():
            s = line.strip()
            if s.startswith(";;#ASM"):
                in_asm = s.startswith(";;#ASMSTART")
                continue
            if not s or s.startswith((";", ".", "_")) or s.endswith(":"):
                continue
            body.append((s, in_asm))
        out[m.group(1)] = body
    return out


def _src0_hi(line):
    """Does a packed instruction's first source read its high half in the high lane (op_sel_hi[0], set when not written)?"""
    m = re.search(r"op_sel_hi:\[(\d)", line)
    return m is None or m.group(1) == "1"


def hazards(body):
    """[(index, kind, producer line, consumer line)] of a kernel_lines() body:
    packed -- a v_pk_{add,mul,fma}_f32 result read by the very next instruction.  Inside or next to inline asm every such
              pair counts.  Between two instructions of the compiler's own only those it pads itself: it keeps the wait state
              when the producer's op_sel_hi[0] is set (the default), and lets a producer with a broadcast first source
              (op_sel_hi:[0,..]) be read at once -- k_frac_apply<14> has 14 such pairs and passes its tests;
    mask   -- a v_cmp mask read by a VALU instruction fewer than two wait states on."""
    found = []
    lines = [l for l, _ in body]
    ins = [_split(l) for l in lines]
    for i, (mn, dst, _) in enumerate(ins):
        packed = re.match(r"v_pk_(add|mul|fma)_f32", mn) is not None
        cmp_ = mn.startswith("v_cmp_")              # v_cmpx writes exec: another rule, none in these kernels
        if not (packed or cmp_) or not dst:
            continue
        need, states = (1 if packed else 2), 0
        for j in range(i + 1, len(ins)):
            mj, dj, sj = ins[j]
            if states >= need:
                break
            if mj.startswith("v_") and dst & sj:
                if cmp_ or body[i][1] or body[j][1] or _src0_hi(lines[i]):
                    found.append((i, "packed" if packed else "mask", lines[i], lines[j]))
                break
            if dst & dj:                                # overwritten: nothing of this result left to read
                break
            states += int(lines[j].split()[1], 0) + 1 if mj == "s_nop" else 1
    return found


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


COLUMNS = ("VALU", "packed", "pk_add", "pk_mul", "pk_fma", "SALU", "nop", "wait", "VGPR", "SGPR", "vspill", "sspill", "scratch")


def table(txt, pattern, loops=False):
    """The table's rows as dicts (the kernel's short name under "kernel", then COLUMNS; the metadata columns are strings),
    in the order they are printed."""
    bodies, meta = kernel_bodies(txt, loops), metadata(txt)
    pat = re.compile(pattern)
    rows = []
    for name, mn in sorted(bodies.items()):
        if not pat.search(name):
            continue
        short = re.search(r"\d+(k_\w+?)E", name)
        short = short.group(1) if short else name[:22]
        pk = {k: sum(1 for x in mn if x.startswith("v_pk_" + k + "_f32")) for k in ("add", "mul", "fma")}
        salu = sum(1 for x in mn if x.startswith("s_") and not x.startswith(("s_waitcnt", "s_nop", "s_barrier",
                                                                             "s_cbranch", "s_branch", "s_setprio",
                                                                             "s_sleep", "s_endpgm")))
        nops = [int(x.split(":")[1], 0) + 1 for x in mn if x.startswith("s_nop")]
        md = meta.get(name, {})
        rows.append({"kernel": short, "VALU": sum(1 for x in mn if x.startswith("v_")), "packed": sum(pk.values()),
                     "pk_add": pk["add"], "pk_mul": pk["mul"], "pk_fma": pk["fma"], "SALU": salu, "nop": len(nops),
                     "wait": sum(nops), "VGPR": md.get("vgpr_count", "?"), "SGPR": md.get("sgpr_count", "?"),
                     "vspill": md.get("vgpr_spill_count", "?"), "sspill": md.get("sgpr_spill_count", "?"),
                     "scratch": md.get("private_segment_fixed_size", "?")})
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--asm", help="read this device assembly instead of compiling")
    ap.add_argument("--pattern", default=r"k_xcorr_lag14[pqr]|k_ref_spectrum14p")
    ap.add_argument("--hazards", action="store_true",
                    help="list unpadded packed-result and compare-mask reads in every kernel; exit status 1 if any")
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
    if args.hazards:
        total = 0
        for name, lines in sorted(kernel_lines(txt).items()):
            hz = hazards(lines)
            total += len(hz)
            short = re.search(r"\d+(k_\w+?)E", name)
            print(f"{short.group(1) if short else name[:40]:40s} {len(lines):6d} instructions {len(hz):4d} hazards")
            for i, kind, a, b in hz:
                print(f"    [{i}] {kind}: {a}  ->  {b}")
        print(f"total {total}")
        return 1 if total else 0
    print(f"{'kernel':22s} {'VALU':>6s} {'packed':>6s} {'pk_add':>6s} {'pk_mul':>6s} {'pk_fma':>6s} {'SALU':>5s} {'nop':>4s} {'wait':>5s} "
          f"{'VGPR':>4s} {'SGPR':>4s} {'vspill':>6s} {'sspill':>6s} {'scratch':>7s}")
    for r in table(txt, args.pattern, args.loops):
        print(f"{r['kernel']:22s} {r['VALU']:6d} {r['packed']:6d} {r['pk_add']:6d} {r['pk_mul']:6d} {r['pk_fma']:6d} {r['SALU']:5d} {r['nop']:4d} {r['wait']:5d} "
              f"{r['VGPR']:>4s} {r['SGPR']:>4s} {r['vspill']:>6s} {r['sspill']:>6s} {r['scratch']:>7s}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
