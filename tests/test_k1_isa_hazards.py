"""No hand-written asm block reads a packed result or a compare mask too early (CPU only: one compile of crsdr.hip).

hipcc pads the two read-after-write distances gfx950 wants padded -- a packed fp32 result read by the next instruction,
a v_cmp mask read by a VALU instruction fewer than two wait states on -- everywhere except inside an inline-asm
statement, whose author owns them.  cpk.hpp's grouped primitives and xcorr14q.hpp's q_first4 are such statements;
tools/k1_isa_count.py --hazards walks the device assembly of every kernel and must find none."""
import importlib.util
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("k1_isa_count", os.path.join(ROOT, "tools", "k1_isa_count.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_scanner_sees_a_hazard_when_there_is_one():
    t = _tool()
    asm = lambda *ls: [(l, True) for l in ls]
    # packed result read by the next instruction, whatever its modifiers, inside asm
    assert len(t.hazards(asm("v_pk_mul_f32 v[0:1], v[2:3], v[4:5] op_sel_hi:[0,1]", "v_pk_add_f32 v[6:7], v[0:1], v[4:5]"))) == 1
    assert t.hazards(asm("v_pk_mul_f32 v[0:1], v[2:3], v[4:5]", "v_pk_mul_f32 v[8:9], v[2:3], v[4:5]", "v_pk_add_f32 v[6:7], v[0:1], v[4:5]")) == []
    assert t.hazards(asm("v_pk_mul_f32 v[0:1], v[2:3], v[4:5]", "s_nop 0", "v_pk_add_f32 v[6:7], v[0:1], v[4:5]")) == []
    # a mask needs two wait states
    assert len(t.hazards(asm("v_cmp_eq_f32_e64 s[4:5], s3, v1", "v_mov_b32 v9, v8", "v_cndmask_b32_e64 v0, v0, v1, s[4:5]"))) == 1
    assert t.hazards(asm("v_cmp_eq_f32_e64 s[4:5], s3, v1", "v_mov_b32 v9, v8", "v_mov_b32 v10, v8", "v_cndmask_b32_e64 v0, v0, v1, s[4:5]")) == []
    assert len(t.hazards(asm("v_cmp_eq_f32_e32 vcc, s3, v1", "s_nop 0", "v_cndmask_b32_e32 v0, v0, v1, vcc"))) == 1
    assert t.hazards(asm("v_cmp_eq_f32_e32 vcc, s3, v1", "s_nop 1", "v_cndmask_b32_e32 v0, v0, v1, vcc")) == []
    # the compiler's own pair with a broadcast first source: it does not pad it, and it is not ours to flag
    own = [("v_pk_mul_f32 v[0:1], v[2:3], v[4:5] op_sel_hi:[0,1]", False), ("v_pk_add_f32 v[6:7], v[0:1], v[4:5]", False)]
    assert t.hazards(own) == []
    assert len(t.hazards([("v_pk_mul_f32 v[0:1], v[2:3], v[4:5]", False), ("v_pk_add_f32 v[6:7], v[0:1], v[4:5]", False)])) == 1


def test_no_kernel_reads_a_packed_result_or_a_mask_too_early(tmp_path):
    t = _tool()
    path = str(tmp_path / "crsdr.s")
    t.compile_asm(path)
    txt = open(path).read()
    kernels = t.kernel_lines(txt)
    assert any("k_xcorr_lag14q" in k for k in kernels) and len(kernels) > 50
    found = {k: t.hazards(body) for k, body in kernels.items()}
    bad = {k: v for k, v in found.items() if v}
    assert not bad, "\n".join(f"{k}: {a} -> {b}" for k, v in bad.items() for _, _, a, b in v)
    # the grouped statements are there to be checked: the two-row kernel holds multi-instruction asm blocks
    q = next(body for k, body in kernels.items() if "k_xcorr_lag14qE" in k)
    assert sum(1 for l, in_asm in q if in_asm and l.startswith("v_cmp_eq_f32_e64")) >= 64
