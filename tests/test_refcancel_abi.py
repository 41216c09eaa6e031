"""CPU checks of the reference-noise canceller's ABI (include/crsdr.h: crsdr_plan_set_refcancel, crsdr_plan_fetch_refcancel,
crsdr_plan_refcancel_buffers, crsdr_refcancel): the symbols are declared, exported and bound, bad arguments are refused before a
device is looked for, and the header's new part compiles as strict C99 and links from C."""
import ctypes as C
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

EINVAL, ENODEV = -1, -4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("crsdr_plan_set_refcancel", "crsdr_plan_fetch_refcancel", "crsdr_plan_refcancel_buffers", "crsdr_refcancel")


@pytest.fixture(scope="module")
def b():
    binding = importlib.import_module("coherent-rtlsdr_amd.binding")
    binding.build()
    return binding


def test_symbols_declared_exported_and_bound(b):
    hdr = open(os.path.join(ROOT, "include", "crsdr.h")).read()
    declared = set(re.findall(r"\b(crsdr_[a-z0-9_]+)\s*\(", hdr))
    for s in NEW:
        assert s in declared and s in b.ABI_SYMBOLS and hasattr(b.lib(), s), s
    for s in ("set_refcancel", "fetch_refcancel", "refcancel_buffers"):
        assert callable(getattr(b.Plan, s))
    assert callable(b.refcancel) and callable(b.refcancel_device)
    assert "not its Toeplitz approximation" in hdr and "2^-40 G_00" in hdr


def test_null_plans_are_refused(b):
    L = b.lib()
    p, i = C.c_void_p(), C.c_int()
    for taps in (0, 1, 9, 4, -1):
        assert L.crsdr_plan_set_refcancel(None, taps) == EINVAL
    assert L.crsdr_plan_fetch_refcancel(None, -1, None, None, None) == EINVAL
    assert L.crsdr_plan_refcancel_buffers(None, C.byref(p), C.byref(p), C.byref(p), C.byref(i)) == EINVAL


def perop(b, rows, lag, ph, taps, flags=0, mem=None, nrows=None, B=None, out=True, skip=None):
    n, bs = rows.shape
    o, coef = np.zeros_like(rows), np.zeros((n, 9), dtype=np.complex64)
    res, st = np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.int32)
    args = dict(out=o.ctypes.data, coef=coef.ctypes.data, residual=res.ctypes.data, status=st.ctypes.data, rows=rows.ctypes.data, lag=lag.ctypes.data,
                phasor=ph.ctypes.data)
    if skip:
        args[skip] = None
    return b.lib().crsdr_refcancel(args["out"], args["coef"], args["residual"], args["status"], args["rows"], n if nrows is None else nrows,
                                   bs if B is None else B, args["lag"], args["phasor"], taps, flags, b.MEM_HOST if mem is None else mem)


def test_argument_validation_precedes_device_use(b):
    """every refusal below is CRSDR_EINVAL also on a machine without a device, where a call that went as far as the device would
    answer CRSDR_ENODEV"""
    rows = np.zeros((4, 64), dtype=np.int8)
    lag, ph = np.zeros(4, dtype=np.int32), np.ones(4, dtype=np.complex64)
    for name in ("out", "coef", "residual", "status", "rows", "lag", "phasor"):
        assert perop(b, rows, lag, ph, 3, skip=name) == EINVAL, name
    for taps in (0, 2, 4, 8, 10, 11, -1, -3):
        assert perop(b, rows, lag, ph, taps) == EINVAL, taps
    assert "taps" in b.lib().crsdr_last_error().decode()
    for B in (0, 8, 48, 100, 32768):
        assert perop(b, rows, lag, ph, 3, B=B) == EINVAL, B
    assert perop(b, rows, lag, ph, 3, nrows=1) == EINVAL
    assert perop(b, rows, lag, ph, 3, flags=b.REFNOISE_ENABLED) == EINVAL
    assert perop(b, rows, lag, ph, 3, flags=b.NO_LAG) == EINVAL
    assert perop(b, rows, lag, ph, 3, mem=7) == EINVAL
    for bad in (33, -33, 1 << 20):
        lg = lag.copy()
        lg[2] = bad
        assert perop(b, rows, lg, ph, 3) == EINVAL, bad
    lg = lag.copy()
    lg[0] = 1000                                                   # entry 0 is ignored
    lg[1], lg[2] = -32, 32                                         # both ends of the range are inside it
    rc = perop(b, rows, lg, ph, 3)
    assert rc == (0 if b.device_count() > 0 else ENODEV)
    # device pointers: alignment is an argument, too
    assert b.lib().crsdr_refcancel(1026, 1024, 1024, 1024, 2048, 4, 64, 1024, 1024, 3, 0, b.MEM_DEVICE) == EINVAL
    assert b.lib().crsdr_refcancel(4096, 1028, 1024, 1024, 2048, 4, 64, 1024, 1024, 3, 0, b.MEM_DEVICE) == EINVAL
    assert b.lib().crsdr_refcancel(2048, 1024, 1024, 1024, 2048, 4, 64, 1024, 1024, 3, 0, b.MEM_DEVICE) == EINVAL     # out == rows


def test_setter_error_codes_need_a_plan(b):
    """the setter's refusals for a faithful-mode or long-block plan and its exclusion with the fractional-delay correction are checked
    on the device (tests/test_gpu_refcancel.py): a plan cannot be made without one, and without one the library says so"""
    if b.device_count() > 0:
        plan = b.Plan(4, 1024, b.MODE_FAITHFUL)
        with pytest.raises(b.CrsdrError) as e:
            plan.set_refcancel(3)
        plan.close()
        assert e.value.code == EINVAL
        return
    with pytest.raises(b.CrsdrError) as e:
        b.Plan(4, 1024, b.MODE_DIGITAL)
    assert e.value.code == ENODEV


def test_header_part_is_plain_c99_and_links_from_c(b, tmp_path):
    so_dir = os.path.dirname(b._SO)
    exe = tmp_path / "refcancel_c99"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe),
                        os.path.join(ROOT, "tests", "c", "refcancel_c99.c"), "-L", so_dir, "-lcrsdr", f"-Wl,-rpath,{so_dir}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    for line in ("set -1", "fetch -1", "buffers -1", "taps -1", "lag -1"):
        assert line in out.stdout, out.stdout
    assert "lag[1] = 33" in out.stdout
