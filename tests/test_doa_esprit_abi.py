"""CPU checks of the gridless directions' ABI (include/crsdr.h: crsdr_doa_set_esprit, crsdr_doa_fetch_esprit, crsdr_doa_esprit_buffers,
crsdr_esprit2d): the symbols are declared, exported and bound, every bad argument of the per-op call is refused before any device use,
and the C++ host layer (cbeamformer.h: batch::set_esprit and the esprit_* vectors) compiles and links with the new members."""
import ctypes as C
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

EINVAL, ENODEV = -1, -4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "coherent-rtlsdr_amd", "host")
NEW = ("crsdr_doa_set_esprit", "crsdr_doa_fetch_esprit", "crsdr_doa_esprit_buffers", "crsdr_esprit2d")


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
    for name, value in (("CRSDR_ESPRIT_OFF", 0), ("CRSDR_ESPRIT_BESIDE", 1), ("CRSDR_ESPRIT_ONLY", 2)):
        assert re.search(rf"\b{name} = {value}\b", hdr), name
    assert (b.ESPRIT_OFF, b.ESPRIT_BESIDE, b.ESPRIT_ONLY) == (0, 1, 2)
    for name in ("set_esprit", "fetch_esprit", "esprit_buffers", "esprit2d"):
        assert callable(getattr(b.Doa, name)), name
    assert callable(b.esprit2d)
    assert b.lib().crsdr_abi_version() == 1
    # the kernel is its own header, included behind the other kernel headers
    src = open(os.path.join(ROOT, "coherent-rtlsdr_amd", "csrc", "crsdr.hip")).read()
    assert src.index('#include "refine.hpp"') < src.index('#include "esprit.hpp"') < src.index('#include "doa_engine.hpp"')
    kern = open(os.path.join(ROOT, "coherent-rtlsdr_amd", "csrc", "esprit.hpp")).read()
    assert "esprit2d_matrix" in kern and "k_esprit2d" in kern and "k_doa_esprit" in kern and "asm" not in kern


def test_bad_arguments_are_refused_before_any_device_use(b):
    L = b.lib()
    for mode in (0, 1, 2, 3, -1):
        assert L.crsdr_doa_set_esprit(None, mode) == EINVAL
    assert L.crsdr_doa_fetch_esprit(None, None, None, None, None, None, None, None) == EINVAL
    assert L.crsdr_doa_esprit_buffers(None, None, None, None, None, None, None, None, None) == EINVAL
    m, mx, my, k = 6, 3, 2, 2
    vec = np.eye(m, dtype=np.complex64)
    sv = np.ones(m, dtype=np.float32)
    found, status = np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32)
    ph, ang, mod = np.zeros((16, 2)), np.zeros((16, 2), dtype=np.float32), np.zeros((16, 2), dtype=np.float32)
    pw, fl = np.zeros(16, dtype=np.float32), np.zeros(16, dtype=np.int32)
    f32p, f64p, i32p = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int32)
    good = dict(found=found.ctypes.data_as(i32p), status=status.ctypes.data_as(i32p), phases=ph.ctypes.data_as(f64p), angles=ang.ctypes.data_as(f32p),
                modulus=mod.ctypes.data_as(f32p), power=pw.ctypes.data_as(f32p), flags=fl.ctypes.data_as(i32p), vec=vec.view(np.float32).ctypes.data_as(f32p),
                sv=sv.ctypes.data_as(f32p), m=m, k=k, d=0.5, mx=mx, my=my, mem_kind=b.MEM_HOST)
    call = lambda **kw: L.crsdr_esprit2d(*[{**good, **kw}[key] for key in good])
    bad = {
        "NULL found": dict(found=None), "NULL status": dict(status=None), "NULL phases": dict(phases=None), "NULL angles": dict(angles=None),
        "NULL modulus": dict(modulus=None), "NULL power": dict(power=None), "NULL flags": dict(flags=None), "NULL vec": dict(vec=None), "NULL sv": dict(sv=None),
        "m is not mx my": dict(mx=2, my=2), "m = 7": dict(m=7), "m = 65 as 13 x 5": dict(m=65, mx=13, my=5), "m = 72": dict(m=72, mx=9, my=8),
        "mx = 1": dict(mx=1, my=6), "my = 1": dict(mx=6, my=1), "mx = 0": dict(mx=0), "my negative": dict(mx=-3, my=-2),
        "k = 0": dict(k=0), "k negative": dict(k=-1), "k = 17": dict(m=64, mx=8, my=8, k=17), "k above the rank limit of 3 x 2": dict(k=4),
        "k above the rank limit of 2 x 2": dict(m=4, mx=2, my=2, k=3), "k above the rank limit of 2 x 5": dict(m=10, mx=2, my=5, k=6),
        "mem_kind": dict(mem_kind=7), "mem_kind negative": dict(mem_kind=-1),
    }
    for what, kw in bad.items():
        assert call(**kw) == EINVAL, what
        assert b.lib().crsdr_last_error()
    # what is left to fail is the device
    if b.device_count() < 1:
        assert call() == ENODEV
        assert call(k=1) == ENODEV and call(k=3) == ENODEV                  # 3 x 2: the rank limit itself
        assert call(m=4, mx=2, my=2, k=2) == ENODEV and call(m=10, mx=2, my=5, k=5) == ENODEV and call(d=1.5) == ENODEV
    with pytest.raises(ValueError):
        b.esprit2d(np.zeros((6, 5)), sv, 1, 0.5, 3, 2)


def test_host_layer_compiles_with_the_new_member(b, tmp_path):
    """cbeamformer.h's new members are declared, defined in cbeamformer.cc and used by coherent_demo."""
    subprocess.run(["make", "-C", HOST, "all", "libcsynth.so"], check=True, stdout=subprocess.DEVNULL)
    src = tmp_path / "use.cc"
    src.write_text('#include "cbeamformer.h"\n'
                   "int (cbeamformer::batch::*g)(int) = &cbeamformer::batch::set_esprit;\n"
                   "int (cbeamformer::batch::*n)() const = &cbeamformer::batch::esprit_slots;\n"
                   "std::vector<float> cbeamformer::batch::*v[3] = {&cbeamformer::batch::esprit_angles, &cbeamformer::batch::esprit_modulus,\n"
                   "                                               &cbeamformer::batch::esprit_power};\n"
                   "std::vector<double> cbeamformer::batch::*p = &cbeamformer::batch::esprit_phases;\n"
                   "std::vector<int32_t> cbeamformer::batch::*f[3] = {&cbeamformer::batch::esprit_found, &cbeamformer::batch::esprit_status,\n"
                   "                                                 &cbeamformer::batch::esprit_flags};\n"
                   "int main() { return g && n && v[0] && v[1] && v[2] && p && f[0] && f[1] && f[2] && crsdr_doa_set_esprit(nullptr, CRSDR_ESPRIT_ONLY) == CRSDR_EINVAL ? 0 : 1; }\n")
    exe = tmp_path / "use"
    lib = os.path.dirname(b.build())
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", HOST, "-o", str(exe), str(src), os.path.join(HOST, "cbeamformer.cc"), "-L", lib, "-lcrsdr",
                    f"-Wl,-rpath,{lib}"], check=True)
    # a NULL object is refused before a device is looked for: the program runs anywhere
    assert subprocess.run([str(exe)], timeout=60).returncode == 0
    demo = open(os.path.join(HOST, "coherent_demo.cc")).read()
    assert "--esprit" in demo and "set_esprit" in demo and "esprit_angles" in demo
