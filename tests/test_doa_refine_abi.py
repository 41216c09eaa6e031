"""CPU checks of the refinement off the scan grid (include/crsdr.h: crsdr_doa_set_refine, crsdr_doa_fetch_refined,
crsdr_doa_refined_buffers, crsdr_refine2d): the symbols are declared, exported and bound, arguments outside the limits are refused before
any device use, and the C++ host layer (cbeamformer.h: batch::set_refine and the refined_* vectors) compiles and links with the new
members."""
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
NEW = ("crsdr_doa_set_refine", "crsdr_doa_fetch_refined", "crsdr_doa_refined_buffers", "crsdr_refine2d")


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
    for name in ("set_refine", "fetch_refined", "refined_buffers", "refine2d"):
        assert callable(getattr(b.Doa, name)), name
    assert callable(b.refine2d)
    assert b.lib().crsdr_abi_version() == 1


def test_bad_arguments_are_refused_before_any_device_use(b):
    L = b.lib()
    for levels in (0, 1, 5, 8, 9, -1):
        assert L.crsdr_doa_set_refine(None, levels) == EINVAL
    assert L.crsdr_doa_fetch_refined(None, None, None, None) == EINVAL
    assert L.crsdr_doa_refined_buffers(None, None, None, None, None) == EINVAL
    m, mx, my, ncx, ncy, n = 6, 3, 2, 10, 7, 2
    vec = np.eye(m, dtype=np.complex64)
    sv = np.ones(m, dtype=np.float32)
    off, ang, val = np.zeros((n, 2), dtype=np.float32), np.zeros((n, 2), dtype=np.float32), np.zeros(n, dtype=np.float32)
    peaks = np.array([[3, 4], [5, 1]], dtype=np.int32)
    f32p, i32p = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    good = dict(offsets=off.ctypes.data_as(f32p), angles=ang.ctypes.data_as(f32p), values=val.ctypes.data_as(f32p),
                vec=vec.view(np.float32).ctypes.data_as(f32p), sv=sv.ctypes.data_as(f32p), m=m, kind=b.SPECTRUM_MUSIC, k=1, loading=1e-2, d=0.5, mx=mx, my=my,
                ncx=ncx, ncy=ncy, peaks=peaks.ctypes.data_as(i32p), npeaks=n, levels=5, mem_kind=b.MEM_HOST)
    call = lambda **kw: L.crsdr_refine2d(*[{**good, **kw}[k] for k in good])
    bad = {
        "NULL offsets": dict(offsets=None), "NULL angles": dict(angles=None), "NULL values": dict(values=None), "NULL vec": dict(vec=None),
        "NULL sv": dict(sv=None), "NULL peaks": dict(peaks=None),
        "kind 3": dict(kind=3), "kind -1": dict(kind=-1),
        "MUSIC k = 0": dict(k=0), "MUSIC k = m": dict(k=m), "MUSIC k negative": dict(k=-2),
        "CAPON loading below 1e-6": dict(kind=b.SPECTRUM_CAPON, loading=5e-7), "CAPON loading above 1": dict(kind=b.SPECTRUM_CAPON, loading=1.5),
        "CAPON loading NaN": dict(kind=b.SPECTRUM_CAPON, loading=float("nan")), "CAPON loading 0": dict(kind=b.SPECTRUM_CAPON, loading=0.0),
        "m = 1": dict(m=1, mx=1, my=1), "m = 65": dict(m=65, mx=65, my=1), "m is not mx my": dict(mx=2, my=2),
        "mx = 0": dict(mx=0), "my negative": dict(my=-2, mx=-3), "no grid": dict(ncx=0), "ncy negative": dict(ncy=-1),
        "grid above 2^24 points": dict(ncx=4097, ncy=4096),
        "npeaks = 0": dict(npeaks=0), "npeaks = 17": dict(npeaks=17), "npeaks negative": dict(npeaks=-1),
        "levels = 0": dict(levels=0), "levels = 9": dict(levels=9), "levels negative": dict(levels=-3),
        "mem_kind": dict(mem_kind=7),
    }
    for what, kw in bad.items():
        assert call(**kw) == EINVAL, what
        assert b.lib().crsdr_last_error()
    # the maps ignore k, MUSIC and BARTLETT the loading: out of the others' range is no error.  What is left to fail is the device
    if b.device_count() < 1:
        assert call() == ENODEV
        assert call(kind=b.SPECTRUM_BARTLETT, k=0, loading=0.0) == ENODEV and call(kind=b.SPECTRUM_CAPON, k=99, loading=1e-6) == ENODEV
        assert call(loading=7.0) == ENODEV and call(k=m - 1) == ENODEV
        assert call(levels=1) == ENODEV and call(levels=8) == ENODEV and call(npeaks=1) == ENODEV


def test_host_layer_compiles_with_the_new_members(b, tmp_path):
    """cbeamformer.h's new members are declared as the issue gives them, defined in cbeamformer.cc and used by coherent_demo."""
    subprocess.run(["make", "-C", HOST, "all", "libcsynth.so"], check=True, stdout=subprocess.DEVNULL)
    src = tmp_path / "use.cc"
    src.write_text('#include "cbeamformer.h"\n'
                   "int (cbeamformer::batch::*g)(int) = &cbeamformer::batch::set_refine;\n"
                   "std::vector<float> cbeamformer::batch::*v[3] = {&cbeamformer::batch::refined_offsets, &cbeamformer::batch::refined_angles,\n"
                   "                                               &cbeamformer::batch::refined_values};\n"
                   "int main() { return g && v[0] && v[1] && v[2] && crsdr_doa_set_refine(nullptr, 5) == CRSDR_EINVAL ? 0 : 1; }\n")
    exe = tmp_path / "use"
    lib = os.path.dirname(b.build())
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", HOST, "-o", str(exe), str(src), os.path.join(HOST, "cbeamformer.cc"), "-L", lib, "-lcrsdr",
                    f"-Wl,-rpath,{lib}"], check=True)
    # a NULL object is refused before a device is looked for: the program runs anywhere
    assert subprocess.run([str(exe)], timeout=60).returncode == 0
    demo = open(os.path.join(HOST, "coherent_demo.cc")).read()
    assert "--refine" in demo and "set_refine" in demo and "refined_angles" in demo
