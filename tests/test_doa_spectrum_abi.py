"""CPU checks of the power maps of crsdr_doa (include/crsdr.h: crsdr_doa_set_spectrum, crsdr_spectrum2d): the symbols are declared,
exported and bound, arguments outside the limits are refused before any device use, and the C++ host layer (cbeamformer.h:
pspectrum2dvec, batch::set_spectrum) compiles and links with the new members."""
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
NEW = ("crsdr_doa_set_spectrum", "crsdr_spectrum2d")


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
    assert callable(b.Doa.set_spectrum) and callable(b.spectrum2d)
    for name, value in (("MUSIC", 0), ("BARTLETT", 1), ("CAPON", 2)):
        assert getattr(b, "SPECTRUM_" + name) == value
        assert re.search(rf"CRSDR_SPECTRUM_{name} = {value}\b", hdr)
    assert b.lib().crsdr_abi_version() == 1


def test_error_codes_are_the_headers(b):
    hdr = open(os.path.join(ROOT, "include", "crsdr.h")).read()
    assert re.search(r"CRSDR_EINVAL\s*=\s*-1\b", hdr) and re.search(r"CRSDR_ENODEV\s*=\s*-4\b", hdr)


def test_bad_arguments_are_refused_before_any_device_use(b):
    L = b.lib()
    assert L.crsdr_doa_set_spectrum(None, b.SPECTRUM_CAPON, 1e-2) == EINVAL
    assert L.crsdr_doa_set_spectrum(None, b.SPECTRUM_MUSIC, 0.0) == EINVAL
    m, mx, my, ncx, ncy = 6, 3, 2, 10, 7
    vec = np.eye(m, dtype=np.complex64)
    sv = np.ones(m, dtype=np.float32)
    pm = np.zeros((ncx, ncy), dtype=np.float32)
    f32p = C.POINTER(C.c_float)
    P, V, S = pm.ctypes.data_as(f32p), vec.view(np.float32).ctypes.data_as(f32p), sv.ctypes.data_as(f32p)
    good = dict(pm=P, vec=V, sv=S, m=m, kind=b.SPECTRUM_CAPON, loading=1e-2, d=0.5, mx=mx, my=my, ncx=ncx, ncy=ncy, mem_kind=b.MEM_HOST)
    call = lambda **kw: L.crsdr_spectrum2d(*[{**good, **kw}[k] for k in good])
    bad = {
        "NULL pm": dict(pm=None), "NULL vec": dict(vec=None), "NULL sv": dict(sv=None),
        "MUSIC is crsdr_pmusic2d": dict(kind=b.SPECTRUM_MUSIC), "kind 3": dict(kind=3), "kind -1": dict(kind=-1),
        "loading below 1e-6": dict(loading=5e-7), "loading above 1": dict(loading=1.5), "loading 0": dict(loading=0.0),
        "loading NaN": dict(loading=float("nan")), "loading negative": dict(loading=-1e-2),
        "m = 1": dict(m=1, mx=1, my=1), "m = 65": dict(m=65, mx=65, my=1), "m is not mx my": dict(mx=2, my=2),
        "mx = 0": dict(mx=0), "my negative": dict(my=-2, mx=-3), "no grid": dict(ncx=0), "ncy negative": dict(ncy=-1),
        "grid above 2^24 points": dict(ncx=4097, ncy=4096), "mem_kind": dict(mem_kind=7),
    }
    for what, kw in bad.items():
        assert call(**kw) == EINVAL, what
        assert b.lib().crsdr_last_error()
    # BARTLETT ignores the loading: out of CAPON's range is no error.  What is left to fail is the device
    if b.device_count() < 1:
        assert call() == ENODEV
        assert call(kind=b.SPECTRUM_BARTLETT, loading=0.0) == ENODEV
        assert call(loading=1e-6) == ENODEV and call(loading=1.0) == ENODEV
        assert call(m=2, mx=2, my=1) == ENODEV and call(m=2, mx=1, my=2) == ENODEV


def test_host_layer_compiles_with_the_new_members(b, tmp_path):
    """cbeamformer.h's new members are declared as the issue gives them, defined in cbeamformer.cc and used by coherent_demo."""
    subprocess.run(["make", "-C", HOST, "all", "libcsynth.so"], check=True, stdout=subprocess.DEVNULL)
    src = tmp_path / "use.cc"
    src.write_text('#include "cbeamformer.h"\n'
                   "int (*f)(const cmatrix &, const std::vector<float> &, int, int, float, float, int, int, int, int, std::vector<float> &) = cbeamformer::pspectrum2dvec;\n"
                   "int (cbeamformer::batch::*g)(int, float) = &cbeamformer::batch::set_spectrum;\n"
                   "int main() { cmatrix U(4); std::vector<float> S(2), pm; return f(U, S, 2, CRSDR_SPECTRUM_MUSIC, 0.f, 0.5f, 2, 1, 3, 3, pm) == CRSDR_EINVAL && g ? 0 : 1; }\n")
    exe = tmp_path / "use"
    lib = os.path.dirname(b.build())
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", HOST, "-o", str(exe), str(src), os.path.join(HOST, "cbeamformer.cc"), "-L", lib, "-lcrsdr",
                    f"-Wl,-rpath,{lib}"], check=True)
    # MUSIC is refused by the per-op call before a device is looked for: the program runs anywhere
    assert subprocess.run([str(exe)], timeout=60).returncode == 0
    demo = open(os.path.join(HOST, "coherent_demo.cc")).read()
    assert "--spectrum" in demo and "set_spectrum" in demo
