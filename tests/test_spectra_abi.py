"""CPU checks of the spectra engine's boundary (crsdr_spectra and crsdr_welch, include/crsdr.h (v)): the binding exists, bad
descriptors and bad calls are refused with CRSDR_EINVAL before any device is touched, and without a device good arguments give
CRSDR_ENODEV -- never a CPU result."""
import ctypes as C
import importlib

import numpy as np
import pytest

EINVAL, ENODEV, ESTATE = -1, -4, -5


@pytest.fixture(scope="module")
def b():
    binding = importlib.import_module("coherent-rtlsdr_amd.binding")
    binding.build()
    return binding


GOOD = dict(nrows=22, blocksize=16384, nfft=256, overlap=1, window=1, band=(-25, 25), max_batch=64, frames=1)

# descriptors whose transform, rows, window or band crsdr_spectra_create must refuse (the per-op call's own list is below)
BAD_SHAPES = [
    dict(nfft=8), dict(nfft=8192, blocksize=16384), dict(nfft=96, blocksize=192 * 4), dict(nfft=0), dict(nfft=-256),      # not a power of two in 16 .. 4096
    dict(blocksize=16384 + 256), dict(blocksize=256), dict(blocksize=0), dict(blocksize=-512),                             # blocksize % (2 nfft), none
    dict(nrows=1), dict(nrows=0), dict(nrows=-3),
    dict(overlap=2), dict(overlap=-1),
    dict(window=2), dict(window=-1),
    dict(band=(-129, 25)), dict(band=(-25, 128)), dict(band=(5, 5)), dict(band=(6, 5)), dict(band=(-128, 128)),            # outside the bins, K < 2
]


def test_binding_names_the_new_symbols(b):
    names = {"crsdr_spectra_create", "crsdr_spectra_destroy", "crsdr_spectra_submit", "crsdr_spectra_submit_plan", "crsdr_spectra_fetch",
             "crsdr_spectra_device_buffers", "crsdr_spectra_last_submit", "crsdr_welch"}
    assert names <= set(b.ABI_SYMBOLS)
    assert all(hasattr(b.lib(), s) for s in names)
    assert C.sizeof(b.SpectraDesc) == 40                   # ten int32: no padding to disagree about


@pytest.mark.parametrize("over", BAD_SHAPES + [
    dict(frames=-1), dict(frames=65, max_batch=64), dict(frames=3, max_batch=2),
    dict(max_batch=65), dict(max_batch=-1),
    dict(nrows=65537, nfft=256, max_batch=64),             # 64 * 65537 * 256 > 2^24 points
    dict(nrows=4097, nfft=4096, max_batch=1),
])
def test_bad_descriptors_are_refused_before_device_use(b, over):
    # CRSDR_EINVAL whether or not a device is present: on a machine without one CRSDR_ENODEV would mean the device was asked first
    with pytest.raises(b.CrsdrError) as e:
        b.Spectra(**{**GOOD, **over}).close()
    assert e.value.code == EINVAL, e.value


def _welch(b, nrows=3, blocksize=1024, nfft=64, overlap=1, window=1, band=(-6, 6), mem_kind=0, outputs=True):
    n = max(nrows, 1) * max(nfft, 1)
    m = np.zeros(max(nrows, 1) * max(blocksize, 1), dtype=np.int8)
    psd, cross, al = np.zeros(n, dtype=np.float32), np.zeros(2 * n, dtype=np.float32), np.zeros(4 * max(nrows, 1), dtype=np.float32)
    f = lambda a: b._p(a, C.c_float) if outputs else None
    return b.lib().crsdr_welch(f(psd), f(cross), f(al), b._p(m, C.c_int8), nrows, blocksize, nfft, overlap, window, band[0], band[1], mem_kind)


@pytest.mark.parametrize("over", [
    dict(nfft=8, blocksize=1024), dict(nfft=8192, blocksize=16384), dict(nfft=96, blocksize=768), dict(nfft=0), dict(nfft=-64),
    dict(blocksize=1024 + 64), dict(blocksize=64), dict(blocksize=0), dict(blocksize=-512),
    dict(nrows=1), dict(nrows=0), dict(nrows=-3),
    dict(overlap=2), dict(overlap=-1),
    dict(window=2), dict(window=-1),
    dict(band=(-33, 6)), dict(band=(-6, 32)), dict(band=(5, 5)), dict(band=(6, 5)),
    dict(mem_kind=2), dict(mem_kind=-1),
    dict(outputs=False),                                   # nothing asked for
])
def test_bad_welch_arguments_are_refused_before_device_use(b, over):
    assert _welch(b, **over) == EINVAL, (over, b.lib().crsdr_last_error())


def test_welch_refuses_more_than_2_24_points(b):
    # (no 64 MiB matrix for a call that must fail on its counts: the pointers are never followed)
    one = np.zeros(16, dtype=np.float32)
    rc = b.lib().crsdr_welch(b._p(one, C.c_float), None, None, C.cast(b._p(one, C.c_float), C.POINTER(C.c_int8)), 4097, 8192, 4096, 0, 0, -6, 6, 0)
    assert rc == EINVAL


def test_null_arguments(b):
    L = b.lib()
    h = C.c_void_p()
    assert L.crsdr_spectra_create(None, None) == EINVAL
    assert L.crsdr_spectra_create(C.byref(h), None) == EINVAL
    assert L.crsdr_spectra_destroy(None) == EINVAL
    assert L.crsdr_spectra_submit(None, None, 0, 0, 1, None) == EINVAL
    assert L.crsdr_spectra_submit_plan(None, None) == EINVAL
    assert L.crsdr_spectra_fetch(None, None, None, None) == EINVAL
    assert L.crsdr_spectra_device_buffers(None, None, None, None) == EINVAL
    assert L.crsdr_spectra_last_submit(None, None, None) == EINVAL
    one = np.zeros(4, dtype=np.float32)
    assert L.crsdr_welch(b._p(one, C.c_float), None, None, None, 3, 1024, 64, 0, 0, -6, 6, 0) == EINVAL


def test_no_cpu_result_without_a_device(b):
    if b.device_count() > 0:
        # a device is here: the same descriptor gives an engine, and a call sequence error is CRSDR_ESTATE, bad counts CRSDR_EINVAL
        s = b.Spectra(**{**GOOD, "frames": 4, "max_batch": 8})
        with pytest.raises(b.CrsdrError) as e:
            s.fetch()
        assert e.value.code == ESTATE
        for nblocks in (6, 0, 12):                         # not a multiple of frames, none, beyond max_batch
            with pytest.raises(b.CrsdrError) as e:
                s.submit(4096, 22 * 16384, 104, nblocks)   # refused before the pointer is looked at
            assert e.value.code == EINVAL
        s.close()
        return
    with pytest.raises(b.CrsdrError) as e:
        b.Spectra(**GOOD).close()
    assert e.value.code == ENODEV
    assert _welch(b) == ENODEV
