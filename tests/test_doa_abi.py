"""CPU checks of the batched direction-of-arrival engine's boundary (crsdr_doa, include/crsdr.h (iv)): the binding exists, bad
descriptors and bad calls are refused with CRSDR_EINVAL before any device is touched, and without a device a good descriptor gives
CRSDR_ENODEV -- never a CPU result."""
import ctypes as C
import importlib

import pytest

import ura

EINVAL, ENODEV, ESTATE = -1, -4, -5


@pytest.fixture(scope="module")
def b():
    binding = importlib.import_module("coherent-rtlsdr_amd.binding")
    binding.build()
    return binding


GOOD = dict(nrows=22, blocksize=16384, k=1, d=float(ura.D), mx=7, my=3, ncx=100, ncy=100, max_batch=64, frames=1, flags=0)


def _create(b, **over):
    d = b.Doa(**{**GOOD, **over})
    d.close()


def test_binding_names_the_new_symbols(b):
    names = {"crsdr_doa_create", "crsdr_doa_destroy", "crsdr_doa_submit", "crsdr_doa_submit_plan", "crsdr_doa_fetch",
             "crsdr_doa_device_buffers", "crsdr_doa_last_submit"}
    assert names <= set(b.ABI_SYMBOLS)
    assert all(hasattr(b.lib(), s) for s in names)
    assert b.lib().crsdr_abi_version() == 1
    assert C.sizeof(b.DoaDesc) == 48                       # ten int32, a float, a uint32: no padding to disagree about


@pytest.mark.parametrize("over", [
    dict(mx=7, my=2),                                      # m != mx * my
    dict(nrows=66, mx=13, my=5),                           # m = 65 > 64
    dict(nrows=2, mx=1, my=1),                             # m = 1
    dict(k=21), dict(k=0), dict(k=40),                     # k >= m, no signal subspace
    dict(frames=-1), dict(frames=65, max_batch=64),        # frames below 1 / beyond the batch
    dict(max_batch=65), dict(max_batch=-1),
    dict(blocksize=16400), dict(blocksize=0), dict(blocksize=16),     # blocksize % 32 != 0, below one MFMA step
    dict(ncx=0), dict(ncy=-3), dict(ncx=8192, ncy=8192),
    dict(flags=4),                                         # an unknown flag
])
def test_bad_descriptors_are_refused_before_device_use(b, over):
    # CRSDR_EINVAL whether or not a device is present: on a machine without one CRSDR_ENODEV would mean the device was asked first
    with pytest.raises(b.CrsdrError) as e:
        _create(b, **over)
    assert e.value.code == EINVAL, e.value


def test_null_arguments(b):
    L = b.lib()
    h = C.c_void_p()
    assert L.crsdr_doa_create(None, None) == EINVAL
    assert L.crsdr_doa_create(C.byref(h), None) == EINVAL
    assert L.crsdr_doa_destroy(None) == EINVAL
    assert L.crsdr_doa_submit(None, None, 0, 0, 1, None) == EINVAL
    assert L.crsdr_doa_submit_plan(None, None) == EINVAL
    assert L.crsdr_doa_fetch(None, None, None, None, None, None, None) == EINVAL
    assert L.crsdr_doa_device_buffers(None, None, None, None, None, None) == EINVAL
    assert L.crsdr_doa_last_submit(None, None, None) == EINVAL


def test_no_cpu_result_without_a_device(b):
    if b.device_count() > 0:
        # a device is here: the same descriptor gives an engine, and a call sequence error is CRSDR_ESTATE, bad counts CRSDR_EINVAL
        d = b.Doa(**{**GOOD, "frames": 4, "max_batch": 8})
        with pytest.raises(b.CrsdrError) as e:
            d.fetch()
        assert e.value.code == ESTATE
        for nblocks in (6, 0, 12):                         # not a multiple of frames, none, beyond max_batch
            with pytest.raises(b.CrsdrError) as e:
                d.submit(4096, 4096, 104, nblocks)         # refused before the pointer is looked at
            assert e.value.code == EINVAL
        d.close()
        return
    with pytest.raises(b.CrsdrError) as e:
        _create(b)
    assert e.value.code == ENODEV
    # (the submit-side checks -- nblocks % frames, alignment -- need an engine, and there is none without a device:
    # tests/test_gpu_doa.py::test_refusals covers them)
