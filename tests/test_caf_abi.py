"""CPU checks of the range-Doppler engine's boundary (crsdr_caf and crsdr_ambiguity, include/crsdr.h (w)): the binding exists, every
limit of the section and every NULL argument is refused with CRSDR_EINVAL before any device is touched, and without a device good
arguments give CRSDR_ENODEV -- never a CPU result."""
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


# the workload's shape: nd = 4 * 8192 / 128 = 256, 16 lines of 22 * 256 * 64 cells
GOOD = dict(nrows=22, blocksize=16384, seg=128, nlags=64, ref_row=0, window=1, guard=2, max_batch=64, frames=4)

# what crsdr_caf_create must refuse; the per-op call's own list (frames = max_batch = 1) is below
BAD = [
    dict(seg=8), dict(seg=8192, blocksize=16384 * 2), dict(seg=96, blocksize=192 * 64), dict(seg=0), dict(seg=-128),      # a power of two in 16 .. 4096
    dict(blocksize=16384 + 128), dict(blocksize=128), dict(blocksize=0), dict(blocksize=-512), dict(blocksize=1 << 23, frames=1, nlags=1, max_batch=1),
    dict(nrows=1), dict(nrows=0), dict(nrows=-3),
    dict(ref_row=-1), dict(ref_row=22),
    dict(nlags=0), dict(nlags=-1), dict(nlags=129),                                # beyond seg
    dict(nlags=1025, seg=2048, frames=8, nrows=2, max_batch=8),                    # beyond 1024 (nd = 32)
    dict(frames=-1), dict(frames=65, max_batch=64), dict(frames=3, max_batch=2), dict(max_batch=65), dict(max_batch=-1),
    dict(frames=3, max_batch=63),                                                  # nd = 192 is no power of two
    dict(frames=1, seg=4096, max_batch=1),                                         # nd = 2 < 8
    dict(frames=16, seg=16, nlags=1, max_batch=16, nrows=2),                       # nd = 8192 > 4096
    dict(nrows=65),                                                                # 16 lines * 65 * 256 * 64 > 2^24 cells
    dict(nrows=1025, max_batch=4),                                                 # one line: 2^24 + 2^14 cells
    dict(window=2), dict(window=-1),
    dict(guard=-1), dict(guard=129),                                               # beyond nd / 2
]


def test_binding_names_the_new_symbols(b):
    names = {"crsdr_caf_create", "crsdr_caf_destroy", "crsdr_caf_submit", "crsdr_caf_submit_plan", "crsdr_caf_fetch", "crsdr_caf_device_buffers",
             "crsdr_caf_last_submit", "crsdr_ambiguity"}
    assert names <= set(b.ABI_SYMBOLS)
    assert all(hasattr(b.lib(), s) for s in names)
    assert C.sizeof(b.CafDesc) == 40                       # ten int32: no padding to disagree about


@pytest.mark.parametrize("over", BAD)
def test_bad_descriptors_are_refused_before_device_use(b, over):
    # CRSDR_EINVAL whether or not a device is present: on a machine without one CRSDR_ENODEV would mean the device was asked first
    with pytest.raises(b.CrsdrError) as e:
        b.Caf(**{**GOOD, **over}).close()
    assert e.value.code == EINVAL, e.value


@pytest.mark.parametrize("over", [dict(nrows=1024, max_batch=4), dict(nrows=64), dict(guard=128), dict(guard=0), dict(nlags=128), dict(frames=0, max_batch=0, seg=16, nlags=16, nrows=2),
                                  dict(ref_row=21), dict(seg=4096, frames=4, max_batch=4, blocksize=16384, nlags=1024, guard=4)])
def test_the_limits_themselves_are_accepted(b, over):
    # at a limit, not beyond it: a device is then the only thing that can be missing
    if b.device_count() > 0:
        b.Caf(**{**GOOD, **over}).close()
        return
    with pytest.raises(b.CrsdrError) as e:
        b.Caf(**{**GOOD, **over}).close()
    assert e.value.code == ENODEV, e.value


def _ambiguity(b, nrows=3, blocksize=2048, seg=64, nlags=16, ref_row=1, window=1, guard=2, mem_kind=0, outputs=True):
    nd = max(blocksize, 1) // (2 * max(seg, 1)) + 1
    m = np.zeros(max(nrows, 1) * max(blocksize, 1), dtype=np.int8)
    n = max(nrows, 1) * nd * max(nlags, 1)
    chi, mp, pk = np.zeros(2 * n, dtype=np.float32), np.zeros(n, dtype=np.float32), np.zeros(6 * (max(nrows, 1) + 1), dtype=np.float32)
    f = lambda a: b._p(a, C.c_float) if outputs else None
    return b.lib().crsdr_ambiguity(f(chi), f(mp), f(pk), b._p(m, C.c_int8), nrows, blocksize, seg, nlags, ref_row, window, guard, mem_kind)


@pytest.mark.parametrize("over", [
    dict(seg=8), dict(seg=8192, blocksize=16384 * 16), dict(seg=96, blocksize=192 * 16), dict(seg=0), dict(seg=-64),
    dict(blocksize=2048 + 64), dict(blocksize=64), dict(blocksize=0), dict(blocksize=-512),
    dict(nrows=1), dict(nrows=0), dict(nrows=-3),
    dict(ref_row=-1), dict(ref_row=3),
    dict(nlags=0), dict(nlags=65),
    dict(seg=256),                                         # nd = 4 < 8
    dict(blocksize=3 * 1024),                              # nd = 24 is no power of two
    dict(seg=16, blocksize=1 << 18, nlags=1),              # nd = 8192
    dict(window=2), dict(window=-1),
    dict(guard=-1), dict(guard=9),
    dict(mem_kind=2), dict(mem_kind=-1),
    dict(outputs=False),                                   # nothing asked for
])
def test_bad_ambiguity_arguments_are_refused_before_device_use(b, over):
    assert _ambiguity(b, **over) == EINVAL, (over, b.lib().crsdr_last_error())


def test_ambiguity_refuses_more_than_2_24_cells(b):
    # (no large matrix for a call that must fail on its counts: the pointers are never followed)
    one = np.zeros(16, dtype=np.float32)
    rc = b.lib().crsdr_ambiguity(b._p(one, C.c_float), None, None, C.cast(b._p(one, C.c_float), C.POINTER(C.c_int8)), 4097, 16384, 16, 8, 0, 0, 0, 0)
    assert rc == EINVAL                                    # 4097 * 512 * 8 > 2^24


def test_null_arguments(b):
    L = b.lib()
    h = C.c_void_p()
    assert L.crsdr_caf_create(None, None) == EINVAL
    assert L.crsdr_caf_create(C.byref(h), None) == EINVAL
    assert L.crsdr_caf_create(None, C.byref(b.CafDesc(22, 16384, 0, 64, 4, 128, 64, 0, 1, 2))) == EINVAL
    assert L.crsdr_caf_destroy(None) == EINVAL
    assert L.crsdr_caf_submit(None, None, 0, 0, 1, None) == EINVAL
    assert L.crsdr_caf_submit_plan(None, None) == EINVAL
    assert L.crsdr_caf_fetch(None, None, None, None) == EINVAL
    assert L.crsdr_caf_device_buffers(None, None, None, None) == EINVAL
    assert L.crsdr_caf_last_submit(None, None, None) == EINVAL
    one = np.zeros(4, dtype=np.float32)
    assert L.crsdr_ambiguity(b._p(one, C.c_float), None, None, None, 3, 2048, 64, 16, 0, 0, 0, 0) == EINVAL


def test_no_cpu_result_without_a_device(b):
    if b.device_count() > 0:
        # a device is here: the same descriptor gives an engine, and a call sequence error is CRSDR_ESTATE, bad counts CRSDR_EINVAL
        s = b.Caf(**GOOD)
        with pytest.raises(b.CrsdrError) as e:
            s.fetch()
        assert e.value.code == ESTATE
        for nblocks in (6, 0, 68):                         # not a multiple of frames, none, beyond max_batch
            with pytest.raises(b.CrsdrError) as e:
                s.submit(4096, 22 * 16384, 104, nblocks)   # refused before the pointer is looked at
            assert e.value.code == EINVAL
        s.close()
        return
    with pytest.raises(b.CrsdrError) as e:
        b.Caf(**GOOD).close()
    assert e.value.code == ENODEV
    assert _ambiguity(b) == ENODEV
