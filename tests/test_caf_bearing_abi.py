"""CPU checks of the bearings' boundary (crsdr_caf_set_bearing, crsdr_caf_fetch_bearing, crsdr_caf_bearing_device_buffers, crsdr_bearing;
include/crsdr.h (w), "Bearings"): the binding exists, every limit of the section and every NULL argument is refused with CRSDR_EINVAL
before any device is touched, and without a device good arguments give CRSDR_ENODEV -- never a CPU result.  With a device the two
CRSDR_ESTATE rules are held as well."""
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


CFAR = dict(gd=1, gr=1, td=2, tr=3, alpha=8.0, min_train=1, max_det=4)
GOOD = dict(mx=3, my=2, d=0.5, ncx=16, ncy=16, mode=2, loading=1e-2, levels=3, flags=0)
# what the one function behind crsdr_caf_set_bearing and crsdr_bearing must refuse, at nrows = 7
BAD = [
    dict(mx=0), dict(my=0), dict(mx=-3, my=-2),
    dict(mx=2), dict(mx=3, my=3), dict(mx=6, my=1, nrows=8), dict(mx=1, my=1, nrows=2), dict(mx=13, my=5, nrows=66), dict(mx=2 ** 16, my=2 ** 16),
    dict(ncx=1), dict(ncy=1), dict(ncx=513), dict(ncy=1024), dict(ncx=0), dict(ncy=-16),
    dict(d=0.0), dict(d=-0.5), dict(d=float("inf")), dict(d=float("nan")),
    dict(mode=0), dict(mode=3), dict(mode=-1),
    dict(loading=0.0), dict(loading=9e-7), dict(loading=1.001), dict(loading=float("nan")),
    dict(levels=-1), dict(levels=9),
    dict(flags=2), dict(flags=0x80000001),
]


def _bearing(b, nrows=7, nd=16, R=8, ref_row=0, guard=1, mem_kind=0, dir_=True, spec=False, chi=True, det=True, count=True, cfar=True, desc=True, **over):
    cf = b.cfar_desc(**{**CFAR, **{k: v for k, v in over.items() if k in CFAR}})
    bd = b.bearing_desc(**{**GOOD, **{k: v for k, v in over.items() if k in GOOD}})
    K = min(max(cf.max_det, 1), 64)
    npts = min(max(bd.ncx, 1), 512) * min(max(bd.ncy, 1), 512)
    out, sp = np.zeros(K * 8, dtype=np.float32), np.zeros(K * npts, dtype=np.float32)
    a = np.zeros(max(nrows, 1) * max(nd, 1) * max(R, 1) * 2, dtype=np.float32)
    dt, n = np.zeros(K * 8, dtype=np.float32), np.zeros(1, dtype=np.int32)
    return b.lib().crsdr_bearing(b._p(out, C.c_float) if dir_ else None, b._p(sp, C.c_float) if spec else None, b._p(a, C.c_float) if chi else None, nrows, nd, R, ref_row,
                                 guard, b._p(dt, C.c_float) if det else None, b._p(n, C.c_int32) if count else None, C.byref(cf) if cfar else None,
                                 C.byref(bd) if desc else None, mem_kind)


def test_binding_names_the_new_symbols(b):
    names = {"crsdr_caf_set_bearing", "crsdr_caf_fetch_bearing", "crsdr_caf_bearing_device_buffers", "crsdr_bearing"}
    assert names <= set(b.ABI_SYMBOLS)
    assert all(hasattr(b.lib(), s) for s in names)
    assert C.sizeof(b.BearingDesc) == 36                   # six int32, two floats and a uint32: no padding to disagree about
    assert (b.BEARING_CONVENTIONAL, b.BEARING_ADAPTIVE, b.BEARING_KEEP_SPECTRUM) == (1, 2, 1)


@pytest.mark.parametrize("over", BAD, ids=[str(o) for o in BAD])
def test_bad_descriptors_are_refused_before_device_use(b, over):
    # CRSDR_EINVAL whether or not a device is present: on a machine without one CRSDR_ENODEV would mean the device was asked first
    assert _bearing(b, **over) == EINVAL, (over, b.lib().crsdr_last_error())


def test_the_kept_spectrum_has_its_limit_in_the_engine(b):
    # K * ncx * ncy = 64 * 2^18 = 2^24 is the limit for one line; the engine multiplies by its lines (with a device: below)
    over = dict(flags=1, ncx=512, ncy=512, max_det=64, mx=8, my=8, nrows=65, nd=8, R=2, guard=0, td=1, tr=1)
    assert _bearing(b, spec=True, **over) == (0 if b.device_count() > 0 else ENODEV), b.lib().crsdr_last_error()


@pytest.mark.parametrize("over", [dict(nd=12), dict(nd=4), dict(nd=8192), dict(nd=0), dict(R=0), dict(R=1025), dict(guard=-1), dict(guard=9), dict(ref_row=-1),
                                  dict(ref_row=7), dict(nrows=1, mx=1, my=1), dict(mem_kind=2), dict(mem_kind=-1), dict(dir_=False), dict(chi=False), dict(det=False),
                                  dict(count=False), dict(cfar=False), dict(desc=False), dict(spec=True), dict(max_det=0), dict(max_det=65), dict(gd=5, td=4),
                                  dict(nd=8, td=3), dict(alpha=0.0)])
def test_bad_bearing_arguments_are_refused_before_device_use(b, over):
    # (spec without the keep flag; the detector's own limits, through the one function crsdr_cfar has)
    assert _bearing(b, **over) == EINVAL, (over, b.lib().crsdr_last_error())


@pytest.mark.parametrize("over", [dict(mx=2, my=1, nrows=3), dict(mx=1, my=2, nrows=3), dict(mx=64, my=1, nrows=65, nd=8, R=4), dict(mx=8, my=8, nrows=65, nd=8, R=4),
                                  dict(ncx=2, ncy=2), dict(ncx=512, ncy=2), dict(d=1e-30), dict(d=3e38), dict(mode=1, loading=0.0), dict(mode=1, loading=float("nan")),
                                  dict(loading=1e-6), dict(loading=1.0), dict(levels=0), dict(levels=8), dict(flags=1, spec=True), dict(flags=1), dict(ref_row=6),
                                  dict(flags=1, spec=True, dir_=False)])
def test_the_limits_themselves_are_accepted(b, over):
    # at a limit, not beyond it: a device is then the only thing that can be missing
    assert _bearing(b, **over) == (0 if b.device_count() > 0 else ENODEV), (over, b.lib().crsdr_last_error())


def test_null_arguments(b):
    L = b.lib()
    assert L.crsdr_caf_set_bearing(None, None) == EINVAL
    assert L.crsdr_caf_set_bearing(None, C.byref(b.bearing_desc(3, 2, 0.5))) == EINVAL
    assert L.crsdr_caf_fetch_bearing(None, None, None) == EINVAL
    assert L.crsdr_caf_bearing_device_buffers(None, None, None) == EINVAL


def test_no_cpu_result_without_a_device(b):
    if b.device_count() > 0:
        # a device is here: the engine takes the bearings, refuses bad ones with its own nrows and K, and holds both state rules
        s = b.Caf(nrows=7, blocksize=2048, seg=64, nlags=16, max_batch=8)        # nd = 16, eight lines
        with pytest.raises(b.CrsdrError) as e:
            s.set_bearing(b.bearing_desc(**GOOD))                                # the detector is off
        assert e.value.code == ESTATE
        s.set_cfar(b.cfar_desc(**{**CFAR, "max_det": 64}))
        for over in BAD:
            if "nrows" in over:
                continue
            with pytest.raises(b.CrsdrError) as e:
                s.set_bearing(b.bearing_desc(**{**GOOD, **{k: v for k, v in over.items() if k in GOOD}}))
            assert e.value.code == EINVAL, over
        with pytest.raises(b.CrsdrError) as e:
            s.set_bearing(b.bearing_desc(**{**GOOD, "flags": 1, "ncx": 512, "ncy": 128}))      # 8 lines * 64 * 2^16 = 2^25
        assert e.value.code == EINVAL
        s.set_bearing(b.bearing_desc(**{**GOOD, "flags": 1, "ncx": 512, "ncy": 64}))           # 2^24: the limit itself
        with pytest.raises(b.CrsdrError) as e:
            s.fetch_bearing()
        assert e.value.code == ESTATE
        with pytest.raises(b.CrsdrError) as e:
            s.set_cfar(b.cfar_desc(**CFAR))                                      # bearings on: the detector stays as it is
        assert e.value.code == ESTATE
        assert all(s.bearing_device_buffers().values())
        s.set_bearing(None)
        s.set_cfar(b.cfar_desc(**CFAR))
        with pytest.raises(b.CrsdrError) as e:
            s.bearing_device_buffers()
        assert e.value.code == ESTATE
        s.close()
        return
    assert _bearing(b) == ENODEV
