"""CPU checks of the CFAR detector's boundary (crsdr_caf_set_cfar, crsdr_caf_fetch_cfar, crsdr_caf_cfar_device_buffers, crsdr_cfar,
crsdr_cfar_alpha; include/crsdr.h (w), "Detections"): the binding exists, every limit of the section and every NULL argument is refused
with CRSDR_EINVAL before any device is touched, crsdr_cfar_alpha is the closed form, and without a device good arguments give
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


GOOD = dict(gd=1, gr=1, td=3, tr=4, alpha=14.93, min_train=1, max_det=16)
# what the one function behind crsdr_caf_set_cfar and crsdr_cfar must refuse, at nd = 16
BAD = [
    dict(gd=-1), dict(gr=-1), dict(td=-1), dict(tr=-1),
    dict(gd=5, td=4), dict(gd=9, td=0), dict(gd=2 ** 31 - 1, td=2 ** 31 - 1),    # Hd <= 8 (and no overflow on the way)
    dict(gr=12, tr=5), dict(gr=0, tr=17), dict(gr=2 ** 31 - 1, tr=2),            # Hr <= 16
    dict(td=0, tr=0),                                                            # nothing trains
    dict(gd=4, td=4),                                                            # 2 Hd + 1 = 17 > nd = 16
    dict(alpha=0.0), dict(alpha=-1.0), dict(alpha=float("inf")), dict(alpha=float("nan")),
    dict(min_train=0), dict(min_train=-4),
    dict(max_det=0), dict(max_det=65), dict(max_det=-1),
]


def _cfar(b, nd=16, R=8, guard=2, comps=1, mem_kind=0, det=True, count=True, src=True, desc=True, **over):
    d = b.cfar_desc(**{**GOOD, **over})
    K = min(max(d.max_det, 1), 64)
    out, n, a = np.zeros(K * 8, dtype=np.float32), np.zeros(1, dtype=np.int32), np.zeros(max(nd, 1) * max(R, 1) * 2, dtype=np.float32)
    return b.lib().crsdr_cfar(b._p(out, C.c_float) if det else None, b._p(n, C.c_int32) if count else None, b._p(a, C.c_float) if src else None, comps, nd, R, guard,
                              C.byref(d) if desc else None, mem_kind)


def test_binding_names_the_new_symbols(b):
    names = {"crsdr_caf_set_cfar", "crsdr_caf_fetch_cfar", "crsdr_caf_cfar_device_buffers", "crsdr_cfar", "crsdr_cfar_alpha"}
    assert names <= set(b.ABI_SYMBOLS)
    assert all(hasattr(b.lib(), s) for s in names)
    assert C.sizeof(b.CfarDesc) == 28                      # six int32 and a float: no padding to disagree about


@pytest.mark.parametrize("over", BAD)
def test_bad_descriptors_are_refused_before_device_use(b, over):
    # CRSDR_EINVAL whether or not a device is present: on a machine without one CRSDR_ENODEV would mean the device was asked first
    assert _cfar(b, **over) == EINVAL, (over, b.lib().crsdr_last_error())


@pytest.mark.parametrize("over", [dict(nd=12), dict(nd=4), dict(nd=8192), dict(nd=0), dict(nd=-16), dict(R=0), dict(R=1025), dict(R=-3), dict(guard=-1), dict(guard=9),
                                  dict(comps=0), dict(comps=3), dict(mem_kind=2), dict(mem_kind=-1), dict(det=False, count=False), dict(src=False), dict(desc=False),
                                  dict(nd=8, gd=1, td=3)])
def test_bad_cfar_arguments_are_refused_before_device_use(b, over):
    assert _cfar(b, **over) == EINVAL, (over, b.lib().crsdr_last_error())


@pytest.mark.parametrize("over", [dict(gd=0, gr=0, td=0, tr=1), dict(gd=8, td=0, nd=32), dict(gd=0, td=8, gr=16, tr=0, nd=32), dict(nd=8, gd=0, td=3), dict(max_det=64),
                                  dict(max_det=1, min_train=10 ** 6), dict(alpha=1e-30), dict(alpha=3e38), dict(nd=4096, R=3, guard=2048), dict(nd=8, R=1024, guard=0, td=2),
                                  dict(comps=2), dict(det=False), dict(count=False)])
def test_the_limits_themselves_are_accepted(b, over):
    # at a limit, not beyond it: a device is then the only thing that can be missing
    assert _cfar(b, **over) == (0 if b.device_count() > 0 else ENODEV), (over, b.lib().crsdr_last_error())


@pytest.mark.parametrize("pfa,n", [(1e-6, 90), (1e-2, 90), (1e-3, 90), (0.5, 1), (1e-12, 560), (0.999, 3), (1e-4, 1)])
def test_alpha_is_the_closed_form(b, pfa, n):
    want = n * (pfa ** (-1.0 / n) - 1.0)
    got = float(b.cfar_alpha(pfa, n))
    assert abs(got - want) <= 2.0 ** -23 * want, (got, want)                     # one rounding to fp32 and the library's pow
    if (pfa, n) == (1e-6, 90):
        assert round(got, 2) == 14.93


@pytest.mark.parametrize("pfa,n", [(0.0, 90), (1.0, 90), (-0.1, 90), (1.5, 90), (float("nan"), 90), (float("inf"), 90), (1e-3, 0), (1e-3, -5)])
def test_alpha_refusals(b, pfa, n):
    a = C.c_float(7.0)
    assert b.lib().crsdr_cfar_alpha(pfa, n, C.byref(a)) == EINVAL
    assert a.value == 7.0                                  # nothing written
    assert b.lib().crsdr_cfar_alpha(1e-3, 16, None) == EINVAL


def test_null_arguments(b):
    L = b.lib()
    assert L.crsdr_caf_set_cfar(None, None) == EINVAL
    assert L.crsdr_caf_set_cfar(None, C.byref(b.cfar_desc(**GOOD))) == EINVAL
    assert L.crsdr_caf_fetch_cfar(None, None, None, None) == EINVAL
    assert L.crsdr_caf_cfar_device_buffers(None, None, None, None) == EINVAL


def test_no_cpu_result_without_a_device(b):
    if b.device_count() > 0:
        # a device is here: the engine takes the detector, refuses a bad one with the engine's own nd, and a fetch before a submit is a call sequence error
        s = b.Caf(nrows=3, blocksize=2048, seg=64, nlags=16, max_batch=2)        # nd = 16
        with pytest.raises(b.CrsdrError) as e:
            s.fetch_cfar()
        assert e.value.code == ESTATE
        for over in BAD:
            with pytest.raises(b.CrsdrError) as e:
                s.set_cfar(b.cfar_desc(**{**GOOD, **over}))
            assert e.value.code == EINVAL, over
        s.set_cfar(b.cfar_desc(**GOOD))
        with pytest.raises(b.CrsdrError) as e:
            s.fetch_cfar()
        assert e.value.code == ESTATE
        assert all(s.cfar_device_buffers().values())
        s.set_cfar(None)
        with pytest.raises(b.CrsdrError) as e:
            s.cfar_device_buffers()
        assert e.value.code == ESTATE
        s.close()
        return
    assert _cfar(b) == ENODEV
