"""CPU checks of the second cancellation stage's boundary (crsdr_caf_set_clean, crsdr_caf_fetch_clean, crsdr_caf_clean_device_buffers,
crsdr_ambiguity_clean; include/crsdr.h (w), "Cleaning"): the binding exists, every limit of the section and every NULL argument is
refused with CRSDR_EINVAL before any device is touched, and without a device good arguments give CRSDR_ENODEV -- never a CPU result.
The state rules need an object, and so a device: with one here they are walked through; tests/test_gpu_caf_clean.py pins them on the
GPU in any case."""
import ctypes as C
import importlib

import numpy as np
import pytest

import caf_clean_model as Z

EINVAL, ENODEV, ESTATE = -1, -4, -5


@pytest.fixture(scope="module")
def b():
    binding = importlib.import_module("coherent-rtlsdr_amd.binding")
    binding.build()
    return binding


def _amb(b, nrows=3, B=2048, seg=32, nlags=16, ref_row=0, window=0, guard=0, mem_kind=0, taps=2, dopp=0, T=2, min_snr=100.0, wl=1, wq=1, max_det=8, matrix=True,
         out=True, cancel=True, cfar=True, clean=True, est=None):
    """crsdr_ambiguity_clean's return code; the outputs are left NULL (any may be): nothing is written before the checks are through"""
    m = np.zeros(max(nrows, 1) * max(B, 1), dtype=np.int8)
    io = b.CleanOut()
    ref = lambda on, v: C.byref(v) if on else None
    return b.lib().crsdr_ambiguity_clean(ref(out, io), b._p(m, C.c_int8) if matrix else None, nrows, B, seg, nlags, ref_row, window, guard, mem_kind,
                                         ref(cancel, b.CancelDesc(taps, dopp)), ref(cfar, b.cfar_desc(alpha=10.0, td=3, tr=2, max_det=max_det)),
                                         None if est is None else C.byref(est), ref(clean, b.CleanDesc(T, min_snr, wl, wq)))


def test_binding_names_the_new_symbols(b):
    names = {"crsdr_caf_set_clean", "crsdr_caf_fetch_clean", "crsdr_caf_clean_device_buffers", "crsdr_ambiguity_clean"}
    assert names <= set(b.ABI_SYMBOLS)
    assert all(hasattr(b.lib(), s) for s in names)
    assert C.sizeof(b.CleanDesc) == 16 and C.sizeof(b.CleanOut) == 17 * C.sizeof(C.c_void_p)
    assert b.CLEAN_LAUNCHES == Z.LAUNCHES and (b.CLEAN_SINGULAR, b.CLEAN_TARGET) == (Z.STATUS_SINGULAR, Z.STATUS_TARGET)


# every limit of the section, at nd = 32, R = 16, nrows = 3, K = 2, P = 0 unless said
BAD = [dict(T=0), dict(T=9), dict(T=-1), dict(T=2 ** 31 - 1), dict(wl=-1), dict(wl=3), dict(wq=-1), dict(wq=3),
       dict(taps=5, T=4, wl=2, wq=1),                                            # 5 + 4 x 15 = 65 members
       dict(taps=15, T=2, wl=2, wq=2), dict(taps=2, dopp=2, T=8, wl=1, wq=1),   # 15 + 50; 10 + 72
       dict(min_snr=0.0), dict(min_snr=-1.0), dict(min_snr=float("inf")), dict(min_snr=float("nan")),
       dict(nrows=5, B=2 ** 22, seg=512, nlags=512, taps=1, T=1, wl=1, wq=0),   # nd (K + 3) R = 2^23 holds, 2 nrows nd R = 10 x 2^21 does not
       dict(nrows=2, B=2 ** 21, seg=256, nlags=256, taps=1, T=8, wl=2, wq=0)]   # nd (K + 40) R = 4096 x 41 x 256 > 2^24


@pytest.mark.parametrize("over", BAD)
def test_bad_descriptors_are_refused_before_device_use(b, over):
    assert _amb(b, **over) == EINVAL, (over, b.lib().crsdr_last_error())


def test_the_limit_function_agrees_with_the_model(b):
    for over in BAD:
        kw = dict(nrows=3, B=2048, seg=32, nlags=16, taps=2, dopp=0, T=2, min_snr=100.0, wl=1, wq=1)
        kw.update(over)
        assert Z.bad_limit(kw["B"] // (2 * kw["seg"]), kw["nlags"], 1, kw["nrows"], kw["taps"], kw["dopp"], Z.Params(kw["T"], kw["min_snr"], kw["wl"], kw["wq"])) != 0, over


@pytest.mark.parametrize("over", [dict(nrows=1), dict(seg=8), dict(nlags=33), dict(ref_row=3), dict(window=7), dict(guard=17), dict(mem_kind=2), dict(matrix=False),
                                  dict(out=False), dict(cancel=False), dict(cfar=False), dict(clean=False), dict(B=250), dict(taps=0), dict(taps=17), dict(dopp=3),
                                  dict(max_det=0), dict(max_det=65)])
def test_bad_arguments_of_the_first_pass_are_refused_as_before(b, over):
    assert _amb(b, **over) == EINVAL, (over, b.lib().crsdr_last_error())


def test_a_bad_estimator_is_refused(b):
    assert _amb(b, est=b.cfar_est_desc(7)) == EINVAL and _amb(b, est=b.cfar_est_desc(b.CFAR_OS, rank=0)) == EINVAL


@pytest.mark.parametrize("over", [dict(T=1, wl=0, wq=0), dict(T=8, wl=0, wq=0), dict(taps=4, T=4, wl=2, wq=1), dict(taps=14, T=2, wl=2, wq=2), dict(T=2, wl=2, wq=2),
                                  dict(min_snr=1e-30), dict(min_snr=3e38), dict(nrows=2, B=2 ** 21, seg=256, nlags=256, taps=1, T=3, wl=2, wq=0)])      # nd (K + 15) R = 2^24
def test_the_limits_themselves_are_accepted(b, over):
    # at a limit, not beyond it: a device is then the only thing that can be missing
    assert _amb(b, **over) == (0 if b.device_count() > 0 else ENODEV), (over, b.lib().crsdr_last_error())


def test_null_arguments(b):
    L = b.lib()
    assert L.crsdr_caf_set_clean(None, None) == EINVAL
    assert L.crsdr_caf_set_clean(None, C.byref(b.CleanDesc(2, 100.0, 1, 1))) == EINVAL
    assert L.crsdr_caf_fetch_clean(None, *[None] * 9) == EINVAL
    assert L.crsdr_caf_clean_device_buffers(None, *[None] * 9) == EINVAL


def test_no_cpu_result_without_a_device(b):
    if b.device_count() < 1:
        assert _amb(b) == ENODEV
        return
    # a device is here: every state rule, and CRSDR_ESTATE before the first submit
    s = b.Caf(nrows=3, blocksize=2048, seg=32, nlags=16, max_batch=2)
    ok = b.CleanDesc(2, 100.0, 1, 1)

    def code(call, *a):
        with pytest.raises(b.CrsdrError) as e:
            call(*a)
        return e.value.code

    assert code(s.fetch_clean) == ESTATE and code(s.clean_device_buffers) == ESTATE
    assert code(s.set_clean, ok) == ESTATE                                       # no canceller
    assert code(s.set_clean, b.CleanDesc(9, 100.0, 1, 1)) == EINVAL              # (the limits come first)
    s.set_cancel(2, 0)
    assert code(s.set_clean, ok) == ESTATE                                       # no detector
    s.set_cfar(b.cfar_desc(alpha=10.0, td=3, tr=2, max_det=8))
    s.set_integrate(b.integrate_desc(0.9))
    assert code(s.set_clean, ok) == ESTATE                                       # CRSDR_INTEGRATE_ARRAY is on
    s.set_integrate(None)
    assert code(s.set_clean, b.CleanDesc(2, 100.0, 3, 1)) == EINVAL
    s.set_clean(ok)
    assert code(s.fetch_clean) == ESTATE                                         # nothing submitted since it was set
    assert all(s.clean_device_buffers().values())
    for call, a in ((s.set_cancel, (3, 0)), (s.set_cancel, (None,)), (s.set_cfar, (None,)), (s.set_cfar_estimator, (None,)), (s.set_integrate, (b.integrate_desc(0.9),))):
        assert code(call, *a) == ESTATE and "turn it off first" in b.lib().crsdr_last_error().decode()
    s.set_clean(None)
    assert code(s.clean_device_buffers) == ESTATE
    s.set_cancel(None)
    s.close()
