"""CPU checks of the canceller's boundary (crsdr_caf_set_cancel, crsdr_caf_fetch_cancel, crsdr_caf_cancel_device_buffers,
crsdr_ambiguity_cancel; include/crsdr.h (w), "Cancellation"): the binding exists, every limit of the section and every NULL argument
is refused with CRSDR_EINVAL before any device is touched, and without a device good arguments give CRSDR_ENODEV -- never a CPU
result."""
import ctypes as C
import importlib

import numpy as np
import pytest

import caf_cancel_model as X

EINVAL, ENODEV, ESTATE = -1, -4, -5


@pytest.fixture(scope="module")
def b():
    binding = importlib.import_module("coherent-rtlsdr_amd.binding")
    binding.build()
    return binding


def _amb(b, nrows=3, B=256, seg=16, nlags=16, ref_row=0, window=0, guard=0, mem_kind=0, taps=2, dopp=0, matrix=True, outs=True):
    nd, R = max(B // (2 * max(seg, 1)), 1), max(nlags, 1)
    n = max(taps, 1) * (2 * min(max(dopp, 0), 8) + 1)
    m = np.zeros(max(nrows, 1) * max(B, 1), dtype=np.int8)
    chi, mp, pk = np.zeros(max(nrows, 1) * nd * R * 2, dtype=np.float32), np.zeros(nd * R, dtype=np.float32), np.zeros((max(nrows, 1) + 1) * 6, dtype=np.float32)
    coef, cinfo = np.zeros(max(nrows, 1) * n * 2, dtype=np.float32), np.zeros(max(nrows, 1) * 2, dtype=np.float32)
    f = lambda a: b._p(a, C.c_float) if outs else None
    return b.lib().crsdr_ambiguity_cancel(f(chi), f(mp), f(pk), b._p(m, C.c_int8) if matrix else None, nrows, B, seg, nlags, ref_row, window, guard, mem_kind, taps, dopp,
                                          f(coef), f(cinfo))


def test_binding_names_the_new_symbols(b):
    names = {"crsdr_caf_set_cancel", "crsdr_caf_fetch_cancel", "crsdr_caf_cancel_device_buffers", "crsdr_ambiguity_cancel"}
    assert names <= set(b.ABI_SYMBOLS)
    assert all(hasattr(b.lib(), s) for s in names)
    assert C.sizeof(b.CancelDesc) == 8


# every limit of the section, at nd = 8, R = 16 unless said: 0 <= P <= 2; 1 <= K <= min(R, 32); K (2 P + 1) <= 48; 2 P + 1 <= nd;
# nd K R <= 2^24
BAD = [dict(dopp=-1), dict(dopp=3), dict(dopp=2 ** 31 - 1), dict(taps=0), dict(taps=-2), dict(taps=17), dict(taps=33, nlags=64, seg=64, B=1024),
       dict(taps=2 ** 31 - 1), dict(taps=10, dopp=2), dict(taps=16, dopp=2), dict(taps=17, dopp=1, nlags=32, seg=32, B=512),
       dict(taps=32, dopp=0, B=2 ** 22, seg=512, nlags=512)]                     # nd K R = 4096 x 32 x 512 = 2^26


@pytest.mark.parametrize("over", BAD)
def test_bad_descriptors_are_refused_before_device_use(b, over):
    assert _amb(b, **over) == EINVAL, (over, b.lib().crsdr_last_error())


def test_the_limit_function_agrees_with_the_model(b):
    for over in BAD:
        kw = dict(B=256, seg=16, nlags=16, taps=2, dopp=0)
        kw.update(over)
        assert X.bad_limit(kw["B"] // (2 * kw["seg"]), kw["nlags"], 1, kw["taps"], kw["dopp"]) != 0, over


@pytest.mark.parametrize("over", [dict(nrows=1), dict(seg=8), dict(nlags=17), dict(ref_row=3), dict(window=7), dict(guard=5), dict(mem_kind=2), dict(matrix=False),
                                  dict(outs=False), dict(B=250)])
def test_bad_ambiguity_arguments_are_refused_as_before(b, over):
    assert _amb(b, **over) == EINVAL, (over, b.lib().crsdr_last_error())


@pytest.mark.parametrize("over", [dict(taps=1), dict(taps=16), dict(taps=9, dopp=2), dict(taps=16, dopp=1, nlags=16), dict(taps=32, nlags=32, seg=32, B=512),
                                  dict(taps=1, dopp=2), dict(taps=32, dopp=0, B=2 ** 20, seg=128, nlags=128)])      # nd K R = 4096 x 32 x 128 = 2^24
def test_the_limits_themselves_are_accepted(b, over):
    # at a limit, not beyond it: a device is then the only thing that can be missing
    assert _amb(b, **over) == (0 if b.device_count() > 0 else ENODEV), (over, b.lib().crsdr_last_error())


def test_null_arguments(b):
    L = b.lib()
    assert L.crsdr_caf_set_cancel(None, None) == EINVAL
    assert L.crsdr_caf_set_cancel(None, C.byref(b.CancelDesc(2, 0))) == EINVAL
    assert L.crsdr_caf_fetch_cancel(None, None, None) == EINVAL
    assert L.crsdr_caf_cancel_device_buffers(None, None, None) == EINVAL


def test_no_cpu_result_without_a_device(b):
    if b.device_count() > 0:
        # a device is here: the fetch calls are call sequence errors with the canceller off, and the engine refuses with its own nd and R
        s = b.Caf(nrows=3, blocksize=256, seg=16, nlags=16, max_batch=2)         # nd = 8
        with pytest.raises(b.CrsdrError) as e:
            s.fetch_cancel()
        assert e.value.code == ESTATE
        with pytest.raises(b.CrsdrError) as e:
            s.cancel_device_buffers()
        assert e.value.code == ESTATE
        for taps, dopp in ((0, 0), (17, 0), (2, 3), (10, 2), (2, -1)):
            with pytest.raises(b.CrsdrError) as e:
                s.set_cancel(taps, dopp)
            assert e.value.code == EINVAL, (taps, dopp)
        s.set_cancel(2, 1)
        with pytest.raises(b.CrsdrError) as e:
            s.fetch_cancel()                                                     # nothing submitted since it was set
        assert e.value.code == ESTATE
        assert all(s.cancel_device_buffers().values())
        s.set_cancel(None)
        with pytest.raises(b.CrsdrError) as e:
            s.cancel_device_buffers()
        assert e.value.code == ESTATE
        s.close()
        return
    assert _amb(b) == ENODEV
