"""CPU checks of the CFAR estimators' boundary (crsdr_caf_set_cfar_estimator, crsdr_cfar_est, crsdr_cfar_alpha_est; include/crsdr.h
(w), "Estimators"): the binding exists, every limit and every NULL argument is refused with CRSDR_EINVAL before any device is touched,
crsdr_cfar_alpha_est is the model's bisection, and without a device good arguments give CRSDR_ENODEV -- never a CPU result."""
import ctypes as C
import importlib

import numpy as np
import pytest

import caf_cfar_est_model as E
import caf_cfar_model as CM

EINVAL, ENODEV, ESTATE = -1, -4, -5
GOOD = dict(gd=1, gr=1, td=3, tr=4, alpha=14.93, min_train=1, max_det=16)        # Nfull = 9 * 11 - 3 * 3 = 90


@pytest.fixture(scope="module")
def b():
    binding = importlib.import_module("coherent-rtlsdr_amd.binding")
    binding.build()
    return binding


def _cfar_est(b, est, nd=16, R=8, guard=2, comps=1, mem_kind=0, det=True, count=True, src=True, desc=True, **over):
    d = b.cfar_desc(**{**GOOD, **over})
    K = min(max(d.max_det, 1), 64)
    out, n, a = np.zeros(K * 8, dtype=np.float32), np.zeros(1, dtype=np.int32), np.zeros(max(nd, 1) * max(R, 1) * 2, dtype=np.float32)
    e = None if est is None else b.CfarEstDesc(*est)
    return b.lib().crsdr_cfar_est(b._p(out, C.c_float) if det else None, b._p(n, C.c_int32) if count else None, b._p(a, C.c_float) if src else None, comps, nd, R, guard,
                                  C.byref(d) if desc else None, None if e is None else C.byref(e), mem_kind)


def test_binding_names_the_new_symbols(b):
    names = {"crsdr_caf_set_cfar_estimator", "crsdr_cfar_est", "crsdr_cfar_alpha_est"}
    assert names <= set(b.ABI_SYMBOLS)
    assert all(hasattr(b.lib(), s) for s in names)
    assert C.sizeof(b.CfarEstDesc) == 12 and C.sizeof(b.CfarDesc) == 28
    assert (b.CFAR_CA, b.CFAR_GO, b.CFAR_SO, b.CFAR_OS) == (0, 1, 2, 3)


# (estimator, axis, rank): what is not read may hold anything
BAD_EST = [(-1, 0, 1), (4, 0, 1), (2 ** 31 - 1, 0, 1), (1, -1, 0), (1, 2, 0), (2, -1, 0), (2, 2, 0), (3, 0, 0), (3, 0, 91), (3, 0, -5), (3, 7, 2 ** 31 - 1)]
GOOD_EST = [None, (0, 0, 0), (0, 9, -9), (1, 0, 0), (1, 1, -4), (2, 0, 10 ** 6), (2, 1, 0), (3, 0, 1), (3, 5, 90), (3, -1, 67)]


@pytest.mark.parametrize("est", BAD_EST)
def test_bad_estimators_are_refused_before_device_use(b, est):
    assert _cfar_est(b, est) == EINVAL, (est, b.lib().crsdr_last_error())


def test_the_rank_limit_is_the_windows_own(b):
    # window 0/0/0/1: Nfull = 2
    assert _cfar_est(b, (3, 0, 3), gd=0, gr=0, td=0, tr=1) == EINVAL
    assert _cfar_est(b, (3, 0, 2), gd=0, gr=0, td=0, tr=1) == (0 if b.device_count() > 0 else ENODEV)


@pytest.mark.parametrize("est", GOOD_EST)
def test_good_estimators_reach_the_device(b, est):
    assert _cfar_est(b, est) == (0 if b.device_count() > 0 else ENODEV), (est, b.lib().crsdr_last_error())


@pytest.mark.parametrize("over", [dict(nd=12), dict(nd=0), dict(R=0), dict(R=1025), dict(guard=-1), dict(guard=9), dict(comps=0), dict(comps=3), dict(mem_kind=2),
                                  dict(mem_kind=-1), dict(det=False, count=False), dict(src=False), dict(desc=False), dict(gd=-1), dict(gd=5, td=4), dict(td=0, tr=0),
                                  dict(alpha=float("nan")), dict(min_train=0), dict(max_det=65)])
@pytest.mark.parametrize("est", [(1, 1, 0), (3, 0, 67)])
def test_the_detectors_own_refusals_stand(b, est, over):
    assert _cfar_est(b, est, **over) == EINVAL, (est, over, b.lib().crsdr_last_error())


ALPHA_CASES = [(1e-5, 42, (1, 0, 0)), (1e-5, 42, (2, 0, 0)), (1e-5, 90, (3, 0, 67)), (1e-2, 12, (1, 1, 0)), (1e-2, 12, (2, 1, 0)), (1e-2, 24, (3, 0, 18)), (0.25, 1, (1, 0, 0)),
               (0.25, 1, (2, 0, 0)), (0.25, 1, (3, 0, 1)), (1e-9, 280, (1, 0, 0)), (1e-9, 280, (2, 0, 0)), (1e-9, 560, (3, 0, 560)), (1e-9, 560, (3, 0, 1)), (0.9, 5, (3, 0, 2))]


@pytest.mark.parametrize("pfa,n,est", ALPHA_CASES)
def test_alpha_is_the_models_bisection(b, pfa, n, est):
    want = E.cfar_alpha_est(pfa, n, E.Est(*est))
    got = b.cfar_alpha_est(pfa, n, b.CfarEstDesc(*est))
    assert got == want or got in (np.nextafter(want, np.float32(np.inf)), np.nextafter(want, np.float32(0))), (got, want)
    # and it solves the equation: the model's probability at the returned alpha, within its fp32 rounding (d log P / d log alpha <= rank or n)
    assert abs(E.pfa(est[0], n, est[2], float(got)) / pfa - 1.0) <= 2.0 ** -22 * max(n, 1) + 1e-9


@pytest.mark.parametrize("pfa,n", [(1e-6, 90), (0.5, 1), (1e-12, 560)])
def test_alpha_of_cell_averaging_is_crsdr_cfar_alpha(b, pfa, n):
    assert b.cfar_alpha_est(pfa, n, None) == b.cfar_alpha(pfa, n) == b.cfar_alpha_est(pfa, n, b.CfarEstDesc(0, 3, -1)) == CM.cfar_alpha(pfa, n)


@pytest.mark.parametrize("pfa,n,est", [(0.0, 42, (1, 0, 0)), (1.0, 42, (2, 0, 0)), (float("nan"), 90, (3, 0, 5)), (1e-3, 0, (1, 0, 0)), (1e-3, -1, (3, 0, 1)),
                                       (1e-3, 65537, (2, 0, 0)), (1e-3, 90, (3, 0, 0)), (1e-3, 90, (3, 0, 91)), (1e-3, 90, (4, 0, 1)), (1e-3, 90, (-1, 0, 1)),
                                       (1e-3, 0, (0, 0, 0)), (2.0, 90, None)])
def test_alpha_refusals(b, pfa, n, est):
    a = C.c_float(7.0)
    e = None if est is None else b.CfarEstDesc(*est)
    assert b.lib().crsdr_cfar_alpha_est(pfa, n, None if e is None else C.byref(e), C.byref(a)) == EINVAL
    assert a.value == 7.0                                  # nothing written
    assert b.lib().crsdr_cfar_alpha_est(1e-3, 16, None if e is None else C.byref(e), None) == EINVAL


def test_null_arguments(b):
    L = b.lib()
    assert L.crsdr_caf_set_cfar_estimator(None, None) == EINVAL
    assert L.crsdr_caf_set_cfar_estimator(None, C.byref(b.CfarEstDesc(3, 0, 1))) == EINVAL


def test_no_cpu_result_without_a_device(b):
    if b.device_count() > 0:
        s = b.Caf(nrows=3, blocksize=2048, seg=64, nlags=16, max_batch=2)        # nd = 16
        with pytest.raises(b.CrsdrError) as e:
            s.set_cfar_estimator(b.CfarEstDesc(1, 0, 0))                         # no detector set
        assert e.value.code == ESTATE
        s.set_cfar(b.cfar_desc(**GOOD))
        for est in BAD_EST:
            with pytest.raises(b.CrsdrError) as e:
                s.set_cfar_estimator(b.CfarEstDesc(*est))
            assert e.value.code == EINVAL, est
        for est in GOOD_EST:
            s.set_cfar_estimator(None if est is None else b.CfarEstDesc(*est))
        s.close()
        return
    assert _cfar_est(b, (3, 0, 67)) == ENODEV and _cfar_est(b, (1, 1, 0)) == ENODEV
