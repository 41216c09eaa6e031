"""CPU checks of spatial smoothing and the source count of crsdr_doa (include/crsdr.h (iv): crsdr_doa_set_smoothing, crsdr_doa_set_order
and their per-op forms): the symbols are declared, exported and bound, a NULL object is refused, and the numpy restatement the GPU
tests compare against (tests/doa_smooth_model.py) gives the known answers and restores the rank of coherent scenes.

The scene conditions are those of the fp64 study the feature was specified from: on the 7 x 3 URA at L = 2048 with two or three
coherent paths the plain covariance has sv[1]/sv[0] < 0.02 and MDL counts one source; averaged over its 5 x 2 sub-arrays and with its
backward image, sv[k-1]/sv[0] > 0.2, sv[k]/sv[0] < 0.05, MDL counts k and every path is within one grid point of a direction."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

import doa_peaks_model as peaks_model
import doa_smooth_model as model
import ura

EINVAL = -1
P = np.pi
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("crsdr_doa_set_smoothing", "crsdr_doa_fetch_smoothed", "crsdr_doa_set_order", "crsdr_doa_fetch_order", "crsdr_doa_order_buffers",
       "crsdr_smooth_covariance", "crsdr_source_order")
DIRS = [(0.35 * P, 0.40 * P), (0.65 * P, 0.62 * P), (0.45 * P, 0.70 * P)]      # on the 100 x 100 grid: (65, 60), (35, 38), (55, 30)


@pytest.fixture(scope="module")
def b():
    binding = importlib.import_module("coherent-rtlsdr_amd.binding")
    binding.build()
    return binding


def coherent_paths(k, rng):
    """k paths of one emitter: amplitudes 1, 0.85, 0.7, arbitrary phases"""
    return [(a, be, (1.0 - 0.15 * i) * np.exp(1j * (rng.uniform(0, 2 * P) if i else 0.0))) for i, (a, be) in enumerate(DIRS[:k])]


def test_symbols_declared_exported_and_bound(b):
    hdr = open(os.path.join(ROOT, "include", "crsdr.h")).read()
    declared = set(re.findall(r"\b(crsdr_[a-z0-9_]+)\s*\(", hdr))
    for s in NEW:
        assert s in declared and s in b.ABI_SYMBOLS and hasattr(b.lib(), s), s
    for s in ("set_smoothing", "fetch_smoothed", "set_order", "fetch_order", "order_buffers"):
        assert callable(getattr(b.Doa, s))
    assert callable(b.smooth_covariance) and callable(b.source_order)
    for name, value in (("SMOOTH_FB", 1), ("ORDER_OFF", 0), ("ORDER_MDL", 1), ("ORDER_AIC", 2)):
        assert getattr(b, name) == value and re.search(r"\bCRSDR_%s\s*=\s*%s" % (name, "1u << 0" if name == "SMOOTH_FB" else value), hdr), name
    assert "k = 0, is not representable" in hdr


def test_null_object_and_bad_arguments_are_refused(b):
    L = b.lib()
    p = C.c_void_p()
    assert L.crsdr_doa_set_smoothing(None, 5, 2, 1) == EINVAL
    assert L.crsdr_doa_fetch_smoothed(None, None) == EINVAL
    assert L.crsdr_doa_set_order(None, 1, 1, 3, 0) == EINVAL
    assert L.crsdr_doa_fetch_order(None, None, None) == EINVAL
    assert L.crsdr_doa_order_buffers(None, C.byref(p), C.byref(p)) == EINVAL
    # the per-op forms validate before they look for a device
    r, rs = np.zeros((21, 21), dtype=np.complex64), np.zeros((21, 21), dtype=np.complex64)
    for mx, my, sx, sy, flags in ((7, 3, 0, 2, 0), (7, 3, 8, 3, 0), (7, 3, 5, 4, 0), (7, 3, 1, 1, 0), (7, 3, 5, 2, 2), (13, 5, 5, 2, 0)):
        assert L.crsdr_smooth_covariance(rs.ctypes.data, r.ctypes.data, mx, my, sx, sy, flags, b.MEM_HOST) == EINVAL, (mx, my, sx, sy, flags)
    assert L.crsdr_smooth_covariance(None, r.ctypes.data, 7, 3, 5, 2, 0, b.MEM_HOST) == EINVAL
    sv, k, crit = np.ones(21, dtype=np.float32), np.zeros(1, dtype=np.int32), np.zeros(21, dtype=np.float32)
    for m, n, c, kmin, kmax in ((21, 1024, 0, 1, 3), (21, 1024, 3, 1, 3), (21, 1024, 1, 0, 3), (21, 1024, 1, 4, 3), (21, 1024, 1, 1, 21), (21, 0, 1, 1, 3),
                                (1, 1024, 1, 1, 1), (65, 1024, 1, 1, 3)):
        assert L.crsdr_source_order(k.ctypes.data, crit.ctypes.data, sv.ctypes.data, m, n, c, kmin, kmax, b.MEM_HOST) == EINVAL, (m, n, c, kmin, kmax)


def _random_hermitian(m, rng):
    x = rng.standard_normal((m, 3 * m)) + 1j * rng.standard_normal((m, 3 * m))
    r = x @ x.conj().T / (3 * m)
    return ((r + r.conj().T) / 2).astype(np.complex64)      # Hermitian to the bit


def test_one_sub_array_without_fb_is_the_identity():
    rng = np.random.default_rng(1)
    for mx, my in ((7, 3), (8, 8), (2, 1), (1, 5)):
        r = _random_hermitian(mx * my, rng)
        assert np.array_equal(model.smooth(r, mx, my, mx, my, 0), r.astype(np.complex128)), (mx, my)


def test_sub_array_selection_and_order():
    # 3 x 2 array, 2 x 2 sub-arrays: (px, py) = (0, 0) and (1, 0), elements iy * 3 + ix
    assert model.select(3, 2, 2, 0, 0).tolist() == [0, 1, 3, 4] and model.select(3, 2, 2, 1, 0).tolist() == [1, 2, 4, 5]
    r = (np.arange(36).reshape(6, 6) + 1j * np.arange(36).reshape(6, 6).T).astype(np.complex64)
    s = model.smooth(r, 3, 2, 2, 2, 0)
    assert s[0, 1] == (r[0, 1] + r[1, 2]) / 2 and s[1, 3] == (r[1, 4] + r[2, 5]) / 2 and s[2, 2] == (r[3, 3] + r[4, 4]) / 2
    assert s[1, 0] == np.conj(s[0, 1])


def test_fb_output_is_persymmetric():
    rng = np.random.default_rng(2)
    for mx, my, sx, sy in ((7, 3, 5, 2), (7, 3, 7, 3), (8, 8, 6, 6), (1, 64, 1, 33)):
        r = _random_hermitian(mx * my, rng)
        s = model.smooth(r, mx, my, sx, sy, model.FB)
        assert np.array_equal(s, s[::-1, ::-1].conj()), (mx, my, sx, sy)           # rs[a][b] = conj(rs[ms-1-a][ms-1-b])
        assert np.array_equal(s, s.conj().T)


def test_rank_one_covariance_of_two_coherent_vectors_gains_a_second_eigenvalue():
    a = ura.steering(0.35 * P, 0.40 * P) + 0.8 * np.exp(0.7j) * ura.steering(0.65 * P, 0.62 * P)
    r = np.outer(a.conj(), a)                                                       # the X^H X convention: conj(a) a^T
    s0 = np.linalg.svd(r, compute_uv=False)
    assert s0[1] / s0[0] < 1e-12
    for flags, floor in ((0, 0.05), (model.FB, 0.2)):
        s = np.linalg.svd(model.smooth(r, 7, 3, 5, 2, flags), compute_uv=False)
        print(f"flags {flags}: sv ratios {np.round(s[:3] / s[0], 4).tolist()}")
        assert s[1] / s[0] > floor and s[2] / s[0] < 1e-9, (flags, s[:3] / s[0])


@pytest.mark.parametrize("k", [2, 3])
@pytest.mark.parametrize("seed", [100, 101, 102])
def test_smoothing_restores_the_rank_of_coherent_scenes(k, seed):
    rng = np.random.default_rng(seed)
    L = 2048
    paths = coherent_paths(k, rng)
    r = model.covariance(model.coherent_scene(L, paths, rng)).astype(np.complex64)
    s0 = np.linalg.svd(r.astype(np.complex128), compute_uv=False)
    o0 = model.order(s0, L, model.MDL)
    assert s0[1] / s0[0] < 0.02 and o0["k"] == 1 and o0["decided"], (s0[:3] / s0[0], o0["k"])
    rs = model.smooth(r, 7, 3, 5, 2, model.FB)
    s, pm = model.spectrum(rs, k, 5, 2)
    o = model.order(s, L, model.MDL)
    n, found, _ = peaks_model.directions(pm.astype(np.float32), k, 2)
    print(f"k {k} seed {seed}: plain {s0[1] / s0[0]:.4f}, smoothed {np.round(s[:k + 1] / s[0], 3).tolist()}, MDL {o['k']} "
          f"(margin {o['margin']:.3g}, bar {o['bar']:.3g}), directions {found.tolist()}")
    assert s[k - 1] / s[0] > 0.2 and s[k] / s[0] < 0.05
    assert o["k"] == k and o["decided"]
    assert n == k and model.all_within(found, paths, tol=1.0), found


def test_fb_alone_keeps_m_and_restores_two_sources_only_sometimes():
    # (the reason sub-arrays are needed: the second eigenvalue under FB alone depends on the path phase)
    ratios = []
    for phase in np.linspace(0, P, 7):
        a = ura.steering(*DIRS[0]) + 0.8 * np.exp(1j * phase) * ura.steering(*DIRS[1])
        s = np.linalg.svd(model.smooth(np.outer(a.conj(), a), 7, 3, 7, 3, model.FB), compute_uv=False)
        ratios.append(s[1] / s[0])
    print("FB alone, sv[1]/sv[0] over the path phase:", np.round(ratios, 3).tolist())
    assert min(ratios) < 0.1 < max(ratios)


@pytest.mark.parametrize("criterion", [model.MDL, model.AIC])
def test_mdl_and_aic_count_incoherent_sources(criterion):
    for k in (1, 2, 3):
        for seed, L in ((7, 1024), (8, 4096)):
            rng = np.random.default_rng(seed)
            r = model.covariance(ura.scene(L, [(a, be, 1.0 - 0.1 * i) for i, (a, be) in enumerate(DIRS[:k])], rng)).astype(np.complex64)
            for sx, sy, flags in ((7, 3, 0), (7, 3, model.FB), (5, 2, model.FB)):
                o = model.order(np.linalg.svd(model.smooth(r, 7, 3, sx, sy, flags), compute_uv=False), L, criterion)
                assert o["k"] == k and o["decided"], (criterion, k, L, sx, sy, flags, o["k"], o["margin"], o["bar"])


def test_order_known_answers():
    # equal values: T_k = 0 for every k, the penalty grows with k, so kmin wins, and MDL_k is exactly the penalty
    o = model.order(np.ones(8, dtype=np.float32), 1000, model.MDL, 2, 5)
    assert o["k"] == 2 and np.allclose(o["values"], [0.5 * k * (16 - k) * np.log(1000.0) for k in range(2, 6)], rtol=0, atol=1e-9)
    o = model.order(np.ones(8, dtype=np.float32), 1000, model.AIC)
    assert o["k"] == 1 and np.allclose(o["values"], [2.0 * k * (16 - k) for k in range(1, 8)], rtol=0, atol=1e-9)
    # an all-zero estimate: kmin, values 0
    o = model.order(np.zeros(5, dtype=np.float32), 512, model.MDL, 2, 4)
    assert o["k"] == 2 and not o["values"].any()
    # the floor: zeros behind one value count as sv[0] 2^-40, so every value is finite
    o = model.order(np.array([3.0, 0, 0, 0], dtype=np.float32), 64, model.MDL)
    assert np.isfinite(o["values"]).all() and o["k"] == 1
    # two large values over a flat floor
    o = model.order(np.array([50, 30, 1, 1, 1, 1], dtype=np.float32), 256, model.AIC)
    assert o["k"] == 2
