"""CPU checks of crsdr_doa_set_peaks / crsdr_doa_fetch_directions / crsdr_doa_direction_buffers (include/crsdr.h (iv)): the symbols
are declared, exported and bound, a NULL object is refused, and the numpy restatement the GPU tests compare against
(tests/doa_peaks_model.py) gives the known answers of hand-built spectra.

The spectra are pyramids, pm = max_i (A_i - s_i (|cx - x_i| + |cy - y_i|)): one step towards the centre of the pyramid that sets a
point's value raises it by s_i, so with radius >= 1 only centres can be local peaks, and the answers follow by hand."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

import doa_peaks_model as model

EINVAL = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("crsdr_doa_set_peaks", "crsdr_doa_fetch_directions", "crsdr_doa_direction_buffers")


@pytest.fixture(scope="module")
def b():
    binding = importlib.import_module("coherent-rtlsdr_amd.binding")
    binding.build()
    return binding


def _pyramids(shape, tops, slope=1.0):
    cx, cy = np.indices(shape)
    pm = np.full(shape, -np.inf)
    for x, y, a in tops:
        pm = np.maximum(pm, a - slope * (np.abs(cx - x) + np.abs(cy - y)))
    return pm.astype(np.float32)


def _check(got, found, peaks, values):
    n, p, v = got
    count = len(p)
    assert n == found, (n, p, v)
    exp_p = np.full((count, 2), -1, dtype=np.int32)
    exp_v = np.full(count, -1.0, dtype=np.float32)
    exp_p[:len(peaks)] = peaks
    exp_v[:len(values)] = values
    assert np.array_equal(p, exp_p), p
    assert np.array_equal(v.view(np.uint32), exp_v.view(np.uint32)), v


def test_symbols_declared_exported_and_bound(b):
    hdr = open(os.path.join(ROOT, "include", "crsdr.h")).read()
    declared = set(re.findall(r"\b(crsdr_[a-z0-9_]+)\s*\(", hdr))
    for s in NEW:
        assert s in declared and s in b.ABI_SYMBOLS and hasattr(b.lib(), s), s
    for s in ("set_peaks", "fetch_directions", "direction_buffers"):
        assert callable(getattr(b.Doa, s))


def test_null_object_is_refused(b):
    L = b.lib()
    assert L.crsdr_doa_set_peaks(None, 4, 1) == EINVAL
    assert L.crsdr_doa_set_peaks(None, 0, 0) == EINVAL
    assert L.crsdr_doa_fetch_directions(None, None, None, None) == EINVAL
    p = C.c_void_p()
    assert L.crsdr_doa_direction_buffers(None, C.byref(p), C.byref(p), C.byref(p)) == EINVAL


def test_two_separated_peaks():
    pm = _pyramids((12, 15), [(3, 4, 50.0), (8, 11, 45.0)])
    _check(model.directions(pm, 4, 1), 2, [(3, 4), (8, 11)], [50.0, 45.0])
    _check(model.directions(pm, 1, 1), 1, [(3, 4)], [50.0])            # capped at count


def test_a_peak_on_an_edge_and_one_in_a_corner():
    # (0, 6) on the first row, (9, 14) the last point of the grid: clipped windows, nothing wraps round to the opposite edge
    pm = _pyramids((10, 15), [(0, 6, 40.0), (9, 14, 45.0)])
    for r in (1, 2, 4):
        _check(model.directions(pm, 3, r), 2, [(9, 14), (0, 6)], [45.0, 40.0])


def test_a_plateau_resolves_to_its_lowest_index():
    # 1 x 20: a run of four equal values at cy = 5 .. 8, falling away on both sides: exactly cy = 5 is the peak
    cy = np.arange(20)
    pm = (20.0 - np.maximum(0, np.maximum(5 - cy, cy - 8))).astype(np.float32)[None, :]
    assert np.array_equal(pm[0, 5:9], [20, 20, 20, 20]) and pm.min() > 0
    for r in (1, 2, 3):
        _check(model.directions(pm, 4, r), 1, [(0, 5)], [20.0])
    assert np.flatnonzero(model.is_local_peak(pm, 1)[0]).tolist() == [5]


def test_a_side_lobe_inside_the_radius():
    # main lobe 50 at (5, 5), side lobe 47 at (5, 8), slope 2: at r = 1 the side lobe beats its window (largest neighbour (5, 7) = 46);
    # at r = 2 the main lobe's flank (5, 6) = 48 is in it, at r = 3 the main lobe itself
    pm = _pyramids((12, 14), [(5, 5, 50.0), (5, 8, 47.0)], slope=2.0)
    assert pm[5, 8] == 47.0 and pm[5, 7] == 46.0 and pm[5, 6] == 48.0
    _check(model.directions(pm, 4, 1), 2, [(5, 5), (5, 8)], [50.0, 47.0])
    _check(model.directions(pm, 4, 2), 1, [(5, 5)], [50.0])
    _check(model.directions(pm, 4, 3), 1, [(5, 5)], [50.0])


def test_a_nan_ranks_first():
    pm = _pyramids((10, 10), [(2, 2, 50.0)])
    pm[6, 6] = np.float32("nan")
    n, p, v = model.directions(pm, 3, 1)
    assert n == 2 and p[:2].tolist() == [[6, 6], [2, 2]] and p[2].tolist() == [-1, -1]
    assert v.view(np.uint32)[0] == 0x7FC00000 and v[1] == 50.0 and v[2] == -1.0
    # a NaN with another payload is the same canonical key
    pm[6, 6] = np.array([0x7FC00123], dtype=np.uint32).view(np.float32)[0]
    assert model.keys(pm)[6, 6] == (0x7FC00000 << 32) | (0xFFFFFFFF - 66)
    assert model.directions(pm, 3, 1)[1][0].tolist() == [6, 6]


def test_fewer_peaks_than_count_on_a_3x3_grid():
    pm = _pyramids((3, 3), [(1, 1, 5.0)])
    _check(model.directions(pm, 16, 1), 1, [(1, 1)], [5.0])
    n, p, v = model.directions(pm, 16, 1)
    assert (p[1:] == -1).all() and (v[1:] == -1.0).all()


def test_batch_form_stacks_the_estimates():
    pm = np.stack([_pyramids((6, 7), [(1, 2, 9.0)]), _pyramids((6, 7), [(4, 5, 8.0), (0, 0, 7.0)])])
    out = model.batch_directions(pm, 2, 1)
    assert out["found"].tolist() == [1, 2]
    assert out["peaks"].tolist() == [[[1, 2], [-1, -1]], [[4, 5], [0, 0]]]
    assert out["values"].tolist() == [[9.0, -1.0], [8.0, 7.0]]
