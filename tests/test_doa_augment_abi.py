"""CPU checks of co-array augmentation of crsdr_doa (include/crsdr.h (iv): crsdr_doa_set_augment, crsdr_doa_fetch_augmented,
crsdr_doa_augment_buffers, crsdr_augment_covariance, crsdr_augment_lags): the symbols are declared, exported and bound, NULL objects and
bad arguments are refused before a device is looked for, and the host arithmetic of the lag counts gives its known answers and the
numpy restatement's (tests/doa_augment_model.py) on random masks."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

import doa_augment_model as model

EINVAL = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("crsdr_doa_set_augment", "crsdr_doa_fetch_augmented", "crsdr_doa_augment_buffers", "crsdr_augment_covariance", "crsdr_augment_lags")


@pytest.fixture(scope="module")
def b():
    binding = importlib.import_module("coherent-rtlsdr_amd.binding")
    binding.build()
    return binding


def test_symbols_declared_exported_and_bound(b):
    hdr = open(os.path.join(ROOT, "include", "crsdr.h")).read()
    declared = set(re.findall(r"\b(crsdr_[a-z0-9_]+)\s*\(", hdr))
    for s in NEW:
        assert s in declared and s in b.ABI_SYMBOLS and hasattr(b.lib(), s), s
    for s in ("set_augment", "fetch_augmented", "augment_buffers"):
        assert callable(getattr(b.Doa, s))
    assert callable(b.augment_covariance) and callable(b.augment_lags)
    assert "not guaranteed positive semidefinite" in hdr and "parity unpinned" in hdr


def test_mask_strings_are_in_element_order(b):
    assert b.mask_bits("1100101") == 0b1010011 == model.mask_of("1100101", 7)
    assert b.mask_bits([0, 1, 4, 6]) == 0b1010011 and b.mask_bits(0) == 0 and b.mask_bits(None) == 0
    assert bin(b.mask_bits(model.THINNED)).count("1") == 12 and bin(b.mask_bits(model.THINNED11)).count("1") == 11


def test_null_objects_are_refused(b):
    L = b.lib()
    p, i = C.c_void_p(), C.c_int()
    assert L.crsdr_doa_set_augment(None, 7, 3, 0) == EINVAL
    assert L.crsdr_doa_set_augment(None, 0, 0, 0) == EINVAL
    assert L.crsdr_doa_fetch_augmented(None, None) == EINVAL
    assert L.crsdr_doa_augment_buffers(None, C.byref(p), C.byref(i), C.byref(i)) == EINVAL
    r = np.zeros((21, 21), dtype=np.complex64)
    assert L.crsdr_augment_covariance(None, r.ctypes.data, 7, 3, 7, 3, 0, b.MEM_HOST) == EINVAL
    assert L.crsdr_augment_covariance(r.ctypes.data, None, 7, 3, 7, 3, 0, b.MEM_HOST) == EINVAL


BAD = [  # (mx, my, vx, vy, mask): refused by both calls for their sizes or mask
    (7, 3, 8, 3, 0),                      # vx > mx
    (7, 3, 7, 4, 0),                      # vy > my
    (7, 3, 1, 1, 0),                      # vx * vy = 1
    (7, 3, 0, 3, 0),
    (13, 5, 5, 2, 0),                     # m = 65
    (1, 1, 1, 1, 0),
    (7, 3, 7, 3, 1 << 21),                # a mask bit >= m
    (7, 3, 7, 3, 1 << 63),
    (7, 3, 7, 3, 1 << 5),                 # a one-bit mask
]


def test_bad_arguments_are_refused_before_a_device_is_looked_for(b):
    L = b.lib()
    r, ra = np.zeros((65, 65), dtype=np.complex64), np.zeros((65, 65), dtype=np.complex64)
    n = C.c_int(-1)
    for mx, my, vx, vy, mask in BAD:
        assert L.crsdr_augment_covariance(ra.ctypes.data, r.ctypes.data, mx, my, vx, vy, mask, b.MEM_HOST) == EINVAL, (mx, my, vx, vy, mask)
        assert L.crsdr_augment_lags(mx, my, vx, vy, mask, None, C.byref(n)) == EINVAL, (mx, my, vx, vy, mask)
    # an uncovered lag: the per-op call refuses and names it, the lag call answers with the count
    mask = b.mask_bits("1100100")
    assert L.crsdr_augment_covariance(ra.ctypes.data, r.ctypes.data, 7, 1, 7, 1, mask, b.MEM_HOST) == EINVAL
    text = L.crsdr_last_error().decode()
    assert "(ux, uy) = (2, 0)" in text and "3 uncovered" in text, text
    assert L.crsdr_augment_lags(7, 1, 7, 1, mask, None, C.byref(n)) == 0 and n.value == 3
    assert L.crsdr_augment_lags(7, 1, 7, 1, mask, None, None) == 0
    assert L.crsdr_augment_covariance(ra.ctypes.data, r.ctypes.data, 7, 3, 7, 3, 0, 7) == EINVAL      # mem_kind


def test_lag_counts_known_answers(b):
    counts, missing = b.augment_lags(7, 3, 7, 3)
    assert missing == 0 and counts.shape == (3, 13)
    for uy in range(3):
        for ux in range(-6, 7):
            assert counts[uy, ux + 6] == (7 - abs(ux)) * (3 - uy), (ux, uy)
    # the ruler: elements 0, 1, 4, 6 of seven in a row
    counts, missing = b.augment_lags(7, 1, 7, 1, model.RULER)
    assert missing == 0 and counts[0, 6:].tolist() == [4, 1, 1, 1, 1, 1, 1] and counts[0, :7].tolist() == [1, 1, 1, 1, 1, 1, 4]
    counts, missing = b.augment_lags(7, 1, 7, 1, "1100100")
    assert missing == 3 and [u for u in range(7) if counts[0, 6 + u] == 0] == [2, 5, 6]
    for mask in (model.THINNED, model.THINNED11, model.dead(21, (4, 16))):
        counts, missing = b.augment_lags(7, 3, 7, 3, mask)
        assert missing == 0 and counts.min() >= 1, mask
    # a virtual array smaller than the physical one counts its own lags only
    counts, missing = b.augment_lags(7, 3, 5, 2, model.dead(21, (4, 16)))
    assert counts.shape == (2, 9) and missing == 0


def test_lag_counts_equal_the_models_on_random_masks(b):
    rng = np.random.default_rng(11)
    uncovered = 0
    for _ in range(200):
        mx = int(rng.integers(1, 17))
        my = int(rng.integers(1 if mx > 1 else 2, 64 // mx + 1))
        m = mx * my
        vx, vy = int(rng.integers(1, mx + 1)), int(rng.integers(1, my + 1))
        if vx * vy < 2:
            vx, vy = (2, 1) if mx >= 2 else (1, 2)
        bits = rng.random(m) < rng.uniform(0.4, 1.0)
        bits[rng.choice(m, 2, replace=False)] = True
        mask = sum(1 << i for i in range(m) if bits[i])
        counts, missing = b.augment_lags(mx, my, vx, vy, mask)
        want, wmiss = model.lag_counts(mx, my, vx, vy, mask)
        assert np.array_equal(counts, want) and missing == wmiss, (mx, my, vx, vy, hex(mask))
        uncovered += missing > 0
    assert 0 < uncovered < 200                                                    # both kinds of mask were met
