"""CPU checks of the band beams of crsdr_doa (include/crsdr.h: crsdr_doa_set_subband_beams, crsdr_doa_fetch_subband_beams,
crsdr_doa_subband_beam_buffers, crsdr_subband_beamform): the symbols are declared, exported and bound, a NULL object and arguments
outside the limits are refused before any device use, and the fp64 numpy model the GPU tests compare against
(tests/doa_subband_beams_model.py) has the properties its definition promises: a float32 restatement of the arithmetic in either order
stays inside the derived bar and every single mistake leaves it, the power identity with the band covariance, and the three-emitter
scene the feature was specified from (two emitters on one carrier, a third on another), which the fp64 pipeline separates."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

import doa_beams_model as beams_model
import doa_subband_beams_model as model
import doa_subband_model as sb

EINVAL = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("crsdr_doa_set_subband_beams", "crsdr_doa_fetch_subband_beams", "crsdr_doa_subband_beam_buffers", "crsdr_subband_beamform")


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
    for s in ("set_subband_beams", "fetch_subband_beams", "subband_beam_buffers"):
        assert callable(getattr(b.Doa, s))
    assert callable(b.subband_beamform) and callable(b.subband_beamform_device)
    assert "[nblocks][nbands][nbeams][J][width][2]" in hdr and "c_w = 1 / sqrt(N sum_n w[n]^2)" in hdr
    assert b.lib().crsdr_abi_version() == 1


def test_null_object_and_bad_arguments_are_refused(b):
    L = b.lib()
    ang = (C.c_float * 2)(1.0, 1.0)
    assert L.crsdr_doa_set_subband_beams(None, b.BEAM_MVDR, 1e-2, 0, None) == EINVAL
    assert L.crsdr_doa_set_subband_beams(None, b.BEAM_OFF, 0.0, 1, ang) == EINVAL
    assert L.crsdr_doa_fetch_subband_beams(None, None, None, None) == EINVAL
    p, n = C.c_void_p(), C.c_int()
    assert L.crsdr_doa_subband_beam_buffers(None, C.byref(p), C.byref(p), C.byref(p), C.byref(n)) == EINVAL
    # the per-op form validates before it looks for a device: every limit of the definition, one case each
    m, B = 4, 1024
    mat = np.zeros((m + 1, B), dtype=np.int8)
    w = np.zeros((256, 16, m), dtype=np.complex64)
    out = np.zeros(16 * B // 2, dtype=np.complex64)
    f32p, i8p = C.POINTER(C.c_float), C.POINTER(C.c_int8)
    call = lambda nrows, blocksize, nfft, first, nbands, width, window, nbeams, kind=None: L.crsdr_subband_beamform(
        out.view(np.float32).ctypes.data_as(f32p), mat.ctypes.data_as(i8p), nrows, blocksize, nfft, first, nbands, width, window,
        w.view(np.float32).ctypes.data_as(f32p), nbeams, b.MEM_HOST if kind is None else kind)
    bad = {
        "nfft below 8": (m + 1, B, 4, 0, 1, 1, 0, 1),
        "nfft above 256": (m + 1, B, 512, 0, 1, 1, 0, 1),
        "nfft no power of two": (m + 1, 960, 24, 0, 1, 1, 0, 1),
        "blocksize no multiple of 2 nfft": (m + 1, 1024 - 32, 64, 0, 1, 1, 0, 1),
        "nbands * width above nfft": (m + 1, B, 16, 0, 5, 4, 0, 1),
        "no band": (m + 1, B, 16, 0, 0, 1, 0, 1),
        "no bin": (m + 1, B, 16, 0, 1, 0, 0, 1),
        "first negative": (m + 1, B, 16, -1, 1, 1, 0, 1),
        "first beyond the bins": (m + 1, B, 16, 16, 1, 1, 0, 1),
        "window": (m + 1, B, 16, 0, 1, 1, 2, 1),
        "one row": (1, B, 16, 0, 1, 1, 0, 1),
        "more than 64 signal rows": (66, B, 16, 0, 1, 1, 0, 1),
        "no beam": (m + 1, B, 16, 0, 1, 1, 0, 0),
        "more than 16 beams": (m + 1, B, 16, 0, 1, 1, 0, 17),
    }
    for what, args in bad.items():
        assert call(*args) == EINVAL, what
    assert call(m + 1, B, 16, 0, 1, 1, 0, 1, kind=7) == EINVAL
    assert L.crsdr_subband_beamform(None, mat.ctypes.data_as(i8p), m + 1, B, 16, 0, 1, 1, 0, w.view(np.float32).ctypes.data_as(f32p), 1, b.MEM_HOST) == EINVAL
    assert L.crsdr_subband_beamform(out.view(np.float32).ctypes.data_as(f32p), mat.ctypes.data_as(i8p), m + 1, B, 16, 0, 1, 1, 0, None, 1, b.MEM_HOST) == EINVAL


def _case(m, N, J, rng, nbands, nbeams):
    """a full-scale matrix (-128 included) and weights of the size of real ones (|u_c| about 1 / m), the last slot empty"""
    mat = rng.integers(-128, 128, size=(m + 1, 2 * N * J), dtype=np.int8)
    mat[1, :8] = -128
    w = ((rng.standard_normal((nbands, nbeams, m)) + 1j * rng.standard_normal((nbands, nbeams, m))) / m).astype(np.complex64)
    if nbeams > 1:
        w[:, -1] = 0
    return mat, w


BAR_CASES = [  # (m, N, J, first, nbands, width, nbeams): the (m, N, J) of the specification
    (2, 8, 1, 7, 2, 3, 1),
    (21, 16, 64, 14, 4, 4, 3),
    (33, 64, 8, 0, 64, 1, 2),
    (64, 256, 4, 250, 3, 5, 2),
    (21, 128, 3, 100, 3, 40, 4),
]


@pytest.mark.parametrize("kind", [model.WINDOW_RECT, model.WINDOW_HANN])
@pytest.mark.parametrize("m,N,J,first,nbands,width,nbeams", BAR_CASES)
def test_bar_holds_a_float32_restatement_in_both_orders_and_no_single_mistake(m, N, J, first, nbands, width, nbeams, kind):
    rng = np.random.default_rng(1000 * N + m)
    mat, w = _case(m, N, J, rng, nbands, nbeams)
    want = model.beams(mat, w, N, first, nbands, width, kind)
    bars = model.bar(mat, w, N, first, nbands, width, kind)
    tight = model.bar(mat, w, N, first, nbands, width, kind, transform_first=True)
    assert want.shape == bars.shape == (nbands, nbeams, J, width) and np.all(tight <= bars)
    for order in ("transform_first", "sum_first"):
        got = model.beams_f32(mat, w, N, first, nbands, width, kind, order)
        ratio = model.worst_ratio(got, want, bars)
        print(f"float32 restatement, {order}: worst error / bar = {ratio:.4f}")
        assert ratio <= 1.0, order
        if order == "transform_first":
            ratio = model.worst_ratio(got, want, tight)
            print(f"float32 restatement, {order}: worst error / bar_transform_first = {ratio:.4f}")
            assert ratio <= 1.0
    if nbeams > 1:
        assert not want[:, -1].any() and not bars[:, -1].any()                    # an empty slot: zeros, and no allowance
    # not too loose: one mistake anywhere leaves it
    for which in model.MUTATIONS:
        if (which == "segment" and J == 1) or (which == "sum_w2" and kind == model.WINDOW_RECT):
            continue                                                             # no mistake there: one segment has nothing to shift, rect has sum w^2 = N
        wrong = model.mutated(mat, w, N, first, nbands, width, kind, which)
        live = slice(0, max(nbeams - 1, 1))
        ratio = model.worst_ratio(wrong[:, live], want[:, live], bars[:, live])
        print(f"{which}: error / bar = {ratio:.0f}")
        assert ratio > 1.0, which


@pytest.mark.parametrize("kind", [model.WINDOW_RECT, model.WINDOW_HANN])
def test_mean_power_of_a_beam_is_the_quadratic_form_of_the_band_covariance(kind):
    """(1 / J') sum |Y|^2 over an estimate's packets, segments and band bins = u^H R_band u, 1e-12 relative in fp64; and with a rect
    window the bands of all bins add up to the beam's mean sample power (Parseval)."""
    m, N, J, F = 5, 16, 12, 2
    rng = np.random.default_rng(4)
    mats = [rng.integers(-128, 128, size=(m + 1, 2 * N * J), dtype=np.int8) for _ in range(F)]
    w = (rng.standard_normal((4, 2, m)) + 1j * rng.standard_normal((4, 2, m))) / m
    rb, _ = sb.subband_covariance(mats, N, 14, 4, 4, kind)
    Y = np.stack([model.beams(mt, w, N, 14, 4, 4, kind) for mt in mats])
    got, want = model.band_power(Y), np.einsum("ibc,icd,ibd->ib", w.conj(), rb, w).real
    assert np.max(np.abs(got - want)) <= 1e-12 * np.max(want)
    if kind == model.WINDOW_RECT:
        w1 = np.repeat(w[:1], 4, axis=0)
        Y = np.stack([model.beams(mt, w1, N, 14, 4, 4, kind) for mt in mats])
        y = np.concatenate([beams_model.beams(mt, w1[0]) for mt in mats], axis=1)
        assert np.max(np.abs(model.band_power(Y).sum(axis=0) - np.mean(np.abs(y) ** 2, axis=1))) <= 1e-12


def test_three_emitters_two_on_one_carrier():
    """The scene of the feature's fp64 study (7 x 3 URA, L = 8192, nfft 16, rect window, k = 2, MVDR loading 1e-2, set_peaks(4, 2),
    default_rng(5)): MVDR own >= 0.95 and the other emitter of the carrier <= 0.05 for both slots of bin 3 and for bin 11, the weak
    slot's conventional leak at least ten times its MVDR leak, the two largest MVDR powers of bin 3 at the two emitters."""
    blk, sig = model.three_emitter_block()
    band, sigs = {}, {}
    for f in (3, 11):
        found, peaks, vec, sv = model.fp64_band([blk], f)
        slots = beams_model.following_slots(found, peaks)
        wm, pw = beams_model.slot_weights(vec, sv, slots, model.MVDR, model.LOADING)
        wc, _ = beams_model.slot_weights(vec, sv, slots, model.CONVENTIONAL, 0.0)
        ym = model.beams(blk, wm[None], model.NFFT, f, 1, 1, model.WINDOW_RECT)[0, :, :, 0]
        yc = model.beams(blk, wc[None], model.NFFT, f, 1, 1, model.WINDOW_RECT)[0, :, :, 0]
        band[f], sigs[f] = (found, peaks, ym, yc, pw), model.channelised(sig, model.NFFT, f, model.WINDOW_RECT)
    model.check_three_emitters(sigs, band, "fp64")
