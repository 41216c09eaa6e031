"""CPU checks of the subband covariance of crsdr_doa (include/crsdr.h: crsdr_doa_set_subbands, crsdr_doa_fetch_subbands,
crsdr_doa_subband_buffers, crsdr_subband_covariance): the symbols are declared, exported and bound, a NULL object and arguments outside
the limits are refused before any device use, and the fp64 numpy model the GPU tests compare against (tests/doa_subband_model.py) has
the properties its definition promises: Parseval, the Hann normalisation, wrapped bands, the two-emitter scene the feature was
specified from, and an error bar that a float32 restatement of the kernel's arithmetic meets and every single mistake misses."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

import doa_subband_model as model
import ura

EINVAL = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("crsdr_doa_set_subbands", "crsdr_doa_fetch_subbands", "crsdr_doa_subband_buffers", "crsdr_subband_covariance")


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
    for s in ("set_subbands", "fetch_subbands", "subband_buffers"):
        assert callable(getattr(b.Doa, s))
    assert callable(b.subband_covariance) and callable(b.subband_covariance_device)
    for name, value in (("WINDOW_RECT", 0), ("WINDOW_HANN", 1)):
        assert getattr(b, name) == value == getattr(model, name) and re.search(r"\bCRSDR_%s\s*=\s*%d" % (name, value), hdr), name
    assert "No mean is removed" in hdr and "e * nbands + i" in hdr


def test_null_object_and_bad_arguments_are_refused(b):
    L = b.lib()
    p = C.c_void_p()
    pw = np.zeros(16, dtype=np.float32)
    assert L.crsdr_doa_set_subbands(None, 16, 0, 16, 1, 0) == EINVAL
    assert L.crsdr_doa_set_subbands(None, 0, 0, 0, 0, 0) == EINVAL
    assert L.crsdr_doa_fetch_subbands(None, pw.ctypes.data_as(C.POINTER(C.c_float))) == EINVAL
    assert L.crsdr_doa_subband_buffers(None, C.byref(p)) == EINVAL
    # the per-op form validates before it looks for a device: every limit of the definition, one case each
    m, B = 4, 1024
    mat = np.zeros((m + 1, B), dtype=np.int8)
    rb, f32p, i8p = np.zeros((256, m, m), dtype=np.complex64), C.POINTER(C.c_float), C.POINTER(C.c_int8)
    call = lambda nrows, blocksize, nfft, first, nbands, width, window, kind=None: L.crsdr_subband_covariance(
        rb.view(np.float32).ctypes.data_as(f32p), pw.ctypes.data_as(f32p), mat.ctypes.data_as(i8p), nrows, blocksize, nfft, first, nbands, width, window,
        b.MEM_HOST if kind is None else kind)
    bad = {
        "nfft below 8": (m + 1, B, 4, 0, 1, 1, 0),
        "nfft above 256": (m + 1, B, 512, 0, 1, 1, 0),
        "nfft no power of two": (m + 1, 960, 24, 0, 1, 1, 0),
        "blocksize no multiple of 2 nfft": (m + 1, 1024 - 32, 64, 0, 1, 1, 0),
        "nbands * width above nfft": (m + 1, B, 16, 0, 5, 4, 0),
        "no band": (m + 1, B, 16, 0, 0, 1, 0),
        "no bin": (m + 1, B, 16, 0, 1, 0, 0),
        "first negative": (m + 1, B, 16, -1, 1, 1, 0),
        "first beyond the bins": (m + 1, B, 16, 16, 1, 1, 0),
        "window": (m + 1, B, 16, 0, 1, 1, 2),
        "one row": (1, B, 16, 0, 1, 1, 0),
        "more than 64 signal rows": (66, B, 16, 0, 1, 1, 0),
    }
    for what, args in bad.items():
        assert call(*args) == EINVAL, what
    assert call(m + 1, B, 16, 0, 1, 1, 0, kind=7) == EINVAL
    assert L.crsdr_subband_covariance(None, None, mat.ctypes.data_as(i8p), m + 1, B, 16, 0, 1, 1, 0, b.MEM_HOST) == EINVAL


def _full_scale(rng, m, B, frames=1):
    return [rng.integers(-128, 128, size=(m + 1, B), dtype=np.int8) for _ in range(frames)]


def test_split_is_a_function_of_blocksize_and_nfft():
    assert model.spb(32, 16) == 1 and model.spb(2048, 16) == 1 and model.spb(4096, 16) == 2 and model.spb(1 << 20, 8) == 16
    assert model.slice_bounds(3200, 8) == [(0, 66), (66, 133), (133, 200)] and model.terms(3200, 8) == 67
    for B, N in ((512, 8), (3200, 8), (1 << 16, 256), (1 << 18, 16)):
        bounds = model.slice_bounds(B, N)
        assert bounds[0][0] == 0 and bounds[-1][1] == B // (2 * N) and all(a[1] == c[0] and a[0] < a[1] for a, c in zip(bounds, bounds[1:]))


@pytest.mark.parametrize("N", [8, 16, 64, 256])
def test_parseval_rect_window(N):
    """sum_f R_f = (1/L') sum conj(x_a) x_b: one band of all bins equals the raw second moment, 1e-12 relative (measured: 1e-15)"""
    rng = np.random.default_rng(N)
    mats = _full_scale(rng, 5, 4 * N * 3, frames=2)
    rb, pw = model.subband_covariance(mats, N, 3, 1, N, model.WINDOW_RECT)
    x = np.concatenate([model.samples(mt) for mt in mats], axis=1)
    raw = x.conj() @ x.T / x.shape[1]
    assert np.max(np.abs(rb[0] - raw)) <= 1e-12 * np.max(np.abs(raw))
    assert abs(pw[0] - np.trace(raw).real / 5) <= 1e-12 * pw[0]
    # and the bands of a split add up to it
    rb4, pw4 = model.subband_covariance(mats, N, N - 2, 4, N // 4, model.WINDOW_RECT)
    assert np.max(np.abs(rb4.sum(axis=0) - raw)) <= 1e-12 * np.max(np.abs(raw))


def test_hann_normalisation_on_white_noise():
    """A unit-power white row: E |X[f]|^2 = sum w^2, so every bin has power 1 / N and the bands sum to 1.  Adjacent Hann bins are
    correlated but segments are not, and |X[f]|^2 of a Gaussian bin has unit relative spread: the sum over N bins of the mean over J'
    segments has a standard deviation below sqrt(N / J') / N * (1 + 2 * (2/3)^2 + 2 * (1/6)^2)^(1/2) < 1.4 / sqrt(N J') (the Hann
    window's bin-to-bin power correlations are (2/3)^2 and (1/6)^2); 5 sigma."""
    N, J, m = 32, 2048, 3
    rng = np.random.default_rng(5)
    x = (rng.standard_normal((m, N * J)) + 1j * rng.standard_normal((m, N * J))) / np.sqrt(2.0)
    w = model.window(N, model.WINDOW_HANN)
    assert abs(np.sum(w * w) - 0.375 * N) < 1e-12
    X = np.fft.fft(x.reshape(m, J, N) * w, axis=2)
    power = np.sum(np.abs(X) ** 2, axis=1) / (J * N * np.sum(w * w))             # [m][N]: R_f[a][a]
    spread = 5 * 1.4 / np.sqrt(N * J)
    assert np.all(np.abs(power.sum(axis=1) - 1.0) < spread), (power.sum(axis=1), spread)
    # the same through the model's int8 path at amplitude 30 (quantisation noise 1/12 per component)
    mat = np.zeros((m + 1, 2 * N * J), dtype=np.int8)
    mat[1:] = ura.quantise(30.0 * x)
    _, pw = model.subband_covariance([mat], N, 0, N, 1, model.WINDOW_HANN)
    want = (900.0 + 1.0 / 6.0) / 127.0 ** 2
    assert abs(pw.sum() - want) < (spread + 1e-3) * want


def test_wrapped_band_sums_the_right_bins():
    N = 16
    assert model.band_bins(N, N - 2, 1, 4) == [[14, 15, 0, 1]]
    assert model.band_bins(N, 14, 4, 4) == [[14, 15, 0, 1], [2, 3, 4, 5], [6, 7, 8, 9], [10, 11, 12, 13]]
    mats = _full_scale(np.random.default_rng(2), 4, 512)
    Rf = model.bin_covariances(mats, N, model.WINDOW_HANN)
    rb, pw = model.bands(Rf, N - 2, 1, 4)
    assert np.array_equal(rb[0], Rf[[14, 15, 0, 1]].sum(axis=0)) and pw[0] == np.trace(rb[0]).real / 4


@pytest.mark.parametrize("B", [4096, 1024])
@pytest.mark.parametrize("kind", [model.WINDOW_RECT, model.WINDOW_HANN])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_two_emitters_on_two_carriers(seed, kind, B):
    """The scene of the feature's fp64 study: the time-domain covariance with k = 1 sees one of the two directions, the bins of the
    two carriers see one each, exactly on the grid, and stand 10 x above every bin not adjacent to an occupied one."""
    N = 16
    blk = model.two_emitter_block(B // 2, np.random.default_rng(seed))
    Rf = model.bin_covariances([blk], N, kind)
    for f, want in zip(model.EMITTER_BINS16, model.EMITTER_PEAKS):
        sv, pm = model.music_from_covariance(Rf[f], 1)
        assert np.unravel_index(np.argmax(pm), pm.shape) == want, (f, want)
        assert sv[0] / sv[1] > 100, (f, sv[:2])
    # the plain engine's view: one spectrum, one peak, a second singular value of the same order as the first
    _, _, sv, pm = ura.music_fp64(blk, 1)
    g = tuple(int(v) for v in np.unravel_index(np.argmax(pm), pm.shape))
    assert g in model.EMITTER_PEAKS and sv[0] / sv[1] < 5, (g, sv[:2])
    power = np.einsum("faa->f", Rf).real / Rf.shape[1]
    near = {(f + d) % N for f in model.EMITTER_BINS16 for d in (-1, 0, 1)}
    rest = max(power[f] for f in range(N) if f not in near)
    assert min(power[f] for f in model.EMITTER_BINS16) >= 10 * rest, power
    # four bands of four bins from bin 14 wrap around and put the emitters in bands 1 and 3
    _, pw = model.bands(Rf, 14, 4, 4)
    assert sorted(np.argsort(pw)[2:].tolist()) == [1, 3], pw


BAR_CASES = [  # (m, N, B, frames, first, nbands, width)
    (5, 16, 512, 1, 0, 16, 1),
    (5, 16, 512, 2, 14, 4, 4),
    (3, 8, 3200, 1, 7, 1, 8),          # three slices of 66, 67, 67 segments
    (4, 64, 1024, 1, 60, 2, 8),
    (3, 256, 2048, 1, 0, 256, 1),
]


@pytest.mark.parametrize("kind", [model.WINDOW_RECT, model.WINDOW_HANN])
@pytest.mark.parametrize("m,N,B,frames,first,nbands,width", BAR_CASES)
def test_bar_holds_a_float32_restatement_and_no_single_mistake(m, N, B, frames, first, nbands, width, kind):
    rng = np.random.default_rng(100 * N + m)
    mats = _full_scale(rng, m, B, frames)
    mats[0][1, :8] = -128                                                       # full scale includes -128
    Rf = model.bin_covariances(mats, N, kind)
    want, pw = model.bands(Rf, first, nbands, width)
    bars = model.bar(Rf, first, nbands, width, model.terms(B, N))
    got, gpw = model.subband_covariance_f32(mats, N, first, nbands, width, kind)
    ratio = model.worst_ratio(got, want, bars)
    print("float32 restatement: worst error / bar = %.3f" % ratio)
    assert ratio <= 1.0
    assert np.all(np.abs(gpw - pw) <= np.einsum("iaa->i", bars) / m + model.U * pw)
    # not too loose: one mistake anywhere leaves it
    for which in model.MUTATIONS:
        if which == "last_segment" and frames * B // (2 * N) == 1:
            continue
        wrong, _ = model.mutated(mats, N, first, nbands, width, kind, which)
        if (which == "bin" and nbands == 1 and width == N) or (which == "sum_w2" and kind == model.WINDOW_RECT):
            continue                                                             # no mistake there: one band of every bin has nothing to shift, rect has sum w^2 = N
        assert model.worst_ratio(wrong, want, bars) > 1.0, which
