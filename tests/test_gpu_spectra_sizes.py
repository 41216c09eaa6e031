"""GPU checks of the k_spectra<LG> instantiations that tests/test_gpu_spectra.py does not run: nfft = 32, 128, 512 and 2048, i.e. a last
pass of radix 2 and of radix 8, the lane splits of N = 32 and 128 (8 and 2 lanes) and the slot counts of N = 512 and 2048 (2 and 8 slots a
thread); at every nfft from 16 to 4096, where each bit of the bin index lands behind digit_reverse<LG>; and the end of an fp32 chain at
N = 1024 and 4096, which that file runs at N = 16, 64 and 256 alone.

The model and the bars are tests/spectra_model.py's, the checks tests/test_gpu_spectra.py's own functions: nothing here is measured, and
no tolerance is added.  The bin-order test needs no bar at all: an on-bin tone of amplitude 50 holds all of its power but the quantiser's
(1 / 12 LSB^2 a part) in one bin (rect) or in that bin and a quarter of it in either neighbour (Hann), so the largest bin is the tone's."""
import importlib

import numpy as np
import pytest

import spectra_model as M
from test_gpu_spectra import ESTATE, Packets, _band, _check_align, _check_spectra, _same_bits

pytestmark = pytest.mark.gpu
SIZES = (32, 128, 512, 2048)                                                     # the rest of 16 .. 4096: tests/test_gpu_spectra.py


@pytest.fixture(scope="module")
def b():
    binding = importlib.import_module("coherent-rtlsdr_amd.binding")
    if binding.device_count() < 1:
        pytest.fail("no HIP device: the product path has no CPU fallback")
    return binding


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


def _per_op(b, nrows, N, B, overlap, window):
    mat = M.gaussian_matrix(nrows, B, 100 * N + B % 97 + nrows)
    lo, hi = _band(N)
    psd, cross, al = b.welch(mat, N, overlap, window, band=(lo, hi))
    tag = f"rows {nrows} nfft {N} B {B} overlap {overlap} window {window} gauss"
    _check_spectra(psd, cross, [mat], N, overlap, window, tag)
    _check_align(al, psd, cross, lo, hi, tag)
    assert np.array_equal(al[0], np.array([0, 0, 1, 1], dtype=np.float32)), al[0]      # row 0 against itself: every quotient is x / x


# (nfft, B / nfft, overlap, window): the six combinations of test_gpu_spectra.PEROP_CASES at every size it leaves out
@pytest.mark.parametrize("N,f,overlap,window", [(N, f, ov, win) for N in SIZES for f, ov, win in ((2, 0, 0), (2, 1, 1), (4, 0, 1), (4, 1, 0), (6, 1, 1), (6, 0, 0))])
def test_per_op_against_the_model(b, N, f, overlap, window):
    _per_op(b, 3, N, f * N, overlap, window)


# (nrows, nfft, B, window): exactly one full fp32 chain per lane at hop N (N = 32: 8 lanes of 32 segments, N = 128: 2 lanes, N = 512 and
# 2048: one lane, 4 and 16 chunks of 8 and 2 segments), and one segment more; each in both overlaps (at hop N / 2 a packet has twice the
# segments less one, so full chains and a last one that is a segment short or starts over).  The bar takes T from spectra_model.terms.
CHAIN_CASES = [(3, 32, 16384, 1), (3, 32, 16384 + 64, 1), (2, 128, 16384, 0), (2, 128, 16384 + 256, 0), (3, 512, 32768, 1), (3, 512, 32768 + 1024, 1),
               (2, 2048, 131072, 0), (2, 2048, 131072 + 4096, 0),
               # the two sizes of tests/test_gpu_spectra.py that have no such shape there: 4 and 16 slots a thread, 8 and 32 chunks a chain
               (2, 1024, 65536, 1), (2, 1024, 65536 + 2048, 1), (2, 4096, 262144, 0), (2, 4096, 262144 + 8192, 0)]


@pytest.mark.parametrize("overlap", [0, 1])
@pytest.mark.parametrize("nrows,N,B,window", CHAIN_CASES)
def test_a_full_chain_per_lane_and_one_segment_more(b, nrows, N, B, window, overlap):
    assert M.segments(B, N, 0) - M.CHAIN * max(M.THREADS // N, 1) in (0, 1) and M.terms(B, N, overlap) == M.CHAIN      # the shape is what it is here for
    _per_op(b, nrows, N, B, overlap, window)


@pytest.mark.parametrize("window", [M.WINDOW_RECT, M.WINDOW_HANN])
@pytest.mark.parametrize("N", [16, 32, 64, 128, 256, 512, 1024, 2048, 4096])
def test_every_bit_of_the_bin_index_lands_in_its_place(b, N, window):
    """an on-bin tone at bin 2^k, k < log2 N, and at N - 1: each power of two moves one bit of the index through digit_reverse<LG> (and
    through the pass that makes it), so a swapped or shifted digit is named by the bins that land wrong; N - 1 sets them all.  White
    noise, whose model spectrum is flat, cannot be relied on to show a permutation.  Hop N under rect, N / 2 under Hann."""
    nrows, B, overlap = 2, 4 * N, 1 if window == M.WINDOW_HANN else 0
    bins = [1 << k for k in range(N.bit_length() - 1)] + [N - 1]
    got = []
    for f in bins:
        mat = M.tone_matrix(nrows, B, N, f)
        psd, cross, _ = b.welch(mat, N, overlap, window)
        assert np.all(np.isfinite(psd))
        got.append(np.argmax(psd, axis=1).tolist())
        if f == N - 1:
            _check_spectra(psd, cross, [mat], N, overlap, window, f"nfft {N} window {window} tone at bin {f}")
    assert got == [[f] * nrows for f in bins], (N, window, dict(zip(bins, got)))


@pytest.mark.parametrize("frames", [1, 2])
def test_engine_lines_bits_and_figures(b, torch, frames):
    """the engine at one of the sizes above, two lanes: a line's bits wherever it sits in a batch, alone, and from the per-op call"""
    nrows, N, B, overlap, window, T = 3, 128, 2048, 1, 1, 4
    blocks = np.stack([M.gaussian_matrix(nrows, B, 500 + 10 * N + t) for t in range(T)])
    if frames == 1:
        blocks[3] = blocks[0]                                                 # the same line at positions 0 and 3
    else:
        blocks[2:] = blocks[:2]                                               # ... and, two packets a line, at lines 0 and 1
    pk = Packets(torch, blocks, pad=40)                                       # a stride larger than the packet
    lo, hi = _band(N)
    sp = b.Spectra(nrows, B, N, overlap, window, band=(lo, hi), max_batch=8, frames=frames)      # nblocks < max_batch
    with pytest.raises(b.CrsdrError) as e:
        sp.fetch()
    assert e.value.code == ESTATE
    sp.submit(pk.ptr, pk.stride, pk.offset, T)
    nest = T // frames
    assert sp._last() == (nest, 3)
    out = sp.fetch()
    psd, cross, al = out["psd"], out["cross"], out["align"]
    assert psd.shape == (nest, nrows, N) and cross.shape == (nest, nrows, N) and al.shape == (nest, nrows, 4)
    for e_ in range(nest):
        tag = f"engine rows {nrows} nfft {N} B {B} frames {frames} line {e_}"
        _check_spectra(psd[e_], cross[e_], list(blocks[e_ * frames:(e_ + 1) * frames]), N, overlap, window, tag)
        _check_align(al[e_], psd[e_], cross[e_], lo, hi, tag)
    last = nest - 1
    assert _same_bits(psd[0], psd[last]) and _same_bits(cross[0].view(np.float32), cross[last].view(np.float32)) and _same_bits(al[0], al[last])
    if frames == 1:
        assert not _same_bits(psd[0], psd[1])
        for t in (0, 1):
            p1, c1, a1 = b.welch(blocks[t], N, overlap, window, band=(lo, hi))
            assert _same_bits(p1, psd[t]) and _same_bits(c1.view(np.float32), cross[t].view(np.float32)) and _same_bits(a1, al[t]), t
    # the last line submitted alone: the same bits as at the end of the full batch, the same launch count
    sp.submit(pk.ptr + (T - frames) * pk.stride, pk.stride, pk.offset, frames)
    assert sp._last() == (1, 3)
    alone = sp.fetch()
    assert _same_bits(alone["psd"][0], psd[last]) and _same_bits(alone["cross"][0].view(np.float32), cross[last].view(np.float32)) and _same_bits(alone["align"][0], al[last])
    sp.close()
