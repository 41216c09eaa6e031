"""GPU checks of crsdr_spectra and its per-op form crsdr_welch against the fp64 numpy model in tests/spectra_model.py, whose docstring
derives the bars used here:

    psd, cross   |dev - model| <= 2^-24 (2 (7 log2 N + 1) + 2 T + 1) sqrt(s_a s_b) on the real and on the imaginary part of a bin,
                 s_c = max(P_c[f], mean bin power of row c), T = the most segments one fp32 chain accumulates (at most 32)
    align        the model evaluated on the device's own published fp32 psd / cross; the bar is the condition of the fp64 sums times
                 a small multiple of K 2^-53, carried through atan2, plus the one fp32 rounding

Everything else is equality of bits and derived, not measured: the per-op call and the engine launch the same kernels on the same
arguments, the fp32 chains are cut by (blocksize, nfft, overlap) alone and everything behind them is fp64 over the line's own packets,
so a line has the same bits wherever it sits in a batch, whatever nblocks is, and from the per-op call."""
import importlib

import numpy as np
import pytest

import spectra_model as M
from peak_cases import _bandlimited_rows

pytestmark = pytest.mark.gpu
EINVAL, ESTATE = -1, -5


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


class Packets:
    """T packet-shaped slots on the device, as a plan lays them out: packet t at base + t * stride, its matrix [nrows][B] at
    + 16 + 4 * nrows (4-byte aligned only when nrows is odd); pad: bytes between one packet's end and the next one's start."""

    def __init__(self, torch, blocks, pad=0):
        blocks = np.ascontiguousarray(blocks)
        self.T, self.nrows, self.B = blocks.shape
        self.offset = 16 + 4 * self.nrows
        self.stride = self.offset + self.nrows * self.B + pad
        host = np.full((self.T, self.stride), 0x55, dtype=np.int8)
        host[:, self.offset:self.offset + self.nrows * self.B] = blocks.reshape(self.T, -1)
        self.buf = torch.from_numpy(host).to(torch.device("cuda", 0))
        self.ptr = self.buf.data_ptr()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32)


def _same_bits(a, c):
    return a.shape == c.shape and np.array_equal(_bits(a), _bits(c))


def _band(N):
    return -(N // 4), N // 4 - 1


def _check_spectra(psd, cross, mats, N, overlap, window, tag):
    """device psd / cross of one line against the fp64 model within the derived bar; returns the largest error / bar"""
    B = np.asarray(mats[0]).shape[1]
    want_p, want_c = M.welch(mats, N, overlap, window)
    bp, bc = M.bars(want_p, N, M.terms(B, N, overlap))
    assert np.all(np.isfinite(psd)) and np.all(np.isfinite(cross.view(np.float32))), tag
    rp, rc = M.worst_ratio(psd.astype(np.float64), want_p, bp), M.worst_ratio(cross.astype(np.complex128), want_c, bc)
    print(f"{tag}: largest error / bar: psd {rp:.4f} cross {rc:.4f}")
    assert rp <= 1.0 and rc <= 1.0, (tag, rp, rc)
    assert _same_bits(cross[0].real, psd[0]) and not cross[0].imag.any(), tag      # S_0 = (P_0, 0), the 0 exact
    return max(rp, rc)


def _check_align(al, psd, cross, lo, hi, tag):
    """device figures against the model on the device's own fp32 arrays; rows with A == 0 or z == 0 (no bar): finite, coherence in [0, 1]"""
    want, bar = M.align(psd, cross, lo, hi)
    assert np.all(np.isfinite(al)) and np.all(al[:, 3] >= 0) and np.all(al[:, 3] <= 1), tag
    err = M.align_errors(al, want)
    live = bar[:, 0] > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        worst = float(np.max(np.where(live[:, None], err / bar, 0.0))) if live.any() else 0.0
    print(f"{tag}: align rows with a bar {int(live.sum())} of {len(live)}, largest error / bar {worst:.4f}")
    assert np.all(err[live] <= bar[live]), (tag, err[live], bar[live])


def _input(kind, nrows, B, N, seed):
    if kind == "gauss":
        return M.gaussian_matrix(nrows, B, seed)
    if kind == "full":
        return np.full((nrows, B), -128, dtype=np.int8)
    if kind == "zero":
        return np.zeros((nrows, B), dtype=np.int8)
    return M.tone_matrix(nrows, B, N, 3 if kind == "tone" else N - 2)


# (nrows, nfft, B, overlap, window, input).  Every second transform size (N = 16, 64, 256, 1024, 4096: a last pass of radix 16 or 4;
# N = 32, 128, 512, 2048 are tests/test_gpu_spectra_sizes.py's) with B = 2N (J = 1 in both overlaps), 4N (J = 2 / 3) and 6N; exactly
# one full fp32 chain per lane and one segment more (N = 16: 16 lanes of 32 segments, N = 64: 4 lanes, N = 256: one); nrows 2, 3 (the
# matrix only 4-byte aligned), 22, 66 and 5 (a workgroup takes one row, so every count is a multiple: 5 stands for "odd and small");
# both windows, both overlaps; Gaussian, full-scale, all-zero and on-bin tone inputs.
PEROP_CASES = [(3, N, f * N, ov, win, "gauss") for N in (16, 64, 256, 1024, 4096) for f, ov, win in ((2, 0, 0), (2, 1, 1), (4, 0, 1), (4, 1, 0), (6, 1, 1), (6, 0, 0))] + [
    (3, 16, 16384, 0, 1, "gauss"), (3, 16, 16384 + 32, 0, 1, "gauss"),
    (2, 64, 16384, 0, 0, "gauss"), (2, 64, 16384 + 128, 0, 0, "gauss"),
    (3, 256, 16384, 0, 1, "gauss"), (3, 256, 16384 + 512, 0, 1, "gauss"), (3, 256, 16384 + 512, 1, 1, "gauss"),
    (2, 64, 1024, 1, 1, "gauss"), (5, 64, 1024, 1, 0, "gauss"), (22, 256, 2048, 1, 1, "gauss"), (66, 64, 1024, 0, 1, "gauss"), (22, 4096, 16384, 1, 1, "gauss"),
    (3, 64, 1024, 1, 1, "full"), (3, 64, 1024, 0, 0, "full"), (3, 1024, 4096, 1, 1, "full"),
    (3, 64, 1024, 1, 1, "zero"), (3, 4096, 8192, 0, 0, "zero"),
    (3, 64, 1024, 1, 0, "tone"), (3, 256, 2048, 0, 1, "tone"), (3, 1024, 4096, 1, 1, "tone-neg"),
]


@pytest.mark.parametrize("nrows,N,B,overlap,window,kind", PEROP_CASES)
def test_per_op_against_the_model(b, nrows, N, B, overlap, window, kind):
    mat = _input(kind, nrows, B, N, 100 * N + B % 97 + nrows)
    lo, hi = _band(N)
    psd, cross, al = b.welch(mat, N, overlap, window, band=(lo, hi))
    tag = f"rows {nrows} nfft {N} B {B} overlap {overlap} window {window} {kind}"
    _check_spectra(psd, cross, [mat], N, overlap, window, tag)
    _check_align(al, psd, cross, lo, hi, tag)
    if kind == "zero":
        assert not psd.any() and not cross.view(np.float32).any() and not al.any()
    else:
        # row 0 against itself: S_0 = P_0 is real and positive, so A and z are, and every quotient is x / x
        assert np.array_equal(al[0], np.array([0, 0, 1, 1], dtype=np.float32)), al[0]
    if kind.startswith("tone"):
        peak = 3 if kind == "tone" else N - 2
        assert np.all(np.argmax(psd, axis=1) == peak)


def test_per_op_from_device_pointers_and_partial_outputs(b, torch):
    nrows, N, B = 3, 64, 1024
    mat = M.gaussian_matrix(nrows, B, 11)
    lo, hi = _band(N)
    psd, cross, al = b.welch(mat, N, 1, 1, band=(lo, hi))
    dev = torch.device("cuda", 0)
    pad = torch.zeros(4 + nrows * B, dtype=torch.int8, device=dev)           # the matrix 4 bytes into an allocation: 4-byte aligned only
    pad[4:] = torch.from_numpy(mat.reshape(-1)).to(dev)
    dp, dc, da = torch.zeros(nrows * N, device=dev), torch.zeros(nrows * N * 2, device=dev), torch.zeros(nrows * 4, device=dev)
    b.welch_device(dp.data_ptr(), dc.data_ptr(), da.data_ptr(), pad.data_ptr() + 4, nrows, B, N, 1, 1, lo, hi)
    assert _same_bits(dp.cpu().numpy().reshape(nrows, N), psd) and _same_bits(dc.cpu().numpy().reshape(nrows, N, 2), cross.view(np.float32).reshape(nrows, N, 2))
    assert _same_bits(da.cpu().numpy().reshape(nrows, 4), al)
    da.zero_()
    b.welch_device(0, 0, da.data_ptr(), pad.data_ptr() + 4, nrows, B, N, 1, 1, lo, hi)      # only the figures asked for
    assert _same_bits(da.cpu().numpy().reshape(nrows, 4), al)
    with pytest.raises(b.CrsdrError) as e:
        b.welch_device(dp.data_ptr(), dc.data_ptr() + 4, da.data_ptr(), pad.data_ptr() + 4, nrows, B, N, 1, 1, lo, hi)      # cross 8-byte aligned
    assert e.value.code == EINVAL


@pytest.mark.parametrize("frames", [1, 2])
@pytest.mark.parametrize("nrows,N,B,overlap,window", [(3, 64, 1024, 1, 1), (22, 256, 2048, 0, 0), (2, 16, 16384 + 32, 1, 1)])
def test_engine_lines_bits_and_figures(b, torch, frames, nrows, N, B, overlap, window):
    T = 4
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
        for t in (0, 1):
            p1, c1, a1 = b.welch(blocks[t], N, overlap, window, band=(lo, hi))
            assert _same_bits(p1, psd[t]) and _same_bits(c1.view(np.float32), cross[t].view(np.float32)) and _same_bits(a1, al[t]), t
    # the last line submitted alone: the same bits as at the end of the full batch, the same launch count
    sp.submit(pk.ptr + (T - frames) * pk.stride, pk.stride, pk.offset, frames)
    assert sp._last() == (1, 3)
    alone = sp.fetch()
    assert _same_bits(alone["psd"][0], psd[last]) and _same_bits(alone["cross"][0].view(np.float32), cross[last].view(np.float32)) and _same_bits(alone["align"][0], al[last])
    bufs = sp.device_buffers()
    assert bufs["psd"] and bufs["cross"] and bufs["align"]
    assert set(sp.fetch(psd=False, cross=False)) == {"align"}
    sp.close()


def test_refusals(b, torch):
    nrows, B, N = 5, 1024, 64
    sp = b.Spectra(nrows, B, N, 1, 1, max_batch=8, frames=2)
    fresh = b.Plan(nrows, B, b.MODE_FAITHFUL, max_batch=8)
    with pytest.raises(b.CrsdrError) as e:
        sp.submit_plan(fresh)                                                # nothing submitted
    assert e.value.code == ESTATE
    rows = np.stack([M.gaussian_matrix(nrows, B, 40 + t) for t in range(3)])
    fresh.submit(rows, seq=0)
    with pytest.raises(b.CrsdrError) as e:
        sp.submit_plan(fresh)                                                # a batch of 3 is not a multiple of frames = 2
    assert e.value.code == EINVAL
    fresh.sync()
    slab = torch.zeros(8 * (nrows - 1) * B, dtype=torch.int8, device=torch.device("cuda", 0))
    fresh.bind_slab(slab.data_ptr(), (nrows - 1) * B, 0, 8)
    with pytest.raises(b.CrsdrError) as e:
        sp.submit_plan(fresh)                                                # slab output: the matrix is not in the packet
    assert e.value.code == ESTATE
    fresh.close()
    other = b.Plan(nrows - 1, B, b.MODE_FAITHFUL, max_batch=8)
    with pytest.raises(b.CrsdrError) as e:
        sp.submit_plan(other)                                                # another nrows
    assert e.value.code == EINVAL
    other.close()
    pk = Packets(torch, rows[:2])
    for args in ((pk.ptr, pk.stride, pk.offset, 3), (pk.ptr, pk.stride, pk.offset, 10), (pk.ptr, pk.stride, pk.offset + 2, 2),
                 (pk.ptr, pk.stride + 2, pk.offset, 2), (0, pk.stride, pk.offset, 2)):
        with pytest.raises(b.CrsdrError) as e:
            sp.submit(*args)                                                 # nblocks % frames, > max_batch, alignment, NULL
        assert e.value.code == EINVAL
    sp.close()


@pytest.mark.parametrize("frac", [False, True])
def test_through_a_plan_on_the_packets_as_published(b, torch, frac):
    """a digital-mode plan with the reference noise on, the spectra behind it on the plan's stream with no host wait in between; the
    device against the model on the plan's own fetched packet.  frac: with crsdr_plan_set_frac_apply on, which changes the published rows"""
    L, N = 512, 64
    delays, phis = (37.3, -7.4, 63.25, 0.0), (0.4, -1.1, 2.5, 0.0)
    rows = _bandlimited_rows(L, delays, phis)
    nrows, B = rows.shape
    lo, hi = -(N // 10), N // 10
    plan = b.Plan(nrows, B, b.MODE_DIGITAL)
    if frac:
        plan.set_frac_apply(True, 1.0, None)
    sp = b.Spectra(nrows, B, N, 1, b.WINDOW_HANN, band=(lo, hi))
    for t in range(3):                                                       # (the plan's phasor settles; the last block is the one held against the model)
        plan.submit(rows, seq=t, flags=b.REFNOISE_ENABLED)
        sp.submit_plan(plan)
        out = sp.fetch()
        pub = plan.fetch()
    assert sp._last() == (1, 3)
    tag = f"plan frac {frac}"
    _check_spectra(out["psd"][0], out["cross"][0], [pub["matrix"]], N, 1, b.WINDOW_HANN, tag)
    _check_align(out["align"][0], out["psd"][0], out["cross"][0], lo, hi, tag)
    p1, c1, a1 = b.welch(pub["matrix"], N, 1, b.WINDOW_HANN, band=(lo, hi))
    assert _same_bits(p1, out["psd"][0]) and _same_bits(c1.view(np.float32), out["cross"][0].view(np.float32)) and _same_bits(a1, out["align"][0])
    print(tag, "lag", pub["lag"], "figures", out["align"][0])
    sp.close()
    plan.close()
