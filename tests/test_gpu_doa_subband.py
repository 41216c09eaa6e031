"""GPU checks of the subband covariance of crsdr_doa (crsdr_doa_set_subbands and its per-op form crsdr_subband_covariance) against the
fp64 numpy model in tests/doa_subband_model.py, whose docstring derives the bar used here:

    |dev - model| <= 2^-24 (2 (7 log2 N + 1) + 2 T + 1) sqrt(s_a s_b) on the real and on the imaginary part of a band's component,
    s_c = max(R_band[c][c], width * mean bin power of row c), T = the most segments one fp32 partial accumulates

Everything else is equality of bits and derived, not measured: the per-op call and the engine launch the same two kernels with a split
that depends on (blocksize, nfft) alone and read an estimate's packets through the same addresses, so an estimate has the same bits
alone, at the end of a batch and from the per-op call; and every stage behind the covariance is the existing one on nest * nbands
matrices."""
import importlib

import numpy as np
import pytest

import doa_peaks_model as peaks_model
import doa_subband_model as model
import ura

pytestmark = pytest.mark.gpu
EINVAL, ESTATE = -1, -5
SHAPES = {2: (2, 1), 21: (7, 3), 32: (8, 4), 33: (11, 3), 64: (8, 8)}


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
    + 16 + 4 * nrows."""

    def __init__(self, torch, blocks):
        blocks = np.ascontiguousarray(blocks)
        self.T, self.nrows, self.B = blocks.shape
        self.offset = 16 + 4 * self.nrows
        self.stride = self.offset + self.nrows * self.B
        host = np.full((self.T, self.stride), 0x55, dtype=np.int8)
        host[:, self.offset:] = blocks.reshape(self.T, -1)
        self.buf = torch.from_numpy(host).to(torch.device("cuda", 0))
        self.ptr = self.buf.data_ptr()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same_bits(a, c):
    return a.shape == c.shape and np.array_equal(_bits(a), _bits(c))


def _hermitian_in_bits(r):
    iu = np.triu_indices(r.shape[-1], 1)
    rt = np.swapaxes(r, -1, -2)
    return (np.array_equal(_bits(r.real[..., iu[0], iu[1]]), _bits(rt.real[..., iu[0], iu[1]]))
            and np.array_equal(_bits(r.imag[..., iu[0], iu[1]]), _bits(-rt.imag[..., iu[0], iu[1]]))
            and not np.einsum("...aa->...a", r.imag).any())


ARITH_CASES = [  # (m, nfft, B, frames, first, nbands, width, window)
    # every row count at which the blocks of 8 x 8 change: one block, 3 x 3 with a ragged edge, 4 x 4 full, 5 x 5 ragged, 8 x 8
    (2, 16, 512, 1, 14, 4, 4, 1),
    (21, 16, 512, 1, 14, 4, 4, 1),
    (32, 16, 512, 4, 5, 1, 1, 0),          # a single bin
    (33, 16, 512, 1, 0, 16, 1, 0),
    (64, 16, 512, 4, 15, 2, 8, 1),         # a wrapped first, the whole band in two halves
    # every transform size: one pass (8, 16), 8 x 4, 8 x 8, 16 x 8, 16 x 16
    (21, 8, 512, 4, 7, 1, 8, 1),           # the whole band as one, wrapped
    (21, 32, 512, 1, 30, 8, 4, 0),
    (21, 64, 512, 4, 0, 64, 1, 1),
    (21, 128, 512, 1, 100, 3, 40, 0),
    (21, 256, 512, 4, 0, 256, 1, 1),       # one segment per packet
    # one segment in all (B = 2 nfft), and three K slices of 66, 67 and 67 segments
    (21, 16, 32, 1, 0, 16, 1, 1),
    (21, 16, 32, 4, 14, 4, 4, 0),
    (21, 8, 3200, 1, 0, 8, 1, 1),
    (21, 8, 3200, 4, 6, 2, 3, 0),
]


@pytest.mark.parametrize("m,N,B,F,first,nbands,width,window", ARITH_CASES)
def test_arithmetic_bits_and_the_chain_behind_it(b, torch, m, N, B, F, first, nbands, width, window):
    T, ncx, ncy, k = 8, 19, 23, 1
    mx, my = SHAPES[m]
    rng = np.random.default_rng(1000 * m + 10 * N + F)
    blocks = rng.integers(-128, 128, size=(T, m + 1, B), dtype=np.int8)
    blocks[0, 1, :16] = -128
    pk = Packets(torch, blocks)
    doa = b.Doa(m + 1, B, k, ura.D, mx, my, ncx, ncy, max_batch=T, frames=F, flags=b.DOA_KEEP_RXX | b.DOA_KEEP_SPECTRUM)
    doa.set_subbands(N, first, nbands, width, window)
    with pytest.raises(b.CrsdrError) as e:
        doa.fetch_subbands()                                                     # nothing submitted since set_subbands
    assert e.value.code == ESTATE
    doa.submit(pk.ptr, pk.stride, pk.offset, T)
    nest = T // F
    assert doa._last() == (nest * nbands, 5)                                     # the plain engine's launch count
    out, power, vec = doa.fetch(), doa.fetch_subbands(), doa.fetch_subspace()
    rb = out["rxx"].reshape(nest, nbands, m, m)
    assert power.shape == (nest, nbands) and out["sv"].shape == (nest * nbands, m) and vec.shape == (nest * nbands, m, m)
    assert out["pm"].shape == (nest * nbands, ncx, ncy) and doa.subband_buffers()["power"]
    assert _hermitian_in_bits(rb)
    worst, Tterms = 0.0, model.terms(B, N)
    for e_ in range(nest):
        Rf = model.bin_covariances(list(blocks[e_ * F:(e_ + 1) * F]), N, window)
        want, pw = model.bands(Rf, first, nbands, width)
        bars = model.bar(Rf, first, nbands, width, Tterms)
        ratio = model.worst_ratio(rb[e_].astype(np.complex128), want, bars)
        worst = max(worst, ratio)
        assert ratio <= 1.0, (e_, ratio)
        # power is the fp64 trace / m of the values before their rounding: the diagonal's bars / m, and its own rounding
        assert np.all(np.abs(power[e_] - pw) <= np.einsum("iaa->i", bars) / m + model.U * pw), e_
    print(f"m {m} nfft {N} B {B} F {F} bands {first}:{nbands}:{width} window {window}: largest error / bar {worst:.4f}")
    # the per-op form on one packet, from host pointers: with one frame per estimate the same bits
    if F == 1:
        for t in (0, T - 1):
            r1, p1 = b.subband_covariance(blocks[t], N, first, nbands, width, window)
            assert _same_bits(r1, rb[t]) and _same_bits(p1, power[t]), t
    # the chain behind it: the existing subspace, scan and peak on the band matrices
    for i in sorted({0, 1 % (nest * nbands), nest * nbands - 1}):
        v1, s1 = b.noisesubspace(out["rxx"][i])
        assert _same_bits(s1, out["sv"][i]) and _same_bits(v1, vec[i]), i
        pm1 = b.pmusic2d(v1, k, ura.D, mx, my, ncx, ncy)
        assert _same_bits(pm1, out["pm"][i]), i
        g = int(np.argmax(peaks_model.keys(pm1)))
        assert out["peak"][i].tolist() == [g // ncy, g % ncy] and _bits(out["peak_value"][i:i + 1])[0] == _bits(pm1.reshape(-1)[g:g + 1])[0]
    # the last estimate submitted alone: the same bits as at the end of the full batch
    doa.submit(pk.ptr + (T - F) * pk.stride, pk.stride, pk.offset, F)
    assert doa._last() == (nbands, 5)
    alone, apower = doa.fetch(), doa.fetch_subbands()
    assert _same_bits(alone["rxx"], out["rxx"][(nest - 1) * nbands:]) and _same_bits(apower[0], power[nest - 1])
    assert _same_bits(alone["sv"], out["sv"][(nest - 1) * nbands:]) and _same_bits(alone["pm"], out["pm"][(nest - 1) * nbands:])
    doa.close()


def test_per_op_from_device_pointers(b, torch):
    m, N, B = 21, 64, 1024
    rng = np.random.default_rng(3)
    blk = rng.integers(-128, 128, size=(m + 1, B), dtype=np.int8)
    want, wpw = b.subband_covariance(blk, N, 60, 2, 8, b.WINDOW_HANN)
    dev = torch.device("cuda", 0)
    d_m = torch.from_numpy(blk).to(dev)
    d_r, d_p = torch.zeros(2 * m * m * 2, dtype=torch.float32, device=dev), torch.zeros(2, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    b.subband_covariance_device(d_r.data_ptr(), d_p.data_ptr(), d_m.data_ptr(), m + 1, B, N, 60, 2, 8, b.WINDOW_HANN)
    assert _same_bits(d_r.cpu().numpy().view(np.complex64).reshape(2, m, m), want) and _same_bits(d_p.cpu().numpy(), wpw)
    d_r.zero_()
    torch.cuda.synchronize()
    b.subband_covariance_device(d_r.data_ptr(), 0, d_m.data_ptr(), m + 1, B, N, 60, 2, 8, b.WINDOW_HANN)      # power may be NULL
    assert _same_bits(d_r.cpu().numpy().view(np.complex64).reshape(2, m, m), want)


@pytest.mark.parametrize("F", [1, 4])
def test_peaks_smoothing_and_order_per_band(b, torch, F):
    m, N, L, T, first, nbands, width, k = 21, 16, 1024, 8, 14, 4, 4, 1
    rng = np.random.default_rng(20 + F)
    blocks = np.stack([model.two_emitter_block(L, rng, n0=t * L) for t in range(T)])
    pk = Packets(torch, blocks)
    doa = b.Doa(m + 1, 2 * L, k, ura.D, 7, 3, max_batch=T, frames=F, flags=b.DOA_KEEP_RXX | b.DOA_KEEP_SPECTRUM)
    doa.set_subbands(N, first, nbands, width, b.WINDOW_HANN)
    doa.set_peaks(3, 2)
    doa.set_smoothing(5, 2, b.SMOOTH_FB)
    doa.set_order(b.ORDER_MDL, 1, 9, limit_directions=True)
    doa.submit(pk.ptr, pk.stride, pk.offset, T)
    nmat = T // F * nbands
    assert doa._last() == (nmat, 9)                                              # as the plain engine with the three of them on
    out, rs, vec, order, dirs = doa.fetch(), doa.fetch_smoothed(), doa.fetch_subspace(), doa.fetch_order(), doa.fetch_directions()
    assert rs.shape == (nmat, 10, 10) and vec.shape == (nmat, 10, 10) and order["k"].shape == (nmat,) and dirs["peaks"].shape == (nmat, 3, 2)
    nsnap = F * (L // N) * width                                                 # J' * width snapshots behind a band
    for i in range(nmat):
        rs1 = b.smooth_covariance(out["rxx"][i], 7, 3, 5, 2, b.SMOOTH_FB)
        assert _same_bits(rs1, rs[i]), i
        v1, s1 = b.noisesubspace(rs1)
        assert _same_bits(s1, out["sv"][i]) and _same_bits(v1, vec[i]), i
        k1, c1 = b.source_order(s1, nsnap, b.ORDER_MDL, 1, 9)
        assert k1 == order["k"][i] and _same_bits(c1, order["criterion"][i]), i
        pm1 = b.pmusic2d(v1, k1, ura.D, 5, 2, 100, 100)
        assert _same_bits(pm1, out["pm"][i]), i
        n, pts, vals = peaks_model.directions(pm1, 3, 2)
        n = min(n, k1)
        assert dirs["found"][i] == n and np.array_equal(dirs["peaks"][i][:n], np.asarray(pts)[:n]), i
        assert _same_bits(dirs["values"][i][:n], np.asarray(vals, dtype=np.float32)[:n]) and (dirs["peaks"][i][n:] == -1).all()
    doa.close()


def test_state_machine(b, torch):
    m, B, T = 21, 512, 8
    rng = np.random.default_rng(9)
    pk = Packets(torch, rng.integers(-128, 128, size=(T, m + 1, B), dtype=np.int8))
    plain = b.Doa(m + 1, B, 1, ura.D, 7, 3, 19, 23, max_batch=T, flags=b.DOA_KEEP_RXX | b.DOA_KEEP_SPECTRUM)
    plain.submit(pk.ptr, pk.stride, pk.offset, T)
    ref, ref_launches = plain.fetch(), plain.last_launches()
    plain.close()
    doa = b.Doa(m + 1, B, 1, ura.D, 7, 3, 19, 23, max_batch=T, flags=b.DOA_KEEP_RXX | b.DOA_KEEP_SPECTRUM)

    def refused(code, call, *args, **kw):
        with pytest.raises(b.CrsdrError) as e:
            call(*args, **kw)
        assert e.value.code == code, (call.__name__, args)

    # the limits that need an object: blocksize against nfft, and the matrices of a full batch
    refused(EINVAL, doa.set_subbands, 512, 0, 1, 1)
    refused(EINVAL, doa.set_subbands, 24, 0, 1, 1)
    refused(EINVAL, doa.set_subbands, 16, 0, 5, 4)
    refused(EINVAL, doa.set_subbands, 16, 16, 1, 1)
    refused(EINVAL, doa.set_subbands, 16, 0, 1, 1, 2)
    odd = b.Doa(m + 1, 96, 1, ura.D, 7, 3, 19, 23, max_batch=64)
    refused(EINVAL, odd.set_subbands, 32, 0, 1, 1)                               # 96 % 64
    odd.set_subbands(16, 0, 16, 1)                                               # 64 * 16 matrices
    odd.close()
    big = b.Doa(m + 1, 512, 1, ura.D, 7, 3, 4, 4, max_batch=64)
    refused(EINVAL, big.set_subbands, 256, 0, 65, 1)                             # 64 * 65 > 4096
    big.set_subbands(256, 0, 64, 1)
    big.close()
    # off while it is off: allowed, and nothing changes
    doa.set_subbands(0)
    refused(ESTATE, doa.fetch_subbands)
    assert doa.subband_buffers()["power"] is None
    # refused, on or off, while peaks, smoothing, order or beams are on
    for on, off in ((lambda: doa.set_peaks(2, 1), lambda: doa.set_peaks(0)),
                    (lambda: doa.set_smoothing(5, 2, b.SMOOTH_FB), lambda: doa.set_smoothing(7, 3, 0)),
                    (lambda: doa.set_order(b.ORDER_MDL, 1, 5), lambda: doa.set_order(b.ORDER_OFF)),
                    (lambda: doa.set_beams(b.BEAM_CONVENTIONAL), lambda: doa.set_beams(b.BEAM_OFF))):
        on()
        refused(ESTATE, doa.set_subbands, 16, 0, 16, 1)
        refused(ESTATE, doa.set_subbands, 0)
        off()
    doa.submit(pk.ptr, pk.stride, pk.offset, T)
    doa.set_subbands(16, 3, 2, 1, b.WINDOW_HANN)
    # the setter discards the last submit
    refused(ESTATE, doa.fetch)
    refused(ESTATE, doa.fetch_subspace)
    refused(ESTATE, doa.fetch_subbands)
    refused(ESTATE, doa._last)
    refused(ESTATE, doa.set_beams, b.BEAM_CONVENTIONAL)
    refused(ESTATE, doa.set_beams, b.BEAM_MVDR, 1e-2, [(1.0, 1.0)])
    doa.set_beams(b.BEAM_OFF)                                                    # off is no beam
    doa.submit(pk.ptr, pk.stride, pk.offset, T)
    assert doa._last() == (2 * T, ref_launches)
    assert doa.fetch()["rxx"].shape == (2 * T, m, m) and doa.fetch_subbands().shape == (T, 2)
    # and off again: the plain engine's bits
    doa.set_subbands(0)
    refused(ESTATE, doa.fetch)
    doa.submit(pk.ptr, pk.stride, pk.offset, T)
    assert doa._last() == (T, ref_launches)
    again = doa.fetch()
    for key in ("rxx", "sv", "pm", "peak", "peak_value", "status"):
        assert _same_bits(again[key], ref[key]), key
    doa.close()


@pytest.mark.parametrize("window", [0, 1])
def test_two_emitters_end_to_end(b, torch, window):
    N, L, T = 16, 2048, 4
    rng = np.random.default_rng(window)
    blocks = np.stack([model.two_emitter_block(L, rng, n0=t * L) for t in range(T)])
    pk = Packets(torch, blocks)
    # the plain engine on these packets: one direction per estimate, one of the two
    plain = b.Doa(22, 2 * L, 1, ura.D, 7, 3, max_batch=T)
    plain.submit(pk.ptr, pk.stride, pk.offset, T)
    seen = [tuple(p) for p in plain.fetch()["peak"].tolist()]
    assert all(p in model.EMITTER_PEAKS for p in seen), seen
    plain.close()
    doa = b.Doa(22, 2 * L, 1, ura.D, 7, 3, max_batch=T)
    doa.set_subbands(N, 0, N, 1, window)
    doa.submit(pk.ptr, pk.stride, pk.offset, T)
    out, power = doa.fetch(), doa.fetch_subbands()
    peak = out["peak"].reshape(T, N, 2)
    for t in range(T):
        Rf = model.bin_covariances([blocks[t]], N, window)
        _, pw = model.bands(Rf, 0, N, 1)
        near = {(f + d) % N for f in model.EMITTER_BINS16 for d in (-1, 0, 1)}
        assert min(pw[f] for f in model.EMITTER_BINS16) >= 10 * max(pw[f] for f in range(N) if f not in near), (t, pw)
        for f, want in zip(model.EMITTER_BINS16, model.EMITTER_PEAKS):
            _, pm = model.music_from_covariance(Rf[f], 1)
            g = np.unravel_index(np.argmax(pm), pm.shape)
            assert g == want and np.abs(peak[t, f] - np.asarray(g)).max() <= 1, (t, f, g, peak[t, f].tolist())
        # the band powers in the model's order, wherever the model separates two bands by more than the device's error
        order = np.argsort(pw)
        gaps = pw[order][1:] - pw[order][:-1]
        tol = 2.0 * model.U * (2.0 * (7.0 * 4.0 + 1.0) + 2.0 * model.terms(2 * L, N) + 2.0) * pw.max()
        assert np.all((power[t][order][1:] > power[t][order][:-1]) | (gaps <= tol)), (t, power[t], pw)
        assert {int(order[-1]), int(order[-2])} == set(model.EMITTER_BINS16)
        print(f"window {window} packet {t}: bins 3 and 11 at {peak[t, 3].tolist()} {peak[t, 11].tolist()}, power {power[t][3]:.3f} {power[t][11]:.3f}, "
              f"plain engine {seen[t]}")
    doa.close()
