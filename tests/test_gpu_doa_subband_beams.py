"""GPU checks of the band beams of crsdr_doa (crsdr_doa_set_subband_beams / crsdr_doa_fetch_subband_beams / crsdr_subband_beamform)
against the fp64 restatement (tests/doa_subband_beams_model.py) fed with what the device published -- fetch_subspace, sv, peak or
peaks / found per (estimate, band), the weights and the packets.

Bars, derived, not measured:
  weights  |u_dev - u_model|_inf <= 2^-22 |u_model|_inf per slot and power to 2^-22 relative: the bars of tests/test_gpu_doa_beams.py (the
           same kernel, launched over nest * nbands matrices).  Empty slots exactly 0 / -1.
  beams    per sample and component the model's bar_transform_first (its docstring derives it; the kernel transforms every row first),
           with the model using the device's fp32 weights.  Every entry.  Empty slots 0.
  power    (1 / J') sum |Y|^2 against u^H R_band u from the fetched rxx: what the beams' bar and doa_subband_model.bar allow.
Everything else is equality of bits: crsdr_subband_beamform on the same matrix and the fetched weights, an estimate alone and at the end
of a batch, and every other output with the beams switched off again.
The three-emitter scene is the one of tests/test_doa_subband_beams_abi.py (same seed), where the fp64 pipeline meets the same conditions."""
import importlib

import numpy as np
import pytest

import doa_beams_model as beams_model
import doa_subband_beams_model as model
import doa_subband_model as sb
import ura

pytestmark = pytest.mark.gpu
EINVAL, ESTATE = -1, -5
P = np.pi
REL = 2.0 ** -22
SHAPES = {2: (2, 1), 21: (7, 3), 33: (11, 3), 64: (8, 8)}
FIXED = np.array([[0.5 * P, 0.5 * P], [0.3 * P, 0.61 * P], [2.0, 1.0]], dtype=np.float32)


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


def _slots(doa, i, dirs, peak, fixed):
    """the model's slots of matrix i = e * nbands + band: fixed angles, the matrix's peaks, or its one peak"""
    if fixed is not None:
        return [tuple(float(x) for x in np.asarray(ang, dtype=np.float32)) for ang in fixed]
    if dirs is not None:
        return beams_model.following_slots(int(dirs["found"][i]), dirs["peaks"][i], doa.ncx, doa.ncy)
    return [beams_model.grid_angles(int(peak[i][0]), int(peak[i][1]), doa.ncx, doa.ncy)]


def _check_against_model(b, doa, blocks, n, mode, loading, mx, my, geom, fixed=None, per_op=(0,), what=""):
    """Everything the device published for the last submit of n blocks against the model; returns the fetched dict."""
    N, first, nbands, width, window = geom
    F, m, J = doa.frames, doa.m, doa.B // (2 * N)
    nest, nb = n // F, doa.nbandbeams
    out, vec = doa.fetch(), doa.fetch_subspace()
    dirs = doa.fetch_directions() if doa.npeaks else None
    got = doa.fetch_subband_beams()
    assert got["weights"].shape == (nest * nbands, nb, m) and got["power"].shape == (nest * nbands, nb)
    assert got["beams"].shape == (n, nbands, nb, J, width)
    assert np.isfinite(got["weights"].view(np.float32)).all() and np.isfinite(got["beams"].view(np.float32)).all()
    worst_w = worst_p = worst_y = 0.0
    for i in range(nest * nbands):
        slots = _slots(doa, i, dirs, out["peak"], fixed)
        assert len(slots) == nb
        w, p = beams_model.slot_weights(vec[i], out["sv"][i], slots, mode, loading, ura.D, mx, my)
        for s_, ang in enumerate(slots):
            e, band = divmod(i, nbands)
            if ang is None:
                assert not got["weights"][i, s_].any() and got["power"][i, s_] == -1.0, (what, i, s_)
                assert not got["beams"][e * F:(e + 1) * F, band, s_].any(), (what, i, s_)
                continue
            dw, ref = np.abs(got["weights"][i, s_].astype(np.complex128) - w[s_].astype(np.complex128)).max(), np.abs(w[s_]).max()
            worst_w = max(worst_w, dw / ref)
            assert dw <= REL * ref, (what, "weights", i, s_, dw, ref)
            dp = abs(float(got["power"][i, s_]) - float(p[s_]))
            worst_p = max(worst_p, dp / max(abs(float(p[s_])), 1e-300))
            assert dp <= REL * abs(float(p[s_])), (what, "power", i, s_, got["power"][i, s_], p[s_])
    W = got["weights"].reshape(nest, nbands, nb, m)
    for t in range(n):
        want = model.beams(blocks[t], W[t // F], N, first, nbands, width, window)
        bars = model.bar(blocks[t], W[t // F], N, first, nbands, width, window, transform_first=True)
        ratio = model.worst_ratio(got["beams"][t].astype(np.complex128), want, bars)
        worst_y = max(worst_y, ratio)
        assert ratio <= 1.0, (what, "beams", t, ratio)
    for t in per_op:
        if t < n:
            one = b.subband_beamform(blocks[t], W[t // F], N, first, nbands, width, window)
            assert _same_bits(one, got["beams"][t]), (what, "crsdr_subband_beamform", t)
    print(f"{what}: n {n} slots {nb}: worst weights {worst_w / REL:.3f} and power {worst_p / REL:.3f} of the 2^-22 bar, largest beam error / bar {worst_y:.4f}")
    return got


ARITH_CASES = [  # (m, nfft, B, frames, first, nbands, width, window, slots)
    (2, 16, 32, 1, 15, 2, 3, 0, "peak"),           # the smallest packet: one segment, wrapped bands, one slot
    (21, 16, 4096, 1, 0, 16, 1, 1, "peaks3"),      # every bin a band; two K slices
    (33, 32, 512, 4, 30, 8, 4, 0, "fixed"),        # 8 x 4, bands of four bins covering all, wrapped
    (64, 64, 1024, 1, 5, 1, 1, 1, "peaks16"),      # 8 x 8, one band of one bin
    (21, 128, 256, 4, 100, 3, 40, 0, "peak"),      # 16 x 8, one segment per packet, wide wrapped bands
    (64, 256, 4096, 1, 250, 3, 5, 1, "peaks3"),    # 16 x 16, a segment of all rows is 128 KiB of LDS
    (33, 256, 512, 4, 0, 256, 1, 0, "fixed"),      # 256 bands: their weights pass through LDS in groups
    (64, 16, 2048, 4, 14, 4, 4, 1, "peaks16"),     # 64 rows x 16 slots: two bands of weights at a time
    (2, 64, 4096, 1, 60, 2, 8, 0, "peaks16"),
    (21, 8, 3200, 1, 6, 2, 3, 1, "peak"),          # three K slices of 66, 67 and 67 segments, chunks of 30
]


@pytest.mark.parametrize("m,N,B,F,first,nbands,width,window,slots", ARITH_CASES)
def test_weights_power_and_every_beam_sample(b, torch, m, N, B, F, first, nbands, width, window, slots):
    T, ncx, ncy, k = 8, 19, 23, 1
    mx, my = SHAPES[m]
    rng = np.random.default_rng(1000 * m + 10 * N + F)
    blocks = rng.integers(-128, 128, size=(T, m + 1, B), dtype=np.int8)
    blocks[0, 1, :16] = -128
    blocks[2] = 0                                                                # an all-zero packet
    pk = Packets(torch, blocks)
    mode, loading = (b.BEAM_MVDR, 1e-2) if window else (b.BEAM_CONVENTIONAL, 0.0)
    doa = b.Doa(m + 1, B, k, ura.D, mx, my, ncx, ncy, max_batch=T, frames=F)
    doa.set_subbands(N, first, nbands, width, window)
    base = 5
    if slots in ("peaks3", "peaks16"):
        doa.set_peaks(3 if slots == "peaks3" else 16, 16 if slots == "peaks3" else 4)      # windows so wide that slots stay empty
        base = 7
    fixed = FIXED if slots == "fixed" else None
    doa.set_subband_beams(mode, loading if mode == b.BEAM_MVDR else 0.5, fixed_angles=fixed)
    assert doa.nbandbeams == {"peak": 1, "peaks3": 3, "peaks16": 16, "fixed": 3}[slots]
    with pytest.raises(b.CrsdrError) as e:
        doa.fetch_subband_beams()                                                # nothing submitted since
    assert e.value.code == ESTATE
    doa.submit(pk.ptr, pk.stride, pk.offset, T)
    assert doa._last() == (T // F * nbands, base + 2)
    geom = (N, first, nbands, width, window)
    what = f"m {m} nfft {N} B {B} F {F} bands {first}:{nbands}:{width} window {window} {slots}"
    got = _check_against_model(b, doa, blocks, T, mode, loading, mx, my, geom, fixed=fixed, per_op=(0, T - 1), what=what)
    if doa.npeaks:
        found = doa.fetch_directions()["found"]
        assert (found >= 1).all() and (found < doa.npeaks).any(), found
    assert not got["beams"][2].any()                                             # the all-zero packet
    if F == 1:
        live = got["power"][2 * nbands:3 * nbands] != -1.0
        assert live[:, 0].all() and (got["power"][2 * nbands:3 * nbands][live] == 0.0).all()
    # the last estimate submitted alone: the same bits as at the end of the full batch
    doa.submit(pk.ptr + (T - F) * pk.stride, pk.stride, pk.offset, F)
    assert doa._last() == (nbands, base + 2)
    alone = doa.fetch_subband_beams()
    assert _same_bits(alone["beams"], got["beams"][T - F:]) and _same_bits(alone["weights"], got["weights"][(T // F - 1) * nbands:])
    assert _same_bits(alone["power"], got["power"][(T // F - 1) * nbands:])
    doa.close()


def test_per_op_from_device_pointers(b, torch):
    m, N, B, geom = 21, 64, 1024, (60, 2, 8, b.WINDOW_HANN)
    rng = np.random.default_rng(3)
    blk = rng.integers(-128, 128, size=(m + 1, B), dtype=np.int8)
    w = ((rng.standard_normal((2, 3, m)) + 1j * rng.standard_normal((2, 3, m))) / m).astype(np.complex64)
    want = b.subband_beamform(blk, w, N, *geom)
    ratio = model.worst_ratio(want.astype(np.complex128), model.beams(blk, w, N, *geom), model.bar(blk, w, N, *geom, transform_first=True))
    assert ratio <= 1.0, ratio
    dev = torch.device("cuda", 0)
    d_m, d_w = torch.from_numpy(blk).to(dev), torch.from_numpy(w.view(np.float32)).to(dev)
    d_o = torch.zeros(want.size * 2, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    b.subband_beamform_device(d_o.data_ptr(), d_m.data_ptr(), m + 1, B, N, *geom, d_w.data_ptr(), 3)
    assert _same_bits(d_o.cpu().numpy().view(np.complex64).reshape(want.shape), want)


@pytest.mark.parametrize("window", [0, 1])
def test_mean_power_is_the_quadratic_form_of_the_band_covariance(b, torch, window):
    """(1 / J') sum |Y|^2 over an estimate's packets, segments and band bins against u^H R_band u with the fetched rxx and weights.
    Allowance: a component of Y within its bar moves |Y|^2 by at most 2 (|Re Y| + |Im Y|) bar + 2 bar^2, and a component of R_band within
    doa_subband_model.bar moves the form by at most sum_ab |u_a| |u_b| sqrt(2) bar_ab; fp64 arithmetic on both sides."""
    m, N, L, T, F, first, nbands, width = 21, 16, 1024, 4, 2, 14, 4, 4
    rng = np.random.default_rng(30 + window)
    blocks = np.stack([sb.two_emitter_block(L, rng, n0=t * L) for t in range(T)])
    pk = Packets(torch, blocks)
    doa = b.Doa(m + 1, 2 * L, 1, ura.D, 7, 3, max_batch=T, frames=F, flags=b.DOA_KEEP_RXX)
    doa.set_subbands(N, first, nbands, width, window)
    doa.set_peaks(2, 2)
    doa.set_subband_beams(b.BEAM_MVDR, 1e-2)
    doa.submit(pk.ptr, pk.stride, pk.offset, T)
    got, rxx = doa.fetch_subband_beams(), doa.fetch()["rxx"].reshape(T // F, nbands, m, m).astype(np.complex128)
    W = got["weights"].reshape(T // F, nbands, 2, m).astype(np.complex128)
    worst = 0.0
    for e in range(T // F):
        mats = list(blocks[e * F:(e + 1) * F])
        Y = got["beams"][e * F:(e + 1) * F].astype(np.complex128)
        ybar = np.stack([model.bar(mt, W[e], N, first, nbands, width, window, transform_first=True) for mt in mats])
        lhs = model.band_power(Y)
        lhs_allow = np.sum(2.0 * (np.abs(Y.real) + np.abs(Y.imag)) * ybar + 2.0 * ybar ** 2, axis=(0, 3, 4)) / (F * Y.shape[3])
        rbar = sb.bar(sb.bin_covariances(mats, N, window), first, nbands, width, sb.terms(2 * L, N))
        rhs = np.einsum("ibc,icd,ibd->ib", W[e].conj(), rxx[e], W[e]).real
        rhs_allow = np.sqrt(2.0) * np.einsum("ibc,icd,ibd->ib", np.abs(W[e]), rbar, np.abs(W[e]))
        live = got["power"].reshape(T // F, nbands, 2)[e] != -1.0
        assert live.any() and np.all(np.abs(lhs - rhs) <= lhs_allow + rhs_allow), (e, lhs, rhs)
        worst = max(worst, float(np.max(np.abs(lhs - rhs)[live] / (lhs_allow + rhs_allow)[live])))
        assert np.all(lhs[live] > 0) and not lhs[~live].any()
    print(f"window {window}: largest |mean |Y|^2 - u^H R u| / allowance {worst:.4f}")
    doa.close()


def test_state_rules(b, torch):
    m, B, T = 21, 512, 8
    rng = np.random.default_rng(9)
    blocks = rng.integers(-128, 128, size=(T, m + 1, B), dtype=np.int8)
    pk = Packets(torch, blocks)
    doa = b.Doa(m + 1, B, 1, ura.D, 7, 3, 19, 23, max_batch=T)
    lib = b.lib()

    def refused(code, call, *args, **kw):
        with pytest.raises(b.CrsdrError) as e:
            call(*args, **kw)
        assert e.value.code == code, (call.__name__, args)

    # subbands off: refused, off is allowed; the arguments are checked first
    refused(ESTATE, doa.set_subband_beams, b.BEAM_CONVENTIONAL)
    refused(ESTATE, doa.set_subband_beams, b.BEAM_MVDR, 1e-2, FIXED)
    doa.set_subband_beams(b.BEAM_OFF)
    refused(ESTATE, doa.fetch_subband_beams)
    ang = np.zeros((17, 2), dtype=np.float32)
    for mode, loading, fixed in ((3, 1e-2, None), (-1, 1e-2, None), (b.BEAM_MVDR, 0.0, None), (b.BEAM_MVDR, 5e-7, None), (b.BEAM_MVDR, 1.5, None),
                                 (b.BEAM_MVDR, float("nan"), None), (b.BEAM_CONVENTIONAL, 0.0, ang), (b.BEAM_MVDR, 1e-2, ang)):
        refused(EINVAL, doa.set_subband_beams, mode, loading, fixed_angles=fixed)
    assert lib.crsdr_doa_set_subband_beams(doa._h, b.BEAM_MVDR, 1e-2, -1, None) == EINVAL
    assert lib.crsdr_doa_set_subband_beams(doa._h, b.BEAM_MVDR, 1e-2, 2, None) == EINVAL      # fixed directions and no angles
    # wideband beams are untouched by the new call's off
    doa.set_beams(b.BEAM_CONVENTIONAL)
    doa.set_subband_beams(b.BEAM_OFF)
    assert doa.beam_buffers()["nbeams"] == 1 and doa.subband_beam_buffers()["nbeams"] == 0
    doa.set_beams(b.BEAM_OFF)
    doa.set_subbands(16, 3, 2, 1, b.WINDOW_HANN)
    # true sub-arrays: refused both ways; forward-backward averaging alone is fine
    doa.set_smoothing(5, 2, 0)
    refused(ESTATE, doa.set_subband_beams, b.BEAM_CONVENTIONAL)
    doa.set_smoothing(7, 3, b.SMOOTH_FB)
    doa.set_subband_beams(b.BEAM_MVDR, 1e-2)
    refused(ESTATE, doa.set_smoothing, 5, 2, 0)
    refused(ESTATE, doa.set_smoothing, 5, 2, b.SMOOTH_FB)
    bufs = doa.subband_beam_buffers()
    assert bufs["nbeams"] == 1 and all(bufs[key] for key in ("weights", "power", "beams"))
    # the wideband calls keep to the wideband beams
    refused(ESTATE, doa.set_beams, b.BEAM_CONVENTIONAL)
    refused(ESTATE, doa.fetch_beams)
    wide = doa.beam_buffers()
    assert wide["nbeams"] == 0 and all(wide[key] is None for key in ("weights", "power", "beams"))
    doa.set_beams(b.BEAM_OFF)                                                    # off is no beam, and not these beams' switch
    assert doa.subband_beam_buffers()["nbeams"] == 1
    # subbands, on or off, and the peaks while the beams follow them
    refused(ESTATE, doa.set_subbands, 16, 0, 16, 1)
    refused(ESTATE, doa.set_subbands, 0)
    refused(ESTATE, doa.set_peaks, 4, 1)
    refused(ESTATE, doa.set_peaks, 0)
    refused(ESTATE, doa.fetch_subband_beams)                                     # before a submit
    doa.submit(pk.ptr, pk.stride, pk.offset, T)
    assert doa._last() == (2 * T, 8)                                             # 5, smoothing, the two beam launches
    assert doa.fetch_subband_beams()["beams"].shape == (T, 2, 1, B // 32, 1)
    # fixed beams are not sized by the count
    doa.set_subband_beams(b.BEAM_CONVENTIONAL, fixed_angles=FIXED)
    doa.set_peaks(3, 2)
    doa.set_order(b.ORDER_MDL, 1, 2, limit_directions=True)
    doa.submit(pk.ptr, pk.stride, pk.offset, T)
    assert doa._last() == (2 * T, 11)
    _check_against_model(b, doa, blocks, T, b.BEAM_CONVENTIONAL, 0.0, 7, 3, (16, 3, 2, 1, b.WINDOW_HANN), fixed=FIXED, what="fixed, peaks and order on")
    # following beams see the capped found: at most k_e <= 2 of the three slots
    doa.set_subband_beams(b.BEAM_OFF)
    refused(ESTATE, doa.fetch_subband_beams)
    doa.set_subband_beams(b.BEAM_MVDR, 1e-2)
    doa.submit(pk.ptr, pk.stride, pk.offset, T)
    assert doa._last() == (2 * T, 11)
    dirs, order = doa.fetch_directions(), doa.fetch_order()
    assert (dirs["found"] <= order["k"]).all() and (dirs["found"] <= 2).all()
    got = _check_against_model(b, doa, blocks, T, b.BEAM_MVDR, 1e-2, 7, 3, (16, 3, 2, 1, b.WINDOW_HANN), what="following the capped directions")
    assert (got["power"][:, 2] == -1.0).all() and not got["beams"][:, :, 2].any()
    doa.close()


def test_switching_off_restores_the_object_and_launches_rise_by_two(b, torch):
    m, L, T, geom = 21, 512, 16, (16, 14, 4, 4, 1)
    rng = np.random.default_rng(5)
    pk = Packets(torch, np.stack([sb.two_emitter_block(L, rng, n0=t * L) for t in range(T)]))
    mk = lambda: b.Doa(m + 1, 2 * L, 1, ura.D, ura.MX, ura.MY, 40, 40, max_batch=T, flags=b.DOA_KEEP_SPECTRUM | b.DOA_KEEP_RXX)
    doa, never = mk(), mk()
    doa.set_subbands(*geom)
    never.set_subbands(*geom)
    for with_peaks, base in ((False, 5), (True, 7)):
        if with_peaks:
            doa.set_peaks(4, 2)
            never.set_peaks(4, 2)
        doa.set_subband_beams(b.BEAM_MVDR, 1e-3)
        counts = {}
        for n in (1, T):
            doa.submit(pk.ptr, pk.stride, pk.offset, n)
            counts[n] = doa.last_launches()
            assert doa.fetch_subband_beams()["beams"].shape == (n, 4, 4 if with_peaks else 1, L // 16, 4)
        assert counts[1] == counts[T] == base + 2, counts
        on = doa.fetch()
        doa.set_subband_beams(b.BEAM_OFF)
        bufs = doa.subband_beam_buffers()
        assert bufs["nbeams"] == 0 and all(bufs[key] is None for key in ("weights", "power", "beams"))
        doa.submit(pk.ptr, pk.stride, pk.offset, T)
        never.submit(pk.ptr, pk.stride, pk.offset, T)
        assert doa.last_launches() == never.last_launches() == base and doa._last() == never._last()
        a, c = doa.fetch(), never.fetch()
        for key in ("peak", "peak_value", "sv", "status", "pm", "rxx"):
            assert _same_bits(a[key], c[key]) and _same_bits(on[key], c[key]), key  # and the beams changed nothing while they were on
        assert _same_bits(doa.fetch_subbands(), never.fetch_subbands()) and _same_bits(doa.fetch_subspace(), never.fetch_subspace())
        if with_peaks:
            x, y = doa.fetch_directions(), never.fetch_directions()
            for key in ("found", "peaks", "values"):
                assert _same_bits(x[key], y[key]), key
        with pytest.raises(b.CrsdrError) as e:
            doa.fetch_subband_beams()
        assert e.value.code == ESTATE
    doa.close()
    never.close()


def _three_emitter_run(b, doa, submit, mats_of, sig, what):
    """MVDR then conventional beams of every bin on the submitted packets; the issue's conditions on packet 0."""
    geom = (model.NFFT, 0, model.NFFT, 1, b.WINDOW_RECT)
    doa.set_subband_beams(b.BEAM_MVDR, model.LOADING)
    submit()
    assert doa.last_launches() == 9
    mats = mats_of()
    n = len(mats)
    mv = _check_against_model(b, doa, mats, n, b.BEAM_MVDR, model.LOADING, ura.MX, ura.MY, geom, per_op=(0, n - 1), what=what + " mvdr")
    dirs = doa.fetch_directions()
    doa.set_subband_beams(b.BEAM_OFF)
    doa.set_subband_beams(b.BEAM_CONVENTIONAL)
    submit()
    mats = mats_of()
    cv = _check_against_model(b, doa, mats, n, b.BEAM_CONVENTIONAL, 0.0, ura.MX, ura.MY, geom, what=what + " conventional")
    for t in range(n):
        band, sigs = {}, {}
        for f in (3, 11):
            i = t * model.NFFT + f
            band[f] = (int(dirs["found"][i]), dirs["peaks"][i], mv["beams"][t, f, :, :, 0], cv["beams"][t, f, :, :, 0], mv["power"][i])
            sigs[f] = model.channelised(sig[t], model.NFFT, f, model.WINDOW_RECT)
        model.check_three_emitters(sigs, band, f"{what} (device), packet {t}")
    doa.set_subband_beams(b.BEAM_OFF)


def test_three_emitters_two_on_one_carrier(b, torch):
    blk, sig = model.three_emitter_block()
    pk = Packets(torch, blk[None])
    doa = b.Doa(22, 2 * model.L, model.K, ura.D, ura.MX, ura.MY, max_batch=1)
    doa.set_subbands(model.NFFT, 0, model.NFFT, 1, b.WINDOW_RECT)
    doa.set_peaks(model.COUNT, model.RADIUS)
    _three_emitter_run(b, doa, lambda: doa.submit(pk.ptr, pk.stride, pk.offset, 1), lambda: blk[None], sig[None], "three emitters")
    doa.close()


def test_three_emitters_through_a_plan_with_no_host_in_between(b, torch):
    # calibrate, freeze, then the scene behind the receivers' phase offsets: plan.submit then doa.submit_plan, fetched at the end
    rng = np.random.default_rng(41)
    M, T = 21, 2
    phi = rng.uniform(-np.pi, np.pi, M)
    plan = b.Plan(M + 1, 2 * model.L, b.MODE_FAITHFUL, max_batch=T)
    doa = b.Doa(M + 1, 2 * model.L, model.K, ura.D, ura.MX, ura.MY, max_batch=T)
    doa.set_subbands(model.NFFT, 0, model.NFFT, 1, b.WINDOW_RECT)
    doa.set_peaks(model.COUNT, model.RADIUS)
    for t in range(16):
        plan.block(ura.calibration_block(model.L, phi, rng), seq=t)
    scene_rng = np.random.default_rng(model.SEED)
    made = [model.three_emitter_block(rng=scene_rng, n0=t * model.L, phi=phi) for t in range(T)]
    rows, sig = np.stack([r for r, _ in made]), np.stack([s for _, s in made])
    seq = [16]

    def submit():
        plan.submit(rows, seq=seq[0], flags=0)
        doa.submit_plan(plan)                                                    # no sync, no fetch in between
        seq[0] += T

    _three_emitter_run(b, doa, submit, lambda: np.stack([plan.fetch(block=t)["matrix"] for t in range(T)]), sig, "three emitters through a plan")
    plan.sync()
    doa.close()
    plan.close()
