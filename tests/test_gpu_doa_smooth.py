"""GPU checks of spatial smoothing, forward-backward averaging and the source count of crsdr_doa (crsdr_doa_set_smoothing /
crsdr_doa_set_order and their per-op forms) against the fp64 numpy restatement in tests/doa_smooth_model.py, whose docstring derives
the bars used here:

    smoothing   |dev - model| <= 2^-24 |model| + 2^-45 max|rxx| per component, the model fed with the device's own rxx
    criterion   |dev - model| <= 2^-23 |model| + N M 2^-44 (1 + max|log lambda|) (twice the second term for AIC), the model fed with
                the device's own sv; k equal wherever the model's best and runner-up differ by more than twice that bar, which the
                tests assert of every estimate they use

Everything else is equality of bits and derived, not measured: the batched kernels and the per-op calls run the same device function
per matrix, the subspace and the scan of a smoothed engine are the existing ones on another matrix, and an estimate scanned with its
own count runs pmusic2d_point with the arguments of a fixed-k engine."""
import importlib

import numpy as np
import pytest

import doa_beams_model as beams_model
import doa_peaks_model as peaks_model
import doa_smooth_model as model
import ura

pytestmark = pytest.mark.gpu
EINVAL, ESTATE = -1, -5
P = np.pi
DIRS = [(0.35 * P, 0.40 * P), (0.65 * P, 0.62 * P), (0.45 * P, 0.70 * P)]      # on the 100 x 100 grid: (65, 60), (35, 38), (55, 30)


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


def _coherent_paths(k, rng):
    return [(a, be, (1.0 - 0.15 * i) * np.exp(1j * (rng.uniform(0, 2 * P) if i else 0.0))) for i, (a, be) in enumerate(DIRS[:k])]


def _mixed_scenes(T, L, mx, my, seed):
    """T blocks with 1, 2, 3, 1, 2, 3 ... incoherent sources; returns (blocks, counts)"""
    rng = np.random.default_rng(seed)
    counts = [1 + t % 3 for t in range(T)]
    return np.stack([ura.scene(L, [(a, be, 1.0 - 0.1 * i) for i, (a, be) in enumerate(DIRS[:k])], rng, mx=mx, my=my) for k in counts]), counts


SMOOTH_CASES = [  # (mx, my, sx, sy, fb)
    (3, 1, 2, 1, 0),
    (64, 1, 2, 1, 1),             # P = 63
    (1, 64, 1, 33, 1),
    (7, 3, 5, 2, 1),
    (7, 3, 7, 3, 1),              # FB only
    (7, 3, 7, 2, 0),
    (8, 8, 6, 6, 1),
    (8, 8, 1, 2, 0),              # ms = 2, P = 56
    (11, 3, 4, 3, 0),
]


@pytest.mark.parametrize("F", [1, 4])
@pytest.mark.parametrize("mx,my,sx,sy,fb", SMOOTH_CASES)
def test_smoothing_arithmetic_and_the_chain_behind_it(b, torch, mx, my, sx, sy, fb, F):
    m, ms, B, T, ncx, ncy, k = mx * my, sx * sy, 256, 8, 19, 23, 1
    rng = np.random.default_rng(1000 * m + 10 * ms + F)
    pk = Packets(torch, rng.integers(-128, 128, size=(T, m + 1, B), dtype=np.int8))
    doa = b.Doa(m + 1, B, k, ura.D, mx, my, ncx, ncy, max_batch=T, frames=F, flags=b.DOA_KEEP_RXX | b.DOA_KEEP_SPECTRUM)
    doa.set_smoothing(sx, sy, b.SMOOTH_FB if fb else 0)
    with pytest.raises(b.CrsdrError) as e:
        doa.fetch_smoothed()                                                     # nothing submitted since set_smoothing
    assert e.value.code == ESTATE
    doa.submit(pk.ptr, pk.stride, pk.offset, T)
    out, rs, vec = doa.fetch(), doa.fetch_smoothed(), doa.fetch_subspace()
    nest = T // F
    assert out["rxx"].shape == (nest, m, m) and rs.shape == (nest, ms, ms) and out["sv"].shape == (nest, ms) and vec.shape == (nest, ms, ms)
    worst = 0.0
    for e_ in range(nest):
        rxx = out["rxx"][e_]
        worst = max(worst, model.assert_smoothed(rs[e_], rxx, mx, my, sx, sy, fb, what=(e_,)))
        assert np.array_equal(rs[e_], rs[e_].conj().T), e_                       # Hermitian: equal values are equal bits (a zero apart)
        iu = np.triu_indices(ms, 1)
        assert np.array_equal(_bits(rs[e_].real[iu]), _bits(rs[e_].real.T[iu])) and np.array_equal(_bits(rs[e_].imag[iu]), _bits(-rs[e_].imag.T[iu]))
        # the per-op form on the same rxx, from host pointers: the same bits
        assert _same_bits(b.smooth_covariance(rxx, mx, my, sx, sy, b.SMOOTH_FB if fb else 0), rs[e_]), e_
        # the chain behind it: the existing subspace and scan on rs, as an sx x sy array
        v1, s1 = b.noisesubspace(rs[e_])
        assert _same_bits(s1, out["sv"][e_]) and _same_bits(v1, vec[e_]), e_
        pm1 = b.pmusic2d(v1, k, ura.D, sx, sy, ncx, ncy)
        assert _same_bits(pm1, out["pm"][e_]), e_
        g = int(np.argmax(peaks_model.keys(pm1)))
        assert out["peak"][e_].tolist() == [g // ncy, g % ncy] and _bits(out["peak_value"][e_:e_ + 1])[0] == _bits(pm1.reshape(-1)[g:g + 1])[0]
    print(f"{mx}x{my} -> {sx}x{sy} fb {fb} F {F}: largest error / bar {worst:.3f}")
    # ... and from device pointers
    dev = torch.device("cuda", 0)
    d_rxx = torch.from_numpy(np.ascontiguousarray(out["rxx"][0]).view(np.float32)).to(dev)
    d_rs = torch.zeros(ms * ms * 2, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    b.smooth_covariance_device(d_rs.data_ptr(), d_rxx.data_ptr(), mx, my, sx, sy, b.SMOOTH_FB if fb else 0)
    assert _same_bits(d_rs.cpu().numpy().view(np.complex64).reshape(ms, ms), rs[0])
    doa.close()


def _check_order(b, torch, sv, got, N, criterion, kmin, kmax, what):
    for e_ in range(sv.shape[0]):
        o = model.order(sv[e_], N, criterion, kmin, kmax)
        bar = model.criterion_bar(o["values"], sv[e_], N, criterion) if sv[e_][0] > 0 else np.zeros(kmax - kmin + 1)
        err = np.abs(got["criterion"][e_].astype(np.float64) - o["values"])
        print(f"{what} e {e_}: k {got['k'][e_]} model {o['k']} margin {o['margin']:.3g} bar {o['bar']:.3g} largest error / bar "
              f"{float((err / np.maximum(bar, 1e-300)).max()) if sv[e_][0] > 0 else 0.0:.3f}")
        assert (err <= bar).all(), (what, e_, err, bar)
        assert o["decided"], (what, e_, o["margin"], o["bar"])                   # no estimate is left out of the k comparison
        assert got["k"][e_] == o["k"], (what, e_)
        # the per-op form on the same sv: the same k, the same bits
        k1, c1 = b.source_order(sv[e_], N, criterion, kmin, kmax)
        assert k1 == got["k"][e_] and _same_bits(c1, got["criterion"][e_]), (what, e_)
    # and from device pointers, the first estimate
    dev = torch.device("cuda", 0)
    d_sv = torch.from_numpy(np.ascontiguousarray(sv[0])).to(dev)
    d_k, d_c = torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(kmax - kmin + 1, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    b.source_order_device(d_k.data_ptr(), d_c.data_ptr(), d_sv.data_ptr(), sv.shape[1], N, criterion, kmin, kmax)
    assert int(d_k.cpu()[0]) == got["k"][0] and _same_bits(d_c.cpu().numpy(), got["criterion"][0]), what


ORDER_CASES = [  # (mx, my, sx, sy, fb): M = 2, 10, 21, 64
    (2, 1, 2, 1, 0),
    (7, 3, 5, 2, 1),
    (7, 3, 7, 3, 0),
    (8, 8, 8, 8, 1),
]


@pytest.mark.parametrize("mx,my,sx,sy,fb", ORDER_CASES)
def test_order_against_the_restatement(b, torch, mx, my, sx, sy, fb):
    m, M, L, T = mx * my, sx * sy, 1024, 8
    blocks, _ = _mixed_scenes(T, L, mx, my, 50 + M)
    blocks[5] = 0                                                               # an all-zero packet: sv[0] = 0, k = kmin, values 0
    pk = Packets(torch, blocks)
    doa = b.Doa(m + 1, 2 * L, 1, ura.D, mx, my, 16, 16, max_batch=T)
    doa.set_smoothing(sx, sy, b.SMOOTH_FB if fb else 0)
    ranges = [(b.ORDER_MDL, 1, M - 1), (b.ORDER_AIC, 1, M - 1), (b.ORDER_MDL, 1, 1)]
    if M > 3:
        ranges += [(b.ORDER_AIC, 2, M - 2), (b.ORDER_MDL, 3, 3)]                # kmin > 1, kmin = kmax > 1
    for criterion, kmin, kmax in ranges:
        doa.set_order(criterion, kmin, kmax)
        with pytest.raises(b.CrsdrError) as e:
            doa.fetch_order()                                                    # nothing submitted since set_order
        assert e.value.code == ESTATE
        doa.submit(pk.ptr, pk.stride, pk.offset, T)
        sv, got = doa.fetch()["sv"], doa.fetch_order()
        assert sv.shape == (T, M) and got["k"].shape == (T,) and got["criterion"].shape == (T, kmax - kmin + 1)
        assert not sv[5].any() and got["k"][5] == kmin and not got["criterion"][5].any()
        assert all(doa.order_buffers().values())
        _check_order(b, torch, sv, got, L, criterion, kmin, kmax, f"M {M} crit {criterion} k {kmin}..{kmax}")
    doa.set_order(b.ORDER_OFF)
    assert all(v is None for v in doa.order_buffers().values())
    with pytest.raises(b.CrsdrError) as e:
        doa.fetch_order()
    assert e.value.code == ESTATE
    doa.close()


def test_auto_k_equals_fixed_k(b, torch):
    M, L, T = 21, 1024, 8
    blocks, counts = _mixed_scenes(T, L, 7, 3, 77)
    pk = Packets(torch, blocks)
    auto = b.Doa(M + 1, 2 * L, 1, ura.D, 7, 3, max_batch=T, flags=b.DOA_KEEP_SPECTRUM)
    auto.set_order(b.ORDER_MDL, 1, M - 1)
    auto.submit(pk.ptr, pk.stride, pk.offset, T)
    a, ke = auto.fetch(), auto.fetch_order()["k"]
    print("k_e", ke.tolist(), "sources", counts)
    assert ke.tolist() == counts and set(counts) == {1, 2, 3}
    for k in sorted(set(ke.tolist())):
        fixed = b.Doa(M + 1, 2 * L, k, ura.D, 7, 3, max_batch=T, flags=b.DOA_KEEP_SPECTRUM)
        fixed.submit(pk.ptr, pk.stride, pk.offset, T)
        f = fixed.fetch()
        sel = ke == k
        for key in ("pm", "peak", "peak_value", "sv"):
            assert _same_bits(a[key][sel], f[key][sel]), (k, key)
        fixed.close()
    auto.close()


def _conditions(k, sv, k_e, found, peaks, paths, what):
    assert sv[k - 1] / sv[0] > 0.2 and sv[k] / sv[0] < 0.05, (what, sv[:k + 1] / sv[0])
    assert k_e == k, (what, k_e)
    assert found == k and model.all_within(peaks, paths, tol=1.0), (what, found, np.asarray(peaks).tolist())


def _model_conditions(blk, k, paths, what):
    """the CPU test's conditions on this very block, in fp64: what the device is then asked to reproduce"""
    L = blk.shape[1] // 2
    r = model.covariance(blk).astype(np.complex64)
    s0 = np.linalg.svd(r.astype(np.complex128), compute_uv=False)
    assert s0[1] / s0[0] < 0.02 and model.order(s0, L)["k"] == 1, (what, "plain")
    s, pm = model.spectrum(model.smooth(r, 7, 3, 5, 2, model.FB), k, 5, 2)
    n, pts, _ = peaks_model.directions(pm.astype(np.float32), k, 2)
    _conditions(k, s, model.order(s, L)["k"], n, pts, paths, (what, "fp64 model"))


@pytest.mark.parametrize("k", [2, 3])
def test_coherent_scenes_end_to_end(b, torch, k):
    rng = np.random.default_rng(100 + k)
    L, M, T = 2048, 21, 2
    paths = _coherent_paths(k, rng)
    blocks = np.stack([model.coherent_scene(L, paths, rng) for _ in range(T)])
    for t in range(T):
        _model_conditions(blocks[t], k, paths, t)
    pk = Packets(torch, blocks)
    # the unsmoothed engine sees one source
    plain = b.Doa(M + 1, 2 * L, 1, ura.D, 7, 3, max_batch=T)
    plain.set_order(b.ORDER_MDL, 1, 9)
    plain.submit(pk.ptr, pk.stride, pk.offset, T)
    sv0 = plain.fetch()["sv"]
    assert (sv0[:, 1] / sv0[:, 0] < 0.02).all() and plain.fetch_order()["k"].tolist() == [1] * T
    plain.close()
    doa = b.Doa(M + 1, 2 * L, 1, ura.D, 7, 3, max_batch=T)
    doa.set_smoothing(5, 2, b.SMOOTH_FB)
    doa.set_order(b.ORDER_MDL, 1, 9, limit_directions=True)
    doa.set_peaks(4, 2)
    doa.submit(pk.ptr, pk.stride, pk.offset, T)
    assert doa.last_launches() == 9
    sv, ke, dirs = doa.fetch()["sv"], doa.fetch_order()["k"], doa.fetch_directions()
    for t in range(T):
        print(f"k {k} block {t}: sv ratios {np.round(sv[t][:k + 1] / sv[t][0], 3).tolist()} k_e {ke[t]} found {dirs['found'][t]} "
              f"directions {dirs['peaks'][t].tolist()}")
        _conditions(k, sv[t], ke[t], dirs["found"][t], dirs["peaks"][t], paths, t)
        assert (dirs["peaks"][t][k:] == -1).all() and (dirs["values"][t][k:] == -1.0).all()
    doa.close()


def test_coherent_scene_through_a_plan(b, torch):
    # calibrate (reference noise on), freeze, a batch of coherent two-path scenes: plan.submit then doa.submit_plan, fetched at the end
    rng = np.random.default_rng(41)
    L, M, T, k = 2048, 21, 2, 2
    paths = _coherent_paths(k, rng)
    phi = rng.uniform(-np.pi, np.pi, M)
    plan = b.Plan(M + 1, 2 * L, b.MODE_FAITHFUL, max_batch=T)
    doa = b.Doa(M + 1, 2 * L, 1, ura.D, 7, 3, max_batch=T)
    doa.set_smoothing(5, 2, b.SMOOTH_FB)
    doa.set_order(b.ORDER_MDL, 1, 9, limit_directions=True)
    doa.set_peaks(4, 2)
    for t in range(16):
        plan.block(ura.calibration_block(L, phi, rng), seq=t)
    rows = np.stack([model.coherent_scene(L, paths, rng, phi=phi) for _ in range(T)])
    plan.submit(rows, seq=16, flags=0)
    doa.submit_plan(plan)                                                        # no sync, no fetch in between
    sv, ke, dirs = doa.fetch()["sv"], doa.fetch_order()["k"], doa.fetch_directions()
    assert doa.last_launches() == 9
    for t in range(T):
        _model_conditions(plan.fetch(block=t)["matrix"], k, paths, ("plan", t))
        print(f"block {t}: k_e {ke[t]} found {dirs['found'][t]} directions {dirs['peaks'][t].tolist()}")
        _conditions(k, sv[t], ke[t], dirs["found"][t], dirs["peaks"][t], paths, ("plan", t))
    plan.sync()
    doa.close()
    plan.close()


def test_beams_with_fb_only_and_refused_with_sub_arrays(b, torch):
    M, L, T, loading = 21, 1024, 2, 1e-2
    blocks, _ = _mixed_scenes(T, L, 7, 3, 9)
    pk = Packets(torch, blocks)
    doa = b.Doa(M + 1, 2 * L, 1, ura.D, 7, 3, max_batch=T)
    doa.set_smoothing(7, 3, b.SMOOTH_FB)
    doa.set_beams(b.BEAM_MVDR, loading)
    doa.submit(pk.ptr, pk.stride, pk.offset, T)
    assert doa.last_launches() == 8
    out, vec, bm = doa.fetch(), doa.fetch_subspace(), doa.fetch_beams()
    assert bm["weights"].shape == (T, 1, M) and bm["beams"].shape == (T, 1, L)
    for t in range(T):
        # the weights are the definition's, from the FB subspace the engine holds: fp64 from the published vec and sv, rounded once
        w, pw = beams_model.slot_weights(vec[t], out["sv"][t], [beams_model.grid_angles(*out["peak"][t])], b.BEAM_MVDR, loading)
        dw = bm["weights"][t].astype(np.complex128) - w.astype(np.complex128)
        top = max(np.abs(w.real).max(), np.abs(w.imag).max())
        assert max(np.abs(dw.real).max(), np.abs(dw.imag).max()) <= 2.0 ** -23 * top, t      # one fp32 step of the largest component
        a = beams_model.steering(*beams_model.grid_angles(*out["peak"][t]))
        assert abs(np.sum(bm["weights"][t][0].astype(np.complex128) * a.conj()) - 1.0) < 1e-5     # distortionless toward the peak
        assert np.isfinite(bm["beams"][t]).all() and np.abs(bm["beams"][t]).max() > 0
    # true sub-arrays: refused, in both call orders
    with pytest.raises(b.CrsdrError) as e:
        doa.set_smoothing(5, 2, b.SMOOTH_FB)                                     # beams on
    assert e.value.code == ESTATE
    doa.set_beams(b.BEAM_OFF)
    doa.set_smoothing(5, 2, b.SMOOTH_FB)
    with pytest.raises(b.CrsdrError) as e:
        doa.set_beams(b.BEAM_MVDR, loading)                                      # sub-arrays on
    assert e.value.code == ESTATE
    with pytest.raises(b.CrsdrError) as e:
        doa.set_beams(b.BEAM_CONVENTIONAL, fixed_angles=[(1.0, 1.0)])
    assert e.value.code == ESTATE
    doa.close()


def test_launch_counts_switching_off_and_refusals(b, torch):
    M, L, T = 21, 512, 8
    blocks, _ = _mixed_scenes(T, L, 7, 3, 5)
    pk = Packets(torch, blocks)
    flags = b.DOA_KEEP_SPECTRUM | b.DOA_KEEP_RXX
    doa = b.Doa(M + 1, 2 * L, 2, ura.D, 7, 3, 40, 40, max_batch=T, flags=flags)
    never = b.Doa(M + 1, 2 * L, 2, ura.D, 7, 3, 40, 40, max_batch=T, flags=flags)

    def launches():
        counts = []
        for n in (1, 8):
            doa.submit(pk.ptr, pk.stride, pk.offset, n)
            counts.append(doa.last_launches())
        return counts

    assert launches() == [5, 5]
    doa.set_smoothing(5, 2, b.SMOOTH_FB)
    assert launches() == [6, 6]
    doa.set_order(b.ORDER_AIC, 1, 9)
    assert launches() == [7, 7]
    doa.set_peaks(4, 2)
    assert launches() == [9, 9]
    doa.set_smoothing(7, 3, 0)                                                   # smoothing off, order and peaks still on
    with pytest.raises(b.CrsdrError) as e:
        doa.fetch()                                                              # set_smoothing discards the last submit
    assert e.value.code == ESTATE
    assert launches() == [8, 8]
    # refusals
    for sx, sy, fl in ((0, 3, 0), (8, 3, 0), (7, 4, 0), (1, 1, 0), (5, 2, 2), (2, 1, 0)):      # (2, 1): desc.k = 2 >= ms
        with pytest.raises(b.CrsdrError) as e:
            doa.set_smoothing(sx, sy, fl)
        assert e.value.code == EINVAL, (sx, sy, fl)
    with pytest.raises(b.CrsdrError) as e:
        doa.set_smoothing(3, 3, 0)                                               # the order range ends at 9 = ms
    assert e.value.code == EINVAL
    for crit, kmin, kmax in ((3, 1, 2), (-1, 1, 2), (1, 0, 2), (1, 3, 2), (1, 1, 21)):
        with pytest.raises(b.CrsdrError) as e:
            doa.set_order(crit, kmin, kmax)
        assert e.value.code == EINVAL, (crit, kmin, kmax)
    with pytest.raises(b.CrsdrError) as e:
        doa.fetch_smoothed()                                                     # smoothing is off
    assert e.value.code == ESTATE
    # everything off again: five launches, and what an object that never had any of it gives
    doa.set_peaks(0)
    doa.set_order(b.ORDER_OFF)
    assert launches() == [5, 5]
    never.submit(pk.ptr, pk.stride, pk.offset, T)
    assert never.last_launches() == 5
    a, c = doa.fetch(), never.fetch()
    for key in ("peak", "peak_value", "sv", "status", "pm", "rxx"):
        assert _same_bits(a[key], c[key]) if a[key].dtype != np.int32 else np.array_equal(a[key], c[key]), key
    assert _same_bits(doa.fetch_subspace(), never.fetch_subspace())
    doa.close()
    never.close()


def test_limit_directions_caps_found_at_the_count(b, torch):
    M, L, T = 21, 1024, 8
    blocks, counts = _mixed_scenes(T, L, 7, 3, 77)
    pk = Packets(torch, blocks)
    free = b.Doa(M + 1, 2 * L, 1, ura.D, 7, 3, max_batch=T)
    capped = b.Doa(M + 1, 2 * L, 1, ura.D, 7, 3, max_batch=T)
    for d, lim in ((free, False), (capped, True)):
        d.set_order(b.ORDER_MDL, 1, 8, limit_directions=lim)
        d.set_peaks(6, 2)
        d.submit(pk.ptr, pk.stride, pk.offset, T)
    f, c, ke = free.fetch_directions(), capped.fetch_directions(), capped.fetch_order()["k"]
    assert ke.tolist() == counts
    assert (f["found"] > ke).any()                                              # side lobes: without the cap there are more peaks than sources
    for t in range(T):
        n = min(int(ke[t]), int(f["found"][t]))
        assert c["found"][t] == n
        assert np.array_equal(c["peaks"][t][:n], f["peaks"][t][:n]) and _same_bits(c["values"][t][:n], f["values"][t][:n])
        assert (c["peaks"][t][n:] == -1).all() and (c["values"][t][n:] == -1.0).all()
    free.close()
    capped.close()


def test_a_small_object_created_after_a_large_one(b, torch):
    # the kernels' dynamic LDS limits are function attributes shared by every live object: a 2-element engine created after a
    # 64-element one must not take the large one's 128 KiB away
    rng = np.random.default_rng(3)
    big_pk = Packets(torch, rng.integers(-128, 128, size=(1, 65, 256), dtype=np.int8))
    small_pk = Packets(torch, rng.integers(-128, 128, size=(1, 3, 256), dtype=np.int8))
    big = b.Doa(65, 256, 1, 0.5, 8, 8, 16, 16)
    big.set_order(b.ORDER_MDL, 1, 63)
    small = b.Doa(3, 256, 1, 0.5, 2, 1, 16, 16)
    small.set_order(b.ORDER_MDL, 1, 1)
    small.submit(small_pk.ptr, small_pk.stride, small_pk.offset, 1)
    big.submit(big_pk.ptr, big_pk.stride, big_pk.offset, 1)
    assert big.fetch()["status"].tolist() == [0] and small.fetch()["status"].tolist() == [0]
    assert 1 <= big.fetch_order()["k"][0] <= 63 and small.fetch_order()["k"].tolist() == [1]
    big.close()
    small.close()


def test_cpp_engine_prints_a_source_count_per_estimate():
    # coherent_demo --bench --music --smooth 5x2 --fb --order mdl: cbeamformer::batch with set_smoothing and set_order; the synthetic
    # channels all carry the reference noise, so every aligned block holds one source
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    host = os.path.join(root, "coherent-rtlsdr_amd", "host")
    importlib.import_module("coherent-rtlsdr_amd.binding").build()
    subprocess.run(["make", "-C", host, "all"], check=True, stdout=subprocess.DEVNULL)
    for extra, size in ((["--smooth", "5x2", "--fb", "--order", "mdl"], 10), (["--fb", "--order", "aic"], 21)):
        r = subprocess.run([os.path.join(host, "coherent_demo"), "--bench", "--music", "--nsig", "21", "--batch", "8", "--blocks", "32", *extra],
                           capture_output=True, text=True, timeout=300)
        print(r.stdout, r.stderr)
        assert r.returncode == 0 and "DEMO OK" in r.stdout, r.stdout + r.stderr
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("doa: batch") and ", k:" in ln]
        assert len(lines) == 4, lines
        for ln in lines:
            assert f"8 estimates of {size} elements" in ln, ln
            ks = [int(x) for x in ln.split(", k:")[1].split()]
            assert len(ks) == 8 and all(1 <= k < size for k in ks), ln
    r = subprocess.run([os.path.join(host, "coherent_demo"), "--bench", "--music", "--nsig", "21", "--batch", "8", "--blocks", "32", "--smooth", "8x3"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "refused" in r.stdout and "DEMO FAILED" in r.stdout, r.stdout + r.stderr
