"""GPU checks of the gridless directions (crsdr_doa_set_esprit / crsdr_doa_fetch_esprit / crsdr_esprit2d) against the fp64 model of
tests/doa_esprit_model.py, whose docstring states the definition and the bars.

The bar on mu and nu: BAR = 1e-11 rad between the device and the model's numpy-eig route, both in fp64 from the same fp32 vec fetched
from the device, for matrices with cond(Gx), cond(Gy), cond(V) <= 4 and gap >= 0.1; where a matrix is worse conditioned than that the
bar grows with the worst of the three condition numbers (both sides lose digits in proportion) and stays below 1e-9.  angles, modulus
and power: within 4 ulp of the model's values rounded to fp32.  Directions against the scene: DIRECTION_BAR, one cell of a 100 x 100
grid.

Measured on the MI355X (the ten shapes of em.SHAPES, three estimates each): 4.4e-16 rad at most on every matrix inside the bar's class;
8.9e-15 at 7 x 3, k = 5 (cond(Gy) 87 .. 100) and 2.6e-14 at 3 x 2, k = 3 (cond(Gy) 946 .. 1328) outside it."""
import importlib

import numpy as np
import pytest

import doa_esprit_model as em
import doa_smooth_model as smooth_model
import doa_subband_model as subband_model
import ura

pytestmark = pytest.mark.gpu
EINVAL, ESTATE = -1, -5
P = np.pi


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


KEYS = ("phases", "angles", "modulus", "power", "flags")


def _same_bits(a, c):
    a, c = np.ascontiguousarray(a), np.ascontiguousarray(c)
    return a.shape == c.shape and a.dtype == c.dtype and a.tobytes() == c.tobytes()


def _assert_empty(got, e, first, what):
    assert not got["phases"][e, first:].view(np.uint64).any(), what
    assert np.all(got["angles"][e, first:] == -1) and np.all(got["modulus"][e, first:] == -1) and np.all(got["power"][e, first:] == -1), what
    assert not got["flags"][e, first:].any(), what


def _bar(model):
    if em.well_conditioned(model):
        return em.BAR
    return min(em.BAR * max(1.0, max(model["cond_gx"], model["cond_gy"], model["cond_v"]) / 4.0), 1e-9)


def _assert_model(got, model, k, what):
    """one matrix of the device (slot arrays) against the model's eig route"""
    assert got["found"] == model["found"] == k and got["status"] == 0, (what, got["found"], got["status"])
    err = em.phase_error(got["phases"][:k], model["phases"][:k])
    bar = _bar(model)
    print(f"{what}: phases differ by {err:.2e} rad (bar {bar:.1e}); cond {model['cond_gx']:.2f} {model['cond_gy']:.2f} {model['cond_v']:.2f} gap {model['gap']:.3f}")
    assert err <= bar, (what, err, bar)
    for key in ("angles", "modulus", "power"):
        g, m = got[key][:k].astype(np.float64), model[key][:k]
        assert np.all(np.abs(g - m.astype(np.float64)) <= 4 * np.spacing(np.abs(m)).astype(np.float64)), (what, key, got[key][:k], m)
    assert np.array_equal(got["flags"][:k], model["flags"][:k]), what
    # slot order: descending power, then ascending mu, then nu (on the device's own fp32 power: ties aside, it is sorted)
    assert np.all(np.diff(got["power"][:k].astype(np.float64)) <= 0), (what, got["power"][:k])
    return err


def _slots(got, e):
    return {"found": int(got["found"][e]), "status": int(got["status"][e]), **{key: got[key][e] for key in KEYS}}


# ---- 1. every shape: per-op against the model, the batched engine against per-op ----------------------------------------------------------

@pytest.mark.parametrize("shape", em.SHAPES, ids=[f"{s[0]}x{s[1]}-k{s[2]}" for s in em.SHAPES])
def test_per_op_against_the_model_and_the_engine_against_per_op(b, torch, shape):
    sx, sy, k = shape
    d, T = em.shape_d(sx, sy), 3
    L = 32 if (sx, sy) == (2, 2) else 2048                     # 2 x 2: blocksize 64
    blocks = np.stack([em.shape_scene(sx, sy, k, L=L, seed=t)[0] for t in range(T)])
    dirs = em.shape_scene(sx, sy, k, L=L)[1]
    pk = Packets(torch, blocks)
    doa = b.Doa(sx * sy + 1, 2 * L, k, d, sx, sy, 20, 20, max_batch=T)
    doa.set_esprit(b.ESPRIT_BESIDE)
    assert doa.esprit_buffers()["slots"] == k and all(doa.esprit_buffers()[key] for key in ("found", "status") + KEYS)
    doa.submit(pk.ptr, pk.stride, pk.offset, T)
    got, vec, sv = doa.fetch_esprit(), doa.fetch_subspace(), doa.fetch()["sv"]
    assert got["phases"].shape == (T, k, 2) and got["phases"].dtype == np.float64 and got["power"].shape == (T, k)
    worst = 0.0
    for e in range(T):
        one = doa.esprit2d(vec[e], sv[e])
        assert one["found"] == got["found"][e] and one["status"] == got["status"][e], e
        for key in KEYS:
            assert _same_bits(one[key], got[key][e]), (shape, e, key)
        model = em.esprit(vec[e], sv[e], k, d, sx, sy)
        worst = max(worst, _assert_model(one, model, k, f"{sx}x{sy} k={k} estimate {e}"))
        if sx >= 7 and sy >= 3:
            assert em.match_error(one["angles"], dirs) <= em.DIRECTION_BAR, (shape, e)
            assert np.all(np.abs(one["modulus"] - 1) < 0.05)
    print(f"{sx}x{sy} k={k}: worst phase error {worst:.2e} rad")
    doa.close()


# ---- 2. the empty results ----------------------------------------------------------------------------------------------------------------

def test_zero_and_rank_deficient_matrices(b, torch):
    sx, sy, k, L, d = 3, 2, 2, 256, 0.5
    zero = b.esprit2d(np.zeros((6, 6)), np.zeros(6), 2, d, sx, sy)
    assert zero["found"] == 0 and zero["status"] == 0
    _assert_empty({key: zero[key][None] for key in KEYS}, 0, 0, "zero per-op")
    # the identity: column 2 is the element (ix = 2, iy = 0), which E1x drops: Gx has an empty column
    flat = b.esprit2d(np.eye(6), np.ones(6), 3, d, sx, sy)
    assert flat["found"] == 0 and flat["status"] == b.ESPRIT_STATUS_PIVOT
    _assert_empty({key: flat[key][None] for key in KEYS}, 0, 0, "identity per-op")
    # in a batch: an all-zero block between two scenes
    blocks = np.stack([em.shape_scene(sx, sy, k, L=L, seed=t)[0] for t in range(3)])
    blocks[1] = 0
    pk = Packets(torch, blocks)
    doa = b.Doa(sx * sy + 1, 2 * L, k, d, sx, sy, 8, 8, max_batch=3)
    doa.set_esprit(b.ESPRIT_BESIDE)
    doa.submit(pk.ptr, pk.stride, pk.offset, 3)
    got, sv = doa.fetch_esprit(), doa.fetch()["sv"]
    assert sv[1, 0] == 0 and got["found"].tolist() == [k, 0, k] and not got["status"].any()
    _assert_empty(got, 1, 0, "zero block")
    doa.close()


# ---- 3. composition ----------------------------------------------------------------------------------------------------------------------

def test_smoothing_finds_both_coherent_paths(b, torch):
    rng = np.random.default_rng(200)
    L, T, k = 2048, 2, 2
    dirs = [(0.35 * P, 0.40 * P), (0.62 * P, 0.58 * P)]
    paths = [(a, be, (1.0 - 0.15 * i) * np.exp(1j * (rng.uniform(0, 2 * P) if i else 0.0))) for i, (a, be) in enumerate(dirs)]
    blocks = np.stack([smooth_model.coherent_scene(L, paths, rng) for _ in range(T)])
    want = [(P - a, P - be) for a, be in dirs]
    pk = Packets(torch, blocks)
    doa = b.Doa(22, 2 * L, k, ura.D, 7, 3, max_batch=T)
    doa.set_esprit(b.ESPRIT_BESIDE)
    doa.submit(pk.ptr, pk.stride, pk.offset, T)
    plain = doa.fetch_esprit()
    doa.set_smoothing(5, 2, b.SMOOTH_FB)
    doa.submit(pk.ptr, pk.stride, pk.offset, T)
    got, vec, sv = doa.fetch_esprit(), doa.fetch_subspace(), doa.fetch()["sv"]
    assert vec.shape == (T, 10, 10)
    for e in range(T):
        model = em.esprit(vec[e], sv[e], k, ura.D, 5, 2)
        _assert_model(_slots(got, e), model, k, f"smoothed estimate {e}")
        err, before = em.match_error(got["angles"][e], want), em.match_error(plain["angles"][e], want)
        print(f"estimate {e}: both paths within {err:.2e} rad (unsmoothed: {before:.2e})")
        assert err <= em.DIRECTION_BAR, (e, got["angles"][e], want)
        one = doa.esprit2d(vec[e], sv[e])                                        # the sub-array's geometry
        assert all(_same_bits(one[key], got[key][e]) for key in KEYS)
    doa.close()


def test_order_gives_every_estimate_its_own_count(b, torch):
    L, T, kmax = 2048, 4, 3
    rng = np.random.default_rng(77)
    dirs = em.lattice_sources(2, 0.5)
    counts = [1, 2, 2, 1]
    blocks = np.stack([ura.scene(L, [(P - a, P - be, 1.0 - 0.3 * i) for i, (a, be) in enumerate(dirs[:c])], rng) for c in counts])
    pk = Packets(torch, blocks)
    doa = b.Doa(22, 2 * L, 1, ura.D, 7, 3, max_batch=T)
    doa.set_order(b.ORDER_MDL, 1, kmax)
    doa.set_esprit(b.ESPRIT_BESIDE)
    assert doa.esprit_buffers()["slots"] == kmax
    doa.submit(pk.ptr, pk.stride, pk.offset, T)
    got, ks, vec, sv = doa.fetch_esprit(), doa.fetch_order()["k"], doa.fetch_subspace(), doa.fetch()["sv"]
    print("counts", ks.tolist(), "of scenes with", counts)
    assert got["found"].tolist() == ks.tolist() and {1, 2} <= set(ks.tolist()) and got["phases"].shape == (T, kmax, 2)
    for e, c in enumerate(ks.tolist()):
        _assert_empty(got, e, c, f"estimate {e}")
        _assert_model(_slots(got, e), em.esprit(vec[e], sv[e], c, ura.D, 7, 3, slots=kmax), c, f"order estimate {e}")
        if c == counts[e]:
            assert em.match_error(got["angles"][e, :c], dirs[:c]) <= em.DIRECTION_BAR
    doa.close()


def test_subbands_give_each_band_its_emitter(b, torch):
    N, L, T = 16, 2048, 2
    rng = np.random.default_rng(5)
    blocks = np.stack([subband_model.two_emitter_block(L, rng, n0=t * L) for t in range(T)])
    pk = Packets(torch, blocks)
    doa = b.Doa(22, 2 * L, 1, ura.D, 7, 3, max_batch=T)
    doa.set_subbands(N, 0, N, 1)
    doa.set_esprit(b.ESPRIT_BESIDE)
    doa.submit(pk.ptr, pk.stride, pk.offset, T)
    got, peak = doa.fetch_esprit(), doa.fetch()["peak"].reshape(T, N, 2)
    assert got["found"].shape == (T * N,) and got["angles"].shape == (T * N, 1, 2)
    ang = got["angles"].reshape(T, N, 2)
    for t in range(T):
        for f, (cx, cy) in zip(subband_model.EMITTER_BINS16, subband_model.EMITTER_PEAKS):
            assert got["found"][t * N + f] == 1
            assert abs(ang[t, f, 0] - cx * P / 100) <= em.DIRECTION_BAR and abs(ang[t, f, 1] - cy * P / 100) <= em.DIRECTION_BAR, (t, f, ang[t, f], cx, cy)
            assert np.abs(peak[t, f] - (cx, cy)).max() <= 1
    doa.close()


# ---- 4. the modes ------------------------------------------------------------------------------------------------------------------------

def _refused(b, code, fn, *a):
    with pytest.raises(b.CrsdrError) as err:
        fn(*a)
    assert err.value.code == code, (getattr(fn, "__name__", fn), a, err.value)


def test_only_runs_no_scan_and_beside_changes_nothing_else(b, torch):
    sx, sy, k, L, T = 7, 3, 2, 1024, 4
    d = em.shape_d(sx, sy)
    blocks = np.stack([em.shape_scene(sx, sy, k, L=L, seed=t)[0] for t in range(T)])
    pk = Packets(torch, blocks)
    never = b.Doa(22, 2 * L, k, d, sx, sy, 20, 20, max_batch=T, flags=b.DOA_KEEP_SPECTRUM)      # an object that never had the feature
    never.submit(pk.ptr, pk.stride, pk.offset, T)
    base, base_launches = never.fetch(), never.last_launches()
    never.close()
    doa = b.Doa(22, 2 * L, k, d, sx, sy, 20, 20, max_batch=T, flags=b.DOA_KEEP_SPECTRUM)
    _refused(b, ESTATE, doa.fetch_esprit)                                        # off
    assert doa.esprit_buffers() == dict(found=None, status=None, phases=None, angles=None, modulus=None, power=None, flags=None, slots=0)
    for mode in (-1, 3):
        _refused(b, EINVAL, doa.set_esprit, mode)
    doa.set_esprit(b.ESPRIT_BESIDE)
    _refused(b, ESTATE, doa.fetch_esprit)                                        # before the first submit after the setter
    doa.submit(pk.ptr, pk.stride, pk.offset, T)
    assert doa.last_launches() == base_launches + 1
    beside, out = doa.fetch_esprit(), doa.fetch()
    for key in ("pm", "peak", "peak_value", "sv"):
        assert _same_bits(out[key], base[key]), key
    # ONLY: the same ESPRIT bits, the scan and the peak not issued
    doa.set_esprit(b.ESPRIT_ONLY)
    _refused(b, ESTATE, doa.fetch_esprit)
    doa.submit(pk.ptr, pk.stride, pk.offset, T)
    assert doa.last_launches() == base_launches + 1 - 2
    only = doa.fetch_esprit()
    for key in ("found", "status") + KEYS:
        assert _same_bits(only[key], beside[key]), key
    rest = doa.fetch()
    assert sorted(rest) == ["status", "sv"] and _same_bits(rest["sv"], base["sv"]) and _same_bits(doa.fetch_subspace(), doa.fetch_subspace())
    _refused(b, ESTATE, doa.fetch_peaks)
    L_ = b.lib()
    import ctypes as C
    val, pm = np.zeros(T, dtype=np.float32), np.zeros((T, 20, 20), dtype=np.float32)
    assert L_.crsdr_doa_fetch(doa._h, None, val.ctypes.data_as(C.POINTER(C.c_float)), None, None, None, None) == ESTATE
    assert L_.crsdr_doa_fetch(doa._h, None, None, None, None, pm.ctypes.data_as(C.POINTER(C.c_float)), None) == ESTATE
    assert L_.crsdr_doa_fetch_directions(doa._h, None, None, None) == ESTATE and L_.crsdr_doa_fetch_refined(doa._h, None, None, None) == ESTATE
    # what needs the scan refuses the submit, before any launch: the last submit's results stay
    for on, off in ((lambda: doa.set_peaks(2, 1), lambda: doa.set_peaks(0)), (lambda: doa.set_refine(3), lambda: doa.set_refine(0)),
                    (lambda: doa.set_beams(b.BEAM_CONVENTIONAL), lambda: doa.set_beams(b.BEAM_OFF))):
        on()
        _refused(b, ESTATE, doa.submit, pk.ptr, pk.stride, pk.offset, T)
        off()
    assert all(_same_bits(doa.fetch_esprit()[key], only[key]) for key in KEYS)
    # beams at fixed angles are fine: the fetched angles are in their convention
    doa.set_beams(b.BEAM_CONVENTIONAL, fixed_angles=only["angles"][0])
    doa.submit(pk.ptr, pk.stride, pk.offset, T)
    beams = doa.fetch_beams()
    assert doa.last_launches() == base_launches + 1 - 2 + 2
    # the conventional beam's power toward an ESPRIT direction is ESPRIT's power: the same expression, at the angles rounded to fp32
    # (a phase step of at most M 2 pi d 2^-23 = 1e-5 per element)
    power = beams["power"].reshape(T, k)
    assert np.all(np.abs(power[0] - only["power"][0]) <= 1e-4 * only["power"][0]), (power[0], only["power"][0])
    doa.set_beams(b.BEAM_OFF)
    # OFF: the bits and the count of an object that never had the feature
    doa.set_esprit(b.ESPRIT_OFF)
    _refused(b, ESTATE, doa.fetch_esprit)
    doa.submit(pk.ptr, pk.stride, pk.offset, T)
    off_out = doa.fetch()
    assert doa.last_launches() == base_launches
    for key in ("pm", "peak", "peak_value", "sv"):
        assert _same_bits(off_out[key], base[key]), key
    doa.close()


def test_geometry_and_slots_are_checked_by_the_submit(b, torch):
    L, T = 64, 1
    rng = np.random.default_rng(3)
    for mx, my, k, ok in ((6, 1, 1, False), (1, 6, 1, False), (3, 2, 4, False), (3, 2, 3, True)):
        blocks = ura.scene(L, [(1.0, 1.3, 1.0)], rng, mx=mx, my=my, d=np.float32(0.5))[None]
        pk = Packets(torch, blocks)
        doa = b.Doa(7, 2 * L, k, 0.5, mx, my, 8, 8, max_batch=T)
        doa.set_esprit(b.ESPRIT_BESIDE)                                          # the setter itself never refuses
        if ok:
            doa.submit(pk.ptr, pk.stride, pk.offset, T)
            assert doa.fetch_esprit()["phases"].shape == (1, k, 2)
        else:
            _refused(b, ESTATE, doa.submit, pk.ptr, pk.stride, pk.offset, T)
            doa.set_esprit(b.ESPRIT_OFF)
            doa.submit(pk.ptr, pk.stride, pk.offset, T)                          # and without it the object works as ever
        doa.close()
    # 17 sources at most 16 slots; an order range that ends above the rank limit
    doa = b.Doa(65, 2 * L, 17, 0.5, 8, 8, 8, 8, max_batch=T)
    pk = Packets(torch, ura.scene(L, [(1.0, 1.3, 1.0)], rng, mx=8, my=8, d=np.float32(0.5))[None])
    doa.set_esprit(b.ESPRIT_ONLY)
    _refused(b, ESTATE, doa.submit, pk.ptr, pk.stride, pk.offset, T)
    doa.close()
    doa = b.Doa(7, 2 * L, 1, 0.5, 3, 2, 8, 8, max_batch=T)
    pk = Packets(torch, ura.scene(L, [(1.0, 1.3, 1.0)], rng, mx=3, my=2, d=np.float32(0.5))[None])
    doa.set_esprit(b.ESPRIT_BESIDE)
    doa.set_order(b.ORDER_MDL, 1, 4)
    _refused(b, ESTATE, doa.submit, pk.ptr, pk.stride, pk.offset, T)
    doa.set_order(b.ORDER_MDL, 1, 3)
    doa.submit(pk.ptr, pk.stride, pk.offset, T)
    assert doa.fetch_esprit()["phases"].shape == (1, 3, 2)
    doa.close()


# ---- 5. end to end -----------------------------------------------------------------------------------------------------------------------

def test_through_a_plan_the_direction_lies_within_a_cell_of_the_peak(b, torch):
    # calibrate (reference noise on), freeze, a batch of scene blocks with a moving source: plan.submit and doa.submit_plan back to back
    rng = np.random.default_rng(31)
    L, M, T = 2048, 21, 4
    phi = rng.uniform(-np.pi, np.pi, M)
    plan = b.Plan(M + 1, 2 * L, b.MODE_FAITHFUL, max_batch=T)
    doa = b.Doa(M + 1, 2 * L, 1, ura.D, ura.MX, ura.MY, max_batch=T)
    doa.set_esprit(b.ESPRIT_BESIDE)
    for t in range(16):
        plan.block(ura.calibration_block(L, phi, rng), seq=t)
    dirs = [(0.8 + 0.1 * t, 2.3 - 0.08 * t) for t in range(T)]
    rows = np.stack([ura.scene(L, [(al, be, 1.0)], rng, phi=phi) for al, be in dirs])
    plan.submit(rows, seq=16, flags=0)
    doa.submit_plan(plan)                                                        # no sync, no fetch in between
    got, peak = doa.fetch_esprit(), doa.fetch()["peak"]
    assert doa.last_launches() == 6 and got["found"].tolist() == [1] * T
    for t, (al, be) in enumerate(dirs):
        alpha, beta = got["angles"][t, 0]
        assert abs(alpha - peak[t, 0] * P / 100) <= em.DIRECTION_BAR and abs(beta - peak[t, 1] * P / 100) <= em.DIRECTION_BAR, (t, alpha, beta, peak[t])
        assert abs(alpha - (P - al)) <= em.DIRECTION_BAR and abs(beta - (P - be)) <= em.DIRECTION_BAR, (t, alpha, beta, al, be)
        assert abs(got["modulus"][t, 0] - 1).max() < 0.05
    plan.sync()
    doa.close()
    plan.close()
