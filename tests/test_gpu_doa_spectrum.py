"""GPU checks of the Bartlett and Capon power maps (crsdr_spectrum2d, crsdr_doa_set_spectrum) against the fp64 model of
tests/doa_spectrum_model.py, whose docstring derives the bound used here (tests/test_doa_spectrum_model.py shows on the CPU that a
float32 restatement meets it and single mistakes do not).  The per-op call is held to the bound at every grid point of every shape,
fed with numpy's eigenvectors so that the scan is tested apart from the Jacobi; the engine is held to the per-op call bit for bit
(the same device function), and what follows the scan -- peak, directions, beams -- to its definition on the fetched map."""
import importlib

import numpy as np
import pytest

import doa_beams_model as beams_model
import doa_peaks_model as peaks_model
import doa_spectrum_model as sm
import music_model as mm
import ura
from music_model import SCAN_CASES, case_id

pytestmark = pytest.mark.gpu
EINVAL, ESTATE = -1, -5
LOADINGS = (1e-6, 1e-2, 1.0)
FAMILY_SHAPES = ((2, 1, 12, 9), (7, 3, 12, 9), (8, 8, 12, 9))          # M = 2, 21, 64
U32 = 2.0 ** -24


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


def _kinds(b):
    return (("bartlett", b.SPECTRUM_BARTLETT, sm.BARTLETT), ("capon", b.SPECTRUM_CAPON, sm.CAPON))


def _subspace32(R):
    lam, V = mm.eigh_by_magnitude(R)
    return V.astype(np.complex64), lam.astype(np.float32)


def _scenes(T, L, mx, my, seed):
    """T blocks of one to three incoherent sources of different strengths"""
    rng = np.random.default_rng(seed)
    dirs = [(0.35 * np.pi, 0.40 * np.pi), (0.65 * np.pi, 0.62 * np.pi), (0.45 * np.pi, 0.70 * np.pi)]
    return np.stack([ura.scene(L, [(a, be, 1.0 - 0.2 * i) for i, (a, be) in enumerate(dirs[:1 + t % 3])], rng, mx=mx, my=my) for t in range(T)])


# ---- crsdr_spectrum2d ---------------------------------------------------------------------------------------------------------------

def _check_perop(b, vec, sv, mx, my, ncx, ncy, label):
    """both kinds, every loading, every grid point against the bound; returns the worst fraction"""
    worst = 0.0
    for name, kind, mkind in _kinds(b):
        for loading in (LOADINGS if mkind == sm.CAPON else (0.0,)):
            S, bound = sm.maps(vec, sv, mkind, loading, ura.D, mx, my, ncx, ncy)
            pm = b.spectrum2d(vec, sv, kind, ura.D, mx, my, ncx, ncy, loading=loading)
            assert pm.shape == (ncx, ncy) and np.all(np.isfinite(pm)) and np.all(pm > 0), (label, name, loading)
            frac, median = sm.fractions(pm, mkind, S, bound)
            print(f"device {name} {label} loading {loading:g}: worst fraction of the bound {frac:.3f}, median relative error {median:.2e}, "
                  f"worst relative bound {float((bound / S).max()):.1e}")
            assert frac <= 1.0, (label, name, loading, frac)
            peak = np.unravel_index(int(np.argmax(peaks_model.keys(pm))), pm.shape)
            assert sm.admissible_peak(S, bound, mkind, peak), (label, name, loading, peak)
            worst = max(worst, frac)
    return worst


@pytest.mark.parametrize("c", SCAN_CASES, ids=case_id)
def test_perop_against_fp64_at_every_point(b, torch, c):
    # M = 2 (both orientations), M = 64 (8 x 8, 64 x 1, 1 x 64: the LDS above 64 KiB), grids whose points do not fill the last wave
    mx, my, ncx, ncy = c["mx"], c["my"], c["ncx"], c["ncy"]
    m = mx * my
    vec, sv = _subspace32(mm.hermitian32(mm.rxx_reference(mm.case_scene(c, L=1024)[0])))
    _check_perop(b, vec, sv, mx, my, ncx, ncy, case_id(c))
    # host and device pointers: the same bits
    dev = torch.device("cuda", 0)
    d_vec = torch.from_numpy(np.ascontiguousarray(vec).view(np.float32)).to(dev)
    d_sv = torch.from_numpy(sv).to(dev)
    for name, kind, _ in _kinds(b):
        d_pm = torch.full((ncx * ncy,), -1.0, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        b.spectrum2d_device(d_pm.data_ptr(), d_vec.data_ptr(), d_sv.data_ptr(), m, kind, ura.D, mx, my, ncx, ncy, loading=1e-2)
        assert _same_bits(d_pm.cpu().numpy().reshape(ncx, ncy), b.spectrum2d(vec, sv, kind, ura.D, mx, my, ncx, ncy, loading=1e-2)), name


@pytest.mark.parametrize("name", mm.FAMILIES)
def test_perop_on_the_spectrum_families(b, name):
    # strong values over a clustered floor, six decades of range, exact rank deficiency (Capon's weights are then 1 / delta), plateaus
    for mx, my, ncx, ncy in FAMILY_SHAPES:
        vec, sv = _subspace32(mm.family(mx * my, name)[0])
        _check_perop(b, vec, sv, mx, my, ncx, ncy, f"{name} {mx}x{my}")


def test_perop_all_zero_estimate_is_a_zero_map(b):
    for mx, my in ((2, 1), (7, 3), (8, 8)):
        m = mx * my
        vec, sv = np.eye(m, dtype=np.complex64), np.zeros(m, dtype=np.float32)
        for name, kind, _ in _kinds(b):
            pm = b.spectrum2d(vec, sv, kind, ura.D, mx, my, 13, 11, loading=1e-2)
            assert pm.shape == (13, 11) and not _bits(pm).any(), (m, name)       # +0.0 at every point


# ---- the engine ---------------------------------------------------------------------------------------------------------------------

def _check_engine(b, doa, out, vec, kind, loading, sx, sy, ncx, ncy, dirs=None, count=0, radius=0):
    """every estimate's pm is the per-op call's on its fetched vec / sv; peak and directions are their definitions on that pm"""
    nest = out["pm"].shape[0]
    assert vec.shape[0] == nest and out["sv"].shape[0] == nest
    for e in range(nest):
        pm1 = b.spectrum2d(vec[e], out["sv"][e], kind, ura.D, sx, sy, ncx, ncy, loading=loading)
        assert _same_bits(pm1, out["pm"][e]), e
        g = int(np.argmax(peaks_model.keys(pm1)))
        assert out["peak"][e].tolist() == [g // ncy, g % ncy], e
        assert _bits(out["peak_value"][e:e + 1])[0] == _bits(pm1.reshape(-1)[g:g + 1])[0], e
    if dirs is not None:
        want = peaks_model.batch_directions(out["pm"], count, radius)
        assert np.array_equal(dirs["found"], want["found"]) and np.array_equal(dirs["peaks"], want["peaks"])
        assert _same_bits(dirs["values"], want["values"])
        assert np.array_equal(dirs["peaks"][:, 0], out["peak"])                  # the first direction is the peak


@pytest.mark.parametrize("frames,nblocks", [(1, 4), (1, 3), (2, 4), (2, 2)])
def test_engine_equals_the_perop_call(b, torch, frames, nblocks):
    mx, my, L, T, ncx, ncy = 7, 3, 512, 4, 33, 17
    m = mx * my
    blocks = _scenes(T, L, mx, my, 11)
    pk = Packets(torch, blocks)
    doa = b.Doa(m + 1, 2 * L, 2, ura.D, mx, my, ncx, ncy, max_batch=T, frames=frames, flags=b.DOA_KEEP_SPECTRUM)
    doa.set_peaks(3, 2)
    for name, kind, _ in _kinds(b):
        doa.set_spectrum(kind, 1e-2)
        doa.submit(pk.ptr, pk.stride, pk.offset, nblocks)
        out, vec, dirs = doa.fetch(), doa.fetch_subspace(), doa.fetch_directions()
        assert out["pm"].shape == (nblocks // frames, ncx, ncy)
        _check_engine(b, doa, out, vec, kind, 1e-2, mx, my, ncx, ncy, dirs, 3, 2)
    doa.close()


def test_engine_same_bits_at_every_position_of_the_batch(b, torch):
    mx, my, L, T, ncx, ncy = 7, 3, 512, 4, 33, 17
    blocks = _scenes(T, L, mx, my, 12)
    doa = b.Doa(mx * my + 1, 2 * L, 1, ura.D, mx, my, ncx, ncy, max_batch=T, flags=b.DOA_KEEP_SPECTRUM)
    for name, kind, _ in _kinds(b):
        doa.set_spectrum(kind, 1e-2)
        first = None
        for shift in range(T):
            pk = Packets(torch, np.roll(blocks, shift, axis=0))
            doa.submit(pk.ptr, pk.stride, pk.offset, T)
            out = doa.fetch()
            pm = np.roll(out["pm"], -shift, axis=0)                              # back to the blocks' own order
            first = pm if first is None else first
            assert _same_bits(pm, first), (name, shift)
    doa.close()


def test_engine_on_smoothed_sub_arrays(b, torch):
    # forward-backward averaging and 2 x 2 sub-arrays of a 3 x 2 array: M = 4, the map is a 2 x 2 array's
    mx, my, sx, sy, L, T, ncx, ncy = 3, 2, 2, 2, 512, 4, 33, 17
    pk = Packets(torch, _scenes(T, L, mx, my, 13))
    doa = b.Doa(mx * my + 1, 2 * L, 1, ura.D, mx, my, ncx, ncy, max_batch=T, flags=b.DOA_KEEP_SPECTRUM)
    doa.set_smoothing(sx, sy, b.SMOOTH_FB)
    for name, kind, _ in _kinds(b):
        doa.set_spectrum(kind, 1e-2)
        doa.submit(pk.ptr, pk.stride, pk.offset, T)
        out, vec = doa.fetch(), doa.fetch_subspace()
        assert vec.shape == (T, 4, 4) and out["sv"].shape == (T, 4)
        _check_engine(b, doa, out, vec, kind, 1e-2, sx, sy, ncx, ncy)
    doa.close()


def test_engine_per_band(b, torch):
    # nfft 8, two bands of two bins: a map per (estimate, band), estimate e's band i at e * 2 + i
    mx, my, L, T, ncx, ncy = 7, 3, 512, 4, 33, 17
    pk = Packets(torch, _scenes(T, L, mx, my, 14))
    doa = b.Doa(mx * my + 1, 2 * L, 1, ura.D, mx, my, ncx, ncy, max_batch=T, flags=b.DOA_KEEP_SPECTRUM)
    doa.set_subbands(8, 1, 2, 2)
    doa.set_peaks(2, 2)
    for name, kind, _ in _kinds(b):
        doa.set_spectrum(kind, 1e-2)
        doa.submit(pk.ptr, pk.stride, pk.offset, T)
        out, vec, dirs = doa.fetch(), doa.fetch_subspace(), doa.fetch_directions()
        assert out["pm"].shape == (2 * T, ncx, ncy)
        _check_engine(b, doa, out, vec, kind, 1e-2, mx, my, ncx, ncy, dirs, 2, 2)
    doa.close()


def test_engine_ignores_the_source_count(b, torch):
    # crsdr_doa_set_order on: pm as with it off (and as with another desc.k); the order is still computed and caps found
    mx, my, L, T, ncx, ncy = 7, 3, 512, 4, 33, 17
    m = mx * my
    pk = Packets(torch, _scenes(T, L, mx, my, 15))
    plain = b.Doa(m + 1, 2 * L, 1, ura.D, mx, my, ncx, ncy, max_batch=T, flags=b.DOA_KEEP_SPECTRUM)
    counted = b.Doa(m + 1, 2 * L, 5, ura.D, mx, my, ncx, ncy, max_batch=T, flags=b.DOA_KEEP_SPECTRUM)
    counted.set_order(b.ORDER_MDL, 1, m - 1, limit_directions=True)
    counted.set_peaks(8, 1)
    plain.set_peaks(8, 1)
    for name, kind, _ in _kinds(b):
        for doa in (plain, counted):
            doa.set_spectrum(kind, 1e-2)
            doa.submit(pk.ptr, pk.stride, pk.offset, T)
        a, c = plain.fetch(), counted.fetch()
        assert _same_bits(a["pm"], c["pm"]) and np.array_equal(a["peak"], c["peak"]) and _same_bits(a["peak_value"], c["peak_value"]), name
        ke = counted.fetch_order()["k"]
        assert ke.shape == (T,) and np.all((ke >= 1) & (ke <= m - 1))
        da, dc = plain.fetch_directions(), counted.fetch_directions()
        assert np.array_equal(dc["found"], np.minimum(da["found"], ke)), (name, da["found"], ke)
        for e in range(T):
            n = int(dc["found"][e])
            assert np.array_equal(dc["peaks"][e, :n], da["peaks"][e, :n]) and np.all(dc["peaks"][e, n:] == -1) and np.all(dc["values"][e, n:] == -1.0)
    plain.close()
    counted.close()


FIND_CASES = [c for c in SCAN_CASES if c["find"]] + [c for c in SCAN_CASES if case_id(c) in ("8x8-k63-30x20", "7x3-k20-24x36")]


@pytest.mark.parametrize("c", FIND_CASES, ids=case_id)
def test_engine_peak_is_the_models_certain_peak(b, torch, c):
    mx, my, ncx, ncy = c["mx"], c["my"], c["ncx"], c["ncy"]
    m = mx * my
    blocks = mm.case_scene(c, L=1024)
    pk = Packets(torch, blocks)
    doa = b.Doa(m + 1, 2048, c["k"], ura.D, mx, my, ncx, ncy, max_batch=1, flags=b.DOA_KEEP_SPECTRUM)
    for name, kind, mkind in _kinds(b):
        doa.set_spectrum(kind, 1e-2)
        doa.submit(pk.ptr, pk.stride, pk.offset, 1)
        out, vec = doa.fetch(), doa.fetch_subspace()
        assert out["status"][0] == 0
        S, bound = sm.maps(vec[0], out["sv"][0], mkind, 1e-2, ura.D, mx, my, ncx, ncy)
        frac, _ = sm.fractions(out["pm"][0], mkind, S, bound)
        certain = sm.certain_peak(S, bound, mkind)
        print(f"engine {name} {case_id(c)}: worst fraction of the bound {frac:.3f}, peak {out['peak'][0].tolist()}, certain {certain}")
        assert frac <= 1.0
        assert certain is not None and certain in c["src"]                       # the strongest source's own grid point
        assert tuple(int(v) for v in out["peak"][0]) == certain
    doa.close()


def _submit_all(doa, pk, T):
    doa.submit(pk.ptr, pk.stride, pk.offset, T)
    return doa.fetch()


def test_launches_are_those_of_music(b, torch):
    mx, my, L, T = 7, 3, 512, 4
    m = mx * my
    pk = Packets(torch, _scenes(T, L, mx, my, 16))
    doa = b.Doa(m + 1, 2 * L, 2, ura.D, mx, my, 33, 17, max_batch=T)
    steps = (("plain", lambda: None, 5), ("peaks", lambda: doa.set_peaks(3, 2), 7), ("beams", lambda: doa.set_beams(b.BEAM_MVDR, 1e-2), 9),
             ("order", lambda: doa.set_order(b.ORDER_MDL, 1, m - 1), 10), ("fb", lambda: doa.set_smoothing(mx, my, b.SMOOTH_FB), 11))
    for what, turn_on, want in steps:
        turn_on()
        for kind in (b.SPECTRUM_MUSIC, b.SPECTRUM_BARTLETT, b.SPECTRUM_CAPON):
            doa.set_spectrum(kind, 1e-2)
            _submit_all(doa, pk, T)
            assert doa.last_launches() == want, (what, kind)
    doa.close()


def test_switching_back_and_forth_gives_the_bits_of_fresh_objects(b, torch):
    mx, my, L, T, ncx, ncy = 7, 3, 512, 4, 33, 17
    m = mx * my
    pk = Packets(torch, _scenes(T, L, mx, my, 17))
    make = lambda: b.Doa(m + 1, 2 * L, 2, ura.D, mx, my, ncx, ncy, max_batch=T, flags=b.DOA_KEEP_SPECTRUM)
    fresh = {}
    for kind in (b.SPECTRUM_MUSIC, b.SPECTRUM_BARTLETT, b.SPECTRUM_CAPON):
        d = make()
        if kind != b.SPECTRUM_MUSIC:
            d.set_spectrum(kind, 1e-2)
        fresh[kind] = _submit_all(d, pk, T)
        d.close()
    assert not _same_bits(fresh[b.SPECTRUM_MUSIC]["pm"], fresh[b.SPECTRUM_CAPON]["pm"])
    assert not _same_bits(fresh[b.SPECTRUM_BARTLETT]["pm"], fresh[b.SPECTRUM_CAPON]["pm"])
    d = make()
    for kind in (b.SPECTRUM_CAPON, b.SPECTRUM_MUSIC, b.SPECTRUM_BARTLETT, b.SPECTRUM_MUSIC, b.SPECTRUM_CAPON, b.SPECTRUM_MUSIC):
        d.set_spectrum(kind, 1e-2 if kind == b.SPECTRUM_CAPON else 0.0)
        out = _submit_all(d, pk, T)
        for key in ("pm", "peak_value", "sv"):
            assert _same_bits(out[key], fresh[kind][key]), (kind, key)
        assert np.array_equal(out["peak"], fresh[kind]["peak"]), kind
    d.close()


def _estate(b, call):
    with pytest.raises(b.CrsdrError) as e:
        call()
    assert e.value.code == ESTATE


def test_setter_discards_the_last_submit_and_is_accepted_with_everything_on(b, torch):
    mx, my, L, T = 7, 3, 512, 4
    m = mx * my
    pk = Packets(torch, _scenes(T, L, mx, my, 18))
    L_ = b.lib()
    doa = b.Doa(m + 1, 2 * L, 2, ura.D, mx, my, 33, 17, max_batch=T, flags=b.DOA_KEEP_SPECTRUM)
    # before any submit, and with nothing else on
    for kind in (b.SPECTRUM_BARTLETT, b.SPECTRUM_CAPON, b.SPECTRUM_MUSIC):
        assert L_.crsdr_doa_set_spectrum(doa._h, kind, 1e-2) == 0
    # every other feature on, in the order the header fixes: bands, then smoothing, order, peaks, band beams
    doa.set_subbands(8, 1, 2, 2)
    doa.set_smoothing(mx, my, b.SMOOTH_FB)
    doa.set_order(b.ORDER_AIC, 1, 3, limit_directions=True)
    doa.set_peaks(3, 2)
    doa.set_subband_beams(b.BEAM_MVDR, 1e-2)
    fetches = (doa.fetch, doa.fetch_subspace, doa.fetch_directions, doa.fetch_order, doa.fetch_subbands, doa.fetch_smoothed,
               lambda: doa.fetch_subband_beams(beams=False), doa.last_launches)
    for kind, loading in ((b.SPECTRUM_CAPON, 1e-6), (b.SPECTRUM_BARTLETT, 0.0), (b.SPECTRUM_MUSIC, -3.0), (b.SPECTRUM_CAPON, 1.0)):
        _submit_all(doa, pk, T)
        for f in fetches:
            f()                                                                  # all there
        assert L_.crsdr_doa_set_spectrum(doa._h, kind, loading) == 0, (kind, loading)   # loading matters to CAPON alone
        for f in fetches:
            _estate(b, f)                                                        # gone until the next submit
        out = _submit_all(doa, pk, T)
        assert out["pm"].shape[0] == 2 * T and doa.last_launches() == 5 + 1 + 1 + 2 + 2
    # refused: a bad kind, CAPON's loading outside [1e-6, 1]; a refusal changes nothing, what the last submit left stays
    for kind, loading in ((3, 1e-2), (-1, 1e-2), (b.SPECTRUM_CAPON, 0.0), (b.SPECTRUM_CAPON, 5e-7), (b.SPECTRUM_CAPON, 1.5), (b.SPECTRUM_CAPON, float("nan"))):
        assert L_.crsdr_doa_set_spectrum(doa._h, kind, loading) == EINVAL, (kind, loading)
    before = doa.fetch()
    assert _same_bits(before["pm"], out["pm"])
    # it refuses no other setter: each one answers as its own rules say, with a map on as with MUSIC
    doa.set_spectrum(b.SPECTRUM_CAPON, 1e-2)
    with pytest.raises(b.CrsdrError) as e:
        doa.set_subbands(0)                                                      # its own rule: the others are on
    assert e.value.code == ESTATE
    with pytest.raises(b.CrsdrError) as e:
        doa.set_peaks(2, 1)                                                      # its own rule: beams follow the directions
    assert e.value.code == ESTATE
    doa.set_subband_beams(b.BEAM_OFF)
    doa.set_peaks(0)
    doa.set_order(b.ORDER_OFF)
    doa.set_smoothing(mx, my, 0)
    doa.set_subbands(0)
    doa.set_smoothing(5, 2, 0)                                                   # true sub-arrays
    doa.set_order(b.ORDER_MDL, 1, 9)
    doa.set_peaks(4, 1)
    with pytest.raises(b.CrsdrError) as e:
        doa.set_beams(b.BEAM_MVDR, 1e-2)                                         # its own rule: no m x m subspace under sub-arrays
    assert e.value.code == ESTATE
    doa.set_smoothing(mx, my, 0)
    doa.set_beams(b.BEAM_CONVENTIONAL)
    out = _submit_all(doa, pk, T)
    assert out["pm"].shape[0] == T and doa.last_launches() == 5 + 1 + 2 + 2
    doa.close()


def test_map_values_agree_with_the_beams_power(b, torch):
    """BARTLETT with following CONVENTIONAL beams, CAPON with following MVDR beams of the same loading: the beam's power toward a found
    direction is the map's value there -- the first in fp64 at the grid angle, rounded once, the second the fp32 scan.  Both are
    within the model's bound of the fp64 S at that point, the power within one rounding: the bar is the bound plus 2u of S."""
    mx, my, L, T, ncx, ncy, count = 7, 3, 1024, 4, 100, 100, 4
    m = mx * my
    pk = Packets(torch, _scenes(T, L, mx, my, 19))
    worst = 0.0
    for (name, kind, mkind), mode, loading in zip(_kinds(b), (b.BEAM_CONVENTIONAL, b.BEAM_MVDR), (0.0, 1e-2)):
        doa = b.Doa(m + 1, 2 * L, 2, ura.D, mx, my, ncx, ncy, max_batch=T)
        doa.set_spectrum(kind, loading if mkind == sm.CAPON else 1e-2)
        doa.set_peaks(count, 2)
        doa.set_beams(mode, loading if mkind == sm.CAPON else 1e-2)
        out = _submit_all(doa, pk, T)
        vec, dirs, bm = doa.fetch_subspace(), doa.fetch_directions(), doa.fetch_beams(weights=False, beams=False)
        doa.close()
        for e in range(T):
            S, bound = sm.maps(vec[e], out["sv"][e], mkind, loading, ura.D, mx, my, ncx, ncy)
            n = int(dirs["found"][e])
            assert n >= 1
            for s in range(count):
                if s >= n:
                    assert bm["power"][e, s] == -1.0 and dirs["values"][e, s] == -1.0
                    continue
                p = tuple(int(v) for v in dirs["peaks"][e, s])
                bar = bound[p] + 2 * U32 * S[p]
                err = abs(float(sm.s_of(dirs["values"][e, s], mkind)) - float(sm.s_of(bm["power"][e, s], mkind)))
                worst = max(worst, err / bar)
                assert err <= bar, (name, e, s, p, dirs["values"][e, s], bm["power"][e, s], err, bar)
        print(f"{name}: largest |value - power| (as S) / bar over the found directions {worst:.3f}")


def test_capon_resolves_what_bartlett_merges(b, torch):
    # the scene of tests/test_doa_spectrum_model.py: two equal sources six grid steps apart; inside the region one direction or two
    pk = Packets(torch, sm.resolution_block()[None])
    doa = b.Doa(ura.MX * ura.MY + 1, 2 * sm.RES_L, 2, ura.D, ura.MX, ura.MY, 100, 100, max_batch=1, flags=b.DOA_KEEP_SPECTRUM)
    doa.set_peaks(16, sm.RES_RADIUS)
    rx, ry = sm.RES_REGION
    for (name, kind, mkind), want in zip(_kinds(b), ([(50, 50)], sorted(sm.RES_PEAKS))):
        doa.set_spectrum(kind, sm.RES_LOADING)
        out = _submit_all(doa, pk, 1)
        dirs = doa.fetch_directions()
        inside = sorted((int(x), int(y)) for x, y in dirs["peaks"][0, :int(dirs["found"][0])] if rx.start <= x < rx.stop and ry.start <= y < ry.stop)
        print(f"{name}: directions in the region {inside} of {int(dirs['found'][0])} found")
        assert inside == want, name
        assert sm.region_peaks(out["pm"][0]) == want
        if mkind == sm.CAPON:
            assert sorted(tuple(int(v) for v in p) for p in dirs["peaks"][0, :2]) == want      # and they are the map's two strongest
    doa.close()
