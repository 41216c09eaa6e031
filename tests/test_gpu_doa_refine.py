"""GPU checks of the directions off the scan grid (crsdr_doa_set_refine / crsdr_doa_fetch_refined / crsdr_refine2d) against the fp64
model of tests/doa_refine_model.py, whose docstring states the search and the allowance tol (the project's own scan bounds with
u = 2^-53, times 4 for the device's libm).

Check 1, on the device's own vec / sv and directions: every non-empty slot's offsets are, exactly, one of the final points the model
can reach within tol (branches); they are multiples of 2^-9 below 2 in magnitude that stay inside the grid's range; angles are
float32((peak + offset) pi / nc); value stands for the model's quantity at that point within tol plus 2^-24 relative; empty slots hold
(0, 0), (-1, -1) and -1.  At most 1 slot in 20 may have more than one reachable point.

End to end (test_end_to_end_against_the_fp64_chain).  Allowance: 2 steps of 2^-9 between the device's direction (fp32 rxx and vec) and the
all-fp64 chain's (own covariance, numpy eigh).  Measured on the device: 0 steps in all nine cases ('Directions off the scan
grid')."""
import importlib

import numpy as np
import pytest

import doa_beams_model as beams_model
import doa_refine_model as rm
import music_model as mm
import ura

pytestmark = pytest.mark.gpu
EINVAL, ESTATE = -1, -5
LEVELS = 5
S_LAST = 2.0 ** -(2 * LEVELS - 1)
LOADING = 1e-2
REL = 2.0 ** -22                       # the beams' existing bar (tests/test_gpu_doa_beams.py)


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
    return (("music", b.SPECTRUM_MUSIC, rm.MUSIC), ("bartlett", b.SPECTRUM_BARTLETT, rm.BARTLETT), ("capon", b.SPECTRUM_CAPON, rm.CAPON))


def _scene(T, L, mx, my, nc, d, seed, nsrc=1, spots=((0.45, 0.55), (0.7, 0.3))):
    """T blocks, each of nsrc emitters whose map peaks sit off the grid points of an nc x nc grid"""
    rng = np.random.default_rng(seed)
    blocks = []
    for t in range(T):
        src = [(*mm.mirrored_source(fx * nc + 0.37 - 0.21 * t, fy * nc - 0.29 + 0.17 * t, nc, nc), 1.0 - 0.3 * i) for i, (fx, fy) in enumerate(spots[:nsrc])]
        blocks.append(ura.scene(L, src, rng, mx=mx, my=my, d=np.float32(d)))
    return np.stack(blocks)


def _directions(doa):
    """(found [n], dirs [n][slots][2]) of the last submit: the local peaks, or the one peak"""
    if doa.npeaks:
        got = doa.fetch_directions()
        return got["found"], got["peaks"]
    peak = doa.fetch_peaks()
    return np.ones(len(peak), dtype=np.int32), peak[:, None, :]


def _check1(doa, ref, mkind, loading, d, sx, sy, ks=None, what=""):
    """check 1 of the module docstring on every matrix and slot of the last submit; returns (non-empty slots, those with several branches)"""
    vec, sv = doa.fetch_subspace(), doa.fetch()["sv"]
    found, dirs = _directions(doa)
    n, slots = dirs.shape[:2]
    ncx, ncy, M = doa.ncx, doa.ncy, sx * sy
    assert ref["offsets"].shape == (n, slots, 2) and ref["angles"].shape == (n, slots, 2) and ref["values"].shape == (n, slots), what
    live = multi = 0
    for e in range(n):
        k = int(ks[e]) if ks is not None else doa.k
        args = (vec[e], sv[e], mkind, k, loading, d, sx, sy, ncx, ncy)
        for s in range(slots):
            o, ang, val = ref["offsets"][e, s], ref["angles"][e, s], ref["values"][e, s]
            if s >= found[e]:
                assert not _bits(o).any() and ang.tolist() == [-1.0, -1.0] and val == -1.0, (what, e, s)
                continue
            live += 1
            peak = dirs[e, s]
            reach = rm.branches(*args, peak, LEVELS)
            multi += len(reach) > 1
            got = (float(o[0]), float(o[1]))
            assert got in reach, (what, e, s, peak.tolist(), got, sorted(reach))
            x, y = float(peak[0]) + got[0], float(peak[1]) + got[1]
            assert all(abs(v) < 2 and v / S_LAST == round(v / S_LAST) for v in got) and 0 <= x <= ncx and 0 <= y <= ncy, (what, e, s, got)
            assert _same_bits(ang, np.array([x * np.pi / ncx, y * np.pi / ncy]).astype(np.float32)), (what, e, s)
            q, tol, f = rm.f_at(*args, x, y)
            qd = rm.q_of(val, mkind, M)
            assert abs(qd - q) <= tol + 2.0 ** -24 * abs(q), (what, e, s, float(val), f, qd, q, tol)
    return live, multi


# ---- 1. exact offsets ----------------------------------------------------------------------------------------------------------------

# The line array's map depends on cos(alpha) sin(beta) alone, which on a square grid has mirror lines (y = x + nc / 2, x = y + nc / 2,
# x + y = nc / 2, x + y = 3 nc / 2, y = nc / 2) that map the lattice onto itself: where its grid peak lies near one of them, mirrored
# lattice points tie exactly and the slot has two reachable points.  Every ridge crosses such lines and the scan's peak is any grid
# point along the ridge, so the line array's slots are where branches are expected; its scene keeps the peak of both blocks away from the
# lines (measured on the device: none of the 78 slots of this test has more than one branch).
SHAPES = (dict(mx=3, my=2, nc=16, k=1, nsrc=1, peaks=None, T=4), dict(mx=7, my=3, nc=20, k=2, nsrc=2, peaks=(4, 2), T=4),
          dict(mx=8, my=8, nc=12, k=1, nsrc=1, peaks=None, T=4), dict(mx=4, my=1, nc=16, k=1, nsrc=1, peaks=None, T=2, spots=((0.62, 0.33),)))


def test_offsets_are_exactly_the_models(b, torch):
    # M = 6, 21 with empty slots, 64 (the LDS limit), a line array (the map is constant along curves of the grid)
    live = multi = 0
    for i, c in enumerate(SHAPES):
        mx, my, nc, L, T = c["mx"], c["my"], c["nc"], 256, c["T"]
        d = 0.5 if (mx, my) != (7, 3) else float(ura.D)
        pk = Packets(torch, _scene(T, L, mx, my, nc, d, 40 + i, c["nsrc"], **({"spots": c["spots"]} if "spots" in c else {})))
        doa = b.Doa(mx * my + 1, 2 * L, c["k"], d, mx, my, nc, nc, max_batch=T)
        if c["peaks"]:
            doa.set_peaks(*c["peaks"])
        doa.set_refine(LEVELS)
        for name, kind, mkind in _kinds(b):
            doa.set_spectrum(kind, LOADING)
            doa.submit(pk.ptr, pk.stride, pk.offset, T)
            l, m_ = _check1(doa, doa.fetch_refined(), mkind, LOADING, d, mx, my, what=f"{mx}x{my} {name}")
            print(f"{mx}x{my} on {nc}x{nc} {name}: {l} slots, {m_} with more than one branch")
            live, multi = live + l, multi + m_
        doa.close()
    assert live >= 60 and 20 * multi <= live, (live, multi)


# ---- 2. end to end -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sc", rm.SCENES, ids=[f"{s['mx']}x{s['my']}" for s in rm.SCENES])
def test_end_to_end_against_the_fp64_chain(b, torch, sc):
    """Measured on the device (steps of 2^-9 between the device's direction and the all-fp64 chain's, the nine cases in the order of
    doa_refine_model.SCENES x OFFSETS): 0, 0, 0; 0, 0, 0; 0, 0, 0.  The allowance of 2 is one for a near-tie at the last level and one for
    the fp32 rxx / vec; the refined direction was 1/18 to 1/133 of the grid peak's distance from the true cell (asserted: 1/5)."""
    mx, my, nc, d, L = sc["mx"], sc["my"], sc["nc"], sc["d"], sc["L"]
    doa = b.Doa(mx * my + 1, 2 * L, 1, d, mx, my, nc, nc, max_batch=1)
    doa.set_refine(LEVELS)
    for off in rm.OFFSETS:
        block = rm.scene_block(sc, off)
        pk = Packets(torch, block[None])
        doa.submit(pk.ptr, pk.stride, pk.offset, 1)
        peak, ref = doa.fetch_peaks()[0], doa.fetch_refined()
        dev = (float(peak[0]) + float(ref["offsets"][0, 0, 0]), float(peak[1]) + float(ref["offsets"][0, 0, 1]))
        sv, vec = rm.fp64_subspace(block)
        args = (vec, sv, rm.MUSIC, 1, 0.0, d, mx, my, nc, nc)
        mpeak = rm.grid_peak(*args)
        o = rm.refine(*args, mpeak, LEVELS)[0]
        model = (mpeak[0] + o[0], mpeak[1] + o[1])
        steps = max(abs(dev[0] - model[0]), abs(dev[1] - model[1])) / S_LAST
        tx, ty = rm.true_cell(sc, off)
        grid, fine = np.hypot(peak[0] - tx, peak[1] - ty), np.hypot(dev[0] - tx, dev[1] - ty)
        print(f"{rm.scene_id(sc, off)}: device {dev} model {model}: {steps:g} steps; grid peak {grid:.3f} cells off, refined {fine:.4f} (1/{grid / fine:.0f})")
        assert steps <= 2, (rm.scene_id(sc, off), dev, model)
        assert fine <= grid / 5.0, (rm.scene_id(sc, off), grid, fine)
    doa.close()


# ---- 3. composition ------------------------------------------------------------------------------------------------------------------

def _compose(b, doa, case):
    """(sx, sy, frames) after the case's setters"""
    if case == "smooth":
        doa.set_smoothing(2, 2, b.SMOOTH_FB)
        return 2, 2
    if case == "order":
        doa.set_order(b.ORDER_MDL, 1, 3)
        doa.set_peaks(3, 1)
    if case == "subbands":
        doa.set_subbands(8, 0, 2, 1)
        doa.set_peaks(2, 1)
    return 3, 2


@pytest.mark.parametrize("case", ["smooth", "order", "subbands", "frames"])
def test_composition(b, torch, case):
    mx, my, B, nc, T, d = 3, 2, 64, 8, 4, 0.5
    frames = 2 if case == "frames" else 1
    # two emitters whose peaks and side lobes stay off the line beta = 0 (cy = 0), where sin(beta) = 0, the map does not depend on alpha
    # and the lattice points along x tie exactly: a local maximum there is a slot with many reachable points
    blocks = _scene(T, B // 2, mx, my, nc, d, 60, nsrc=2, spots=((0.3, 0.6), (0.7, 0.35)))
    doa = b.Doa(mx * my + 1, B, 1, d, mx, my, nc, nc, max_batch=T, frames=frames)
    sx, sy = _compose(b, doa, case)
    pk = Packets(torch, blocks)
    live = multi = 0
    for name, kind, mkind in _kinds(b):
        doa.set_spectrum(kind, LOADING)
        doa.set_refine(0)
        doa.submit(pk.ptr, pk.stride, pk.offset, T)
        plain = doa.last_launches()
        doa.set_refine(LEVELS)
        doa.submit(pk.ptr, pk.stride, pk.offset, T)
        assert doa.last_launches() == plain + 1, (case, name)
        ref = doa.fetch_refined()
        ks = doa.fetch_order()["k"] if case == "order" else None
        l, m_ = _check1(doa, ref, mkind, LOADING, d, sx, sy, ks=ks, what=f"{case} {name}")
        live, multi = live + l, multi + m_
        # the per-op call on the fetched subspace and directions: the same bits
        vec, sv = doa.fetch_subspace(), doa.fetch()["sv"]
        found, dirs = _directions(doa)
        nmat = len(found)
        assert nmat == (T // frames) * (2 if case == "subbands" else 1)
        for e in range(nmat):
            if found[e] == 0:
                continue
            one = doa.refine2d(vec[e], sv[e], dirs[e, :found[e]], kind=kind, k=int(ks[e]) if ks is not None else 1, loading=LOADING, levels=LEVELS)
            for key in ("offsets", "angles", "values"):
                assert _same_bits(one[key], ref[key][e, :found[e]]), (case, name, e, key)
        # every position of the batch: the same bits
        for shift in range(frames, T, frames):
            pk2 = Packets(torch, np.roll(blocks, shift, axis=0))
            doa.submit(pk2.ptr, pk2.stride, pk2.offset, T)
            moved = doa.fetch_refined()
            per = nmat // (T // frames)
            for key in ("offsets", "angles", "values"):
                assert _same_bits(np.roll(moved[key], -(shift // frames) * per, axis=0), ref[key]), (case, name, shift, key)
    print(f"{case}: {live} slots, {multi} with more than one branch")
    doa.close()
    assert live >= 6 and 20 * multi <= live, (case, live, multi)


# ---- 4. beams ------------------------------------------------------------------------------------------------------------------------

def _check_weights(got, vec, sv, found, dirs, ref, mode, loading, d, mx, my, nc, what):
    n, nb = got["weights"].shape[:2]
    worst = 0.0
    for e in range(n):
        slots = [((float(dirs[e, s, 0]) + float(ref["offsets"][e, s, 0])) * np.pi / nc, (float(dirs[e, s, 1]) + float(ref["offsets"][e, s, 1])) * np.pi / nc)
                 if s < found[e] else None for s in range(nb)]
        w, p = beams_model.slot_weights(vec[e], sv[e], slots, mode, loading, np.float32(d), mx, my)
        for s in range(nb):
            if slots[s] is None:
                assert not got["weights"][e, s].view(np.float32).any() and got["power"][e, s] == -1.0, (what, e, s)
                continue
            dw, r = np.abs(got["weights"][e, s].astype(np.complex128) - w[s].astype(np.complex128)).max(), np.abs(w[s]).max()
            dp = abs(float(got["power"][e, s]) - float(p[s]))
            worst = max(worst, dw / r, dp / abs(float(p[s])))
            assert dw <= REL * r and dp <= REL * abs(float(p[s])), (what, e, s, dw, r, dp)
    return worst


def test_following_beams_steer_at_the_refined_direction(b, torch):
    mx, my, nc, L, T, d = 7, 3, 20, 256, 2, float(ura.D)
    pk = Packets(torch, _scene(T, L, mx, my, nc, d, 70, nsrc=2))
    for mode, loading in ((b.BEAM_CONVENTIONAL, 0.0), (b.BEAM_MVDR, LOADING)):
        doa = b.Doa(mx * my + 1, 2 * L, 2, d, mx, my, nc, nc, max_batch=T)          # a fresh object: `before` is of one whose setter was never called
        doa.set_peaks(3, 2)
        doa.set_beams(mode, loading if mode == b.BEAM_MVDR else 0.5)
        doa.submit(pk.ptr, pk.stride, pk.offset, T)
        before = doa.fetch_beams()
        doa.set_refine(LEVELS)
        doa.submit(pk.ptr, pk.stride, pk.offset, T)
        got, ref = doa.fetch_beams(), doa.fetch_refined()
        found, dirs = _directions(doa)
        assert np.abs(ref["offsets"]).max() > 0 and not _same_bits(got["weights"], before["weights"])
        worst = _check_weights(got, doa.fetch_subspace(), doa.fetch()["sv"], found, dirs, ref, mode, loading, d, mx, my, nc, f"mode {mode}")
        print(f"mode {mode}: worst weights / power {worst / REL:.3f} of the 2^-22 bar")
        doa.set_refine(0)
        doa.submit(pk.ptr, pk.stride, pk.offset, T)
        after = doa.fetch_beams()
        for key in ("weights", "power", "beams"):
            assert _same_bits(after[key].view(np.float32), before[key].view(np.float32)), (mode, key)
        doa.close()


def test_band_beams_steer_at_the_refined_direction(b, torch):
    mx, my, nc, B, T, d = 3, 2, 8, 256, 2, 0.5
    pk = Packets(torch, _scene(T, B // 2, mx, my, nc, d, 71, nsrc=1))
    doa = b.Doa(mx * my + 1, B, 1, d, mx, my, nc, nc, max_batch=T)
    doa.set_subbands(8, 0, 2, 1)
    doa.set_subband_beams(b.BEAM_MVDR, LOADING)
    doa.submit(pk.ptr, pk.stride, pk.offset, T)
    before = doa.fetch_subband_beams()
    doa.set_refine(LEVELS)
    doa.submit(pk.ptr, pk.stride, pk.offset, T)
    got, ref = doa.fetch_subband_beams(), doa.fetch_refined()
    found, dirs = _directions(doa)
    assert ref["offsets"].shape == (2 * T, 1, 2) and np.abs(ref["offsets"]).max() > 0
    _check_weights(got, doa.fetch_subspace(), doa.fetch()["sv"], found, dirs, ref, b.BEAM_MVDR, LOADING, d, mx, my, nc, "band beams")
    doa.set_refine(0)
    doa.submit(pk.ptr, pk.stride, pk.offset, T)
    after = doa.fetch_subband_beams()
    for key in ("weights", "power", "beams"):
        assert _same_bits(after[key].view(np.float32), before[key].view(np.float32)), key
    doa.close()


# ---- 5. states -----------------------------------------------------------------------------------------------------------------------

def test_states(b, torch):
    mx, my, nc, L, T, d = 3, 2, 8, 64, 2, 0.5
    pk = Packets(torch, _scene(T, L, mx, my, nc, d, 80, nsrc=2))
    doa = b.Doa(mx * my + 1, 2 * L, 1, d, mx, my, nc, nc, max_batch=T)

    def refused(code, fn, *a):
        with pytest.raises(b.CrsdrError) as err:
            fn(*a)
        assert err.value.code == code, (fn.__name__, a, err.value)

    refused(ESTATE, doa.fetch_refined)                                           # no setter
    assert doa.refined_buffers() == dict(offsets=None, angles=None, values=None, slots=0)
    for levels in (-1, 9):
        refused(EINVAL, doa.set_refine, levels)
    doa.submit(pk.ptr, pk.stride, pk.offset, T)
    doa.set_refine(LEVELS)
    refused(ESTATE, doa.fetch_refined)                                           # before the first submit after it
    bufs = doa.refined_buffers()
    assert all(bufs[k] for k in ("offsets", "angles", "values")) and bufs["slots"] == 1
    doa.set_peaks(3, 1)
    doa.submit(pk.ptr, pk.stride, pk.offset, T)
    first = doa.fetch_refined()
    assert first["offsets"].shape == (T, 3, 2)
    doa.set_peaks(2, 2)                                                          # between submit and fetch: the old layout is still read
    again = doa.fetch_refined()
    assert all(_same_bits(again[k], first[k]) for k in first)
    doa.submit(pk.ptr, pk.stride, pk.offset, T)
    assert doa.fetch_refined()["offsets"].shape == (T, 2, 2)
    doa.set_spectrum(b.SPECTRUM_BARTLETT)                                        # discards what the last submit left
    refused(ESTATE, doa.fetch_refined)
    doa.submit(pk.ptr, pk.stride, pk.offset, T)
    assert doa.fetch_refined()["values"].shape == (T, 2)
    doa.set_refine(0)
    refused(ESTATE, doa.fetch_refined)
    assert doa.refined_buffers()["slots"] == 0
    doa.set_refine(1)                                                            # one level: offsets are multiples of 1/2
    doa.submit(pk.ptr, pk.stride, pk.offset, T)
    one = doa.fetch_refined()["offsets"]
    assert np.array_equal(one * 2, np.round(one * 2)) and np.abs(one).max() <= 1.5
    # the per-op call: a direction outside [0, nc] x [0, nc] is an empty slot; and a call on a small matrix leaves the kernel fit for M = 64
    vec, sv = doa.fetch_subspace()[0], doa.fetch()["sv"][0]
    got = doa.refine2d(vec, sv, [[3, 4], [nc + 1, 2], [-1, 0], [nc, nc]], kind=b.SPECTRUM_BARTLETT)
    assert not _bits(got["offsets"][1:3]).any() and got["angles"][1:3].tolist() == [[-1.0, -1.0]] * 2 and got["values"][1:3].tolist() == [-1.0, -1.0]
    assert got["values"][0] > 0 and got["values"][3] > 0 and np.all(got["offsets"][3] <= 0)
    doa.close()
    big = b.Doa(65, 2 * L, 1, d, 8, 8, nc, nc, max_batch=1)
    big.set_refine(2)
    pk64 = Packets(torch, _scene(1, L, 8, 8, nc, d, 81))
    big.submit(pk64.ptr, pk64.stride, pk64.offset, 1)
    assert big.fetch_refined()["values"][0, 0] > 0
    big.close()
