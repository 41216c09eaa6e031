"""GPU checks of co-array augmentation of crsdr_doa (crsdr_doa_set_augment / crsdr_doa_fetch_augmented / crsdr_augment_covariance)
against the fp64 numpy restatement in tests/doa_augment_model.py, whose docstring derives the bar used here:

    |dev - model| <= 2^-24 |model| + 2^-45 max|rxx| per component, the model fed with the device's own rxx

Everything behind the augmented matrix is an existing step on another matrix: the subspace against numpy (music_model's bars) and,
bit for bit, the per-op calls on the fetched ra; the source count, the Capon map, the refinement and ESPRIT each against their own
models fed the device's vec and sv with the virtual array's shape.  The 24 scenes are those of tests/test_doa_augment_model.py, which
holds the fp64 model to the same condition on the CPU."""
import importlib

import numpy as np
import pytest

import doa_augment_model as model
import doa_esprit_model as em
import doa_refine_model as rm
import doa_smooth_model as smooth_model
import doa_spectrum_model as sp
import music_model as mm
import ura

pytestmark = pytest.mark.gpu
EINVAL, ESTATE = -1, -5
D = float(ura.D)
THIN = model.mask_of(model.THINNED, 21)
DEAD = model.dead(21, (4, 16))


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


def _same_bits(a, c):
    a, c = np.ascontiguousarray(a), np.ascontiguousarray(c)
    return a.shape == c.shape and a.dtype == c.dtype and a.tobytes() == c.tobytes()


def _refused(b, code, fn, *a, **kw):
    with pytest.raises(b.CrsdrError) as err:
        fn(*a, **kw)
    assert err.value.code == code, (fn.__name__, a, err.value)
    return str(err.value)


@pytest.fixture(scope="module")
def scene_packets(torch):
    """the 24 scenes by source count, absent receivers' rows full-scale garbage: {(mask, k): (Packets of the 8 seeds' blocks, blocks)}"""
    out = {}
    for mask in (THIN, DEAD):
        for k in (1, 2, 3):
            blocks = np.stack([model.overwrite_absent(blk, mask) for _, kk, blk in model.scenes() if kk == k])
            assert blocks.shape == (8, 22, 2 * model.L)
            out[(mask, k)] = (Packets(torch, blocks), blocks)
    return out


# ---- 1. the matrix -------------------------------------------------------------------------------------------------------------------

SHAPES = [  # (mx, my, vx, vy, mask)
    (2, 1, 2, 1, 0),
    (1, 2, 1, 2, 0),
    (7, 1, 7, 1, model.mask_of(model.RULER, 7)),
    (7, 3, 7, 3, 0),
    (7, 3, 7, 3, DEAD),
    (7, 3, 7, 3, THIN),
    (7, 3, 5, 2, DEAD),
    (8, 8, 8, 8, 0),
    (8, 8, 4, 4, 0),
    (2, 32, 2, 32, 0),
    (64, 1, 64, 1, 0),
]


@pytest.mark.parametrize("mx,my,vx,vy,mask", SHAPES, ids=[f"{s[0]}x{s[1]}-{s[2]}x{s[3]}-{s[4]:x}" for s in SHAPES])
def test_matrix_against_the_model_per_op_and_batch_position(b, torch, mx, my, vx, vy, mask):
    m, mv, B, T = mx * my, vx * vy, 64, 4
    rng = np.random.default_rng(100 * m + mv)
    blocks = rng.integers(-128, 128, size=(T, m + 1, B), dtype=np.int8)
    blocks[3] = blocks[0]                                                        # the same packet at batch positions 0 and 3
    pk = Packets(torch, blocks)
    worst = 0.0
    for F in (1, 2):
        doa = b.Doa(m + 1, B, 1, D, mx, my, 8, 8, max_batch=T, frames=F, flags=b.DOA_KEEP_RXX)
        doa.set_augment(vx, vy, mask)
        assert doa.augment_buffers()["ra"] and (doa.augment_buffers()["vx"], doa.augment_buffers()["vy"]) == (vx, vy)
        _refused(b, ESTATE, doa.fetch_augmented)                                 # nothing submitted since set_augment
        doa.submit(pk.ptr, pk.stride, pk.offset, T)
        out, ra, vec = doa.fetch(), doa.fetch_augmented(), doa.fetch_subspace()
        nest = T // F
        assert out["rxx"].shape == (nest, m, m) and ra.shape == (nest, mv, mv) and out["sv"].shape == (nest, mv) and vec.shape == (nest, mv, mv)
        for e in range(nest):
            rxx = out["rxx"][e]
            worst = max(worst, model.assert_augmented(ra[e], rxx, mx, my, vx, vy, mask, what=(F, e)))
            assert np.array_equal(ra[e], ra[e].conj().T) and not ra[e].imag.diagonal().any(), (F, e)
            assert not np.signbit(ra[e].imag.diagonal()).any()                   # exactly +0
            # the per-op form on the same rxx, from host pointers: the same bits
            assert _same_bits(b.augment_covariance(rxx, mx, my, vx, vy, mask), ra[e]), (F, e)
            # the chain behind it: the existing subspace on ra
            v1, s1 = b.noisesubspace(ra[e])
            assert _same_bits(s1, out["sv"][e]) and _same_bits(v1, vec[e]), (F, e)
        if F == 1:
            assert _same_bits(ra[0], ra[3]) and _same_bits(out["sv"][0], out["sv"][3]) and _same_bits(vec[0], vec[3])
            # ... and from device pointers
            dev = torch.device("cuda", 0)
            d_rxx = torch.from_numpy(np.ascontiguousarray(out["rxx"][1]).view(np.float32)).to(dev)
            d_ra = torch.zeros(mv * mv * 2, dtype=torch.float32, device=dev)
            torch.cuda.synchronize()
            b.augment_covariance_device(d_ra.data_ptr(), d_rxx.data_ptr(), mx, my, vx, vy, mask)
            assert _same_bits(d_ra.cpu().numpy().view(np.complex64).reshape(mv, mv), ra[1])
        else:
            # two frames stack as before: the covariance of the stacked record, augmented
            stacked = mm.rxx_reference_frames(blocks[0:2])
            s = model.present(mask, m)
            assert np.abs(out["rxx"][0] - stacked)[np.ix_(s, s)].max() <= 2.0 ** -20 * np.abs(stacked).max()
        doa.close()
    print(f"{mx}x{my} -> {vx}x{vy} mask {mask:x}: largest error / bar {worst:.3f}")


def test_absent_receivers_rows_are_ignored(b, torch):
    rng = np.random.default_rng(3)
    T, k = 2, 2
    blocks = np.stack([blk for _, kk, blk in model.scenes() if kk == k][:T])
    gone = [i for i in range(21) if i not in model.present(THIN, 21)]
    garbage = np.array(blocks)
    garbage[:, [1 + i for i in gone]] = rng.integers(-128, 128, size=(T, len(gone), 2 * model.L), dtype=np.int8)
    got = []
    for rows in (0, 127, garbage):
        pk = Packets(torch, rows if isinstance(rows, np.ndarray) else np.stack([model.overwrite_absent(blk, THIN, rows) for blk in blocks]))
        doa = b.Doa(22, 2 * model.L, k, D, 7, 3, max_batch=T, flags=b.DOA_KEEP_SPECTRUM | b.DOA_KEEP_RXX)
        doa.set_augment(7, 3, THIN)
        doa.submit(pk.ptr, pk.stride, pk.offset, T)
        out = doa.fetch()
        got.append(dict(ra=doa.fetch_augmented(), vec=doa.fetch_subspace(), sv=out["sv"], peak=out["peak"], pm=out["pm"], rxx=out["rxx"]))
        doa.close()
    # (a constant row has no covariance once its mean is removed: only the random rows reach the raw matrix, in the absent rows alone)
    assert not _same_bits(got[0]["rxx"], got[2]["rxx"])
    for other in (1, 2):
        for key in ("ra", "sv", "vec", "peak", "pm"):
            assert _same_bits(got[0][key], got[other][key]), (other, key)
    # garbage of another kind: NaN in the absent rows and columns of a matrix, through the per-op call
    r = np.array(got[1]["rxx"][0])
    r[gone, :] = np.nan
    r[:, gone] = np.nan
    assert _same_bits(b.augment_covariance(r, 7, 3, 7, 3, THIN), got[1]["ra"][0])


# ---- 2. downstream -------------------------------------------------------------------------------------------------------------------

def test_subspace_against_numpy_launch_counts_and_switching_off(b, torch, scene_packets):
    k = 2
    pk, _ = scene_packets[(THIN, k)]
    T, flags = pk.T, b.DOA_KEEP_SPECTRUM | b.DOA_KEEP_RXX
    doa = b.Doa(22, pk.B, k, D, 7, 3, 40, 40, max_batch=T, flags=flags)
    never = b.Doa(22, pk.B, k, D, 7, 3, 40, 40, max_batch=T, flags=flags)
    doa.submit(pk.ptr, pk.stride, pk.offset, T)
    assert doa.last_launches() == 5
    doa.set_augment(7, 3, THIN)
    _refused(b, ESTATE, doa.fetch)                                               # the setter discards the last submit
    _refused(b, ESTATE, doa.fetch_subspace)
    for n in (1, T):
        doa.submit(pk.ptr, pk.stride, pk.offset, n)
        assert doa.last_launches() == 6
    ra, vec, sv = doa.fetch_augmented(), doa.fetch_subspace(), doa.fetch()["sv"]
    for e in range(T):
        fr = mm.subspace_fractions(ra[e], vec[e], sv[e], gaps=[k])
        # ra is not positive semidefinite: a singular value is |lambda|, and the residual is taken with the eigenvalue's sign
        R, V = ra[e].astype(np.complex128), vec[e].astype(np.complex128)
        lam = np.sign(np.einsum("ir,ij,jr->r", V.conj(), R, V).real) * sv[e].astype(np.float64)
        fr["resid"] = float(np.abs(R @ V - V * lam[None, :]).max() / (2.0 ** -22 * float(sv[e][0])))
        print(f"estimate {e}: subspace fractions of their bars {fr}")
        assert max(fr.values()) <= 1.0, (e, fr)
    doa.set_peaks(3, 2)
    doa.set_order(b.ORDER_MDL, 1, 9)
    doa.submit(pk.ptr, pk.stride, pk.offset, T)
    assert doa.last_launches() == 9
    doa.set_peaks(0)
    doa.set_order(b.ORDER_OFF)
    doa.set_augment(0)
    _refused(b, ESTATE, doa.fetch)
    _refused(b, ESTATE, doa.fetch_augmented)
    assert doa.augment_buffers() == dict(ra=None, vx=0, vy=0)
    doa.submit(pk.ptr, pk.stride, pk.offset, T)
    never.submit(pk.ptr, pk.stride, pk.offset, T)
    assert doa.last_launches() == never.last_launches() == 5
    a, c = doa.fetch(), never.fetch()
    for key in ("peak", "peak_value", "sv", "status", "pm", "rxx"):
        assert _same_bits(a[key], c[key]), key
    assert _same_bits(doa.fetch_subspace(), never.fetch_subspace())
    doa.close()
    never.close()


# ---- 3. the scenes -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mask,vx,vy", [(THIN, 7, 3), (DEAD, 5, 2)], ids=["12-of-21", "dead-4-16-5x2"])
def test_every_scene_is_resolved(b, torch, scene_packets, mask, vx, vy):
    seen = 0
    for k in (1, 2, 3):
        pk, _ = scene_packets[(mask, k)]
        doa = b.Doa(22, pk.B, k, D, 7, 3, max_batch=pk.T)
        doa.set_augment(vx, vy, mask)
        doa.set_peaks(k, 2)
        doa.submit(pk.ptr, pk.stride, pk.offset, pk.T)
        dirs = doa.fetch_directions()
        for e in range(pk.T):
            ok = dirs["found"][e] == k and smooth_model.all_within(dirs["peaks"][e], model.SOURCES[:k], tol=1.0)
            assert ok, (k, e, dirs["found"][e], dirs["peaks"][e].tolist())
            seen += 1
        doa.close()
    assert seen == 24


# ---- 4. combinations -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mask,vx,vy", [(THIN, 7, 3), (DEAD, 5, 2)], ids=["12-of-21", "dead-4-16-5x2"])
def test_source_count_on_the_virtual_array(b, torch, scene_packets, mask, vx, vy):
    mv, N = vx * vy, model.L
    for k in (1, 2, 3):
        pk, _ = scene_packets[(mask, k)]
        doa = b.Doa(22, pk.B, 1, D, 7, 3, 16, 16, max_batch=pk.T)
        doa.set_augment(vx, vy, mask)
        doa.set_order(b.ORDER_MDL)                                               # kmax = mv - 1
        assert doa.order == (1, mv - 1)
        doa.submit(pk.ptr, pk.stride, pk.offset, pk.T)
        assert doa.last_launches() == 7
        sv, got = doa.fetch()["sv"], doa.fetch_order()
        assert sv.shape == (pk.T, mv) and got["criterion"].shape == (pk.T, mv - 1)
        for e in range(pk.T):
            o = smooth_model.order(sv[e], N, smooth_model.MDL, 1, mv - 1)
            err = np.abs(got["criterion"][e].astype(np.float64) - o["values"])
            assert (err <= smooth_model.criterion_bar(o["values"], sv[e], N, smooth_model.MDL)).all(), (k, e)
            assert o["decided"], (k, e, o["margin"], o["bar"])                   # no scene is left out of the k comparison
            assert got["k"][e] == o["k"], (k, e, got["k"][e], o["k"])
        print(f"{vx}x{vy} sources {k}: MDL counts {got['k'].tolist()}")
        doa.close()


def test_capon_map_and_refinement(b, torch, scene_packets):
    k, nc, levels, loading = 2, 40, 2, 1e-2
    pk, _ = scene_packets[(THIN, k)]
    T = 4
    doa = b.Doa(22, pk.B, k, D, 7, 3, nc, nc, max_batch=T, flags=b.DOA_KEEP_SPECTRUM)
    doa.set_augment(7, 3, THIN)
    doa.set_spectrum(b.SPECTRUM_CAPON, loading)
    doa.set_peaks(k, 2)
    doa.set_refine(levels)
    doa.submit(pk.ptr, pk.stride, pk.offset, T)
    assert doa.last_launches() == 9
    out, vec, dirs, ref = doa.fetch(), doa.fetch_subspace(), doa.fetch_directions(), doa.fetch_refined()
    s_last = 2.0 ** -(2 * levels - 1)
    for e in range(T):
        S, bound = sp.maps(vec[e], out["sv"][e], sp.CAPON, loading, D, 7, 3, nc, nc)
        worst, _ = sp.fractions(out["pm"][e], sp.CAPON, S, bound)
        assert worst <= 1.0, (e, worst)
        assert dirs["found"][e] == k
        one = doa.refine2d(vec[e], out["sv"][e], dirs["peaks"][e], kind=b.SPECTRUM_CAPON, loading=loading, levels=levels)
        for key in ("offsets", "angles", "values"):
            assert _same_bits(one[key], ref[key][e]), (e, key)
        args = (vec[e], out["sv"][e], rm.CAPON, k, loading, D, 7, 3, nc, nc)
        for s in range(k):
            peak, o = dirs["peaks"][e, s], (float(ref["offsets"][e, s, 0]), float(ref["offsets"][e, s, 1]))
            assert o in rm.branches(*args, peak, levels), (e, s, o)
            assert all(v / s_last == round(v / s_last) for v in o)
            q, tol, _ = rm.f_at(*args, float(peak[0]) + o[0], float(peak[1]) + o[1])
            assert abs(rm.q_of(ref["values"][e, s], rm.CAPON, 21) - q) <= tol + 2.0 ** -24 * abs(q), (e, s)
    doa.close()


ES_KEYS = ("phases", "angles", "modulus", "power", "flags")


def test_esprit_beside_the_scan_on_the_thinned_array(b, torch, scene_packets):
    for k in (1, 2, 3):
        pk, _ = scene_packets[(THIN, k)]
        doa = b.Doa(22, pk.B, k, D, 7, 3, 16, 16, max_batch=pk.T)
        doa.set_augment(7, 3, THIN)
        doa.set_esprit(b.ESPRIT_BESIDE)
        doa.submit(pk.ptr, pk.stride, pk.offset, pk.T)
        assert doa.last_launches() == 7
        got, vec, sv = doa.fetch_esprit(), doa.fetch_subspace(), doa.fetch()["sv"]
        want = [(np.pi - a, np.pi - be) for a, be, _ in model.SOURCES[:k]]      # where MUSIC peaks: the mirrored directions
        for e in range(pk.T):
            m_ = em.esprit(vec[e], sv[e], k, D, 7, 3)
            bar = em.BAR if em.well_conditioned(m_) else min(em.BAR * max(1.0, max(m_["cond_gx"], m_["cond_gy"], m_["cond_v"]) / 4.0), 1e-9)
            assert got["found"][e] == m_["found"] == k and got["status"][e] == 0, (k, e)
            err = em.phase_error(got["phases"][e, :k], m_["phases"][:k])
            assert err <= bar, (k, e, err, bar)
            for key in ("angles", "modulus", "power"):
                g, w = got[key][e, :k].astype(np.float64), m_[key][:k]
                assert np.all(np.abs(g - w.astype(np.float64)) <= 4 * np.spacing(np.abs(w)).astype(np.float64)), (k, e, key)
            one = doa.esprit2d(vec[e], sv[e])
            for key in ES_KEYS:
                assert _same_bits(one[key], got[key][e]), (k, e, key)
            assert em.match_error(got["angles"][e], want) <= em.DIRECTION_BAR, (k, e, got["angles"][e])
        doa.close()


def test_subbands_augment_every_band(b, torch):
    mx, my, B, T, nfft, first, nbands = 7, 3, 512, 2, 16, 1, 2
    rng = np.random.default_rng(9)
    pk = Packets(torch, rng.integers(-128, 128, size=(T, 22, B), dtype=np.int8))
    doa = b.Doa(22, B, 1, D, mx, my, 16, 16, max_batch=T, flags=b.DOA_KEEP_RXX)
    doa.set_subbands(nfft, first, nbands, 1)
    doa.set_augment(5, 2, DEAD)
    _refused(b, ESTATE, doa.set_subbands, 0)                                     # ra is sized by the bands
    doa.submit(pk.ptr, pk.stride, pk.offset, T)
    plain = b.Doa(22, B, 1, D, mx, my, 16, 16, max_batch=T)
    plain.set_subbands(nfft, first, nbands, 1)
    plain.submit(pk.ptr, pk.stride, pk.offset, T)
    assert doa.last_launches() == plain.last_launches() + 1
    out, ra, vec = doa.fetch(), doa.fetch_augmented(), doa.fetch_subspace()
    assert out["rxx"].shape == (T * nbands, 21, 21) and ra.shape == (T * nbands, 10, 10) and out["sv"].shape == (T * nbands, 10)
    for i in range(T * nbands):
        model.assert_augmented(ra[i], out["rxx"][i], mx, my, 5, 2, DEAD, what=("band matrix", i))
        assert _same_bits(b.augment_covariance(out["rxx"][i], mx, my, 5, 2, DEAD), ra[i]), i
        v1, s1 = b.noisesubspace(ra[i])
        assert _same_bits(s1, out["sv"][i]) and _same_bits(v1, vec[i]), i
    assert not _same_bits(ra[0], ra[1])                                          # two bands, two matrices
    doa.close()
    plain.close()


# ---- 5. states -----------------------------------------------------------------------------------------------------------------------

def test_state_rules(b, torch):
    rng = np.random.default_rng(4)
    pk = Packets(torch, rng.integers(-128, 128, size=(2, 22, 256), dtype=np.int8))
    doa = b.Doa(22, 256, 3, D, 7, 3, 16, 16, max_batch=2)
    _refused(b, ESTATE, doa.fetch_augmented)                                     # off
    # bad arguments
    for vx, vy, mask in ((8, 3, 0), (7, 4, 0), (1, 1, 0), (-1, 3, 0), (7, 3, 1 << 21), (7, 3, 1 << 7), (3, 1, 0), (1, 3, 0)):      # 3 elements: desc.k = 3 >= mv
        _refused(b, EINVAL, doa.set_augment, vx, vy, mask)
    text = _refused(b, EINVAL, doa.set_augment, 7, 3, model.dead(21, range(7, 21)) & ~0b0011000)      # a sparse first row alone
    assert "lag (ux, uy) = " in text, text
    doa.set_order(b.ORDER_MDL, 1, 9)
    _refused(b, EINVAL, doa.set_augment, 3, 3, 0)                                # the order range ends at 9 = mv
    doa.set_order(b.ORDER_OFF)
    # smoothing, both ways round
    doa.set_smoothing(5, 2, b.SMOOTH_FB)
    assert "crsdr_doa_set_smoothing" in _refused(b, ESTATE, doa.set_augment, 7, 3, 0)
    doa.set_smoothing(7, 3, 0)
    doa.set_augment(7, 3, THIN)
    assert "crsdr_doa_set_augment" in _refused(b, ESTATE, doa.set_smoothing, 5, 2, b.SMOOTH_FB)
    assert "crsdr_doa_set_augment" in _refused(b, ESTATE, doa.set_smoothing, 7, 3, b.SMOOTH_FB)
    # beams, both ways round
    assert "crsdr_doa_set_augment" in _refused(b, ESTATE, doa.set_beams, b.BEAM_MVDR, 1e-2)
    assert "crsdr_doa_set_augment" in _refused(b, ESTATE, doa.set_beams, b.BEAM_CONVENTIONAL, fixed_angles=[(1.0, 1.0)])
    doa.set_augment(0)
    doa.set_beams(b.BEAM_CONVENTIONAL)
    assert "crsdr_doa_set_beams" in _refused(b, ESTATE, doa.set_augment, 7, 3, 0)
    doa.set_beams(b.BEAM_OFF)
    # subbands: refused while augmentation is on; band beams both ways round
    doa.set_augment(7, 3, 0)
    assert "crsdr_doa_set_augment" in _refused(b, ESTATE, doa.set_subbands, 16, 1, 2, 1)
    doa.set_augment(0)
    doa.set_subbands(16, 1, 2, 1)
    doa.set_subband_beams(b.BEAM_CONVENTIONAL)
    assert "_set_subband_beams" in _refused(b, ESTATE, doa.set_augment, 7, 3, 0)
    doa.set_subband_beams(b.BEAM_OFF)
    doa.set_augment(7, 3, 0)
    assert "crsdr_doa_set_augment" in _refused(b, ESTATE, doa.set_subband_beams, b.BEAM_CONVENTIONAL)
    doa.set_augment(0)
    doa.set_subbands(0)
    # fetches between the setter and the next submit
    doa.set_peaks(3, 1)
    doa.submit(pk.ptr, pk.stride, pk.offset, 2)
    doa.fetch(), doa.fetch_directions()
    doa.set_augment(5, 2, DEAD)
    for fn in (doa.fetch, doa.fetch_subspace, doa.fetch_augmented, doa.fetch_directions, doa.last_launches):
        _refused(b, ESTATE, fn)
    doa.submit(pk.ptr, pk.stride, pk.offset, 2)
    assert doa.fetch()["sv"].shape == (2, 10) and doa.fetch_augmented().shape == (2, 10, 10) and doa.fetch_directions()["found"].shape == (2,)
    doa.close()
