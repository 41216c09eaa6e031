"""CPU checks of the beams' boundary (crsdr_caf_set_beams, crsdr_caf_fetch_beams, crsdr_caf_beams_device_buffers, crsdr_beam_maps,
crsdr_beam_fuse, crsdr_caf_beam_steer; include/crsdr.h (w), "Beams"): the binding exists, every limit of the section and every NULL
argument is refused with CRSDR_EINVAL before any device is touched, and without a device good arguments give CRSDR_ENODEV -- never a CPU
result.  crsdr_caf_beam_steer is the host's own and is held against the model.  With a device the state rules are held as well."""
import ctypes as C
import importlib

import numpy as np
import pytest

import caf_beams_model as B
import caf_bearing_model as BM

EINVAL, ENODEV, ESTATE = -1, -4, -5


@pytest.fixture(scope="module")
def b():
    binding = importlib.import_module("coherent-rtlsdr_amd.binding")
    binding.build()
    return binding


def _maps(b, nrows=7, nd=16, R=8, ref_row=0, nbeams=4, mem_kind=0, bmap=True, chi=True, weights=True, poison=None):
    m, nb = max(nrows - 1, 1), min(max(nbeams, 1), 64)
    w = np.full(nb * m * 2, 0.25, dtype=np.float32)
    if poison is not None:
        w[poison[0]] = poison[1]
    a = np.zeros(max(nrows, 1) * max(nd, 1) * max(R, 1) * 2, dtype=np.float32)
    out = np.zeros(nb * max(nd, 1) * max(R, 1), dtype=np.float32)
    return b.lib().crsdr_beam_maps(b._p(out, C.c_float) if bmap else None, b._p(a, C.c_float) if chi else None, nrows, nd, R, ref_row,
                                   b._p(w, C.c_float) if weights else None, nbeams, mem_kind)


def _fuse(b, nbeams=4, K=4, nd=16, R=8, mem_kind=0, fused=True, nfused=True, bdet=True, bcount=True):
    nb, k = min(max(nbeams, 1), 64), min(max(K, 1), 64)
    t, n = np.zeros(nb * k * 8, dtype=np.float32), np.zeros(nb, dtype=np.int32)
    f, nf = np.zeros(k * 8, dtype=np.float32), np.zeros(1, dtype=np.int32)
    return b.lib().crsdr_beam_fuse(b._p(f, C.c_float) if fused else None, b._p(nf, C.c_int32) if nfused else None, b._p(t, C.c_float) if bdet else None,
                                   b._p(n, C.c_int32) if bcount else None, nbeams, K, nd, R, mem_kind)


def test_binding_names_the_new_symbols(b):
    names = {"crsdr_caf_set_beams", "crsdr_caf_fetch_beams", "crsdr_caf_beams_device_buffers", "crsdr_beam_maps", "crsdr_beam_fuse", "crsdr_caf_beam_steer"}
    assert names <= set(b.ABI_SYMBOLS)
    assert all(hasattr(b.lib(), s) for s in names)
    assert C.sizeof(b.BeamsDesc) == 24 and b.BeamsDesc.weights.offset == 8 and b.BeamsDesc.flags.offset == 16


BAD_MAPS = [dict(nrows=1), dict(nrows=66), dict(nrows=0), dict(nbeams=0), dict(nbeams=65), dict(nbeams=-1), dict(weights=False),
            dict(poison=(0, float("nan"))), dict(poison=(5, float("inf"))), dict(poison=(47, float("-inf"))),
            dict(nbeams=64, nd=4096, R=128),                                     # nbeams nd R = 2^25
            dict(nd=0), dict(nd=8192), dict(R=0), dict(R=1025), dict(ref_row=-1), dict(ref_row=7), dict(mem_kind=2), dict(mem_kind=-1), dict(bmap=False), dict(chi=False)]


@pytest.mark.parametrize("over", BAD_MAPS, ids=[str(o) for o in BAD_MAPS])
def test_bad_map_arguments_are_refused_before_device_use(b, over):
    # CRSDR_EINVAL whether or not a device is present: on a machine without one CRSDR_ENODEV would mean the device was asked first
    assert _maps(b, **over) == EINVAL, (over, b.lib().crsdr_last_error())


@pytest.mark.parametrize("over", [dict(nrows=2), dict(nrows=65, nd=8, R=4), dict(nbeams=1), dict(nbeams=64), dict(nbeams=64, nd=4096, R=64, nrows=2), dict(nd=31, R=1),
                                  dict(ref_row=6), dict(poison=(3, 3e38)), dict(poison=(3, -1e-45))])
def test_the_map_limits_themselves_are_accepted(b, over):
    # at a limit, not beyond it: a device is then the only thing that can be missing
    assert _maps(b, **over) == (0 if b.device_count() > 0 else ENODEV), (over, b.lib().crsdr_last_error())


@pytest.mark.parametrize("over", [dict(nbeams=0), dict(nbeams=65), dict(K=0), dict(K=65), dict(nd=12), dict(nd=4), dict(nd=8192), dict(R=0), dict(R=1025), dict(mem_kind=2),
                                  dict(fused=False, nfused=False), dict(bdet=False), dict(bcount=False)])
def test_bad_fuse_arguments_are_refused_before_device_use(b, over):
    assert _fuse(b, **over) == EINVAL, (over, b.lib().crsdr_last_error())


@pytest.mark.parametrize("over", [dict(nbeams=1, K=1), dict(nbeams=64, K=64), dict(nd=8, R=1), dict(nd=4096, R=1024), dict(fused=False), dict(nfused=False)])
def test_the_fuse_limits_themselves_are_accepted(b, over):
    assert _fuse(b, **over) == (0 if b.device_count() > 0 else ENODEV), (over, b.lib().crsdr_last_error())


def test_null_arguments(b):
    L = b.lib()
    assert L.crsdr_caf_set_beams(None, None) == EINVAL
    assert L.crsdr_caf_set_beams(None, C.byref(b.beams_desc(np.ones((2, 6), dtype=np.complex64)))) == EINVAL
    assert L.crsdr_caf_fetch_beams(None, None, None, None, None, None) == EINVAL
    assert L.crsdr_caf_beams_device_buffers(None, None, None, None, None, None) == EINVAL


@pytest.mark.parametrize("mx, my, d, nc, xy", [(7, 3, float(BM.SCENES[1][2]), 100, B.lattice(8, 8, 100)), (1, 1, 0.5, 2, [[0.0, 2.0]]), (3, 2, 0.5, 16, [[5.0, 9.0], [0.0, 0.0]]),
                                               (8, 8, 0.5, 512, [[0.0, 0.0], [511.5, 17.25], [256.0, 256.0]]), (64, 1, 1e-3, 32, [[3.0, 16.0]]), (1, 64, 3.0, 32, [[3.0, 7.5]])])
def test_the_steering_helper_against_the_model(b, mx, my, d, nc, xy):
    q = BM.Desc(mx, my, d, nc, nc)
    got = b.beam_steer(mx, my, d, xy, nc, nc).astype(np.complex128)
    dw = got - B.steer_weights(q, xy).astype(np.complex128)
    assert np.all(np.abs(dw.real) <= B.steer_bar(q)[None]) and np.all(np.abs(dw.imag) <= B.steer_bar(q)[None]), float(np.max(np.abs(dw)))
    assert np.allclose((np.abs(got) ** 2).sum(1), 1.0, atol=1e-6) and np.all(got[:, 0] == np.complex64(1.0 / np.sqrt(np.float64(q.m))))


@pytest.mark.parametrize("over", [dict(mx=0), dict(my=0), dict(mx=13, my=5), dict(mx=2 ** 16, my=2 ** 16), dict(d=0.0), dict(d=float("nan")), dict(d=float("inf")), dict(ncx=1),
                                  dict(ncy=513), dict(xy=[[float("nan"), 1.0]]), dict(xy=[[1.0, float("inf")]]), dict(n=0), dict(n=65)])
def test_the_steering_helper_refuses(b, over):
    a = dict(mx=3, my=2, d=0.5, ncx=16, ncy=16, xy=[[5.0, 9.0]], n=None)
    a.update(over)
    pts = np.ascontiguousarray(a["xy"], dtype=np.float64)
    n = len(pts) if a["n"] is None else a["n"]
    pts = np.resize(pts, (max(n, 1), 2))
    w = np.zeros(max(n, 1) * 64 * 2, dtype=np.float32)
    assert b.lib().crsdr_caf_beam_steer(b._p(w, C.c_float), a["mx"], a["my"], a["d"], a["ncx"], a["ncy"], pts.ctypes.data_as(C.POINTER(C.c_double)), n) == EINVAL
    assert b.lib().crsdr_caf_beam_steer(None, 3, 2, 0.5, 16, 16, pts.ctypes.data_as(C.POINTER(C.c_double)), 1) == EINVAL
    assert b.lib().crsdr_caf_beam_steer(b._p(w, C.c_float), 3, 2, 0.5, 16, 16, None, 1) == EINVAL


def test_no_cpu_result_without_a_device(b):
    if b.device_count() > 0:
        # a device is here: the engine takes the beams, refuses bad ones with its own nrows and lines, and holds the state rules
        s = b.Caf(nrows=7, blocksize=2048, seg=64, nlags=16, max_batch=8)        # nd = 16, eight lines of 256 cells
        W = np.full((4, 6), 0.25, dtype=np.complex64)
        for bad in (np.zeros((65, 6), dtype=np.complex64), np.full((2, 6), np.nan, dtype=np.complex64), np.full((2, 6), -np.inf, dtype=np.complex64)):
            with pytest.raises(b.CrsdrError) as e:
                s.set_beams(bad)
            assert e.value.code == EINVAL
        with pytest.raises(b.CrsdrError) as e:
            s.set_beams(W, flags=2)
        assert e.value.code == EINVAL
        assert b.lib().crsdr_caf_set_beams(s._h, C.byref(b.BeamsDesc(4, None, 0))) == EINVAL
        with pytest.raises(b.CrsdrError) as e:
            s.fetch_beams()                                                      # no beams set
        assert e.value.code == ESTATE
        s.set_beams(W)                                                           # the detector is off: maps alone
        with pytest.raises(b.CrsdrError) as e:
            s.fetch_beams()                                                      # nothing submitted since
        assert e.value.code == ESTATE
        with pytest.raises(b.CrsdrError) as e:
            s.set_cfar(b.cfar_desc(8.0))                                         # beams on: the detector stays as it is
        assert e.value.code == ESTATE
        bufs = s.beams_device_buffers()
        assert bufs["bmap"] and not bufs["fused"] and not bufs["bdet"]
        s.set_beams(None)
        s.set_cfar(b.cfar_desc(8.0))
        s.set_beams(W)
        assert all(s.beams_device_buffers().values())
        s.set_beams(None)
        with pytest.raises(b.CrsdrError) as e:
            s.beams_device_buffers()
        assert e.value.code == ESTATE
        s.close()
        big = b.Caf(nrows=2, blocksize=16384, seg=64, nlags=64, max_batch=64)    # nd = 128, R = 64: 64 lines of 2^13 cells
        with pytest.raises(b.CrsdrError) as e:
            big.set_beams(np.ones((64, 1), dtype=np.complex64))                  # 64 lines * 64 beams * 2^13 = 2^25
        assert e.value.code == EINVAL
        big.set_beams(np.ones((32, 1), dtype=np.complex64))                      # 2^24: the limit itself
        big.close()
        return
    assert _maps(b) == ENODEV and _fuse(b) == ENODEV
