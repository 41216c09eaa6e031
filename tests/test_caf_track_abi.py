"""CPU checks of the tracker's boundary (crsdr_caf_set_track, crsdr_caf_track_reset, crsdr_caf_fetch_track,
crsdr_caf_track_device_buffers, crsdr_track_state_bytes, crsdr_track; include/crsdr.h (w), "Tracks"): the binding exists, its
descriptor has the C layout, every limit of the section and every NULL argument is refused with CRSDR_EINVAL before any device is
touched, and without a device good arguments give CRSDR_ENODEV -- never a CPU result.  With a device the state rules are held as well."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

EINVAL, ENODEV, ESTATE = -1, -4, -5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"crsdr_caf_set_track", "crsdr_caf_track_reset", "crsdr_caf_fetch_track", "crsdr_caf_track_device_buffers", "crsdr_track_state_bytes", "crsdr_track"}


@pytest.fixture(scope="module")
def b():
    binding = importlib.import_module("coherent-rtlsdr_amd.binding")
    binding.build()
    return binding


def _desc(b, **over):
    a = dict(max_tracks=8, m=3, n=5, gate=9.0, sigma_r=0.5, sigma_f=0.5, p0_g=1.0, q_r=1e-3, q_f=1e-3, q_g=1e-4, coupling=0.1, tent_miss=2, conf_miss=4, source=0)
    a.update({k: v for k, v in over.items() if k in a})
    return b.track_desc(**a)


def _track(b, nlines=3, K=4, nd=16, R=16, mem_kind=0, trk=True, ntrk=True, state=True, det=True, count=True, aux=True, desc=True, **over):
    d = _desc(b, **over)
    T, L, k = min(max(d.max_tracks, 1), 128), min(max(nlines, 1), 4096), min(max(K, 1), 64)
    t, n, s = np.zeros(L * T * 16, dtype=np.float32), np.zeros(L * 4, dtype=np.int32), np.zeros(2 + 16 * T, dtype=np.float64)
    dd, c, a = np.zeros(L * k * 8, dtype=np.float32), np.zeros(L, dtype=np.int32), np.zeros(L * k * 2, dtype=np.float32)
    return b.lib().crsdr_track(b._p(t, C.c_float) if trk else None, b._p(n, C.c_int32) if ntrk else None, s.ctypes.data_as(C.c_void_p) if state else None,
                               b._p(dd, C.c_float) if det else None, b._p(c, C.c_int32) if count else None, b._p(a, C.c_float) if aux else None, nlines, K, nd, R,
                               C.byref(d) if desc else None, mem_kind)


def test_binding_names_the_new_symbols(b):
    assert NAMES <= set(b.ABI_SYMBOLS)
    assert all(hasattr(b.lib(), s) for s in NAMES)


def test_the_descriptor_has_the_layout_of_the_header(b, tmp_path):
    fields = [name for name, _ in b.TrackDesc._fields_]
    src = tmp_path / "probe.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "crsdr.h"\nint main(void)\n{\n    printf("%zu", sizeof(crsdr_caf_track_desc));\n'
                   + "".join(f'    printf(" %zu", offsetof(crsdr_caf_track_desc, {f}));\n' for f in fields)
                   + '    printf(" %d %d\\n", CRSDR_TRACK_SRC_ARRAY, CRSDR_TRACK_SRC_FUSED);\n    return 0;\n}\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert out[0] == C.sizeof(b.TrackDesc) == 88
    assert out[1:-2] == [getattr(b.TrackDesc, f).offset for f in fields]
    assert out[-2:] == [b.TRACK_SRC_ARRAY, b.TRACK_SRC_FUSED]


BAD = [dict(max_tracks=0), dict(max_tracks=129), dict(max_tracks=-1), dict(source=2), dict(source=-1),
       dict(sigma_r=0.0), dict(sigma_r=-1.0), dict(sigma_r=float("nan")), dict(sigma_r=float("inf")), dict(sigma_f=0.0), dict(sigma_f=float("nan")), dict(sigma_f=float("inf")),
       dict(gate=0.0), dict(gate=float("nan")), dict(gate=float("inf")), dict(p0_g=0.0), dict(p0_g=float("inf")), dict(p0_g=float("nan")),
       dict(q_r=-1e-9), dict(q_r=float("nan")), dict(q_f=-1.0), dict(q_f=float("inf")), dict(q_g=-1.0), dict(q_g=float("nan")),
       dict(coupling=float("nan")), dict(coupling=float("inf")), dict(coupling=float("-inf")),
       dict(m=0), dict(m=6, n=5), dict(n=33, m=33), dict(n=33), dict(tent_miss=0), dict(conf_miss=0), dict(conf_miss=-3)]
BAD_CALL = [dict(nlines=0), dict(nlines=4097), dict(K=0), dict(K=65), dict(nd=12), dict(nd=4), dict(nd=8192), dict(R=0), dict(R=1025), dict(mem_kind=2), dict(mem_kind=-1),
            dict(trk=False, ntrk=False), dict(state=False), dict(det=False), dict(count=False), dict(desc=False)]


@pytest.mark.parametrize("over", BAD + BAD_CALL, ids=[str(o) for o in BAD + BAD_CALL])
def test_bad_arguments_are_refused_before_device_use(b, over):
    # CRSDR_EINVAL whether or not a device is present: on a machine without one CRSDR_ENODEV would mean the device was asked first
    assert _track(b, **over) == EINVAL, (over, b.lib().crsdr_last_error())


GOOD = [dict(max_tracks=1), dict(max_tracks=128, K=64), dict(source=1), dict(q_r=0.0, q_f=0.0, q_g=0.0), dict(coupling=0.0), dict(coupling=-2.5), dict(m=1, n=1),
        dict(m=32, n=32), dict(m=1, n=32), dict(tent_miss=1, conf_miss=1), dict(nlines=1, K=1), dict(nd=8, R=1), dict(nd=4096, R=1024), dict(trk=False), dict(ntrk=False),
        dict(aux=False), dict(sigma_r=1e-300, gate=1e300)]


@pytest.mark.parametrize("over", GOOD, ids=[str(o) for o in GOOD])
def test_the_limits_themselves_are_accepted(b, over):
    # at a limit, not beyond it: a device is then the only thing that can be missing
    assert _track(b, **over) == (0 if b.device_count() > 0 else ENODEV), (over, b.lib().crsdr_last_error())


def test_state_bytes(b):
    for T in (1, 2, 63, 64, 65, 128):
        assert b.track_state_bytes(_desc(b, max_tracks=T)) == 16 + 128 * T
    n = C.c_size_t(7)
    for over in BAD:
        assert b.lib().crsdr_track_state_bytes(C.byref(_desc(b, **over)), C.byref(n)) == EINVAL and n.value == 7, over
    assert b.lib().crsdr_track_state_bytes(None, C.byref(n)) == EINVAL and b.lib().crsdr_track_state_bytes(C.byref(_desc(b)), None) == EINVAL


def test_null_arguments(b):
    L = b.lib()
    assert L.crsdr_caf_set_track(None, None) == EINVAL and L.crsdr_caf_set_track(None, C.byref(_desc(b))) == EINVAL
    assert L.crsdr_caf_track_reset(None) == EINVAL
    assert L.crsdr_caf_fetch_track(None, None, None) == EINVAL
    assert L.crsdr_caf_track_device_buffers(None, None, None) == EINVAL


def test_no_cpu_result_without_a_device(b):
    if b.device_count() > 0:
        # a device is here: the engine takes the tracker, refuses bad ones, and holds the state rules
        s = b.Caf(nrows=4, blocksize=2048, seg=64, nlags=16, max_batch=8)
        for call in (s.fetch_track, s.track_reset, s.track_device_buffers):
            with pytest.raises(b.CrsdrError) as e:
                call()                                                           # no tracker set
            assert e.value.code == ESTATE
        with pytest.raises(b.CrsdrError) as e:
            s.set_track(_desc(b))                                                # no detector
        assert e.value.code == ESTATE
        with pytest.raises(b.CrsdrError) as e:
            s.set_track(_desc(b, max_tracks=129))                                # the limits come first
        assert e.value.code == EINVAL
        s.set_cfar(b.cfar_desc(8.0, max_det=4))
        with pytest.raises(b.CrsdrError) as e:
            s.set_track(_desc(b, source=b.TRACK_SRC_FUSED))                      # no beams
        assert e.value.code == ESTATE
        s.set_track(_desc(b))
        with pytest.raises(b.CrsdrError) as e:
            s.fetch_track()                                                      # nothing submitted since
        assert e.value.code == ESTATE
        assert all(s.track_device_buffers().values())
        s.track_reset()
        for call in (lambda: s.set_cfar(b.cfar_desc(8.0)), lambda: s.set_cfar(None), lambda: s.set_beams(np.ones((2, 3), dtype=np.complex64)),
                     lambda: s.set_bearing(b.bearing_desc(3, 1, 0.5, 8, 8)), lambda: s.set_bearing(None)):
            with pytest.raises(b.CrsdrError) as e:
                call()                                                           # the tracker is on: turn it off first
            assert e.value.code == ESTATE
        s.set_track(None)
        s.set_beams(np.ones((2, 3), dtype=np.complex64))
        s.set_track(_desc(b, source=b.TRACK_SRC_FUSED))
        s.set_track(None)
        s.set_beams(None)
        s.set_cfar(None)
        s.close()
        return
    assert _track(b) == ENODEV
