"""CPU checks of the boundary of the adaptive beams (crsdr_caf_set_beam_adapt, crsdr_caf_fetch_beam_adapt,
crsdr_caf_beam_adapt_device_buffers, crsdr_beam_adapt; include/crsdr.h (w), "Adaptive beams"): the binding exists, its descriptor has
the C layout, every limit of the section and every NULL argument is refused with CRSDR_EINVAL before any device is touched, and without a
device good arguments give CRSDR_ENODEV -- never a CPU result.  With a device: the state rules, both ways round."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

EINVAL, ENODEV, ESTATE = -1, -4, -5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"crsdr_caf_set_beam_adapt", "crsdr_caf_fetch_beam_adapt", "crsdr_caf_beam_adapt_device_buffers", "crsdr_beam_adapt"}


@pytest.fixture(scope="module")
def b():
    binding = importlib.import_module("coherent-rtlsdr_amd.binding")
    binding.build()
    return binding


def _call(b, nrows=4, nd=12, R=5, ref_row=1, nbeams=2, mem_kind=0, d_lo=0, d_n=12, r_lo=0, r_n=5, loading=1e-2, flags=0, wbad=None, aw=True, ainfo=True, astat=True,
          chi=True, weights=True, desc=True):
    n, d, r, nb = min(max(nrows, 2), 65), min(max(nd, 1), 4096), min(max(R, 1), 1024), min(max(nbeams, 1), 64)
    x = np.ones(n * d * r * 2, dtype=np.float32)
    w = np.ones(nb * (n - 1) * 2, dtype=np.float32)
    if wbad is not None:
        w[-1] = wbad
    o, i, s = np.zeros(nb * (n - 1) * 2, dtype=np.float32), np.zeros(nb * 2, dtype=np.float32), np.zeros(1, dtype=np.int32)
    dsc = b.BeamAdaptDesc(d_lo, d_n, r_lo, r_n, loading, flags)
    return b.lib().crsdr_beam_adapt(b._p(o, C.c_float) if aw else None, b._p(i, C.c_float) if ainfo else None, b._p(s, C.c_int32) if astat else None,
                                    b._p(x, C.c_float) if chi else None, nrows, nd, R, ref_row, b._p(w, C.c_float) if weights else None, nbeams,
                                    C.byref(dsc) if desc else None, mem_kind)


def test_binding_names_the_new_symbols(b):
    assert NAMES <= set(b.ABI_SYMBOLS)
    assert all(hasattr(b.lib(), s) for s in NAMES)


def test_the_descriptor_has_the_layout_of_the_header(b, tmp_path):
    fields = [name for name, _ in b.BeamAdaptDesc._fields_]
    assert fields == ["d_lo", "d_n", "r_lo", "r_n", "loading", "flags"]
    src = tmp_path / "probe.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "crsdr.h"\nint main(void)\n{\n    printf("%zu", sizeof(crsdr_caf_beam_adapt_desc));\n'
                   + "".join(f'    printf(" %zu", offsetof(crsdr_caf_beam_adapt_desc, {f}));\n' for f in fields) + '    printf("\\n");\n    return 0;\n}\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert out[0] == C.sizeof(b.BeamAdaptDesc) == 24
    assert out[1:] == [getattr(b.BeamAdaptDesc, f).offset for f in fields]


BAD = [dict(d_lo=-1), dict(d_lo=12), dict(d_n=0), dict(d_n=13), dict(d_n=-3), dict(r_lo=-1), dict(r_n=0), dict(r_n=-1), dict(r_lo=1, r_n=5), dict(r_lo=5, r_n=1),
       dict(r_lo=2 ** 31 - 1, r_n=2 ** 31 - 1), dict(loading=0.0), dict(loading=9e-7), dict(loading=1.0000001), dict(loading=-0.5), dict(loading=float("nan")),
       dict(loading=float("inf")), dict(flags=1), dict(flags=0x80000000)]
BAD_CALL = [dict(nd=0), dict(nd=4097), dict(R=0), dict(R=1025), dict(nrows=1), dict(nrows=66), dict(ref_row=-1), dict(ref_row=4), dict(nbeams=0), dict(nbeams=65),
            dict(wbad=float("nan")), dict(wbad=float("inf")), dict(mem_kind=2), dict(mem_kind=-1), dict(aw=False, ainfo=False, astat=False), dict(chi=False),
            dict(weights=False), dict(desc=False)]


@pytest.mark.parametrize("over", BAD + BAD_CALL, ids=[str(o) for o in BAD + BAD_CALL])
def test_bad_arguments_are_refused_before_device_use(b, over):
    # CRSDR_EINVAL whether or not a device is present: on a machine without one CRSDR_ENODEV would mean the device was asked first
    assert _call(b, **over) == EINVAL, (over, b.lib().crsdr_last_error())


GOOD = [dict(), dict(d_lo=11, d_n=12), dict(d_n=1), dict(r_lo=4, r_n=1), dict(loading=1e-6), dict(loading=1.0), dict(nd=1, d_n=1), dict(nd=4096, R=1, d_n=4096, r_n=1),
        dict(nrows=65, ref_row=64, nbeams=64), dict(aw=False, ainfo=False), dict(astat=False)]


@pytest.mark.parametrize("over", GOOD, ids=[str(o) for o in GOOD])
def test_the_limits_themselves_are_accepted(b, over):
    # at a limit, not beyond it (nd need not be a power of two): a device is then the only thing that can be missing
    assert _call(b, **over) == (0 if b.device_count() > 0 else ENODEV), (over, b.lib().crsdr_last_error())


def test_null_arguments(b):
    L = b.lib()
    d = b.beam_adapt_desc(1e-2, 0, 8, 0, 4)
    assert L.crsdr_caf_set_beam_adapt(None, None) == EINVAL and L.crsdr_caf_set_beam_adapt(None, C.byref(d)) == EINVAL
    assert L.crsdr_caf_fetch_beam_adapt(None, None, None, None) == EINVAL
    assert L.crsdr_caf_beam_adapt_device_buffers(None, None, None, None) == EINVAL


def test_no_cpu_result_without_a_device(b):
    if b.device_count() > 0:
        # a device is here: the engine refuses bad descriptors with EINVAL and holds the state rules, both ways round
        s = b.Caf(nrows=4, blocksize=2048, seg=64, nlags=16, max_batch=8)
        good = b.beam_adapt_desc(1e-2, 0, s.nd, 0, 16)
        W = np.ones((3, 3), dtype=np.complex64)
        for call in (s.fetch_beam_adapt, s.beam_adapt_device_buffers):
            with pytest.raises(b.CrsdrError) as e:
                call()                                                           # no adaptation set
            assert e.value.code == ESTATE
        with pytest.raises(b.CrsdrError) as e:
            s.set_beam_adapt(good)                                               # no beams set
        assert e.value.code == ESTATE
        s.set_beam_adapt(None)                                                   # (off while off: fine)
        with pytest.raises(b.CrsdrError) as e:
            s.set_beam_adapt(b.beam_adapt_desc(2.0, 0, s.nd, 0, 16))            # the limits come before the state
        assert e.value.code == EINVAL
        s.set_beams(W)
        for bad in (dict(d_lo=s.nd), dict(d_n=s.nd + 1), dict(r_lo=1, r_n=16), dict(loading=0.0), dict(flags=2)):
            a = dict(loading=1e-2, d_lo=0, d_n=s.nd, r_lo=0, r_n=16, flags=0)
            a.update(bad)
            with pytest.raises(b.CrsdrError) as e:
                s.set_beam_adapt(b.beam_adapt_desc(**a))
            assert e.value.code == EINVAL, bad
        s.set_beam_adapt(good)
        with pytest.raises(b.CrsdrError) as e:
            s.fetch_beam_adapt()                                                 # nothing submitted since
        assert e.value.code == ESTATE
        assert all(s.beam_adapt_device_buffers().values())
        # the order is beams, adapt, integrate, track: with the integration on the adaptation stays as it is, set or turned off
        s.set_integrate(b.integrate_desc(0.5, 0.0, what=b.INTEGRATE_BEAMS))
        for desc in (good, None):
            with pytest.raises(b.CrsdrError) as e:
                s.set_beam_adapt(desc)
            assert e.value.code == ESTATE
        with pytest.raises(b.CrsdrError) as e:
            s.set_beams(None)                                                    # (and so do the beams)
        assert e.value.code == ESTATE
        assert all(s.beam_adapt_device_buffers().values())
        s.set_integrate(None)
        s.set_beams(W)                                                           # every set_beams turns the adaptation off
        with pytest.raises(b.CrsdrError) as e:
            s.beam_adapt_device_buffers()
        assert e.value.code == ESTATE
        s.set_beam_adapt(good)
        s.set_beams(None)                                                        # off as well
        with pytest.raises(b.CrsdrError) as e:
            s.beam_adapt_device_buffers()
        assert e.value.code == ESTATE
        # the tracker likewise
        s.set_cfar(b.cfar_desc(8.0, max_det=4))
        s.set_beams(W)
        s.set_track(b.track_desc(4, source=b.TRACK_SRC_FUSED))
        for desc in (good, None):
            with pytest.raises(b.CrsdrError) as e:
                s.set_beam_adapt(desc)
            assert e.value.code == ESTATE
        s.set_track(None)
        s.set_beam_adapt(good)
        s.set_track(b.track_desc(4, source=b.TRACK_SRC_FUSED))                   # the tracker behind the adaptation: fine
        s.close()
        return
    assert _call(b) == ENODEV
