"""CPU checks of the boundary of the integration across lines (crsdr_caf_set_integrate, crsdr_caf_integrate_reset,
crsdr_caf_fetch_integrate, crsdr_caf_integrate_device_buffers, crsdr_map_integrate_state_bytes, crsdr_map_integrate; include/crsdr.h (w),
"Integration across lines"): the binding exists, its descriptor has the C layout, every limit of the section and every NULL argument is
refused with CRSDR_EINVAL before any device is touched, and without a device good arguments give CRSDR_ENODEV -- never a CPU result."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

EINVAL, ENODEV, ESTATE = -1, -4, -5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"crsdr_caf_set_integrate", "crsdr_caf_integrate_reset", "crsdr_caf_fetch_integrate", "crsdr_caf_integrate_device_buffers", "crsdr_map_integrate_state_bytes",
         "crsdr_map_integrate"}


@pytest.fixture(scope="module")
def b():
    binding = importlib.import_module("coherent-rtlsdr_amd.binding")
    binding.build()
    return binding


def _call(b, nlines=3, nmaps=2, nd=16, R=5, mem_kind=0, forget=0.25, coupling=0.5, what=0, imap=True, state=True, maps=True, desc=True):
    L, n, d, r = min(max(nlines, 1), 8), min(max(nmaps, 1), 4), min(max(nd, 1), 4096), min(max(R, 1), 1024)
    m, o, s = np.ones(L * n * d * r, dtype=np.float32), np.zeros(L * n * d * r, dtype=np.float32), np.zeros(2 + n * d * r, dtype=np.float64)
    dsc = b.IntegrateDesc(what, 0, forget, coupling)
    return b.lib().crsdr_map_integrate(b._p(o, C.c_float) if imap else None, s.ctypes.data_as(C.c_void_p) if state else None, b._p(m, C.c_float) if maps else None, nlines, nmaps,
                                       nd, R, C.byref(dsc) if desc else None, mem_kind)


def test_binding_names_the_new_symbols(b):
    assert NAMES <= set(b.ABI_SYMBOLS)
    assert all(hasattr(b.lib(), s) for s in NAMES)


def test_the_descriptor_has_the_layout_of_the_header(b, tmp_path):
    fields = [name for name, _ in b.IntegrateDesc._fields_]
    src = tmp_path / "probe.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "crsdr.h"\nint main(void)\n{\n    printf("%zu", sizeof(crsdr_caf_integrate_desc));\n'
                   + "".join(f'    printf(" %zu", offsetof(crsdr_caf_integrate_desc, {f}));\n' for f in fields)
                   + '    printf(" %d %d\\n", CRSDR_INTEGRATE_ARRAY, CRSDR_INTEGRATE_BEAMS);\n    return 0;\n}\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert out[0] == C.sizeof(b.IntegrateDesc) == 24
    assert out[1:-2] == [getattr(b.IntegrateDesc, f).offset for f in fields]
    assert out[-2:] == [b.INTEGRATE_ARRAY, b.INTEGRATE_BEAMS] == [1, 2]


BAD = [dict(forget=0.0), dict(forget=-0.5), dict(forget=1.0000001), dict(forget=2.0), dict(forget=float("nan")), dict(forget=float("inf")),
       dict(coupling=float("nan")), dict(coupling=float("inf")), dict(coupling=float("-inf")), dict(coupling=128.5, nd=16), dict(coupling=-128.5, nd=16),
       dict(coupling=0.5001, nd=4096, R=1, nmaps=1), dict(coupling=257.0, nd=8)]
BAD_CALL = [dict(nlines=0), dict(nlines=4097), dict(nlines=-1), dict(nmaps=0), dict(nmaps=-2), dict(nd=12), dict(nd=4), dict(nd=8192), dict(R=0), dict(R=1025),
            dict(nmaps=17, nd=4096, R=256), dict(mem_kind=2), dict(mem_kind=-1), dict(imap=False), dict(state=False), dict(maps=False), dict(desc=False)]


@pytest.mark.parametrize("over", BAD + BAD_CALL, ids=[str(o) for o in BAD + BAD_CALL])
def test_bad_arguments_are_refused_before_device_use(b, over):
    # CRSDR_EINVAL whether or not a device is present: on a machine without one CRSDR_ENODEV would mean the device was asked first
    assert _call(b, **over) == EINVAL, (over, b.lib().crsdr_last_error())


GOOD = [dict(forget=1.0), dict(forget=2.0 ** -20), dict(forget=5e-324), dict(coupling=0.0), dict(coupling=128.0, nd=16), dict(coupling=-128.0, nd=16),
        dict(coupling=0.5, nd=4096, R=1, nmaps=1), dict(coupling=256.0, nd=8), dict(what=0), dict(what=7), dict(what=-1), dict(nlines=1, nmaps=1, nd=8, R=1)]


@pytest.mark.parametrize("over", GOOD, ids=[str(o) for o in GOOD])
def test_the_limits_themselves_are_accepted(b, over):
    # at a limit, not beyond it (and `what` is not read by the per-op call): a device is then the only thing that can be missing
    assert _call(b, **over) == (0 if b.device_count() > 0 else ENODEV), (over, b.lib().crsdr_last_error())


def test_state_bytes(b):
    for nmaps, nd, R in ((1, 8, 1), (1, 64, 48), (3, 16, 65), (2, 4096, 1024), (64, 4096, 64)):
        assert b.map_integrate_state_bytes(nmaps, nd, R) == 16 + 8 * nmaps * nd * R
    n = C.c_size_t(7)
    for nmaps, nd, R in ((0, 8, 1), (1, 12, 4), (1, 4, 4), (1, 8192, 4), (1, 8, 0), (1, 8, 1025), (5, 4096, 1024), (-1, 8, 8)):
        assert b.lib().crsdr_map_integrate_state_bytes(nmaps, nd, R, C.byref(n)) == EINVAL and n.value == 7, (nmaps, nd, R)
    assert b.lib().crsdr_map_integrate_state_bytes(1, 8, 1, None) == EINVAL


def test_null_arguments(b):
    L = b.lib()
    d = b.integrate_desc(0.25, 0.5)
    assert L.crsdr_caf_set_integrate(None, None) == EINVAL and L.crsdr_caf_set_integrate(None, C.byref(d)) == EINVAL
    assert L.crsdr_caf_integrate_reset(None) == EINVAL
    assert L.crsdr_caf_fetch_integrate(None, None, None) == EINVAL
    assert L.crsdr_caf_integrate_device_buffers(None, None, None, None) == EINVAL


def test_no_cpu_result_without_a_device(b):
    if b.device_count() > 0:
        # a device is here: the engine takes the integration, refuses bad descriptors with EINVAL, and holds the state rules
        s = b.Caf(nrows=4, blocksize=2048, seg=64, nlags=16, max_batch=8)
        for call in (s.fetch_integrate, s.integrate_reset, s.integrate_device_buffers):
            with pytest.raises(b.CrsdrError) as e:
                call()                                                           # no integration set
            assert e.value.code == ESTATE
        for bad in (dict(forget=0.0), dict(forget=1.5), dict(coupling=float("nan")), dict(coupling=129.0), dict(what=0), dict(what=4), dict(what=-1)):
            a = dict(forget=0.25, coupling=0.5, what=1)
            a.update(bad)
            with pytest.raises(b.CrsdrError) as e:
                s.set_integrate(b.integrate_desc(**a))
            assert e.value.code == EINVAL, bad
        with pytest.raises(b.CrsdrError) as e:
            s.set_integrate(b.integrate_desc(0.25, 0.5, what=b.INTEGRATE_BEAMS))  # no beams
        assert e.value.code == ESTATE
        s.set_integrate(b.integrate_desc(0.25, 0.5))
        with pytest.raises(b.CrsdrError) as e:
            s.fetch_integrate()                                                  # nothing submitted since
        assert e.value.code == ESTATE
        bufs = s.integrate_device_buffers()
        assert bufs["imap"] and bufs["state"] and not bufs["ibmap"]
        s.integrate_reset()
        s.set_integrate(None)
        s.close()
        return
    assert _call(b) == ENODEV
