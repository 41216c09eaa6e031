"""The state machine of crsdr_caf's setters, replayed against a recorded trace (tests/golden/caf_states.json).

Who must be on before whom, who must be off before whom, what a setter discards, which fetch answers CRSDR_ESTATE and when: for every
ordered pair (A, B) of the features below a fresh object goes through  A's prerequisites, set A, submit, B's prerequisites not yet on,
set B, probe, submit, probe, A off, probe, B off, probe, the prerequisites off in reverse order, probe.  A probe calls every fetch*,
every *_device_buffers, track_reset and last_submit and records the return code, the message after a failure, which buffer pointers
are non-NULL, nest and launches; every set and submit call's code and message are recorded too: a refusal is data, and the sequence
goes on behind it.  No kernel result is compared: the device is needed because crsdr_caf_create needs one.

The object is the smallest at which every rule can fire: nrows = 4 (the three other rows a 3 x 1 array for the bearings), blocksize
256, seg 16 (nd = 8), nlags 4, max_batch 2, frames 1; a detector of one training cell each way that keeps 4; bearings on an 8 x 8 grid
with the spectrum kept; 2 beams of unit weights; a canceller of 2 taps; a tracker of 4 slots.

The trace is a fixture, recorded from the library before the engine's host code was folded into stages and frames:
    CRSDR_LIB=<that build's libcrsdr.so> python tests/test_gpu_caf_states.py [out.json]
writes it (this module produces the trace and compares it); the test requires equality, entry by entry.  The fixture has the form of
doa_states.json (test_gpu_doa_states.unpack reads it)."""
import ctypes as C
import importlib
import json
import os
import sys

import numpy as np
import pytest

from test_gpu_doa_states import unpack

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "caf_states.json")
NROWS, B, SEG, NLAGS, T = 4, 256, 16, 4, 2
OFFSET = 16 + 4 * NROWS
STRIDE = OFFSET + NROWS * B
WEIGHTS = np.ones((2, NROWS - 1, 2), dtype=np.float32)
F32, I32, VP = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.c_void_p


def _track(b, source):
    return lambda: b.TrackDesc(4, source, 0.5, 0.5, 9.0, 1.0, 1e-3, 1e-3, 1e-4, 0.0, 1, 1, 2, 4)


def setters(b):
    """setter -> (function name, its descriptor when on); a feature below names its setter and the setters that go before it"""
    return {
        "cancel": ("crsdr_caf_set_cancel", lambda: b.CancelDesc(2, 0)),
        "cfar": ("crsdr_caf_set_cfar", lambda: b.CfarDesc(0, 0, 1, 1, 1.0, 1, 4)),
        "bearing": ("crsdr_caf_set_bearing", lambda: b.BearingDesc(3, 1, 8, 8, 0.5, b.BEARING_CONVENTIONAL, 1e-2, 0, b.BEARING_KEEP_SPECTRUM)),
        "beams": ("crsdr_caf_set_beams", lambda: b.BeamsDesc(2, WEIGHTS.ctypes.data_as(F32), 0)),
        "track_array": ("crsdr_caf_set_track", _track(b, b.TRACK_SRC_ARRAY)),
        "track_fused": ("crsdr_caf_set_track", _track(b, b.TRACK_SRC_FUSED)),
    }


# name -> (setter, the setters that go before it, in order)
FEATURES = {
    "cancel": ("cancel", ()),
    "cfar": ("cfar", ()),
    "bearing": ("bearing", ("cfar",)),
    "beams": ("beams", ()),
    "beams_det": ("beams", ("cfar",)),
    "track": ("track_array", ("cfar",)),
    "track_dir": ("track_array", ("cfar", "bearing")),
    "track_fused": ("track_fused", ("cfar", "beams")),
}
PAIRS = [(a, c) for a in FEATURES for c in FEATURES]
PROBE = 14      # entries of a probe


class Rig:
    """The library, the packets on the device and host buffers large enough for every fetch in every state."""

    def __init__(self):
        import torch
        self.b = importlib.import_module("coherent-rtlsdr_amd.binding")
        if self.b.device_count() < 1:
            pytest.fail("no HIP device: the product path has no CPU fallback")
        self.L = self.b.lib()
        self.set = setters(self.b)
        rng = np.random.default_rng(20240917)
        host = np.full((T, STRIDE), 0x55, dtype=np.int8)
        host[:, OFFSET:] = rng.integers(-128, 128, size=(T, NROWS * B), dtype=np.int8)
        self.packets = torch.from_numpy(host).to(torch.device("cuda", 0))
        self.f = [np.zeros(1 << 12, dtype=np.float32) for _ in range(3)]      # (the largest fetch: 2 x 4 x 32 complex chi, 2 x 4 x 64 spectra)
        self.i = [np.zeros(1 << 8, dtype=np.int32) for _ in range(2)]

    def fp(self, j):
        return self.f[j].ctypes.data_as(F32)

    def ip(self, j):
        return self.i[j].ctypes.data_as(I32)

    def call(self, name, *args):
        """[name without its crsdr_caf_ prefix, return code, the message if the call failed]"""
        rc = getattr(self.L, name)(*args)
        return [name[len("crsdr_caf_"):], rc, self.L.crsdr_last_error().decode() if rc else ""]

    def probe(self, h):
        out = []
        out.append(self.call("crsdr_caf_fetch", h, self.fp(0), self.fp(1), self.fp(2)))
        out.append(self.call("crsdr_caf_fetch_cfar", h, self.fp(0), self.ip(0), self.fp(1)))
        out.append(self.call("crsdr_caf_fetch_cancel", h, self.fp(0), self.fp(1)))
        out.append(self.call("crsdr_caf_fetch_bearing", h, self.fp(0), self.fp(1)))
        out.append(self.call("crsdr_caf_fetch_beams", h, self.fp(0), self.fp(1), self.ip(0), self.fp(2), self.ip(1)))
        out.append(self.call("crsdr_caf_fetch_track", h, self.fp(0), self.ip(0)))
        for name, n in (("crsdr_caf_device_buffers", 3), ("crsdr_caf_cfar_device_buffers", 3), ("crsdr_caf_cancel_device_buffers", 2),
                        ("crsdr_caf_bearing_device_buffers", 2), ("crsdr_caf_beams_device_buffers", 5), ("crsdr_caf_track_device_buffers", 2)):
            ptrs = [VP() for _ in range(n)]
            out.append(self.call(name, h, *[C.byref(p) for p in ptrs]) + [[p.value is not None for p in ptrs]])
        out.append(self.call("crsdr_caf_track_reset", h))
        nest, launches = C.c_int(-1), C.c_int(-1)
        out.append(self.call("crsdr_caf_last_submit", h, C.byref(nest), C.byref(launches)) + [nest.value, launches.value])
        assert len(out) == PROBE
        return out

    def sequence(self, a, c):
        """the trace of the pair: entries, and each probe as one list of its entries"""
        desc = self.b.CafDesc(NROWS, B, 0, T, 1, SEG, NLAGS, 0, 0, 0)
        h = VP()
        trace = [self.call("crsdr_caf_create", C.byref(h), C.byref(desc))]
        assert trace[0][1] == 0, trace

        def on(which):
            name, make = self.set[which]
            d = make()
            return self.call(name, h, C.byref(d))

        def off(which):
            return self.call(self.set[which][0], h, None)

        def submit():
            return self.call("crsdr_caf_submit", h, VP(self.packets.data_ptr()), C.c_size_t(STRIDE), C.c_size_t(OFFSET), T, None)

        (sa, before_a), (sc, before_c) = FEATURES[a], FEATURES[c]
        try:
            before = list(before_a)
            trace += [on(s) for s in before_a] + [on(sa), submit()]
            for s in before_c:
                if s not in before and s != sa:
                    trace.append(on(s))
                    before.append(s)
            trace += [on(sc), self.probe(h), submit(), self.probe(h), off(sa), self.probe(h), off(sc), self.probe(h)]
            trace += [off(s) for s in reversed(before)] + [self.probe(h)]
        finally:
            trace.append(self.call("crsdr_caf_destroy", h))
        return trace


def flat(trace):
    return json.loads(json.dumps([e for item in trace for e in (item if isinstance(item[0], list) else [item])]))


def pack(traces):
    """doa_states.json's form: each distinct entry once ("entries"), each distinct probe once as its entries' indices ("probes"), a
    sequence a list of n = entries[n] and [k] = the entries of probes[k]"""
    entries, probes, sequences = [], [], {}

    def index(table, item):
        if item not in table:
            table.append(item)
        return table.index(item)

    for key, trace in traces.items():
        sequences[key] = [[index(probes, [index(entries, e) for e in item])] if isinstance(item[0], list) else index(entries, item) for item in trace]
    return {"entries": entries, "probes": probes, "sequences": sequences}


def record(path):
    rig = Rig()
    traces = json.loads(json.dumps({f"{a}|{c}": rig.sequence(a, c) for a, c in PAIRS}))
    packed = pack(traces)
    assert unpack(packed) == {k: flat(v) for k, v in traces.items()}
    line = lambda v: json.dumps(v, separators=(",", ":"))
    with open(path, "w") as f:          # one entry, one probe, one sequence per line
        f.write('{"entries":[\n' + ",\n".join(line(e) for e in packed["entries"]) + '\n],"probes":[\n' + ",\n".join(line(q) for q in packed["probes"]) +
                '\n],"sequences":{\n' + ",\n".join(f"{json.dumps(k)}:{line(v)}" for k, v in packed["sequences"].items()) + "\n}}\n")
    return traces


@pytest.fixture(scope="module")
def rig():
    return Rig()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return unpack(json.load(f))


def test_every_pair_is_recorded(golden):
    assert sorted(golden) == sorted(f"{a}|{c}" for a, c in PAIRS) and len(PAIRS) == 64


@pytest.mark.parametrize("a,c", PAIRS, ids=[f"{a}-{c}" for a, c in PAIRS])
def test_states_replay(rig, golden, a, c):
    got, want = flat(rig.sequence(a, c)), golden[f"{a}|{c}"]
    for step, (g, w) in enumerate(zip(got, want)):
        assert g == w, (a, c, step, g, w)
    assert len(got) == len(want)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch  # noqa: F401  -- before the library (tests/conftest.py says why)
    out = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    print(f"{len(record(out))} sequences -> {out}")
