"""The state machine of crsdr_doa's setters, replayed against a recorded trace (tests/golden/doa_states.json).

Who refuses whom, what a setter discards, which fetch answers CRSDR_ESTATE and when: for every ordered pair (A, B) of the features
below a fresh object goes through  set A, submit, set B, probe, submit, probe, A off, probe, B off, probe  (subbands on first where A
or B is a band-beam feature).  A probe calls every fetch_*, every *_buffers and last_submit and records the return code, the message
after a failure, which buffer pointers are non-NULL, nbeams, nest and launches; every set call's code and message are recorded too.
No kernel result is compared: the device is needed because crsdr_doa_create needs one.

The object is the smallest at which every rule can fire: nrows = 7 (m = 6 = 3 x 2), blocksize 64, k = 1, an 8 x 8 grid, max_batch 2,
frames 1, both keep flags.  Sub-arrays of 2 x 2 leave a subspace of 4; an order range of 1 .. 4 fits m = 6 but not that subspace;
nfft 8 divides the block.

The trace is a fixture, recorded from the library before the engine's host code was regrouped into csrc/doa_engine.hpp:
    CRSDR_LIB=<that build's libcrsdr.so> python tests/test_gpu_doa_states.py [out.json]
writes it (this module produces the trace and compares it); the test requires equality, entry by entry."""
import ctypes as C
import importlib
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "doa_states.json")
NROWS, B, K, MX, MY, NC, T = 7, 64, 1, 3, 2, 8, 2
OFFSET = 16 + 4 * NROWS
STRIDE = OFFSET + NROWS * B
ANGLES = np.array([[0.5 * np.pi, 0.5 * np.pi]], dtype=np.float32)
CONV, MDL, FB, RECT = 1, 1, 1, 0
F32, I32, VP = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.c_void_p


def _angles():
    return ANGLES.ctypes.data_as(F32)


# name -> (on, off, needs subbands first); each a (function name, arguments behind the handle)
FEATURES = {
    "peaks": (("crsdr_doa_set_peaks", lambda: (2, 1)), ("crsdr_doa_set_peaks", lambda: (0, 0)), False),
    "beams_fixed": (("crsdr_doa_set_beams", lambda: (CONV, C.c_float(0.0), 1, _angles())), ("crsdr_doa_set_beams", lambda: (0, C.c_float(0.0), 0, None)), False),
    "beams_follow": (("crsdr_doa_set_beams", lambda: (CONV, C.c_float(0.0), 0, None)), ("crsdr_doa_set_beams", lambda: (0, C.c_float(0.0), 0, None)), False),
    "smooth_fb": (("crsdr_doa_set_smoothing", lambda: (MX, MY, FB)), ("crsdr_doa_set_smoothing", lambda: (MX, MY, 0)), False),
    "smooth_2x2": (("crsdr_doa_set_smoothing", lambda: (2, 2, 0)), ("crsdr_doa_set_smoothing", lambda: (MX, MY, 0)), False),
    "order_1_3": (("crsdr_doa_set_order", lambda: (MDL, 1, 3, 0)), ("crsdr_doa_set_order", lambda: (0, 0, 0, 0)), False),
    "order_1_3_limit": (("crsdr_doa_set_order", lambda: (MDL, 1, 3, 1)), ("crsdr_doa_set_order", lambda: (0, 0, 0, 0)), False),
    "order_1_4": (("crsdr_doa_set_order", lambda: (MDL, 1, 4, 0)), ("crsdr_doa_set_order", lambda: (0, 0, 0, 0)), False),
    "subbands": (("crsdr_doa_set_subbands", lambda: (8, 0, 2, 1, RECT)), ("crsdr_doa_set_subbands", lambda: (0, 0, 1, 1, RECT)), False),
    "band_beams_fixed": (("crsdr_doa_set_subband_beams", lambda: (CONV, C.c_float(0.0), 1, _angles())),
                         ("crsdr_doa_set_subband_beams", lambda: (0, C.c_float(0.0), 0, None)), True),
    "band_beams_follow": (("crsdr_doa_set_subband_beams", lambda: (CONV, C.c_float(0.0), 0, None)),
                          ("crsdr_doa_set_subband_beams", lambda: (0, C.c_float(0.0), 0, None)), True),
}
PAIRS = [(a, c) for a in FEATURES for c in FEATURES]


class Rig:
    """The library, the packets on the device and host buffers large enough for every fetch in every state."""

    def __init__(self):
        import torch
        self.b = importlib.import_module("coherent-rtlsdr_amd.binding")
        if self.b.device_count() < 1:
            pytest.fail("no HIP device: the product path has no CPU fallback")
        self.L = self.b.lib()
        rng = np.random.default_rng(20240607)
        host = np.full((T, STRIDE), 0x55, dtype=np.int8)
        host[:, OFFSET:] = rng.integers(-128, 128, size=(T, NROWS * B), dtype=np.int8)
        self.packets = torch.from_numpy(host).to(torch.device("cuda", 0))
        self.f = [np.zeros(1 << 14, dtype=np.float32) for _ in range(4)]      # (the largest fetch: 2 x 2 x 32 complex beams, 4 x 64 spectra)
        self.i = [np.zeros(1 << 10, dtype=np.int32) for _ in range(2)]

    def fp(self, j):
        return self.f[j].ctypes.data_as(F32)

    def ip(self, j):
        return self.i[j].ctypes.data_as(I32)

    def call(self, name, *args):
        """[name without its crsdr_doa_ prefix, return code, the message if the call failed]"""
        rc = getattr(self.L, name)(*args)
        return [name[len("crsdr_doa_"):], rc, self.L.crsdr_last_error().decode() if rc else ""]

    def probe(self, h):
        out = []
        out.append(self.call("crsdr_doa_fetch", h, self.ip(0), self.fp(0), self.fp(1), self.ip(1), self.fp(2), self.fp(3)))
        out.append(self.call("crsdr_doa_fetch_subspace", h, self.fp(0)))
        out.append(self.call("crsdr_doa_fetch_directions", h, self.ip(0), self.ip(1), self.fp(0)))
        out.append(self.call("crsdr_doa_fetch_beams", h, self.fp(0), self.fp(1), self.fp(2)))
        out.append(self.call("crsdr_doa_fetch_smoothed", h, self.fp(0)))
        out.append(self.call("crsdr_doa_fetch_order", h, self.ip(0), self.fp(0)))
        out.append(self.call("crsdr_doa_fetch_subbands", h, self.fp(0)))
        out.append(self.call("crsdr_doa_fetch_subband_beams", h, self.fp(0), self.fp(1), self.fp(2)))
        for name, n, count in (("crsdr_doa_device_buffers", 5, False), ("crsdr_doa_direction_buffers", 3, False), ("crsdr_doa_beam_buffers", 3, True),
                               ("crsdr_doa_order_buffers", 2, False), ("crsdr_doa_subband_buffers", 1, False), ("crsdr_doa_subband_beam_buffers", 3, True)):
            ptrs, nb = [VP() for _ in range(n)], C.c_int(-1)
            entry = self.call(name, h, *[C.byref(p) for p in ptrs], *([C.byref(nb)] if count else []))
            out.append(entry + [[p.value is not None for p in ptrs]] + ([nb.value] if count else []))
        nest, launches = C.c_int(-1), C.c_int(-1)
        out.append(self.call("crsdr_doa_last_submit", h, C.byref(nest), C.byref(launches)) + [nest.value, launches.value])
        return out

    def sequence(self, a, c):
        desc = self.b.DoaDesc(NROWS, B, 0, T, 1, K, MX, MY, NC, NC, 0.5, self.b.DOA_KEEP_SPECTRUM | self.b.DOA_KEEP_RXX)
        h = VP()
        trace = [self.call("crsdr_doa_create", C.byref(h), C.byref(desc))]
        assert trace[0][1] == 0, trace

        def setter(which):
            name, args = which
            return self.call(name, h, *args())

        def submit():
            return self.call("crsdr_doa_submit", h, VP(self.packets.data_ptr()), C.c_size_t(STRIDE), C.c_size_t(OFFSET), T, None)

        try:
            if FEATURES[a][2] or FEATURES[c][2]:
                trace.append(setter(FEATURES["subbands"][0]))
            trace += [setter(FEATURES[a][0]), submit(), setter(FEATURES[c][0])]
            trace += self.probe(h)
            trace.append(submit())
            trace += self.probe(h)
            trace.append(setter(FEATURES[a][1]))
            trace += self.probe(h)
            trace.append(setter(FEATURES[c][1]))
            trace += self.probe(h)
        finally:
            trace.append(self.call("crsdr_doa_destroy", h))
        return trace


PROBE = 15      # entries of a probe


def pack(traces):
    """The fixture's form: most entries and most probes recur, so each distinct entry is stored once ("entries"), each distinct probe
    once as its entries' indices ("probes"), and a sequence is a list of n = entries[n] and [k] = the entries of probes[k]."""
    entries, probes, sequences = [], [], {}

    def index(table, item):
        if item not in table:
            table.append(item)
        return table.index(item)

    for key, trace in traces.items():
        # the layout of Rig.sequence: the probes are the PROBE entries behind a set or submit entry, found from the end
        seq, i, starts = [], 0, set()
        n = len(trace) - 1                       # destroy
        for _ in range(4):
            n -= PROBE
            starts.add(n)
            n -= 1
        while i < len(trace):
            if i in starts:
                seq.append([index(probes, [index(entries, e) for e in trace[i:i + PROBE]])])
                i += PROBE
            else:
                seq.append(index(entries, trace[i]))
                i += 1
        sequences[key] = seq
    return {"entries": entries, "probes": probes, "sequences": sequences}


def unpack(packed):
    entries, probes = packed["entries"], packed["probes"]
    return {key: [e for item in seq for e in ([entries[j] for j in probes[item[0]]] if isinstance(item, list) else [entries[item]])]
            for key, seq in packed["sequences"].items()}


def record(path):
    rig = Rig()
    traces = json.loads(json.dumps({f"{a}|{c}": rig.sequence(a, c) for a, c in PAIRS}))
    packed = pack(traces)
    assert unpack(packed) == traces
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
    assert sorted(golden) == sorted(f"{a}|{c}" for a, c in PAIRS) and len(PAIRS) == 121


@pytest.mark.parametrize("a,c", PAIRS, ids=[f"{a}-{c}" for a, c in PAIRS])
def test_states_replay(rig, golden, a, c):
    got, want = json.loads(json.dumps(rig.sequence(a, c))), golden[f"{a}|{c}"]
    for step, (g, w) in enumerate(zip(got, want)):
        assert g == w, (a, c, step, g, w)
    assert len(got) == len(want)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch  # noqa: F401  -- before the library (tests/conftest.py says why)
    out = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    print(f"{len(record(out))} sequences -> {out}")
