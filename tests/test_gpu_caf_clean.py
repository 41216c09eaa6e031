"""crsdr_caf's second cancellation stage on the device (crsdr_caf_set_clean, crsdr_ambiguity_clean; csrc/caf_clean.hpp and k_caf<LG, 3>
of csrc/caf.hpp) against tests/caf_clean_model.py.  The device is held against the model on the device's OWN published det: the picks
are decided in fp64 on published fp32 figures, so tgt and ntgt are equal, no line left out; tcoef, tinfo and rchi within the bars the
model derives (each scene asserts the cond(A) they assume); rmap, rdet, rcount and rsnap against the first pass's models on the
device's own rchi.  Then the bits: a line without picks, a line wherever it sits, per op, behind a plan, every existing output with the
stage on against the stage off; the masking scene end to end; and the launch count."""
import importlib

import numpy as np
import pytest

import caf_cancel_model as X
import caf_cfar_est_model as CE
import caf_cfar_model as C
import caf_clean_model as Z
import caf_model as M

pytestmark = pytest.mark.gpu
EINVAL, ESTATE = -1, -5
RECT, HANN = M.WINDOW_RECT, M.WINDOW_HANN
STAGE1 = 9                                                                       # launches of a submit with the canceller and the detector
FIRST = ("chi", "map", "peak", "coef", "cinfo", "det", "count", "snap")
SECOND = ("tgt", "ntgt", "tcoef", "tinfo", "rchi", "rmap", "rdet", "rcount", "rsnap")
TWIN = dict(rchi="chi", rmap="map", rdet="det", rcount="count", rsnap="snap")


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
    """T packet-shaped slots on the device, as a plan lays them out: packet t at base + t * stride, its matrix [nrows][B] at + 16 + 4 nrows"""

    def __init__(self, torch, blocks, pad=0):
        blocks = np.ascontiguousarray(blocks)
        self.T, self.nrows, self.B = blocks.shape
        self.offset = 16 + 4 * self.nrows
        self.stride = self.offset + self.nrows * self.B + pad
        host = np.full((self.T, self.stride), 0x55, dtype=np.int8)
        host[:, self.offset:self.offset + self.nrows * self.B] = blocks.reshape(self.T, -1)
        self.buf = torch.from_numpy(host).to(torch.device("cuda", 0))
        self.ptr = self.buf.data_ptr()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype != np.complex64 else a.view(np.float32).view(np.uint32)


def _same(x, y, keys):
    return all(np.array_equal(_bits(x[k]), _bits(y[k])) for k in keys)


def _line(out, e, keys=FIRST + SECOND):
    return {k: out[k][e] for k in keys}


def _cq(b, q):
    return b.cfar_desc(alpha=float(q.alpha), gd=q.gd, gr=q.gr, td=q.td, tr=q.tr, min_train=q.min_train, max_det=q.max_det)


def _lq(b, p):
    return b.CleanDesc(p.T, float(p.min_snr), p.wl, p.wq)


def _detector(nd, alpha=None, max_det=8):
    td = 3 if nd >= 16 else 2
    return C.Params(C.cfar_alpha(1e-6, 54) if alpha is None else alpha, gd=1, gr=1, td=td, tr=2, min_train=4, max_det=max_det)


def _engine(b, torch, blocks, sh, q, prm, frames=1, pad=0, max_batch=None, nblocks=None, extra=None):
    """blocks [T][nrows][B] through the engine with canceller, detector and cleaning on -> every output, [nest] first"""
    T, nrows, B = blocks.shape
    pk = Packets(torch, blocks, pad)
    cf = b.Caf(nrows, B, sh["seg"], sh["R"], sh["ref"], sh["kind"], sh["guard"], max_batch=max_batch or T, frames=frames)
    cf.set_cancel(sh["K"], sh["P"])
    cf.set_cfar(_cq(b, q))
    cf.set_clean(_lq(b, prm))
    cf.submit(pk.ptr, pk.stride, pk.offset, nblocks or T)
    assert cf._last() == ((nblocks or T) // frames, STAGE1 + Z.LAUNCHES)
    out = {**cf.fetch(), **cf.fetch_cancel(), **cf.fetch_cfar(), **cf.fetch_clean()}
    cf.close()
    return out


def _hold(got, line, sh, q, prm, tag, cond_max=Z.COND_MAX, est=None):
    """one line's outputs (dict, no line axis) against the model on the device's own det; returns the model's dict.  est: the detector's
    estimator (caf_cfar_est_model.Est), under which the residual's lists are held as well"""
    nrows, ref, guard = got["chi"].shape[0], sh["ref"], sh["guard"]
    assert all(np.all(np.isfinite(got[k])) for k in FIRST + SECOND), tag
    det, count = got["det"][nrows], int(got["count"][nrows])
    r = Z.clean(line, sh["seg"], sh["R"], ref, sh["kind"], sh["K"], sh["P"], det, count, prm)
    assert int(np.ravel(got["ntgt"])[0]) == r["ntgt"] and np.array_equal(_bits(got["tgt"]), _bits(r["tgt"])), (tag, got["tgt"], r["tgt"])
    assert np.array_equal(got["tinfo"][:, 1], r["status"]), (tag, got["tinfo"], r["status"])
    st = int(r["status"].max())
    if st == 0:
        assert r["cond"] <= cond_max, (tag, r["cond"])
    rc = M.worst_ratio(got["rchi"], r["rchi"], r["rbar"])
    et = np.maximum(np.abs(got["tcoef"].real - r["tcoef"].real), np.abs(got["tcoef"].imag - r["tcoef"].imag))
    rt = float(np.max(et / np.maximum(r["tbar"], 1e-300))) if r["members"] else 0.0
    assert not got["tcoef"][r["tbar"] == 0].any() and not got["tcoef"][ref].any(), tag
    rs = float(np.max(np.abs(got["tinfo"][:, 0] - r["share"]) / np.maximum(r["sbar"], 1e-300)))
    wm, bm = M.array_map(got["rchi"], ref)
    rm = M.worst_ratio(got["rmap"].astype(np.float64), wm, bm)
    print(f"{tag}: picks {r['ntgt']} members {len(r['members'])} status {st} cond {r['cond']:.1f}; largest error / bar: rchi {rc:.4f} tcoef {rt:.4f} share {rs:.4f} rmap {rm:.4f}")
    assert rc <= 1.0 and rt <= 1.0 and rs <= 1.0 and rm <= 1.0, (tag, rc, rt, rs, rm)
    assert tuple(got["tinfo"][ref]) == (1.0, 0.0), tag
    # the residual's lists: the first pass's models on the device's own rchi and rmap
    maps = C.maps_of(got["rchi"], got["rmap"])
    for entry in range(nrows + 1):
        want = CE.detect(maps[entry], guard, q, est)
        assert want["ambiguous"] == 0 and want["half_ambiguous"] == 0, f"{tag}: the model finds ambiguous cells in the device's residual, entry {entry}"
        d = got["rdet"][entry]
        assert int(got["rcount"][entry]) == want["count"] and np.array_equal(d[:, [0, 1, 7]].astype(np.float64), want["det"][:, [0, 1, 7]]), (tag, entry, d, want["det"])
        assert np.all(np.abs(d.astype(np.float64) - want["det"]) <= want["bar"]), (tag, entry)
        if entry == nrows:
            assert np.array_equal(_bits(got["rsnap"]), _bits(C.snapshot(got["rchi"], want["cells"], q.max_det))), tag
    if r["ntgt"] == 0 or st != 0:                                                # nothing joined the basis: the first pass's bytes
        assert all(np.array_equal(_bits(got[k]), _bits(got[v])) for k, v in TWIN.items()), tag
    return r


def _scene(sh, targets, seed, thermal=1.0, frames=1):
    """the direct path and `targets` [(lag, bins, a)] in every row but ref, phases constant within a segment; a list of `frames` matrices"""
    return X.clutter_scene(seed, seg=sh["seg"], nd=sh["nd"], paths=((0, 0, 0.8),) + tuple(targets[:-1]), echo=targets[-1], thermal=thermal, nrows=sh["nrows"],
                           ref=sh["ref"], per_segment=True, frames=frames)


def _shape(nrows=3, seg=32, nd=32, R=16, ref=0, kind=HANN, guard=0, K=2, P=0):
    return dict(nrows=nrows, seg=seg, nd=nd, R=R, ref=ref, kind=kind, guard=guard, K=K, P=P)


def _per_op(b, line, sh, q, prm, est=None):
    e = None if est is None else b.cfar_est_desc(est.est, est.axis, est.rank)
    return b.ambiguity_clean(line[0], sh["seg"], sh["R"], b.CancelDesc(sh["K"], sh["P"]), _cq(b, q), _lq(b, prm), e, sh["ref"], sh["kind"], sh["guard"])


# (name, shape, targets, (T, min_snr, wl, wq), picks expected, members expected or None)
EDGES = [
    ("lag 0 and R - 1: clipped clusters", _shape(K=1), [(0, 6.3, 0.5), (15, -5.4, 0.4)], (2, 50.0, 1, 1), 2, 12),
    ("across the Doppler wrap", _shape(), [(5, 15.8, 0.5), (10, -15.7, 0.4)], (2, 50.0, 1, 2), 2, 30),
    ("zero picks", _shape(), [(6, 4.3, 0.5)], (2, 1e30, 1, 1), 0, 0),
    ("T picks, candidates behind them", _shape(), [(4, 6.3, 0.5), (8, -4.4, 0.45), (12, 10.2, 0.4)], (2, 50.0, 1, 1), 2, 18),
    ("two candidates that touch", _shape(), [(6, 4.3, 0.5), (8, 5.6, 0.4)], (2, 10.0, 1, 1), 1, 9),
    ("a candidate on the clutter basis", _shape(), [(2, 1.2, 0.5), (9, 7.3, 0.4)], (2, 50.0, 1, 1), 1, 9),
    ("64 members, R 48", _shape(seg=64, R=48, K=4), [(8, 5.3, 0.5), (18, -6.4, 0.45), (28, 10.2, 0.4), (38, -11.6, 0.35)], (4, 50.0, 2, 1), 4, 60),
    ("R 1", _shape(R=1, K=1), [(0, 7.3, 0.5)], (1, 50.0, 1, 1), 1, 3),
    ("R 17, ref 2, rect", _shape(R=17, ref=2, kind=RECT), [(16, 6.3, 0.5), (7, -9.4, 0.4)], (2, 50.0, 2, 1), 2, 24),
    ("nd 8", _shape(nrows=2, seg=64, nd=8, R=4, K=1), [(2, 3.3, 0.5)], (1, 20.0, 1, 1), 1, 9),
    ("nd 64, ref 1, P 1", _shape(nrows=2, seg=16, nd=64, R=5, ref=1, K=1, P=1, guard=1), [(3, -20.4, 0.5)], (1, 50.0, 1, 2), 1, 15),
    ("nd 4096: one-lag tiles", _shape(nrows=2, seg=16, nd=4096, R=4, K=1), [(2, 700.3, 0.5)], (1, 50.0, 1, 1), 1, 9),
]


@pytest.mark.parametrize("case", EDGES, ids=[c[0] for c in EDGES])
def test_per_op_at_the_edges(b, case):
    name, sh, targets, (T, min_snr, wl, wq), picks, members = case
    q, prm = _detector(sh["nd"]), Z.Params(T, min_snr, wl, wq)
    line = _scene(sh, targets, seed=len(name))
    got = _per_op(b, line, sh, q, prm)
    r = _hold(got, line, sh, q, prm, name)
    assert r["ntgt"] == picks and len(r["members"]) == members, (name, r["ntgt"], len(r["members"]), got["det"][sh["nrows"]][:4])
    if picks:
        assert not np.array_equal(_bits(got["rchi"]), _bits(got["chi"]))
        assert np.array_equal(_bits(got["rchi"][sh["ref"]]), _bits(got["chi"][sh["ref"]]))   # row r is left alone


@pytest.mark.parametrize("est", [CE.Est(CE.GO, CE.DOPPLER), CE.Est(CE.SO, CE.LAG), CE.Est(CE.OS, rank=40)], ids=["GO", "SO", "OS"])
def test_the_residual_is_detected_under_the_descriptors_estimator(b, torch, est):
    """the masking scene under greatest-of, smallest-of and the ordered statistic, per op and through the engine with the estimator set:
    both lists are the estimator's (the first pass's picks come from it), and the engine has the per-op call's bytes"""
    mk = Z.MASK
    sh = _shape(nrows=mk["nrows"], seg=mk["seg"], nd=mk["nd"], R=mk["R"], ref=mk["ref"], K=mk["taps"], P=mk["dopp"])
    q, prm = Z.masking_detector(), Z.Params(2, 50.0, 1, 1)
    line = Z.masking_scene(2)
    got = _per_op(b, line, sh, q, prm, est)
    n = mk["nrows"]
    first = CE.detect(np.asarray(got["map"], dtype=np.float64), 0, q, est)
    assert first["ambiguous"] == 0 and first["half_ambiguous"] == 0 and int(got["count"][n]) == first["count"]
    assert np.array_equal(got["det"][n][:, [0, 1, 7]].astype(np.float64), first["det"][:, [0, 1, 7]])
    r = _hold(got, line, sh, q, prm, f"estimator {est.est}", est=est)
    assert r["ntgt"] >= 1 and int(got["rcount"][n]) >= 1
    pk = Packets(torch, np.stack(line))
    cf = b.Caf(n, line[0].shape[1], sh["seg"], sh["R"], sh["ref"], sh["kind"], sh["guard"])
    cf.set_cancel(sh["K"], sh["P"])
    cf.set_cfar(_cq(b, q))
    cf.set_cfar_estimator(b.cfar_est_desc(est.est, est.axis, est.rank))
    cf.set_clean(_lq(b, prm))
    cf.submit(pk.ptr, pk.stride, pk.offset, 1)
    out = {**cf.fetch(), **cf.fetch_cancel(), **cf.fetch_cfar(), **cf.fetch_clean()}
    cf.close()
    assert _same(_line(out, 0), got, FIRST + SECOND)


def test_a_reference_confined_to_one_segment_trips_status_2_and_an_all_zero_one_status_1(b):
    """One live segment gives every Doppler the same column up to a unit factor, so a cluster's second Doppler is rank deficient: the
    target pivot fails while the canceller's single member stands.  (A periodic reference does not get there exactly: the zeros in
    front of the packet keep two lags apart by a few samples, a pivot some 10^-3 of A_00, far over the floor.)"""
    sh = _shape(K=1, guard=3)
    q, prm = _detector(sh["nd"], alpha=3.0), Z.Params(2, 2.0, 0, 1)             # (the plateau over Doppler stands some 3.5 over its window's mean)
    line = _scene(sh, [(6, 4.3, 0.5)], seed=5)
    m = line[0].copy()
    keep = m[sh["ref"]].copy()
    m[sh["ref"]] = 0
    a, z = 2 * sh["seg"] * 5, 2 * sh["seg"] * 5 + 2 * 12                         # 12 samples at the head of segment 5: every lag stays inside it
    m[sh["ref"], a:z] = keep[a:z]
    got = _per_op(b, [m], sh, q, prm)
    r = _hold(got, [m], sh, q, prm, "one live segment")
    assert r["ntgt"] >= 1 and np.array_equal(got["tinfo"][:, 1], [0.0, 2.0, 2.0]) and not got["tcoef"].any()
    assert np.array_equal(_bits(got["tinfo"][:, 0]), _bits(got["cinfo"][:, 0]))  # the share is the first stage's
    m[sh["ref"]] = 0
    got = _per_op(b, [m], sh, q, prm)
    r = _hold(got, [m], sh, q, prm, "an all-zero reference")
    assert r["ntgt"] == 0 and np.array_equal(got["tinfo"][:, 1], [0.0, 1.0, 1.0]) and np.array_equal(got["cinfo"][:, 1], [0.0, 1.0, 1.0])


def test_the_engine_equals_the_per_op_call_anywhere_in_a_batch_with_frames_and_behind_a_plan(b, torch):
    sh = _shape(seg=32, nd=32, R=17, ref=1, K=2, P=1)
    q, prm = _detector(sh["nd"]), Z.Params(2, 50.0, 1, 1)
    lines = [_scene(sh, [(5 + t, 6.3 - t, 0.5), (12, -9.4, 0.3)], seed=900 + t)[0] for t in range(4)]
    lines[2] = _scene(sh, [(5, 6.3, 0.5)], seed=950, thermal=100.0)[0]            # a line without picks among lines with them
    blocks = np.stack(lines)
    alone = [_per_op(b, [m], sh, q, prm) for m in lines]
    assert int(alone[0]["ntgt"][0]) >= 1 and int(alone[2]["ntgt"][0]) == 0
    for order in ([0, 1, 2, 3], [3, 0, 1, 2], [2, 3, 0, 1], [1, 2, 3, 0]):       # every line through every position
        out = _engine(b, torch, blocks[order], sh, q, prm, pad=24)
        for e, t in enumerate(order):
            assert _same(_line(out, e), alone[t], FIRST + SECOND), (order, e)
    one = _engine(b, torch, blocks[:1], sh, q, prm, max_batch=4)
    assert _same(_line(one, 0), alone[0], FIRST + SECOND)
    _hold(_line(one, 0), [lines[0]], sh, q, prm, "engine, line 0")
    _hold(alone[2], [lines[2]], sh, q, prm, "no picks")
    # frames 2: two packets a line, nd 32 from 16 segments each
    sh2 = dict(sh)
    two = _scene(sh, [(5, 6.3, 0.5), (12, -9.4, 0.3)], seed=77, frames=2)
    pair = np.stack(two + two)
    out = _engine(b, torch, pair, sh2, q, prm, frames=2)
    assert _same(_line(out, 0), _line(out, 1), FIRST + SECOND)
    r = _hold(_line(out, 0), two, sh2, q, prm, "frames 2")
    assert r["ntgt"] >= 1
    # behind a plan, on the plan's stream, against a submit on the packets it published
    nrows, B = blocks.shape[1:]
    # the per-op call on device memory
    dev = torch.device("cuda", 0)
    m = torch.from_numpy(lines[0].copy()).to(dev)
    shapes = b.clean_shapes(nrows, sh["nd"], sh["R"], X.basis(sh["K"], sh["P"]), q.max_det, _lq(b, prm))
    bufs = {k: torch.zeros(int(np.prod(shp)) * (2 if dt is np.complex64 else 1), dtype=torch.int32 if dt is np.int32 else torch.float32, device=dev)
            for k, (shp, dt) in shapes.items()}
    b.ambiguity_clean_device({k: t.data_ptr() for k, t in bufs.items()}, m.data_ptr(), nrows, B, sh["seg"], sh["R"], sh["ref"], sh["kind"], sh["guard"],
                             b.CancelDesc(sh["K"], sh["P"]), _cq(b, q), _lq(b, prm))
    for k, t in bufs.items():
        assert np.array_equal(t.cpu().numpy().view(np.uint32).ravel(), _bits(alone[0][k]).ravel()), k
    plan = b.Plan(nrows, B, b.MODE_DIGITAL, max_batch=4)
    plan.submit(blocks, seq=0)
    cf = b.Caf(nrows, B, sh["seg"], sh["R"], sh["ref"], sh["kind"], sh["guard"], max_batch=4)
    cf.set_cancel(sh["K"], sh["P"])
    cf.set_cfar(_cq(b, q))
    cf.set_clean(_lq(b, prm))
    cf.submit_plan(plan)
    assert cf._last() == (4, STAGE1 + Z.LAUNCHES)
    behind = {**cf.fetch(), **cf.fetch_cancel(), **cf.fetch_cfar(), **cf.fetch_clean()}
    pub = Packets(torch, np.stack([plan.fetch(block=t)["matrix"].copy() for t in range(4)]))
    cf.submit(pub.ptr, pub.stride, pub.offset, 4)
    again = {**cf.fetch(), **cf.fetch_cancel(), **cf.fetch_cfar(), **cf.fetch_clean()}
    assert _same(behind, again, FIRST + SECOND)
    assert all(cf.clean_device_buffers().values())
    cf.close()
    plan.close()


def _both(b, torch, blocks, sh, q, prm, setup, fetch, submits=1):
    """the outputs `fetch` names with the cleaning off and on, the rest of the engine set up alike"""
    T, nrows, B = blocks.shape
    pk = Packets(torch, blocks)
    got = []
    for on in (False, True):
        cf = b.Caf(nrows, B, sh["seg"], sh["R"], sh["ref"], sh["kind"], sh["guard"], max_batch=T)
        cf.set_cancel(sh["K"], sh["P"])
        cf.set_cfar(_cq(b, q))
        if on:
            cf.set_clean(_lq(b, prm))
        extra = setup(cf)
        for _ in range(submits):
            cf.submit(pk.ptr, pk.stride, pk.offset, T)
        assert cf._last() == (T, STAGE1 + extra + (Z.LAUNCHES if on else 0))
        got.append({**cf.fetch(), **cf.fetch_cancel(), **cf.fetch_cfar(), **fetch(cf)})
        if on:
            assert int(cf.fetch_clean()["ntgt"].max()) >= 1                      # the stage did pick
        cf.close()
    return got


@pytest.mark.parametrize("feature", ["bearings", "beams", "beam integration", "tracker"])
def test_every_existing_output_keeps_its_bits_with_the_stage_on(b, torch, feature):
    sh = _shape(seg=32, nd=32, R=16, K=2)
    q, prm = _detector(sh["nd"]), Z.Params(2, 50.0, 1, 1)
    blocks = np.stack([_scene(sh, [(6, 4.3, 0.5), (11, -9, 0.2)], seed=300 + t)[0] for t in range(3)])
    w = b.beam_steer(2, 1, 0.5, [[30, 50], [70, 50]])

    def setup(cf):
        if feature == "bearings":
            cf.set_bearing(b.bearing_desc(2, 1, 0.5, ncx=16, ncy=16))
            return 3
        if feature == "beams":
            cf.set_beams(w)
            return 4
        if feature == "beam integration":
            cf.set_beams(w)
            cf.set_integrate(b.integrate_desc(0.9, what=b.INTEGRATE_BEAMS))
            return 5
        cf.set_track(b.track_desc(8))
        return 1

    fetch = {"bearings": lambda cf: cf.fetch_bearing(), "beams": lambda cf: cf.fetch_beams(), "beam integration": lambda cf: {**cf.fetch_beams(), **cf.fetch_integrate()},
             "tracker": lambda cf: cf.fetch_track()}[feature]
    off, on = _both(b, torch, blocks, sh, q, prm, setup, fetch, submits=2)
    assert off.keys() == on.keys() and len(off) > len(FIRST)
    for k in off:
        assert np.array_equal(np.ascontiguousarray(off[k]).view(np.uint8), np.ascontiguousarray(on[k]).view(np.uint8)), (feature, k)


def test_the_masking_scene_end_to_end(b, torch):
    """The first pass lists the strong mover and not the echo under its floor; the residual's list holds exactly the echo, and nothing
    at the mover's cell.  With wq = 0 the one integer-bin member leaves enough of the mover for the detector to list it again."""
    mk = Z.MASK
    sh = _shape(nrows=mk["nrows"], seg=mk["seg"], nd=mk["nd"], R=mk["R"], ref=mk["ref"], K=mk["taps"], P=mk["dopp"])
    q = Z.masking_detector()
    blocks = np.stack([Z.masking_scene(seed)[0] for seed in range(4)])
    out = _engine(b, torch, blocks, sh, q, Z.Params(2, 100.0, 1, 1))
    coarse = _engine(b, torch, blocks, sh, q, Z.Params(2, 100.0, 1, 0))
    n = mk["nrows"]
    cells = lambda det, count: [(int(r[0]), int(r[1])) for r in det[:count]]
    strong, weak = (mk["strong"][0], int(round(mk["strong"][1]))), (mk["weak"][0], mk["weak"][1])
    for e in range(4):
        r = _hold(_line(out, e), [blocks[e]], sh, q, Z.Params(2, 100.0, 1, 1), f"masking scene {e}")
        assert cells(out["det"][e][n], out["count"][e][n]) == [strong], (e, out["det"][e][n])
        assert int(out["ntgt"][e]) == 1 and cells(out["rdet"][e][n], out["rcount"][e][n]) == [weak], (e, out["rdet"][e][n])
        d = strong[1] % mk["nd"]
        depth = 10.0 * np.log10(out["map"][e][d, strong[0]] / out["rmap"][e][d, strong[0]])
        print(f"masking scene {e}: the mover's cell falls by {depth:.1f} dB; the echo's snr {out['rdet'][e][n][0][3]:.0f}; cond {r['cond']:.1f}")
        assert depth > 40.0
        got = cells(coarse["rdet"][e][n], coarse["rcount"][e][n])
        assert weak in got and len(got) > 1 and any(c[0] == strong[0] for c in got if c != weak), (e, got)


def test_the_launch_count_and_the_state_rules(b, torch):
    sh = _shape(R=8)
    q, prm = _detector(sh["nd"]), Z.Params(2, 50.0, 1, 1)
    blocks = np.stack([M.random_matrix(3, 2 * sh["seg"] * sh["nd"], 60 + t) for t in range(8)])
    pk = Packets(torch, blocks)
    cf = b.Caf(3, blocks.shape[2], sh["seg"], sh["R"], 0, HANN, 0, max_batch=8)

    def refused(call, *a):
        with pytest.raises(b.CrsdrError) as e:
            call(*a)
        return e.value.code

    assert refused(cf.set_clean, _lq(b, prm)) == ESTATE and refused(cf.fetch_clean) == ESTATE and refused(cf.clean_device_buffers) == ESTATE
    cf.set_cancel(2, 0)
    assert refused(cf.set_clean, _lq(b, prm)) == ESTATE                          # no detector
    cf.set_cfar(_cq(b, q))
    cf.set_integrate(b.integrate_desc(0.9))
    assert refused(cf.set_clean, _lq(b, prm)) == ESTATE                          # the array map is integrated
    cf.set_integrate(None)
    assert refused(cf.set_clean, b.CleanDesc(9, 50.0, 1, 1)) == EINVAL
    cf.set_clean(_lq(b, prm))
    assert refused(cf.fetch_clean) == ESTATE                                     # nothing submitted since it was set
    for call, a in ((cf.set_cancel, (3, 0)), (cf.set_cancel, (None,)), (cf.set_cfar, (None,)), (cf.set_cfar_estimator, (None,)), (cf.set_integrate, (b.integrate_desc(0.9),))):
        assert refused(call, *a) == ESTATE
        assert "turn it off first" in b.lib().crsdr_last_error().decode()
    for nblocks in (1, 8, 3):
        cf.submit(pk.ptr, pk.stride, pk.offset, nblocks)
        assert cf._last() == (nblocks, STAGE1 + Z.LAUNCHES) and Z.LAUNCHES == b.CLEAN_LAUNCHES
        assert cf.fetch_clean()["rchi"].shape == (nblocks, 3, sh["nd"], sh["R"])
    cf.set_clean(_lq(b, prm))
    assert refused(cf.fetch_clean) == ESTATE                                     # set again: its "ran" bit is cleared
    cf.set_clean(None)
    cf.submit(pk.ptr, pk.stride, pk.offset, 8)
    assert cf._last() == (8, STAGE1) and refused(cf.fetch_clean) == ESTATE
    cf.set_integrate(b.integrate_desc(0.9))
    cf.set_clean(None)                                                           # turning it off, or leaving it off, is never refused
    cf.set_integrate(None)
    cf.set_cancel(None)                                                          # free again
    cf.close()
