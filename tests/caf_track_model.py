"""The tracker of crsdr_caf ("Tracks." in include/crsdr.h) in fp64 numpy, written as the header's sequential sentences -- predict,
range exit, gate, the greedy walk over the candidates sorted by (d2, i, j), update and coast, status, initiation -- and NOT as the
kernel's mutual-first rounds (rounds() below states those, for the test that pins the two equal).

Tracker.line() returns the line's records UNROUNDED (fp64; the device rounds each figure once to fp32), its four counts and its
MARGIN: the smallest of |d2 - gate| / gate over all gate tests of the line and, over every taken candidate, the relative gap in d2
(|a - b| / max(a, b)) to the nearest other candidate of its row or column that was free at that point.  Candidates whose inputs are
bitwise equal (the same track against two measurements of equal z, or two tracks of equal state against one measurement) are ties by
rule -- the lower index -- and no ambiguity: they are left out of the gap.  A line whose margin is far above the arithmetic's error
has the same decisions in any correct fp64 evaluation; test_caf_track_model.py asserts margin >= 1000 BAR for every scene of SCENES,
and no test uses the margin to leave anything out.

The bar.  A track's figures come out of a recursion of data-dependent length (a Kalman filter whose gain depends on P, whose P depends on
the hit pattern): there is no closed form for its rounding error short of a running bound that would restate the filter.  So the bar on
r, f, g, sqrt(P00) and sqrt(P11) is fixed the other way the issue allows: 64 x the largest deviation, over every line, slot and figure of
every scene of SCENES, between this model and restated(): the same recursion in np.longdouble with the operations in another order
(F (P F^T) for (F P) F^T, the gain through an explicit inverse matrix, P' - K (H P') for P' - K S K^T, d2 as nu . (S^-1 nu)).  The
deviation is measured by deviation() and was 2.3e-15 (scene size_64_64; 80-bit long double) when this was written:
    BAR = 64 x 2.3e-15 = 1.5e-13        absolute, in cells, bins and bins per line
test_caf_track_model.py re-measures it and fails if 64 x the deviation exceeds BAR.  f is compared modulo nd.  The device's and the host
program's figures are held to BAR plus half an fp32 ulp of the expected figure (the one rounding of the record).  A float32 restatement
(single()) misses BAR by five orders of magnitude.
"""
import itertools

import numpy as np

BAR = 1.5e-13
ND, R = 16, 16
FREE, TENTATIVE, CONFIRMED, ENDED = 0, 1, 2, 3
ID_PERIOD = (1 << 24) - 1
MUTATIONS = ("no_wrap", "gate_p", "tie_reversed", "highest_slot", "coast_no_q", "misses_kept", "reuse_ended", "hist_unmasked")

SLOT = np.dtype([("x", "<f8", 3), ("P", "<f8", 6), ("d2", "<f8"), ("power", "<f4"), ("snr", "<f4"), ("aux0", "<f4"), ("aux1", "<f4"), ("id", "<i4"), ("status", "<i4"),
                 ("age", "<i4"), ("hits", "<i4"), ("misses", "<i4"), ("hist", "<u4"), ("reserved", "<u4", 2)])
assert SLOT.itemsize == 128
HEADER = 16
TRI = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))


class Desc:
    def __init__(self, T, m=3, n=5, gate=9.0, sigma_r=0.5, sigma_f=0.5, p0_g=1.0, q_r=1e-3, q_f=1e-3, q_g=1e-4, coupling=0.0, tent_miss=2, conf_miss=4, source=0):
        self.T, self.m, self.n, self.gate, self.sigma_r, self.sigma_f, self.p0_g = T, m, n, gate, sigma_r, sigma_f, p0_g
        self.q_r, self.q_f, self.q_g, self.coupling, self.tent_miss, self.conf_miss, self.source = q_r, q_f, q_g, coupling, tent_miss, conf_miss, source

    def fields(self):
        """in the order of crsdr_caf_track_desc"""
        return (self.T, self.source, self.sigma_r, self.sigma_f, self.gate, self.p0_g, self.q_r, self.q_f, self.q_g, self.coupling, self.m, self.n, self.tent_miss,
                self.conf_miss)


def wrap(v, nd):
    D = type(v)
    return v - D(nd) * np.floor((v + D(nd // 2)) / D(nd))


def is_measurement(rec, nd, R):
    return bool(0.0 <= rec[0] < R and -(nd // 2) <= rec[1] < nd // 2 and np.isfinite(rec[5]) and np.isfinite(rec[6]))


class Track:
    __slots__ = ("x", "P", "d2", "power", "snr", "aux", "id", "status", "age", "hits", "misses", "hist")


class Tracker:
    """dtype, order: np.float64, 0 is the model; restated() and single() are the other two.  mutate: one of MUTATIONS."""

    def __init__(self, q, nd=ND, R=R, dtype=np.float64, order=0, mutate=None):
        self.q, self.nd, self.R, self.D, self.order, self.mutate = q, nd, R, dtype, order, mutate
        self.slots, self.counter = [None] * q.T, 0

    # ---- the state in the layout of the per-op call's buffer ----
    def state(self):
        s = np.zeros(self.q.T, dtype=SLOT)
        for i, t in enumerate(self.slots):
            if t is None:
                continue
            s[i]["x"], s[i]["P"], s[i]["d2"] = t.x, [t.P[a, b] for a, b in TRI], t.d2
            s[i]["power"], s[i]["snr"], s[i]["aux0"], s[i]["aux1"] = t.power, t.snr, t.aux[0], t.aux[1]
            s[i]["id"], s[i]["status"], s[i]["age"], s[i]["hits"], s[i]["misses"], s[i]["hist"] = t.id, t.status, t.age, t.hits, t.misses, t.hist & 0xFFFFFFFF
        return np.concatenate([np.array([self.counter, 0, 0, 0], dtype="<i4").view(np.uint8), s.view(np.uint8)])

    def load(self, blob):
        blob = np.asarray(blob, dtype=np.uint8)
        self.counter = int(blob[:HEADER].view("<i4")[0])
        s = blob[HEADER:].view(SLOT)
        for i in range(self.q.T):
            if s[i]["status"] == FREE:
                self.slots[i] = None
                continue
            t = Track()
            t.x = s[i]["x"].astype(self.D)
            t.P = np.zeros((3, 3), dtype=self.D)
            for v, (a, b) in zip(s[i]["P"], TRI):
                t.P[a, b] = t.P[b, a] = v
            t.d2, t.power, t.snr, t.aux = self.D(s[i]["d2"]), s[i]["power"], s[i]["snr"], (s[i]["aux0"], s[i]["aux1"])
            t.id, t.status, t.age, t.hits, t.misses, t.hist = (int(s[i][k]) for k in ("id", "status", "age", "hits", "misses", "hist"))
            self.slots[i] = t
        return self

    # ---- the arithmetic ----
    def _predict(self, t):
        D, q = self.D, self.q
        c = D(q.coupling)
        F = np.array([[1, c, c / D(2)], [0, 1, 1], [0, 0, 1]], dtype=D)
        Q = np.diag(np.array([q.q_r, q.q_f, q.q_g], dtype=D))
        r, f, g = t.x
        x = np.array([r + c * (f + g / D(2)), wrap(f + g, self.nd), g], dtype=D)
        P = ((F @ t.P) @ F.T if self.order == 0 else F @ (t.P @ F.T)) + Q
        return x, P

    def _gate(self, x, P, z):
        D, q = self.D, self.q
        dfreq = z[1] - x[1]
        nu = np.array([z[0] - x[0], dfreq if self.mutate == "no_wrap" else wrap(dfreq, self.nd)], dtype=D)
        S = P[:2, :2] + np.diag(np.array([D(q.sigma_r) * D(q.sigma_r), D(q.sigma_f) * D(q.sigma_f)], dtype=D))
        G = P[:2, :2] if self.mutate == "gate_p" else S
        det = G[0, 0] * G[1, 1] - G[0, 1] * G[0, 1]
        if self.order == 0:
            d2 = (G[1, 1] * nu[0] * nu[0] - D(2) * G[0, 1] * nu[0] * nu[1] + G[0, 0] * nu[1] * nu[1]) / det
        else:
            d2 = nu @ (np.array([[G[1, 1], -G[0, 1]], [-G[0, 1], G[0, 0]]], dtype=D) / det @ nu)
        return nu, S, d2

    def _update(self, x, P, nu, S):
        D = self.D
        det = S[0, 0] * S[1, 1] - S[0, 1] * S[0, 1]
        Sinv = np.array([[S[1, 1], -S[0, 1]], [-S[0, 1], S[0, 0]]], dtype=D) / det
        if self.order == 0:
            K = (P[:, :2] @ np.array([[S[1, 1], -S[0, 1]], [-S[0, 1], S[0, 0]]], dtype=D)) / det
            Pn = P - (K @ S) @ K.T
        else:
            K = P[:, :2] @ Sinv
            Pn = P - K @ P[:2, :]
        xn = x + K @ nu
        xn[1] = wrap(xn[1], self.nd)
        Pn = np.triu(Pn) + np.triu(Pn, 1).T
        return xn, Pn

    # ---- a line ----
    def line(self, det, count, aux=None):
        """det [K][8], count, aux [K][2] or None -> (trk [T][16] float64, ntrk [4], margin)"""
        D, q, nd, R, T = self.D, self.q, self.nd, self.R, self.q.T
        K = len(det)
        nm = min(max(int(count), 0), K)
        meas = {}
        for j in range(nm):
            rec = det[j]
            if is_measurement(rec, nd, R):
                z = np.array([D(np.float64(rec[0])) + D(np.float64(rec[5])), D(np.float64(rec[1])) + D(np.float64(rec[6]))], dtype=D)
                meas[j] = (z, np.float32(rec[2]), np.float32(rec[3]), (np.float32(-1), np.float32(-1)) if aux is None else (np.float32(aux[j][0]), np.float32(aux[j][1])))
        was_free = [t is None for t in self.slots]
        reported, slot_of = [FREE if t is None else t.status for t in self.slots], [-1] * T
        margin = np.inf

        # 1, 2: predict, range exit
        pred = {}
        for i, t in enumerate(self.slots):
            if t is None:
                continue
            x, P = self._predict(t)
            if x[0] < -1 or x[0] > R:
                t.x, t.P, t.d2, t.status = x, P, D(0), ENDED
                reported[i] = ENDED
                continue
            pred[i] = (x, P)
        # 3: gate
        cand, inno = {}, {}
        for i, (x, P) in pred.items():
            for j, (z, *_rest) in meas.items():
                nu, S, d2 = self._gate(x, P, z)
                margin = min(margin, abs(float(d2) - q.gate) / q.gate)
                if d2 <= q.gate:
                    cand[(i, j)], inno[(i, j)] = d2, (nu, S)
        # 4: the greedy walk in the strict order
        sign = -1 if self.mutate == "tie_reversed" else 1
        order = sorted(cand, key=lambda ij: (cand[ij], sign * ij[0], sign * ij[1]))
        track_free, meas_free, taken = set(pred), set(meas), {}
        for (i, j) in order:
            if i not in track_free or j not in meas_free:
                continue
            for (a, b), d in cand.items():
                if (a, b) == (i, j) or not ((a == i and b in meas_free) or (b == j and a in track_free)):
                    continue
                same = (a == i and np.array_equal(meas[b][0], meas[j][0])) or \
                       (b == j and np.array_equal(pred[a][0], pred[i][0]) and np.array_equal(pred[a][1], pred[i][1]))
                if not same:
                    top = max(float(d), float(cand[(i, j)]))
                    margin = min(margin, abs(float(d) - float(cand[(i, j)])) / top if top > 0 else 0.0)
            taken[i] = j
            track_free.discard(i)
            meas_free.discard(j)
        # 5, 6: update or coast, status
        mask = (1 << 32) - 1 if self.mutate == "hist_unmasked" else (1 << q.n) - 1
        for i, (x, P) in pred.items():
            t = self.slots[i]
            if i in taken:
                j = taken[i]
                nu, S = inno[(i, j)]
                t.x, t.P = self._update(x, P, nu, S)
                t.hits, t.hist = t.hits + 1, ((t.hist << 1) | 1) & 0xFFFFFFFF
                if self.mutate != "misses_kept":
                    t.misses = 0
                t.d2, t.power, t.snr, t.aux = cand[(i, j)], meas[j][1], meas[j][2], meas[j][3]
                slot_of[i] = j
            else:
                t.x, t.P = x, (P - np.diag(np.array([q.q_r, q.q_f, q.q_g], dtype=D)) if self.mutate == "coast_no_q" else P)
                t.misses, t.hist, t.d2 = t.misses + 1, (t.hist << 1) & 0xFFFFFFFF, D(0)
            t.age += 1
            if t.status == TENTATIVE:
                if bin(t.hist & mask).count("1") >= q.m:
                    t.status = CONFIRMED
                elif t.misses >= q.tent_miss or t.age >= q.n:
                    t.status = ENDED
            elif t.misses >= q.conf_miss:
                t.status = ENDED
            reported[i] = t.status
        # 7: initiate
        if self.mutate == "reuse_ended":
            was_free = [w or reported[i] == ENDED for i, w in enumerate(was_free)]
        free = [i for i in range(T) if was_free[i]]
        if self.mutate == "highest_slot":
            free.reverse()
        ninit = ndrop = 0
        for j in sorted(meas_free):
            if not free:
                ndrop += 1
                continue
            i = free.pop(0)
            z = meas[j][0]
            t = Track()
            t.x = np.array([z[0], wrap(z[1], nd), 0], dtype=D)
            t.P = np.diag(np.array([D(q.sigma_r) * D(q.sigma_r), D(q.sigma_f) * D(q.sigma_f), q.p0_g], dtype=D))
            t.d2, t.power, t.snr, t.aux = D(0), meas[j][1], meas[j][2], meas[j][3]
            t.id, t.status, t.age, t.hits, t.misses, t.hist = self.counter % ID_PERIOD + 1, TENTATIVE, 0, 1, 0, 1
            self.counter = (self.counter + 1) % ID_PERIOD
            self.slots[i], reported[i], slot_of[i] = t, TENTATIVE, j
            ninit += 1
        # the records
        trk = np.zeros((T, 16), dtype=np.float64 if D is np.float32 else D)
        for i, t in enumerate(self.slots):
            if t is None or reported[i] == FREE:
                continue
            trk[i] = [t.id, reported[i], t.x[0], t.x[1], t.x[2], np.sqrt(t.P[0, 0]), np.sqrt(t.P[1, 1]), t.age, t.hits, t.misses, slot_of[i],
                      t.d2 if slot_of[i] >= 0 else 0, t.power, t.snr, t.aux[0], t.aux[1]]
            if reported[i] == ENDED:
                self.slots[i] = None
        live = sum(r in (TENTATIVE, CONFIRMED) for r in reported)
        return trk, np.array([live, reported.count(CONFIRMED), ninit, ndrop], dtype=np.int32), margin


def run(q, det, count, aux=None, nd=ND, R=R, tracker=None, counter=0, **kw):
    """every line of det [L][K][8], count [L] (aux [L][K][2] or None) -> trk [L][T][16], ntrk [L][4], margin [L], the tracker.
    counter: the ids issued before the first line (a new tracker only)"""
    tr = tracker or Tracker(q, nd, R, **kw)
    if tracker is None:
        tr.counter = counter % ID_PERIOD
    out = [tr.line(det[k], count[k], None if aux is None else aux[k]) for k in range(len(det))]
    return np.array([o[0] for o in out]), np.array([o[1] for o in out]), np.array([o[2] for o in out]), tr


def restated(q, det, count, aux=None, nd=ND, R=R):
    return run(q, det, count, aux, nd, R, dtype=np.longdouble, order=1)


def single(q, det, count, aux=None, nd=ND, R=R):
    return run(q, det, count, aux, nd, R, dtype=np.float32, order=0)


INTS = (0, 1, 7, 8, 9, 10)          # id, status, age, hits, misses, slot
FLOATS = (2, 3, 4, 5, 6)            # r, f, g, sqrt(P00), sqrt(P11): held to the bar; d2 (11) is a ratio of them and is not
COPIED = (12, 13, 14, 15)           # power, snr, aux: copied


def figure_error(got, want, nd=ND):
    """|got - want| of the five figures, f modulo nd"""
    e = np.abs(np.asarray(got, dtype=np.longdouble)[..., FLOATS] - np.asarray(want, dtype=np.longdouble)[..., FLOATS])
    e[..., 1] = np.minimum(e[..., 1], np.abs(nd - e[..., 1]))
    return e.astype(np.float64)


def same_decisions(a, b, na, nb):
    return a.shape == b.shape and np.array_equal(np.asarray(a)[..., INTS].astype(np.int64), np.asarray(b)[..., INTS].astype(np.int64)) and np.array_equal(na, nb)


def hold(got, ngot, want, wn, tag="", nd=ND):
    """a device's or the host program's records against the model's: ids, statuses, ages, hits, misses, slots and counts equal; r, f, g
    and the two deviations within BAR plus half an fp32 ulp (the record's one rounding); power, snr and the auxiliary pair copied; free
    slots all zero; d2, a ratio of the figures, to a part in a million"""
    assert same_decisions(got, want, ngot, wn), tag
    allow = BAR + 0.5 * np.spacing(np.abs(want[..., FLOATS]).astype(np.float32)).astype(np.float64)
    err = figure_error(got, want, nd)
    assert np.all(err <= allow), (tag, float(np.max(err / allow)))
    assert np.array_equal(got[..., COPIED], want[..., COPIED].astype(np.float32)), tag
    assert not got[want[..., 1] == 0].any(), tag
    d2 = np.abs(got[..., 11].astype(np.float64) - want[..., 11].astype(np.float64))
    assert np.all(d2 <= 1e-6 * np.maximum(np.abs(want[..., 11].astype(np.float64)), 1e-6)), tag
    return float(np.max(err / allow, initial=0.0))


def deviation(q, det, count, aux=None, nd=ND, R=R):
    """the largest deviation of the five figures between the model and restated(); the decisions must agree"""
    a, na, _, _ = run(q, det, count, aux, nd, R)
    b, nb, _, _ = restated(q, det, count, aux, nd, R)
    assert same_decisions(a, b, na, nb)
    return float(np.max(figure_error(a, b, nd), initial=0.0))


def rounds(cand):
    """the kernel's assignment on {(i, j): d2}: rounds of "take every candidate that is the first of its row and of its column among
    the free ones" under (d2, i, j); returns {i: j}"""
    taken, rows, cols = {}, {i for i, _ in cand}, {j for _, j in cand}
    while True:
        free = {ij: d for ij, d in cand.items() if ij[0] in rows and ij[1] in cols}
        rb, cb = {}, {}
        for (i, j), d in sorted(free.items(), key=lambda kv: (kv[1], kv[0][0], kv[0][1])):
            rb.setdefault(i, j)
            cb.setdefault(j, i)
        hit = [(i, j) for i, j in rb.items() if cb[j] == i]
        if not hit:
            return taken
        for i, j in hit:
            taken[i] = j
            rows.discard(i)
            cols.discard(j)


def greedy(cand):
    """the definition: the walk over the candidates sorted by (d2, i, j)"""
    taken, cols = {}, set()
    for (i, j) in sorted(cand, key=lambda ij: (cand[ij], ij[0], ij[1])):
        if i not in taken and j not in cols:
            taken[i] = j
            cols.add(j)
    return taken


# ---- scenes ----
def record(r, f, power=10.0, snr=20.0, nd=ND):
    """the detection record of a measurement at (r, f): lag, doppler, power, snr, noise, dlag, ddop, ntrain"""
    lag, dop = np.floor(r + 0.5), np.floor(f + 0.5)
    dlag, ddop = np.float32(r - lag), np.float32(f - dop)
    if dop >= nd // 2:
        dop -= nd
    if dop < -(nd // 2):
        dop += nd
    return np.array([lag, dop, power, snr, power / snr, dlag, ddop, 40.0], dtype=np.float32)


def lists(lines, K):
    """lines: per line a list of records (more than K: count says so, the first K are kept) -> det [L][K][8], count [L]"""
    det, count = np.zeros((len(lines), K, 8), dtype=np.float32), np.zeros(len(lines), dtype=np.int32)
    for k, recs in enumerate(lines):
        count[k] = len(recs)
        for j, rec in enumerate(recs[:K]):
            det[k, j] = rec
    return det, count


def target(r0, f0, g, L, coupling=0.0, nd=ND):
    """the truth of a target of constant Doppler rate: [(r, f)] per line, f unwrapped"""
    out, r, f = [], r0, f0
    for _ in range(L):
        out.append((r, f))
        r, f = r + coupling * (f + g / 2), f + g
    return out


def _noisy(path, rng, s=0.05):
    return [(r + s * rng.standard_normal(), f + s * rng.standard_normal()) for r, f in path]


def _scene_constant():
    q = Desc(4, coupling=0.05)
    path = target(4.0, -3.0, 0.5, 12, q.coupling)
    return q, *lists([[record(r, f)] for r, f in path], 3), None


def _scene_crossing():
    rng = np.random.default_rng(11)
    q = Desc(4)
    a, b = _noisy(target(4.0, -4.0, 1.0, 10), rng), _noisy(target(9.0, 5.0, -1.0, 10), rng)
    return q, *lists([[record(*pa, power=9.0), record(*pb, power=7.0)] for pa, pb in zip(a, b)], 3), None


COAST_MISSED = (6, 7, 8)


def _scene_coast():
    """confirmed by line 2, lines 6 .. 8 missed and coasted through, re-acquired at 9, gone from 13: four misses end it at line 16, where a
    new detection elsewhere arrives: slot 0 is reported ended, the newcomer takes slot 1"""
    rng = np.random.default_rng(12)
    q = Desc(3, q_f=2e-2, q_r=2e-2)
    path = _noisy(target(5.0, -2.0, 0.25, 13), rng)
    lines = [[] if k in COAST_MISSED else [record(*p)] for k, p in enumerate(path)] + [[], [], [], [record(12.0, 6.0)], [record(12.0, 6.0)]]
    return q, *lists(lines, 2), None


def _scene_wrap():
    rng = np.random.default_rng(13)
    q = Desc(2)
    up, down = _noisy(target(6.0, 5.25, 0.75, 10), rng), _noisy(target(11.0, -5.25, -0.75, 10), rng)
    return q, *lists([[record(*pa), record(*pb)] for pa, pb in zip(up, down)], 2), None


def _scene_full():
    """five detections a line on two slots: the table is full from line 0 on, the rest is dropped and counted"""
    q = Desc(2)
    cells = [(2.0, -6.0), (5.0, -2.0), (8.0, 1.0), (11.0, 4.0), (14.0, 7.0)]
    return q, *lists([[record(r, f + 0.1 * k) for r, f in cells] for k in range(4)], 8), None


def _scene_tie():
    """two bitwise-equal measurements against one track: the lower slot is taken and the other initiates; then both coast (another
    detection there would be at d2 = 0 from both tracks, which no rule but the order separates)"""
    q = Desc(3)
    one = record(7.25, 3.5)
    aux = np.zeros((4, 2, 2), dtype=np.float32)
    aux[:, 0], aux[:, 1] = (3.0, 4.0), (5.0, 6.0)
    return q, *lists([[one], [one, one], [], []], 2), aux


def _scene_gate_s():
    """line 1 lies 1.2 cells off in lag: d2 = 2.9 under S, 5.7 under P' alone, and the gate is 4"""
    q = Desc(3, gate=4.0)
    return q, *lists([[record(5.0, 2.0)], [record(6.2, 2.0)], [record(6.2, 2.0)], [record(6.2, 2.0)]], 2), None


def _scene_history():
    """hits at lines 0, 2, 5 of a 3-of-5 rule: three hits in six lines, two in the last five, so the track ends unconfirmed at age 5"""
    q = Desc(2, tent_miss=4)
    one = record(8.0, -1.0)
    return q, *lists([[one], [], [one], [], [], [one], []], 2), None


def _scene_exit():
    """coupled targets that leave the map at either end: predicted r below -1 and above R"""
    q = Desc(4, coupling=0.5)
    lo, hi = target(2.0, -3.0, 0.0, 3, q.coupling), target(14.0, 3.0, 0.0, 3, q.coupling)
    return q, *lists([[record(*a), record(*b)] for a, b in zip(lo, hi)] + [[]] * 3, 4), None


def _scene_outside():
    """a slot whose lag or Doppler lies outside the map is no measurement; count above K; a negative count"""
    q = Desc(3)
    bad_lag, bad_dop = record(5.0, 1.0), record(6.0, 2.0)
    bad_lag[0], bad_dop[1] = 16.0, 8.0
    det, count = lists([[bad_lag, record(3.0, 3.0), bad_dop], [record(3.0, 3.0)] * 1, [record(3.0, 3.0), record(9.0, -4.0), record(1.0, 1.0), record(2.0, 2.0)], []], 3)
    count[3] = -2
    return q, det, count, None


def _scene_notfinite():
    """a slot whose dlag or ddop is not finite is no measurement either: it is not assigned, starts nothing and is not counted as dropped"""
    q = Desc(3)
    nan_lag, inf_dop, good = record(5.0, 1.0), record(9.0, -3.0), record(3.0, 3.0)
    nan_lag[5], inf_dop[6] = np.nan, -np.inf
    return q, *lists([[nan_lag, good, inf_dop], [inf_dop, nan_lag, good], [good, nan_lag], [nan_lag]], 3), None


# the ids issued before the first line in the tests of the counter's wrap: the next three are 2^24 - 2, 2^24 - 1 and 1
WRAP_COUNTER, WRAP_SCENE = ID_PERIOD - 2, "fill"
CLUTTER_SEED = 2024


def _scene_clutter():
    """a planted target among uniform false alarms over the 16 x 16 cells (one a line on average, a rate of 4e-3 a cell), 32 lines, 3-of-5, seed 2024: the
    confirmed tracks are exactly the planted one (checked in test_caf_track_model.py)"""
    rng = np.random.default_rng(CLUTTER_SEED)
    q = Desc(16, gate=6.0, sigma_r=0.3, sigma_f=0.3, p0_g=0.1)
    path = _noisy(target(3.0, -6.0, 0.3, 32, 0.0), rng, 0.1)
    lines = []
    for p in path:
        recs = [record(*p, power=30.0)] + [record(rng.uniform(-0.49, 15.49), rng.uniform(-8.0, 7.49), power=rng.uniform(5.0, 8.0)) for _ in range(rng.poisson(1.0))]
        lines.append([recs[k] for k in rng.permutation(len(recs))])
    return q, *lists(lines, 8), None


def _scene_sizes(T, K, seed):
    """8 lines for the per-op sizes: min(T, K, 6) targets on their own lag rows and uniform false alarms up to K a line"""
    rng = np.random.default_rng(seed)
    q = Desc(T, gate=6.0, sigma_r=0.3, sigma_f=0.3, p0_g=0.1, tent_miss=3)
    nt = min(T, K, 6)
    paths = [_noisy(target(1.0 + 2.5 * a, rng.uniform(-7, 7), rng.uniform(-0.6, 0.6), 8), rng, 0.1) for a in range(nt)]
    lines = []
    for k in range(8):
        recs = [record(*p[k], power=30.0 - a) for a, p in enumerate(paths) if rng.uniform() > 0.15]
        recs += [record(rng.uniform(-0.49, 15.49), rng.uniform(-8.0, 7.49), power=rng.uniform(5.0, 8.0)) for _ in range(min(rng.poisson(K / 4), K - len(recs)))]
        lines.append([recs[i] for i in rng.permutation(len(recs))])
    det, count = lists(lines, K)
    aux = rng.integers(0, 100, size=(8, K, 2)).astype(np.float32)
    return q, det, count, aux


SIZES = [(T, K) for T in (1, 2, 63, 64, 65, 128) for K in (1, 3, 64)]


def _scene_fill():
    """a table of three slots that fills at line 2: one, two, then four detections a line"""
    q = Desc(3)
    cells = [(2.0, -6.0), (6.0, -1.0), (10.0, 3.0), (14.0, 6.0)]
    return q, *lists([[record(*c) for c in cells[:n]] for n in (1, 2, 4, 4, 4, 4, 4, 4)], 4), None


def _scene_empty():
    q = Desc(5)
    return q, np.zeros((8, 3, 8), dtype=np.float32), np.zeros(8, dtype=np.int32), None


def _scene_cuts():
    """12 lines for the cuts: two targets, a miss each, a false alarm"""
    rng = np.random.default_rng(14)
    q = Desc(4)
    a, b = _noisy(target(3.0, -5.0, 0.5, 12), rng), _noisy(target(12.0, 4.0, -0.25, 12), rng)
    lines = [[record(*pa)] * (k != 4) + [record(*pb)] * (k != 7) + [record(8.0, 0.0)] * (k == 5) for k, (pa, pb) in enumerate(zip(a, b))]
    return q, *lists(lines, 3), None


_BUILD = {"constant": _scene_constant, "crossing": _scene_crossing, "coast": _scene_coast, "wrap": _scene_wrap, "full": _scene_full, "tie": _scene_tie,
          "gate_s": _scene_gate_s, "history": _scene_history, "exit": _scene_exit, "outside": _scene_outside, "notfinite": _scene_notfinite, "clutter": _scene_clutter, "fill": _scene_fill,
          "empty": _scene_empty, "cuts": _scene_cuts}
_BUILD.update({f"size_{T}_{K}": (lambda T=T, K=K: _scene_sizes(T, K, 1000 + 7 * T + K)) for T, K in SIZES})
SCENE_NAMES = tuple(_BUILD)
_CACHE = {}


def scene(name):
    """(q, det, count, aux) of a named scene; built once, never changed"""
    if name not in _CACHE:
        q, det, count, aux = _BUILD[name]()
        for a in (det, count, aux):
            if a is not None:
                a.setflags(write=False)
        _CACHE[name] = (q, det, count, aux)
    return _CACHE[name]


_WANT = {}


def expected(name):
    """the model's (trk, ntrk, margin) of a named scene; computed once and shared"""
    if name not in _WANT:
        q, det, count, aux = scene(name)
        _WANT[name] = run(q, det, count, aux)[:3]
    return _WANT[name]


def compositions(n):
    """every cut of n lines into consecutive submits"""
    for bits in itertools.product((0, 1), repeat=n - 1):
        cut, last = [], 0
        for k, b in enumerate(bits, 1):
            if b:
                cut.append((last, k))
                last = k
        yield cut + [(last, n)]
