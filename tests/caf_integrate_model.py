"""fp64 numpy statement of crsdr_caf's integration across lines (include/crsdr.h, section (w), "Integration across lines";
crsdr_caf_set_integrate, crsdr_map_integrate): the header's four sentences taken literally.  caf_model.py's signed bin s(d) is imported.

State: I [nd][R] in fp64 and the counter m, lines since the last reset; empty is all zero and m = 0.  Per line, in this order:

 1. delta(d) = c * s(d), one multiplication;  o(m, d) = floor(m * delta(d) + 0.5), one multiplication and one addition;
    D(d) = o(m, d) - o(m - 1, d) for m >= 1, D = 0 at m = 0.
 2. I'[d][tau] = I[d][min(max(tau - D(d), 0), R - 1)]: whole cells, clamped, no arithmetic on the values, no wrap.
 3. lambda = max(a, 1 / (m + 1));  diff = P - I',  t = lambda * diff,  I = I' + t: three fp64 operations, each rounded on its own.
 4. imap = float32(I), rounded once;  m + 1.

numpy does not contract a multiplication and an addition of two array expressions into one operation, and neither may the device or
the host header: the device's imap and its final state are therefore held against this model BYTE FOR BYTE, with no bar at all.

The state buffer is the device's: a 16-byte header (int64 m, int64 0) and the doubles of every map.

`which` names one mistake at a time (MUTATIONS), for the tests that show each of them is caught."""
import numpy as np

import caf_model as M

MUTATIONS = ["shift_sign", "truncate", "unsigned_bin", "no_warmup", "zeros_at_edges", "lag_wrap", "float32_state", "update_first"]
HEADER_BYTES = 16


def offsets(m, coupling, nd, which=None):
    """o(m, d) of every bin, int64 [nd]"""
    s = np.arange(nd, dtype=np.float64) if which == "unsigned_bin" else M.signed_bins(nd).astype(np.float64)
    delta = np.float64(coupling) * s
    x = np.float64(m) * delta
    return (np.trunc(x) if which == "truncate" else np.floor(x + 0.5)).astype(np.int64)


def steps(m, coupling, nd, which=None):
    """D(d) of line m, int64 [nd]"""
    if m < 1:
        return np.zeros(nd, dtype=np.int64)
    D = offsets(m, coupling, nd, which) - offsets(m - 1, coupling, nd, which)
    return -D if which == "shift_sign" else D


def lam(m, forget, which=None):
    return np.float64(forget) if which == "no_warmup" else max(np.float64(forget), np.float64(1.0) / np.float64(m + 1))


def shift(I, D, which=None):
    """I'[d][tau] = I[d][clamp(tau - D(d))]"""
    nd, R = I.shape
    src = np.arange(R, dtype=np.int64)[None, :] - D[:, None]
    rows = np.arange(nd)[:, None]
    if which == "lag_wrap":
        return I[rows, src % R]
    out = I[rows, np.clip(src, 0, R - 1)]
    if which == "zeros_at_edges":
        out = np.where((src < 0) | (src >= R), 0.0, out)
    return out


class Integrator:
    """one map's state; line(P) -> imap float32 [nd][R]"""

    def __init__(self, nd, R, forget, coupling, which=None):
        self.nd, self.R, self.forget, self.coupling, self.which = int(nd), int(R), float(forget), float(coupling), which
        self.I = np.zeros((self.nd, self.R), dtype=np.float32 if which == "float32_state" else np.float64)
        self.m = 0

    def line(self, P):
        P = np.asarray(P, dtype=np.float32).astype(np.float64)
        w, dt = self.which, self.I.dtype
        l = lam(self.m, self.forget, w)
        D = steps(self.m, self.coupling, self.nd, w)
        if w == "update_first":
            diff = P - self.I
            t = l * diff
            self.I = shift(self.I + t, D, w)
        else:
            Is = shift(self.I, D, w)
            diff = P - Is
            t = l * diff
            self.I = (Is + t).astype(dt)
        self.m += 1
        return self.I.astype(np.float32)


def run(maps, forget, coupling, which=None, state=None):
    """maps [nlines][nmaps][nd][R] float32 -> (imap of the same shape, the state buffer behind the last line as uint8).  state: a buffer an
    earlier run returned, or None for the empty state"""
    maps = np.asarray(maps, dtype=np.float32)
    L, nmaps, nd, R = maps.shape
    its = [Integrator(nd, R, forget, coupling, which) for _ in range(nmaps)]
    if state is not None:
        raw = np.asarray(state, dtype=np.uint8)
        m = int(raw[:8].view("<i8")[0])
        body = raw[HEADER_BYTES:].view(np.float64).reshape(nmaps, nd, R)
        for k, it in enumerate(its):
            it.m, it.I = m, body[k].copy()
    out = np.zeros(maps.shape, dtype=np.float32)
    for l in range(L):
        for k, it in enumerate(its):
            out[l, k] = it.line(maps[l, k])
    return out, pack_state(its)


def pack_state(its):
    header = np.array([its[0].m, 0], dtype="<i8").view(np.uint8)
    return np.concatenate([header] + [it.I.astype(np.float64).reshape(-1).view(np.uint8) for it in its])


def offset_by_integers(m, num, log2den, s):
    """o(m, d) for the dyadic coupling num / 2^log2den, in integers alone: floor(m num s / 2^k + 1 / 2) = (2 m num s + 2^k) >> (k + 1)"""
    return (2 * m * num * s + (1 << log2den)) >> (log2den + 1)


# ---- the scene of the issue: a weak echo that walks along the lags, found only behind the integration ----
NLINES, ND, R, NROWS = 32, 64, 48, 3
ECHO, WALK, FORGET, COUPLING, WARM = 2.5, 0.05, 1.0 / 8.0, 0.05, 8
CASES = [(20, 4), (13, 4), (-27, 44)]          # (signed Doppler bin, the lag of line 0)
SEEDS = [0, 1, 2]


def scene(seed, sd, lag0, echo=True):
    """(maps [32][64][48] float32, the echo's (d, lag) per line)"""
    rng = np.random.default_rng(seed)
    z = (rng.standard_normal((NLINES, NROWS, ND, R)) + 1j * rng.standard_normal((NLINES, NROWS, ND, R))) / np.sqrt(2.0)
    cells = []
    for m in range(NLINES):
        lag = int(np.floor(lag0 + m * WALK * sd + 0.5))
        phase = rng.random(NROWS)
        if echo:
            z[m, :, sd % ND, lag] += np.sqrt(ECHO) * np.exp(2j * np.pi * phase)
        cells.append((sd % ND, lag))
    return (np.abs(z) ** 2).sum(axis=1).astype(np.float32), cells
