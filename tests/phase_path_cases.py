"""Inputs of the phase-path tests -- TEST INFRASTRUCTURE ONLY (tests/test_phase_path_model.py, tests/test_gpu_phase_path.py).

K2's shift comes from K1, so a test cannot set it: it STEERS it.  A steering block's reference row is low-level noise with one
full-scale marker sample at n0; a steered signal row is that row delayed by its shift d on the overlap (the marker lands at
n0 + d) and holds independent, never-zero values outside it: they must not reach the output, and every one that does is visible
there.  K1 then reports lag = d -- the marker's product dominates every other lag: tests/test_phase_path_model.py holds the
peak-to-runner-up power ratio of the fp64 correlation at >= 4 for every (L, d) used here -- and K2 shifts by it.  The delayed copy
is turned by a multiple of 90 degrees that changes with the row and the block (exact in int8), so the unit phasor of a steering
block is one of 1, -j, -1, j and the chain moves in tracked batches as well.

All rows of a block share ONE reference row, and both markers must lie inside the row: n0 in [max(0, -d), min(L, L - d)).  No n0
serves d = L - 1 (n0 = 0 only) and d = -(L - 1) (n0 = L - 1 only) at once, so a plan whose shift set spans both is steered by TWO
submits: the rows with d >= 0 through the lag mask with the marker at n0 = 0, then the rows with d < 0 with the marker at L - 1.
A row that is not selected keeps its carried lag (K1 republishes it), holds low-level noise of its own and is shifted by that lag.

The carried lags then shift the LOCKED blocks (CRSDR_NO_LAG), which hold full-scale random int8 in every row, -128 and 127
included, uncorrelated with the reference row: one wrong sample in the dot product moves the phasor by about 1e-2 rad.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

FILL = 4                    # steering rows: fill values in [-FILL, FILL]
MARKER = (127, -127)        # the full-scale marker sample (I, Q)


def shift_set(L: int) -> list:
    """The shifts the rows of a plan are steered to, one row each: every one for L <= 64; for longer rows every residue mod 8
    with both signs, odd and even, a straddling 16-byte vector at each end of the row, half the row and the last lag."""
    if L <= 64:
        return list(range(-(L - 1), L))
    mags = list(range(1, 10)) + [15, 16, 17, L // 2, L // 2 - 1, L - 9, L - 8, L - 7, L - 1]
    return [0] + [s * m for m in mags for s in (1, -1)]


def marker_position(L: int, shifts) -> int:
    """n0 that keeps both markers inside [0, L) for every shift of the group (the middle of the feasible range), or -1."""
    lo = max([0] + [-int(d) for d in shifts])
    hi = min([L] + [L - int(d) for d in shifts])
    return (lo + hi) // 2 if hi - lo > 1 else (lo if hi > lo else -1)


def _nonzero_fill(rng, n):
    return (rng.integers(1, FILL + 1, size=n) * rng.choice([-1, 1], size=n)).astype(np.int8)


def steering_block(L: int, shifts, select, seed: int, t: int = 0) -> np.ndarray:
    """int8 [1 + len(shifts)][2 L]: the reference row and one signal row per shift; rows with select[k] true are steered."""
    shifts = [int(d) for d in shifts]
    rng = np.random.default_rng([seed, L, t, 1])
    n0 = marker_position(L, [d for d, s in zip(shifts, select) if s])
    assert n0 >= 0, "no marker position serves every selected shift"
    ref = rng.integers(-FILL, FILL + 1, size=(L, 2)).astype(np.int8)
    ref[n0] = MARKER
    rows = np.empty((1 + len(shifts), L, 2), dtype=np.int8)
    rows[0] = ref
    for k, (d, sel) in enumerate(zip(shifts, select)):
        row = _nonzero_fill(rng, 2 * L).reshape(L, 2)            # outside the overlap / a row that is not steered
        if sel:
            lo, hi = max(0, d), min(L, L + d)                    # s[n] = r[n - d] on the overlap ...
            seg = ref[lo - d:hi - d]
            for _ in range((k + t) % 4):                         # ... times j^(k + t), exactly: (I, Q) -> (-Q, I).  The lag and the
                seg = np.stack([-seg[:, 1], seg[:, 0]], axis=1)  # peak's size stay; the unit phasor is conj(j^(k + t)) and changes
            row[lo:hi] = seg                                     # from block to block, so the chain moves in tracked batches too
        rows[1 + k] = row
    return rows.reshape(1 + len(shifts), 2 * L)


def fullscale_block(nrows: int, B: int, seed: int, t: int = 0) -> np.ndarray:
    """int8 [nrows][B] uniform over all 256 values in every row, the reference row included."""
    rng = np.random.default_rng([seed, B, t, 2])
    return rng.integers(-128, 128, size=(nrows, B)).astype(np.int8)


@dataclass
class Submit:
    kind: str                       # "steer" (K1 runs, lag mask below) or "locked" (CRSDR_NO_LAG)
    rows: np.ndarray                # int8 [T][nrows][B], signed
    lag_mask: np.ndarray | None     # uint8 [nrows] or None (every row)
    lag: np.ndarray                 # int64 [T][nrows]: the lag every row of every block is shifted by (and K1 / the plan reports)
    seq: int
    refnoise: bool = True
    steered: list = field(default_factory=list)      # rows (indices) K1 measures in this submit


@dataclass(frozen=True)
class Case:
    name: str
    B: int
    shifts: tuple | None = None     # None: shift_set(L)
    T: int = 1                      # blocks per submit (max_batch)
    locked: int = 1                 # locked submits behind the steering ones
    offset_binary: bool = False
    seed: int = 20
    variant: str = ""               # "", or a chain case: "chain", "chain_zeroed", "chain_refnoise_off" (chain_submits)

    @property
    def L(self):
        return self.B // 2

    @property
    def shift_list(self):
        return list(self.shifts) if self.shifts is not None else shift_set(self.L)

    @property
    def nrows(self):
        return 1 + len(self.shift_list)


def steering_groups(L: int, shifts) -> list:
    """The shifts split into groups that one marker position serves: all of them, or d >= 0 and d < 0."""
    if marker_position(L, shifts) >= 0:
        return [[True] * len(shifts)]
    return [[d >= 0 for d in shifts], [d < 0 for d in shifts]]


def _steer(case, select, carried, seed, seq):
    rows = np.stack([steering_block(case.L, case.shift_list, select, seed, t) for t in range(case.T)])
    for k, s in enumerate(select):
        if s:
            carried[1 + k] = case.shift_list[k]
    mask = None if all(select) else np.array([0] + [int(s) for s in select], dtype=np.uint8)
    return Submit("steer", rows, mask, np.tile(carried, (case.T, 1)), seq, steered=[1 + k for k, s in enumerate(select) if s])


def _locked(case, carried, seed, seq, refnoise=True):
    rows = np.stack([fullscale_block(case.nrows, case.B, seed, t) for t in range(case.T)])
    return Submit("locked", rows, None, np.tile(carried, (case.T, 1)), seq, refnoise=refnoise)


def submits(case: Case) -> list:
    """The submits of a case, in order: its steering submits, then case.locked locked ones."""
    if case.variant:
        return chain_submits(case)
    carried = np.zeros(case.nrows, dtype=np.int64)
    out, seq = [], 100
    for g, select in enumerate(steering_groups(case.L, case.shift_list)):
        out.append(_steer(case, select, carried, case.seed + 7 * g, seq))
        seq += case.T
    for j in range(case.locked):
        out.append(_locked(case, carried, case.seed + 1000 + j, seq))
        seq += case.T
    return out


def chain_submits(case: Case) -> list:
    """The chain cases: two tracked batches of T blocks and locked ones behind them, the phasor carried across all submits.
    chain_zeroed: in the second batch row 1 is zero in block T // 3 and row 3 in the LAST block.  A zero row reports lag = -L
    (the first index of an all-zero correlation) and holds its phasor; row 3 carries lag = -L into the locked batch, whose
    non-zero rows are then shifted out entirely: the output row is all zero and the phasor is held through the batch.
    chain_refnoise_off: the second tracked batch and the first locked one run with the reference noise off (phasor frozen, the
    rotation still applied), a last locked batch takes the chain up again from the frozen value."""
    L, T = case.L, case.T
    select = [True] * len(case.shift_list)
    carried = np.zeros(case.nrows, dtype=np.int64)
    off = case.variant == "chain_refnoise_off"
    a = _steer(case, select, carried, case.seed, 100)
    b = _steer(case, select, carried, case.seed + 7, 100 + T)
    b.refnoise = not off
    if case.variant == "chain_zeroed":
        for t, r in ((T // 3, 1), (T - 1, 3)):
            b.rows[t, r] = 0
            b.lag[t, r] = -L
        carried[3] = -L
    out = [a, b, _locked(case, carried, case.seed + 1000, 100 + 2 * T, refnoise=not off)]
    if off:
        out.append(_locked(case, carried, case.seed + 1001, 100 + 3 * T))
    return out


def readcnt_for(sub: Submit) -> np.ndarray:
    """uint32 [T][nrows] read counters of a submit: distinct words, so a header word read from the wrong place shows."""
    T, n = sub.rows.shape[:2]
    return (np.uint32(0x01000000) * np.uint32(1 + sub.seq % 64) + np.arange(T * n, dtype=np.uint32).reshape(T, n) * np.uint32(3)).astype(np.uint32)


def run_plan(b, case: Case, in_off=None) -> list:
    """The case on the device: one digital-mode plan, every submit of the case, every block fetched.  b: the binding module.
    in_off: None submits host rows; a byte offset submits caller-owned device memory at (16-byte boundary + in_off), with a block
    stride larger than one block -- in_off = 4 is word-aligned only and takes the word kernels.
    Returns one fetch dict per block, in order."""
    n, B, T = case.nrows, case.B, case.T
    plan = b.Plan(n, B, b.MODE_DIGITAL, max_batch=T)
    assert plan.matrix_offset == 16 + 4 * n and plan.packet_bytes == 16 + 4 * n + n * B
    res = []
    for sub in submits(case):
        flags = (b.REFNOISE_ENABLED if sub.refnoise else 0) | (b.NO_LAG if sub.kind == "locked" else 0) | (b.OFFSET_BINARY if case.offset_binary else 0)
        rows = sub.rows.view(np.uint8) ^ np.uint8(0x80) if case.offset_binary else sub.rows
        kw = dict(readcnt=readcnt_for(sub), lag_mask=sub.lag_mask, seq=sub.seq, flags=flags)
        if in_off is None:
            plan.submit(rows, **kw)
        else:
            import torch
            dev = torch.device("cuda", 0)
            stride = n * B + 64
            raw = torch.zeros(T * stride + 64, dtype=torch.uint8, device=dev)
            base = (-raw.data_ptr()) % 16 + in_off
            for t in range(T):
                raw[base + t * stride: base + t * stride + n * B] = torch.from_numpy(np.ascontiguousarray(rows[t]).view(np.uint8).reshape(-1)).to(dev)
            torch.cuda.synchronize()
            plan.submit(raw.data_ptr() + base, nblocks=T, block_stride=stride, **kw)
            plan.sync()
        res += [plan.fetch(block=t) for t in range(T)]
        plan.sync()
    plan.close()
    return res


def model_results(case: Case) -> list:
    """What run_plan returns, from the exact model alone (the lags taken as the targets): the comparison's own known answer."""
    import phase_path_model as pm
    m = pm.PhasePathModel(case.nrows, case.B)
    res = []
    for sub in submits(case):
        rc = readcnt_for(sub)
        for t in range(case.T):
            e = m.block(sub.rows[t], lag=sub.lag[t] if sub.kind == "steer" else None, refnoise=sub.refnoise, seq=sub.seq + t, readcnt=rc[t])
            res.append(dict(lag=e["lag"].astype(np.int32), phasor=e["phasor"], packet=e["packet"], matrix=e["matrix"]))
    return res


def _ulps(a, e) -> int:
    """largest distance in float32 ulps between two complex64 arrays, component-wise"""
    def key(x):
        u = np.ascontiguousarray(x).view(np.uint32).astype(np.int64)
        return np.where(u & 0x80000000, -(u & 0x7FFFFFFF), u)
    return int(np.abs(key(a) - key(e)).max())


def compare(case: Case, res: list) -> None:
    """res: one fetch dict per block (run_plan) against the exact model.  The precondition -- the reported lags are the targets --
    is asserted at once; every other mismatch is collected and reported by kind:
      phasor   bit for bit against the model's chain;
      given    matrix byte for byte against the model fed the DEVICE's phasor bits: a shift / rotate / quantise defect alone;
      matrix   byte for byte with the model's own chain;
      header   hdr0, the readcnt words, and the reference row copied verbatim."""
    import phase_path_model as pm
    n, B, T = case.nrows, case.B, case.T
    own, given = pm.PhasePathModel(n, B), pm.PhasePathModel(n, B)
    subs = submits(case)
    assert len(res) == T * len(subs), (len(res), T, len(subs))
    bad, i = [], 0
    for s, sub in enumerate(subs):
        rc = readcnt_for(sub)
        rows = sub.rows.view(np.uint8) ^ np.uint8(0x80) if case.offset_binary else sub.rows
        for t in range(T):
            got = res[i]
            i += 1
            where = f"{case.name} submit {s} ({sub.kind}) block {t}"
            assert np.array_equal(got["lag"][1:], sub.lag[t, 1:]), f"{where}: PRECONDITION (K1 / input, not K2): lags {got['lag'][1:]} != {sub.lag[t, 1:]}"
            kw = dict(lag=sub.lag[t] if sub.kind == "steer" else None, refnoise=sub.refnoise, offset_binary=case.offset_binary,
                      seq=sub.seq + t, readcnt=rc[t])
            exp = own.block(rows[t], **kw)
            giv = given.block(rows[t], phasor=got["phasor"], **kw)
            gb, eb = pm.phasor_bits(got["phasor"][1:]), pm.phasor_bits(exp["phasor"][1:])
            if not np.array_equal(gb, eb):
                rws = 1 + np.flatnonzero(np.any(gb != eb, axis=-1))
                gp, ep = got["phasor"][rws], exp["phasor"][rws]
                bad.append(f"{where}: phasor differs in rows {rws[:8].tolist()} (shifts {[int(sub.lag[t, r]) for r in rws[:8]]}; {rws.size} rows), "
                           f"largest distance {_ulps(gp, ep)} ulp, {np.abs(np.angle(gp * np.conj(ep))).max():.3g} rad; "
                           f"got {gp[:2].tolist()} expected {ep[:2].tolist()}, integer sums {[exp['sums'][r] for r in rws[:2]]}")
            for name, e in (("given the device's phasor", giv), ("with the model's chain", exp)):
                if not np.array_equal(got["matrix"], e["matrix"]):
                    rws = np.flatnonzero(np.any(got["matrix"] != e["matrix"], axis=1))
                    r = int(rws[0])
                    cols = np.flatnonzero(got["matrix"][r] != e["matrix"][r])
                    bad.append(f"{where}: matrix {name} differs in rows {rws[:8].tolist()} ({rws.size} rows); row {r} (shift {int(sub.lag[t, r])}): "
                               f"{cols.size} bytes, samples {sorted(set((cols // 2).tolist()))[:12]}, got {got['matrix'][r][cols[:6]].tolist()} "
                               f"expected {e['matrix'][r][cols[:6]].tolist()}")
            mo = own.matrix_offset
            if not np.array_equal(got["packet"][:mo], exp["packet"][:mo]):
                bad.append(f"{where}: header {got['packet'][:mo].view(np.uint32).tolist()} != {exp['packet'][:mo].view(np.uint32).tolist()}")
            if got["packet"].size != exp["packet"].size or not np.array_equal(got["packet"][mo:mo + B], exp["packet"][mo:mo + B]):
                bad.append(f"{where}: the reference row is not copied verbatim")
        if len(bad) > 12:
            break
    assert not bad, "\n".join(bad)


def chain_properties(case: Case, res: list) -> None:
    """What the chain cases are for, asserted on the results themselves (beside the comparison with the model)."""
    T, L = case.T, case.L
    ph = np.stack([r["phasor"] for r in res])
    if case.variant == "chain":
        assert np.all(ph[1:, 1:] != ph[:-1, 1:])                       # the chain moved at every block, tracked and locked
    if case.variant == "chain_zeroed":
        t0 = T + T // 3
        assert res[t0]["lag"][1] == -L and ph[t0, 1] == ph[t0 - 1, 1] and not res[t0]["matrix"][1].any()
        assert ph[t0 + 1, 1] != ph[t0, 1] and ph[t0 - 1, 1] != ph[t0 - 2, 1]
        assert res[2 * T - 1]["lag"][3] == -L and ph[2 * T - 1, 3] == ph[2 * T - 2, 3]
        for r in res[2 * T:]:                                          # the locked batch: non-zero input, shifted out entirely
            assert r["lag"][3] == -L and not r["matrix"][3].any() and r["phasor"][3] == ph[2 * T - 1, 3]
            assert r["matrix"][1].any() and r["matrix"][2].any()
    if case.variant == "chain_refnoise_off":
        assert np.all(ph[T:3 * T, 1:] == ph[T - 1, 1:])                # frozen through the tracked and the locked batch ...
        assert all(r["matrix"][1:].any() for r in res[T:3 * T])        # ... while the rows are still rotated and published
        assert np.all(ph[3 * T:, 1:] != ph[3 * T - 1:-1, 1:])          # and taken up again from the frozen value


# ---- the cases of tests/test_gpu_phase_path.py; tests/test_phase_path_model.py checks the steering of every one ---------------

# in-process on the default (fused) path where rows are 16-byte aligned and B <= 16384; the three-kernel path for longer rows
PATH_CASES = [
    Case("fused_full_signed", 16384, T=2),                          # k_align_fused<true, false>
    Case("fused_full_offset_binary", 16384, T=2, offset_binary=True),   # k_align_fused<true, true>
    Case("fused_one_vector", 16, T=2),                              # <false, true>: one 16-byte vector in the whole row
    Case("fused_exhaustive", 128, T=2),                             # every shift of a 64-sample row
    Case("fused_exhaustive_offset_binary", 128, T=2, offset_binary=True),
    Case("fused_one_vector_per_thread", 4096, T=2),
    Case("fused_two_of_four_slots", 8192, T=2),
    Case("long_two_chunks", 1 << 15, locked=2),                     # k_phase_dot<true, 8> one z-slice, k_align_quant two, inline_chain
    Case("long_two_slices", 1 << 16, locked=2),                     # two z-slices: the atomic accumulation
]
# each environment in a fresh child process: the three-kernel path and the fused kernel's forced local fallback
CHILD_ENVS = {"three": {"CRSDR_K2_FUSED": "0"}, "fallback": {"CRSDR_K2_SPIN": "-1"}}
CHILD_CASES = [Case("child_full", 16384, T=3), Case("child_exhaustive", 128, T=3)]
# device input at a 4-byte offset: the word kernels (VEC = false)
WORD_CASES = [Case("word_exhaustive", 128, T=2), Case("word_full", 16384, T=2), Case("word_long", 1 << 15)]
# the chain: 3 signal rows at B = 1024, T = 64 = kMaxBatch, one marker position for all three shifts
CHAIN_SHIFTS = (7, -251, 256)         # odd with the row end, odd with the row start inside a vector, half the row
CHAIN_CASES = [Case(v, 1024, shifts=CHAIN_SHIFTS, T=64, variant=v) for v in ("chain", "chain_zeroed", "chain_refnoise_off")]

ALL_CASES = PATH_CASES + CHILD_CASES + WORD_CASES + CHAIN_CASES
