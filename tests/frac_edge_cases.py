"""Inputs, runners and the criterion of the fractional-delay edge tests -- TEST INFRASTRUCTURE ONLY
(tests/test_frac_delay_model.py on the CPU, tests/test_gpu_frac_edges.py on the device).

The submits are those of tests/phase_path_cases.py (steering blocks that put every row at a chosen lag in (-L, L), a zero row for
lag = -L, then locked full-scale blocks with -128 and 127 in every row), run on a digital-mode plan WITH the correction on.  Every
block is judged per sample against the unrounded fp64 model (tests/frac_delay_model.py) fed the block's own lag, phasor and D.

A FAMILY is a set of (case, setting) runs that reach one kernel.  Its bar is derived from the fp32 CPU reference alone:

    bar(row) = 4 * excess(oracle.Engine over the whole family) + [|D| > 1] * 2 pi |D| 2^-24 max|z_row|

(the kernels use other fp32 factorisations and a polynomial sine: the same order of error, not the same value; the second term is
the rounding of the fp32 phase argument, of size up to |D| / 2 turns, which the oracle -- it forms the ramp in double -- does not
show).  No bar may exceed MAX_BAR = 0.1 count: above that the criterion stops separating a wrong sample from a rounding.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

import frac_delay_model as fm
import phase_path_cases as pc

MAX_BAR = 0.1
MARGIN = 4.0
D_SET = (0.0, 0.25, -0.25, 0.3, -0.45, 0.5, -0.5, 1.0, -1.0, 7.3, -7.3, 64.0, -64.0)
GAINS = (1.0, 128.0, -128.0)


def d_vector(nrows: int) -> np.ndarray:
    """The override: D_SET cycled over the signal rows; entry 0 (the reference row) is garbage and must be ignored."""
    D = np.empty(nrows, dtype=np.float32)
    D[0] = 777.0
    D[1:] = [D_SET[k % len(D_SET)] for k in range(nrows - 1)]
    return D


@dataclass(frozen=True)
class Setting:
    gain: float = 1.0
    override: bool = True

    @property
    def name(self):
        return "override" if self.override else f"gain{self.gain:g}"

    def vector(self, nrows):
        return d_vector(nrows) if self.override else None


OVERRIDE = Setting()
SETTINGS = (OVERRIDE,) + tuple(Setting(g, False) for g in GAINS)


# ---- the steered cases --------------------------------------------------------------------------------------------------------
# generic LDS kernel k_frac_apply<LOG2N>: one, two, three and four passes of the radix-16 network (B = 16384 under CRSDR_FRAC_GENERIC=1)
GENERIC_CASES = [pc.Case(f"generic_{B}", B, T=2) for B in (16, 32, 64, 128, 256, 512, 4096, 8192)]
GENERIC14_CASE = pc.Case("generic_16384", 16384, T=2)
# k_frac_apply14: K1's 32 x 32 x 16 network
FAST14_CASES = [pc.Case("fast14_signed", 16384, T=2), pc.Case("fast14_offset_binary", 16384, T=2, offset_binary=True)]
# lag = -L rows with D != 0, a held phasor, a frozen phasor: three rows that one marker position serves
CHAIN_CASES = [pc.Case(f"{v}_{B}", B, shifts=s, T=4, variant=v) for B, s in ((128, (7, -27, 32)), (16384, (7, -251, 4096)))
               for v in ("chain_zeroed", "chain_refnoise_off")]
# long blocks, one line per workgroup: k_rows14_cf32p<false, true> (N1 * rows < 1024 lines)
LONG1_CASES = [pc.Case(f"long1_{B}", B, T=1) for B in (1 << 15, 1 << 16)]
# sharded plans: 16 signal rows, both signs, both ends of the row
def _shard_shifts(L):
    return (0, 1, -1, 2, -3, 5, -8, 17, -16, L // 2, -(L // 2), L - 8, -(L - 7), L - 1, -(L - 1), 9)
SHARD_CASES = [pc.Case(f"shard_{B}", B, shifts=_shard_shifts(B // 2), T=2) for B in (2048, 16384)]

# a family is a kernel: the chain cases belong to the kernel their block size takes
FAMILIES = {
    "generic": [(c, s) for c in GENERIC_CASES + [GENERIC14_CASE] + CHAIN_CASES[:2] for s in SETTINGS],
    "fast14": [(c, s) for c in FAST14_CASES + CHAIN_CASES[2:] for s in SETTINGS],
    "long1": [(c, s) for c in LONG1_CASES for s in SETTINGS],
}
STEERED_CASES = GENERIC_CASES + [GENERIC14_CASE] + FAST14_CASES + CHAIN_CASES + LONG1_CASES + SHARD_CASES


def family_of(case) -> str:
    for f, runs in FAMILIES.items():
        if any(c.name == case.name for c, _ in runs):
            return f
    raise KeyError(case.name)


# ---- the two-line long-block kernel: B = 2^18, 64 signal rows (N1 * rows = 1024 lines), synth rows with known lags ---------------
LONG2_B, LONG2_NSIG, LONG2_SEED = 1 << 18, 64, 4318
LONG2_RUNS = ((OVERRIDE, 2), (Setting(128.0, False), 1))        # (setting, submits): a tracked block [+ a locked one]


def long2_blocks(synth):
    """(rows int8 [2][65][B], lags int64 [64]): dmax = 3 L / 4, so lags of both signs and beyond half the row."""
    L = LONG2_B // 2
    params = synth.RowParams(LONG2_NSIG, L, LONG2_SEED, dmax=3 * L // 4)
    d = params.d
    assert (d > L // 2).any() and (d < -(L // 2)).any() and (np.abs(d) < L // 8).any()
    rows = np.stack([synth.make_block(LONG2_NSIG, L, LONG2_SEED, t, params=params)[0] for t in range(2)])
    return rows, d


# ---- runners ------------------------------------------------------------------------------------------------------------------

def _oracle_mask(sub, nrows):
    if sub.kind == "locked":
        return np.zeros(nrows, dtype=np.uint8)
    return np.ones(nrows, dtype=np.uint8) if sub.lag_mask is None else sub.lag_mask


def run_oracle(oracle, case, setting) -> list:
    """The case on the fp32 CPU reference (oracle.Engine) with the correction on: one result dict per block."""
    orc = oracle.Engine(case.nrows, case.B, oracle.DIGITAL)
    orc.set_frac_apply(True, setting.gain, setting.vector(case.nrows))
    res = []
    for sub in pc.submits(case):
        rc = pc.readcnt_for(sub)
        for t in range(case.T):
            res.append(orc.block(sub.rows[t], readcnt=rc[t], lag_mask=_oracle_mask(sub, case.nrows), refnoise_enabled=sub.refnoise, seq=sub.seq + t))
    orc.close()
    return res


def run_plan(b, case, setting=None, enable=1, bound=False) -> list:
    """The case on the device: a digital-mode plan, the correction on (setting) or off (None), every block fetched.
    bound: the packets go to a caller's buffer whose matrix is only 4-byte aligned, and are read back from there."""
    n, B, T = case.nrows, case.B, case.T
    plan = b.Plan(n, B, b.MODE_DIGITAL, max_batch=T)
    if setting is not None:
        plan.set_frac_apply(enable, setting.gain, setting.vector(n))
    if bound:
        import torch
        pstride = (plan.packet_bytes + 255) // 256 * 256
        buf = torch.zeros(T * pstride + 256, dtype=torch.uint8, device=torch.device("cuda", 0))
        off = (-buf.data_ptr()) % 256
        assert (buf.data_ptr() + off + plan.matrix_offset) % 16 != 0 and (buf.data_ptr() + off + plan.matrix_offset) % 4 == 0
        plan.bind_packet(buf.data_ptr() + off, pstride)
    res = []
    for sub in pc.submits(case):
        flags = (b.REFNOISE_ENABLED if sub.refnoise else 0) | (b.NO_LAG if sub.kind == "locked" else 0) | (b.OFFSET_BINARY if case.offset_binary else 0)
        rows = sub.rows.view(np.uint8) ^ np.uint8(0x80) if case.offset_binary else sub.rows
        plan.submit(rows, readcnt=pc.readcnt_for(sub), lag_mask=sub.lag_mask, seq=sub.seq, flags=flags)
        out = [plan.fetch(want_packet=not bound, block=t) for t in range(T)]
        plan.sync()
        if bound:
            for t in range(T):
                pk = buf[off + t * pstride: off + t * pstride + plan.packet_bytes].cpu().numpy().view(np.int8)
                out[t].update(packet=pk, matrix=pk[plan.matrix_offset:].reshape(n, B))
        res += out
    plan.close()
    return res


KEYS = ("lag", "mag", "frac", "phasor", "packet")


def pack(res: list) -> dict:
    """Results as arrays (for a child process to save)."""
    return {k: np.stack([r[k] for r in res]) for k in KEYS}


def unpack(z, nrows: int, B: int, prefix: str = "") -> list:
    mo = 16 + 4 * nrows
    n = z[prefix + "lag"].shape[0]
    return [dict({k: z[prefix + k][i] for k in KEYS}, matrix=z[prefix + "packet"][i][mo:].reshape(nrows, B)) for i in range(n)]


# ---- the criterion -------------------------------------------------------------------------------------------------------------

def argument_term(D, zmax):
    """Counts the fp32 phase argument's rounding may move a sample by, for |D| > 1 (0 otherwise)."""
    D = np.abs(np.asarray(D, dtype=np.float64))
    return np.where(D > 1.0, 2.0 * np.pi * D * 2.0 ** -24 * np.asarray(zmax), 0.0)


def block_delays(setting, got, nrows):
    return setting.vector(nrows) if setting.override else fm.delay_of(setting.gain, got["frac"])


def judge_block(rows_signed, got, D, own=None):
    """Per owned signal row of one block: (excess, argument term).  got: lag, phasor, matrix as fetched."""
    idx = np.arange(1, rows_signed.shape[0]) if own is None else np.asarray(own)
    z = fm.unrounded(rows_signed[idx], got["lag"][idx], D[idx], got["phasor"][idx])
    return fm.excess_rows(got["matrix"][idx], z), argument_term(D[idx], np.abs(z).max(axis=1))


def judge(case, setting, res) -> tuple:
    """(excess [blocks][signal rows], argument term [same]) of a steered case.  Every lag must be the steered one: the criterion
    leaves out no sample."""
    subs = pc.submits(case)
    assert len(res) == case.T * len(subs)
    ex, arg, i = [], [], 0
    for s, sub in enumerate(subs):
        for t in range(case.T):
            got = res[i]
            i += 1
            assert np.array_equal(got["lag"][1:], sub.lag[t, 1:]), f"{case.name} submit {s} ({sub.kind}) block {t}: lags {got['lag'][1:]} != {sub.lag[t, 1:]}"
            e, a = judge_block(sub.rows[t], got, block_delays(setting, got, case.nrows))
            ex.append(e)
            arg.append(a)
    return np.stack(ex), np.stack(arg)


def assert_within(name, ex, arg, ref, tag=""):
    """excess <= MARGIN * ref + argument term for every row, and no bar above MAX_BAR."""
    bar = MARGIN * ref + arg
    assert bar.max() <= MAX_BAR, f"{name}: bar {bar.max():.3g} above {MAX_BAR} count"
    over = ex > bar
    if over.any():
        w = np.unravel_index(np.argmax(ex - bar), ex.shape)
        raise AssertionError(f"{name} {tag}: excess {ex[w]:.4g} count over the bar {bar[w]:.4g} (4 x reference {ref:.4g} + argument term {arg[w]:.3g}) "
                             f"at block/row {w}; {int(over.sum())} of {over.size} rows over; largest excess {ex.max():.4g}")


# ---- the reference's own excess, per family (CPU only; shared by the CPU test and the device test) ---------------------------------

@functools.lru_cache(maxsize=None)
def _reference_run(case_name: str, setting: Setting) -> float:
    import oracle_py
    oracle_py.build()
    case = next(c for c in STEERED_CASES if c.name == case_name)
    ex, _ = judge(case, setting, run_oracle(oracle_py, case, setting))
    return float(ex.max())


@functools.lru_cache(maxsize=None)
def reference_excess(family: str) -> float:
    """excess(oracle.Engine) against the model over every run of the family (fed the oracle's own lag, phasor and frac)."""
    if family == "long2":
        return _reference_long2()
    if family == "fuzz":
        return max(fuzz_reference(seed)[0] for seed in range(FUZZ_SEEDS))
    return max(_reference_run(c.name, s) for c, s in FAMILIES[family])


def _reference_long2() -> float:
    import importlib
    import oracle_py
    oracle_py.build()
    synth = importlib.import_module("coherent-rtlsdr_amd.synth")
    rows, d = long2_blocks(synth)
    n = LONG2_NSIG + 1
    worst = -1.0
    for setting, nsub in LONG2_RUNS:
        orc = oracle_py.Engine(n, LONG2_B, oracle_py.DIGITAL)
        orc.set_frac_apply(True, setting.gain, setting.vector(n))
        for t in range(nsub):
            got = orc.block(rows[t], lag_mask=np.full(n, 1 - t, dtype=np.uint8), seq=t, nthreads=8)
            assert np.array_equal(got["lag"][1:], d)
            e, _ = judge_block(rows[t], got, block_delays(setting, got, n))
            worst = max(worst, float(e.max()))
        orc.close()
    return worst


# ---- fuzz: the configuration draw of tests/test_gpu_fuzz.py restricted to the digital mode, with the correction on ---------------
FUZZ_SEEDS = 32


def fuzz_config(seed: int, synth) -> dict:
    rng = np.random.default_rng(31000 + seed)
    log2B = int(rng.integers(4, 18)) if seed % 4 else int(rng.choice([14, 14, 15, 16]))
    B, L = 1 << log2B, 1 << (log2B - 1)
    nsig = int(rng.integers(1, 10))
    nrows = nsig + 1
    long_block = B > 16384
    T = 1 if long_block else int(rng.integers(1, 6))
    dmax = int(rng.integers(0, max(1, L // 4) + 1))
    params = synth.RowParams(nsig, L, 7000 + seed, dmax=dmax)
    if rng.random() < 0.3 and nsig >= 2:
        rb = int(rng.integers(1, nsig + 1))
        rcnt = int(rng.integers(1, nsig - rb + 2))
    else:
        rb, rcnt = 1, nsig
    offset_binary = bool(rng.random() < 0.3)
    if rng.random() < 0.5:
        setting, D = OVERRIDE, np.concatenate([[777.0], rng.choice(D_SET, size=nsig)]).astype(np.float32)
    else:
        setting, D = Setting(float(rng.choice(GAINS)), False), None
    batches, t_abs = [], 0
    for ib in range(2):
        blocks = np.stack([synth.make_block(nsig, L, 7000 + seed, t_abs + t, params=params)[0] for t in range(T)])
        mask = (rng.random(nrows) < 0.7).astype(np.uint8) if rng.random() < 0.5 else None
        refnoise = bool(rng.random() < 0.8)
        locked = (not long_block) and bool(rng.random() < 0.2)
        readcnt = rng.integers(0, 2 ** 32, size=(T, nrows), dtype=np.uint32) if rng.random() < 0.5 else None
        batches.append(dict(blocks=blocks, mask=mask, refnoise=refnoise, locked=locked, readcnt=readcnt, seq=77 + t_abs))
        t_abs += T
    own = np.zeros(nrows, dtype=bool)
    own[rb: rb + rcnt] = True
    return dict(B=B, L=L, nsig=nsig, nrows=nrows, T=T, rb=rb, rcnt=rcnt, own=own, offset_binary=offset_binary, setting=setting, D=D, batches=batches)


def fuzz_oracle(oracle, cfg) -> list:
    """One oracle result per block of the configuration, in order."""
    n, own = cfg["nrows"], cfg["own"]
    orc = oracle.Engine(n, cfg["B"], oracle.DIGITAL)
    orc.set_frac_apply(True, cfg["setting"].gain, cfg["D"])
    res = []
    for bt in cfg["batches"]:
        omask = np.zeros(n, dtype=np.uint8) if bt["locked"] else (bt["mask"] if bt["mask"] is not None else np.ones(n, dtype=np.uint8))
        omask = omask * own.astype(np.uint8)                 # the oracle only correlates the rows the plan owns
        for t in range(cfg["T"]):
            res.append(orc.block(bt["blocks"][t], readcnt=None if bt["readcnt"] is None else bt["readcnt"][t], lag_mask=omask,
                                 refnoise_enabled=bt["refnoise"], seq=bt["seq"] + t))
    orc.close()
    return res


def fuzz_delays(cfg, got):
    return cfg["D"] if cfg["setting"].override else fm.delay_of(cfg["setting"].gain, got["frac"])


@functools.lru_cache(maxsize=None)
def fuzz_reference(seed: int) -> tuple:
    """(excess of the oracle over the owned rows of every block, its results) for one seed."""
    import importlib
    import oracle_py
    oracle_py.build()
    cfg = fuzz_config(seed, importlib.import_module("coherent-rtlsdr_amd.synth"))
    res = fuzz_oracle(oracle_py, cfg)
    rows = np.flatnonzero(cfg["own"])
    worst, i = -1.0, 0
    for bt in cfg["batches"]:
        for t in range(cfg["T"]):
            e, _ = judge_block(bt["blocks"][t], res[i], fuzz_delays(cfg, res[i]), own=rows)
            worst = max(worst, float(e.max()))
            i += 1
    return worst, res


# ---- device runners of the cases that are not steered ---------------------------------------------------------------------------

def run_long2(b, synth) -> dict:
    """The two-line family on the device: per setting a fresh plan, a tracked block [and a locked one]; packed arrays per setting."""
    rows, _ = long2_blocks(synth)
    n = LONG2_NSIG + 1
    out = {}
    for setting, nsub in ((None, 2),) + LONG2_RUNS:                # first the same blocks with the correction off
        plan = b.Plan(n, LONG2_B, b.MODE_DIGITAL)
        if setting is not None:
            plan.set_frac_apply(1, setting.gain, setting.vector(n))
        res = []
        for t in range(nsub):
            plan.submit(rows[t], seq=t, flags=b.REFNOISE_ENABLED | (b.NO_LAG if t else 0))
            res.append(plan.fetch())
        plan.close()
        out.update({f"{setting.name if setting else 'off'}_{k}": v for k, v in pack(res).items()})
    return out


def run_fuzz(b, cfg) -> list:
    """One device result per block of a fuzz configuration, in order."""
    plan = b.Plan(cfg["nrows"], cfg["B"], b.MODE_DIGITAL, row_begin=cfg["rb"], row_count=cfg["rcnt"], max_batch=cfg["T"])
    plan.set_frac_apply(True, cfg["setting"].gain, cfg["D"])
    res = []
    for bt in cfg["batches"]:
        flags = (b.REFNOISE_ENABLED if bt["refnoise"] else 0) | (b.NO_LAG if bt["locked"] else 0) | (b.OFFSET_BINARY if cfg["offset_binary"] else 0)
        data = (bt["blocks"].view(np.uint8) ^ np.uint8(0x80)) if cfg["offset_binary"] else bt["blocks"]
        plan.submit(data, readcnt=bt["readcnt"], lag_mask=bt["mask"], seq=bt["seq"], flags=flags)
        res += [plan.fetch(block=t) for t in range(cfg["T"])]
        plan.sync()
    plan.close()
    return res
