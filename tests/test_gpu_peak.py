"""GPU: the four correlation peak estimators at chosen peak positions, against a correlation known in closed form.

tests/peak_cases.py builds rows whose zero-padded correlation is exactly three numbers (ym, peak, yp) at idx-1, idx, idx+1, all else
zero; lag, mag and frac follow in closed form and a neighbour read from anywhere else moves frac by > 1e-2 (tests/test_peak_cases_model.py),
against a bar of 2.8e-6.  Digital mode throughout: the aligned rows are the taps themselves and every EMA phasor stays exactly 1.

Which position set is aimed at which code (csrc/ = coherent-rtlsdr_amd/csrc/):
  every idx 1 .. B-1, B = 16 .. 8192        csrc/kernels.hpp k_xcorr_lag: A[idx -+ 1].x read back by thread 0, the idx > 0 && idx < N-1 guard
  B = 16384, (idx & 63) in {0, 1, 62, 63}   csrc/xcorr14p.hpp in_wave / __shfl_up,down against red[32], red[33]; csrc/xcorr14q.hpp edge[] for ln == 0 / 63
  B = 16384, (idx & 511) in {0,255,256,511} csrc/xcorr14q.hpp (cl >> 8) * 32 half select (vt0 / vt1); both kernels' nl >> 9, nr >> 9 output index change
  B = 16384, idx 1,2,3, B-3..B-1, L-1..L+1  both kernels' gi > 0 / gi < N-1 guards; shifted_word (csrc/kernels.hpp) at d = -(L-1) .. L-1
  long, (idx & (N2-1)) in {0,1,N2-2,N2-1}   csrc/longblock.hpp k_long_finalize: n1 = n >> LOG2N2, n2 = n & (N2-1) of the neighbours, per n1
  long, first / last index of a tile        csrc/longblock.hpp k_long_inv_cols: n = rev_n1(j) * N2 + tile * C + c and the [row][tile] partials
  long, idx 1, 2, B-2, B-1, L-1, L, L+1     k_long_finalize's n >= 0 && n < B and gi > 0 && gi < B-1 guards
  an all-zero correlation                   every reduction's tie rule (first maximum = index 0), den == 0, the zero dot product
  band-limited rows, real fractional delays the arithmetic of frac on live neighbours (|frac| 0.23 .. 0.39), bar from the fp64 model's own ym, mp, yp

  every idx 1 .. 16383 of B = 16384         each lane, wave, register index and column of the last inverse pass and of the argmax epilogue in
                                            k_xcorr_lag14p (folded and not), k_xcorr_lag14q, k_xcorr_lag14r, and in what k1_pick takes by itself
  every idx 1 .. 32767 of B = 2^15          the same of k_long_inv_cols / k_long_finalize behind both stage-B kernels (k_rows14_cf32q, the packed one)

B = 16384 picks its kernel once per process (CRSDR_K1_VARIANT, CRSDR_K1_FOLD), a long block its stage B (CRSDR_LONG_Q): those cases run
in one child per selection, one after the other, and the parent compares the selections bit for bit.
"""
import importlib
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import long_chunk_cases as lc
import peak_cases as pc

pytestmark = pytest.mark.gpu

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
K1_VARIANTS = {"packed": {"CRSDR_K1_VARIANT": "packed", "CRSDR_K1_FOLD": "1"}, "q": {"CRSDR_K1_VARIANT": "q", "CRSDR_K1_FOLD": "1"},
               "r": {"CRSDR_K1_VARIANT": "r", "CRSDR_K1_FOLD": "1"}, "packed_nofold": {"CRSDR_K1_VARIANT": "packed", "CRSDR_K1_FOLD": "0"}}
K1_SELECTIONS = dict(K1_VARIANTS, auto={})                 # auto: neither switch in the environment, the kernel k1_pick takes by itself
LONG_STAGE_B = {"two_line": {}, "one_line": {"CRSDR_LONG_Q": "0"}}       # the default environment; the packed one-line stage B


@pytest.fixture(scope="module")
def b():
    binding = importlib.import_module("coherent-rtlsdr_amd.binding")
    if binding.device_count() < 1:
        pytest.fail("no HIP device: the product path has no CPU fallback")
    return binding


# ---- the sections (run in this process, or in a child for B = 16384) --------------------------------------------------------
def pulse_section(b, L, blocks, submits=1, what=""):
    """blocks: [(q, ps)] of equal row counts, submitted as ONE batch (max_batch = len(blocks): blockIdx.y > 0, a reference spectrum per
    block), `submits` times.  Returns dict(fails, emag, efrac, lag, mag, frac)."""
    return pulse_run(b, L, [blocks] * submits, what)


def pulse_run(b, L, batches, what=""):
    """batches: one [(q, ps)] per submit, all of one shape, submitted one after the other on ONE plan (the carried state and the seq
    numbering run through them; the per-row read counters differ from submit to submit).  Returns what pulse_section returns, lag,
    mag and frac [submits * blocks][rows] in the order fetched."""
    nblk, n = len(batches[0]), len(batches[0][0][1])
    assert all(len(blocks) == nblk and all(len(ps) == n for _, ps in blocks) for blocks in batches)
    plan = b.Plan(n + 1, 2 * L, b.MODE_DIGITAL, max_batch=nblk)
    res = dict(fails=[], emag=0.0, efrac=0.0, lag=[], mag=[], frac=[])
    rows = prev = None
    for s, blocks in enumerate(batches):
        if blocks is not prev:
            rows, prev = np.stack([pc.pulse_block(L, q, ps) for q, ps in blocks]), blocks
        readcnt = (100000 * s + 1000 * np.arange(1, nblk + 1, dtype=np.uint32)[:, None] + np.arange(n + 1, dtype=np.uint32)[None, :]).astype(np.uint32)
        seq = 7 + 10 * s
        plan.submit(rows, readcnt=readcnt, seq=seq)
        for t, (q, ps) in enumerate(blocks):
            out = plan.fetch(block=t)
            emag, efrac, fails = pc.check_pulse_output(out, L, q, ps, seq + t, readcnt[t], f"{what} submit {s} block {t} (q = {q})")
            res["fails"] += fails
            res["emag"], res["efrac"] = max(res["emag"], emag), max(res["efrac"], efrac)
            for key in ("lag", "mag", "frac"):
                res[key].append(out[key])
        plan.sync()
    plan.close()
    for key in ("lag", "mag", "frac"):
        res[key] = np.stack(res[key])
    return res


def ties_section(b, model, L, what=""):
    """Item "all ties": an all-zero row beside live ones, then an all-zero reference."""
    B = 2 * L
    ps = np.array([0, L // 3, 5])
    rows = pc.pulse_block(L, 0, ps)
    rows[1] = 0
    plan, mod = b.Plan(4, B, b.MODE_DIGITAL), model.Model(4, B, model.DIGITAL)
    fails = []
    exp = pc.closed_form(L, 0, ps)
    got = plan.block(rows, seq=1)
    mlag, mmag, mfrac, mph, mmat = mod.block(rows)
    if not (got["lag"][1] == -L and got["mag"][1] == 0 and got["frac"][1] == 0):
        fails.append(f"{what}: the all-zero row reports lag {got['lag'][1]}, mag {got['mag'][1]}, frac {got['frac'][1]}")
    if not all(np.all(np.isfinite(got[k])) for k in ("mag", "frac", "phasor")):
        fails.append(f"{what}: non-finite outputs beside an all-zero row")
    live = {k: v[1:] if isinstance(v, np.ndarray) else v for k, v in exp.items()}
    emag, efrac, f = pc.compare({k: got[k][2:] for k in ("lag", "mag", "frac")}, live, f"{what} live rows")
    fails += f
    if not (np.array_equal(got["matrix"], mmat) and np.all(got["phasor"][1:] == 1.0)):
        fails.append(f"{what}: first submit's matrix or phasors differ from the model's")
    first_phasor = got["phasor"].copy()
    rows2 = rows.copy()
    rows2[0] = 0
    rows2[3] = 0
    got = plan.block(rows2, seq=2)
    mlag, mmag, mfrac, mph, mmat = mod.block(rows2)
    if not (np.all(got["lag"][1:] == -L) and np.all(got["mag"] == 0) and np.all(got["frac"] == 0)):
        fails.append(f"{what}: all-zero reference: lag {got['lag'].tolist()}, mag {got['mag'].tolist()}, frac {got['frac'].tolist()}")
    if not np.array_equal(got["phasor"].view(np.uint8), first_phasor.view(np.uint8)):
        fails.append(f"{what}: a zero dot product moved the phasors: {got['phasor'].tolist()}")
    if not np.array_equal(got["matrix"], mmat):
        fails.append(f"{what}: all-zero reference: matrix differs from the model's")
    assert np.array_equal(mlag[1:], [-L] * 3) and np.all(mph[1:] == 1.0)          # (the model itself: as the issue states it)
    plan.close()
    return dict(fails=fails, emag=emag, efrac=efrac)


def fractional_section(b, model, L, what=""):
    rows = pc.fractional_rows(L)
    ref = pc.model_reference(model, rows)
    plan = b.Plan(rows.shape[0], 2 * L, b.MODE_DIGITAL)
    got = plan.block(rows)
    plan.close()
    emag, efrac, fails = pc.compare({k: got[k][1:] for k in ("lag", "mag", "frac")}, ref, what)
    return dict(fails=fails, emag=emag, efrac=efrac)


def _report(name, res):
    print(f"{name}: worst mag rel err {res['emag']:.3e}  worst frac abs err {res['efrac']:.3e}")
    assert not res["fails"], "\n".join(res["fails"])


# ---- 1: the generic kernels, every position ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("log2B", range(4, 14))
def test_generic_kernel_at_every_peak_position(b, log2B):
    L = (1 << log2B) // 2
    blocks = list(zip(pc.ref_positions(L), pc.split_by_reference(L, pc.full_positions(L))))
    assert all(len(ps) == L for _, ps in blocks)                     # every p in [0, L) under both references: every idx 1 .. B-1
    _report(f"generic B = 2^{log2B}", pulse_section(b, L, blocks, what=f"B = 2^{log2B}"))


# ---- 2 (+ the B = 16384 cases of 4 and 5): one child per K1 selection ------------------------------------------------------------------
def sweep_section(b, L, batches, what=""):
    """pulse_run over batches that together put a peak on every idx 1 .. B - 1.  Returns (dict(fails, emag, efrac, seconds),
    pc.gather_by_idx's arrays): the fails include an index that was not reached."""
    t0 = time.perf_counter()
    res = pulse_run(b, L, batches, what)
    g = pc.gather_by_idx(L, [blk for blocks in batches for blk in blocks], res)
    reached = g.pop("reached")
    out = {k: res[k] for k in ("fails", "emag", "efrac")}
    out["fails"] = out["fails"] + pc.sweep_is_complete(L, reached)
    out["reached"], out["reached_L"] = int(np.count_nonzero(reached.sum(axis=0))), [int(reached[0, L]), int(reached[1, L])]
    out["seconds"] = time.perf_counter() - t0
    return out, g


def k1_child(out_path, sections):
    """Runs in a child (the selection is in its environment).  "designed": the designed positions twice, the ties, the band-limited
    rows.  "sweep": every idx 1 .. 16383, four submits of two blocks of pc.K1_SWEEP_ROWS signal rows on one plan -- 4096 items a
    launch, so every group of a two-row kernel runs several rows and, under r, almost every row on carried chains."""
    import torch
    import model_fp64 as model
    b = importlib.import_module("coherent-rtlsdr_amd.binding")
    L = 8192
    summary, arrays = {}, {}
    if "designed" in sections:
        blocks = list(zip(pc.ref_positions(L), pc.split_by_reference(L, pc.k1_positions(L)[1])))
        pulse = pulse_section(b, L, blocks, submits=2, what="B = 16384")
        ties = ties_section(b, model, L, what="B = 16384 ties")
        fract = fractional_section(b, model, L, what="B = 16384 band-limited")
        summary = {name: {k: r[k] for k in ("fails", "emag", "efrac")} for name, r in (("pulse", pulse), ("ties", ties), ("fractional", fract))}
        summary["rows_per_block"] = int(len(blocks[0][1]))
        arrays = {k: pulse[k] for k in ("lag", "mag", "frac")}
    if "sweep" in sections:
        (q0, s0), (q1, s1) = pc.sweep_batches(L, pc.K1_SWEEP_ROWS)
        batches = [[(q0, a), (q1, c)] for a, c in zip(s0, s1)]
        summary["sweep"], g = sweep_section(b, L, batches, what="B = 16384 sweep")
        summary["sweep"].update(submits=len(batches), items=pc.K1_SWEEP_ROWS * len(batches[0]),      # row_count * nblocks of a launch
                                cus=int(torch.cuda.get_device_properties(0).multi_processor_count))
        arrays.update({"sweep_" + k: v for k, v in g.items()})
    np.savez(out_path, summary=np.array(json.dumps(summary)), **arrays)


def run_children(tmp, code, envs, strip, timeout):
    """{name: npz} or {name: message} for a child that did not run: the children run one after the other, each in os.environ without
    `strip` plus its own settings, and nothing more is started after the first non-zero exit."""
    res, stopped = {}, None
    base = {k: v for k, v in os.environ.items() if k not in strip}
    for name, (env, args) in envs.items():
        if stopped:
            res[name] = f"not run: {stopped}"
            continue
        out = tmp / f"{name}.npz"
        t0 = time.perf_counter()
        r = subprocess.run([sys.executable, "-c", code, str(out)] + list(args), env=dict(base, **env), capture_output=True, text=True, timeout=timeout)
        if r.returncode != 0:
            stopped = f"the child {name} exited with {r.returncode}"
            res[name] = stopped + "\n" + r.stdout + r.stderr
            continue
        print(f"child {name}: {time.perf_counter() - t0:.1f} s")
        res[name] = np.load(out)
    return res


CHILD = "import sys; sys.path[:0] = [%r, %r, %r]; import torch, test_gpu_peak; test_gpu_peak.{0}(*sys.argv[1:])" % (TESTS, ROOT, os.path.join(ROOT, "oracle"))


@pytest.fixture(scope="module")
def k1_children(tmp_path_factory):
    """{selection: (summary, arrays)} or {selection: message}: the four forced variants run both sections, auto the sweep."""
    envs = {name: (env, ["designed,sweep" if name in K1_VARIANTS else "sweep"]) for name, env in K1_SELECTIONS.items()}
    res = run_children(tmp_path_factory.mktemp("k1_peak"), CHILD.format("k1_child"), envs, ("CRSDR_K1_VARIANT", "CRSDR_K1_FOLD"), 300)
    return {name: z if isinstance(z, str) else (json.loads(str(z["summary"])), {k: z[k] for k in z.files if k != "summary"}) for name, z in res.items()}


def _child(children, name):
    assert not isinstance(children[name], str), children[name]
    return children[name]


def _same_bits(base, other, keys, tag):
    for key in keys:
        assert base[key].shape == other[key].shape and base[key].size, (tag, key)
        assert np.array_equal(base[key].view(np.uint8), other[key].view(np.uint8)), (tag, key)


def _report_sweep(name, sweep, B):
    print(f"{name}: {sweep['reached']} of {B - 1} indices reached, idx = L {sweep['reached_L']} times under q = 0 / q = L - 1, {sweep['seconds']:.1f} s")
    assert sweep["reached"] == B - 1 and min(sweep["reached_L"]) >= 1
    _report(name, sweep)


@pytest.mark.parametrize("variant", list(K1_VARIANTS))
def test_k1_at_designed_peak_positions(k1_children, variant):
    summary, _ = _child(k1_children, variant)
    print(f"{summary['rows_per_block']} signal rows per block, two blocks per submit, two submits")
    _report(f"K1 {variant}", summary["pulse"])


def test_k1_variants_agree_bit_for_bit_at_designed_positions(k1_children):
    base = _child(k1_children, "packed")[1]
    for variant in ("q", "r", "packed_nofold"):
        _same_bits(base, _child(k1_children, variant)[1], ("lag", "mag", "frac"), variant)


@pytest.mark.parametrize("selection", list(K1_SELECTIONS))
def test_k1_at_every_peak_position(k1_children, selection):
    sweep = _child(k1_children, selection)[0]["sweep"]
    print(f"{sweep['submits']} submits of {sweep['items']} rows on one plan, {sweep['cus']} CUs")
    assert sweep["submits"] == 4 and sweep["items"] == 2 * pc.K1_SWEEP_ROWS
    # crsdr.hip k1_pick: a launch of >= 12 rows per CU takes the two-row kernel r under the default selection ("auto" proves that
    # the kernel large launches take is one of those swept) and several rows per group under q and r
    assert sweep["items"] >= 12 * sweep["cus"]
    _report_sweep(f"K1 {selection}, every idx", sweep, 16384)


def test_k1_selections_agree_bit_for_bit_at_every_position(k1_children):
    keys = ["sweep_" + k for k in ("lag", "mag", "frac", "lag_L", "mag_L", "frac_L")]      # 16 383 entries each, and idx = L's second row
    base = _child(k1_children, "packed")[1]
    assert base["sweep_lag"].shape == (16383,) and np.array_equal(base["sweep_lag"], np.arange(1, 16384) - 8192) and base["sweep_lag_L"][0] == 0
    for selection in ("q", "r", "auto", "packed_nofold"):
        _same_bits(base, _child(k1_children, selection)[1], keys, selection)


# ---- 3: long blocks -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log2B", [15, 16, 18])
def test_long_blocks_at_designed_peak_positions(b, log2B):
    L = (1 << log2B) // 2
    res = dict(fails=[], emag=0.0, efrac=0.0)
    for q, ps in pc.long_blocks(log2B):
        assert 1 <= len(ps) <= pc.LONG_MAX_ROWS
        r = pulse_section(b, L, [(q, ps)], what=f"B = 2^{log2B}")
        res["fails"] += r["fails"]
        res["emag"], res["efrac"] = max(res["emag"], r["emag"]), max(res["efrac"], r["efrac"])
    _report(f"long B = 2^{log2B}", res)


def long_child(out_path):
    """Runs in a child (CRSDR_LONG_Q is read once per process): every idx 1 .. 32767 of B = 2^15, the smallest long block (N1 = 2),
    as submits of one block of pc.LONG_SWEEP_ROWS signal rows on one plan, first those of q = 0, then those of q = L - 1."""
    b = importlib.import_module("coherent-rtlsdr_amd.binding")
    L = 1 << 14
    batches = [[(q, ps)] for q, slices in pc.sweep_batches(L, pc.LONG_SWEEP_ROWS) for ps in slices]
    sweep, g = sweep_section(b, L, batches, what="B = 2^15 sweep")
    sweep["submits"] = len(batches)
    np.savez(out_path, summary=np.array(json.dumps({"sweep": sweep})), **{"sweep_" + k: v for k, v in g.items()})


@pytest.fixture(scope="module")
def long_children(tmp_path_factory):
    """{stage B: (summary, arrays)} or {stage B: message}, as k1_children."""
    envs = {name: (env, []) for name, env in LONG_STAGE_B.items()}
    res = run_children(tmp_path_factory.mktemp("long_peak"), CHILD.format("long_child"), envs, lc.SWITCHES, 300)
    return {name: z if isinstance(z, str) else (json.loads(str(z["summary"])), {k: z[k] for k in z.files if k != "summary"}) for name, z in res.items()}


@pytest.mark.parametrize("stage_b", list(LONG_STAGE_B))
def test_long_block_at_every_peak_position(long_children, stage_b):
    B, n = 1 << 15, pc.LONG_SWEEP_ROWS
    # what the plan does with a block of n signal rows (crsdr.hip k1_long, two_line()): more than one chunk of the work area, and
    # every chunk large enough for the two-line stage B -- which the default environment then takes and CRSDR_LONG_Q=0 never does
    chunks = lc.split(B, n)
    assert len(chunks) > 1 and sum(chunks) == n
    assert all((B // 16384) * cnt >= 1024 for cnt in chunks) and all(lc.two_line(B, chunks, True)) and not any(lc.two_line(B, chunks, False))
    sweep = _child(long_children, stage_b)[0]["sweep"]
    print(f"{sweep['submits']} submits of one block of {n} signal rows on one plan, chunks of {chunks} rows")
    assert sweep["submits"] == 2 * -(-(B // 2) // n)
    _report_sweep(f"long B = 2^15 {stage_b}, every idx", sweep, B)


def test_long_block_stage_b_kernels_agree_bit_for_bit_at_every_position(long_children):
    base, other = _child(long_children, "two_line")[1], _child(long_children, "one_line")[1]
    assert base["sweep_lag"].shape == ((1 << 15) - 1,)
    _same_bits(base, other, ["sweep_" + k for k in ("lag", "mag", "frac", "lag_L", "mag_L", "frac_L")], "one_line against two_line")


# ---- 4: all ties ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log2B", [8, 15])
def test_all_zero_correlation_reports_the_first_index(b, model, log2B):
    _report(f"ties B = 2^{log2B}", ties_section(b, model, (1 << log2B) // 2, what=f"B = 2^{log2B} ties"))


@pytest.mark.parametrize("variant", ["packed", "q", "r"])
def test_all_zero_correlation_reports_the_first_index_k1(k1_children, variant):
    _report(f"ties K1 {variant}", _child(k1_children, variant)[0]["ties"])


# ---- 5: real fractional delays ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [2048, 1 << 15])
def test_frac_of_band_limited_rows_against_fp64(b, model, L):
    _report(f"band-limited L = {L}", fractional_section(b, model, L, what=f"band-limited L = {L}"))


@pytest.mark.parametrize("variant", ["packed", "q", "r"])
def test_frac_of_band_limited_rows_against_fp64_k1(k1_children, variant):
    _report(f"band-limited K1 {variant}", _child(k1_children, variant)[0]["fractional"])
