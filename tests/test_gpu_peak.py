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

B = 16384 picks its kernel once per process (CRSDR_K1_VARIANT, CRSDR_K1_FOLD): those cases run in one child per variant, one after the
other, and the parent compares the variants bit for bit.
"""
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import peak_cases as pc

pytestmark = pytest.mark.gpu

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
K1_VARIANTS = {"packed": {"CRSDR_K1_VARIANT": "packed", "CRSDR_K1_FOLD": "1"}, "q": {"CRSDR_K1_VARIANT": "q", "CRSDR_K1_FOLD": "1"},
               "packed_nofold": {"CRSDR_K1_VARIANT": "packed", "CRSDR_K1_FOLD": "0"}}


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
    n = len(blocks[0][1])
    rows = np.stack([pc.pulse_block(L, q, ps) for q, ps in blocks])
    readcnt = (1000 * np.arange(1, len(blocks) + 1, dtype=np.uint32)[:, None] + np.arange(n + 1, dtype=np.uint32)[None, :])
    plan = b.Plan(n + 1, 2 * L, b.MODE_DIGITAL, max_batch=len(blocks))
    res = dict(fails=[], emag=0.0, efrac=0.0, lag=[], mag=[], frac=[])
    for s in range(submits):
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


# ---- 2 (+ the B = 16384 cases of 4 and 5): one child per K1 variant -------------------------------------------------------------------
def k1_child(out_path):
    """Runs in a child (the variant is in its environment): the designed positions twice, the ties, the band-limited rows."""
    import model_fp64 as model
    b = importlib.import_module("coherent-rtlsdr_amd.binding")
    L = 8192
    blocks = list(zip(pc.ref_positions(L), pc.split_by_reference(L, pc.k1_positions(L)[1])))
    pulse = pulse_section(b, L, blocks, submits=2, what="B = 16384")
    ties = ties_section(b, model, L, what="B = 16384 ties")
    fract = fractional_section(b, model, L, what="B = 16384 band-limited")
    summary = {name: {k: r[k] for k in ("fails", "emag", "efrac")} for name, r in (("pulse", pulse), ("ties", ties), ("fractional", fract))}
    summary["rows_per_block"] = int(len(blocks[0][1]))
    np.savez(out_path, lag=pulse["lag"], mag=pulse["mag"], frac=pulse["frac"], summary=np.array(json.dumps(summary)))


@pytest.fixture(scope="module")
def k1_children(tmp_path_factory):
    """{variant: (summary, arrays)} or {variant: message} for a variant that did not run: the children run one after the other and
    nothing more is started after the first non-zero exit."""
    tmp = tmp_path_factory.mktemp("k1_peak")
    code = "import sys; sys.path[:0] = [%r, %r, %r]; import torch, test_gpu_peak; test_gpu_peak.k1_child(sys.argv[1])" % (TESTS, ROOT, os.path.join(ROOT, "oracle"))
    res, stopped = {}, None
    for variant, env in K1_VARIANTS.items():
        if stopped:
            res[variant] = f"not run: {stopped}"
            continue
        out = tmp / f"{variant}.npz"
        r = subprocess.run([sys.executable, "-c", code, str(out)], env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
        if r.returncode != 0:
            stopped = f"the child of variant {variant} exited with {r.returncode}"
            res[variant] = stopped + "\n" + r.stdout + r.stderr
            continue
        z = np.load(out)
        res[variant] = (json.loads(str(z["summary"])), {k: z[k] for k in ("lag", "mag", "frac")})
    return res


def _child(k1_children, variant):
    assert not isinstance(k1_children[variant], str), k1_children[variant]
    return k1_children[variant]


@pytest.mark.parametrize("variant", list(K1_VARIANTS))
def test_k1_at_designed_peak_positions(k1_children, variant):
    summary, _ = _child(k1_children, variant)
    print(f"{summary['rows_per_block']} signal rows per block, two blocks per submit, two submits")
    _report(f"K1 {variant}", summary["pulse"])


def test_k1_variants_agree_bit_for_bit_at_designed_positions(k1_children):
    base = _child(k1_children, "packed")[1]
    for variant in ("q", "packed_nofold"):
        other = _child(k1_children, variant)[1]
        for key in ("lag", "mag", "frac"):
            assert np.array_equal(base[key].view(np.uint8), other[key].view(np.uint8)), (variant, key)


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


# ---- 4: all ties ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log2B", [8, 15])
def test_all_zero_correlation_reports_the_first_index(b, model, log2B):
    _report(f"ties B = 2^{log2B}", ties_section(b, model, (1 << log2B) // 2, what=f"B = 2^{log2B} ties"))


@pytest.mark.parametrize("variant", ["packed", "q"])
def test_all_zero_correlation_reports_the_first_index_k1(k1_children, variant):
    _report(f"ties K1 {variant}", _child(k1_children, variant)[0]["ties"])


# ---- 5: real fractional delays ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [2048, 1 << 15])
def test_frac_of_band_limited_rows_against_fp64(b, model, L):
    _report(f"band-limited L = {L}", fractional_section(b, model, L, what=f"band-limited L = {L}"))


@pytest.mark.parametrize("variant", ["packed", "q"])
def test_frac_of_band_limited_rows_against_fp64_k1(k1_children, variant):
    _report(f"band-limited K1 {variant}", _child(k1_children, variant)[0]["fractional"])
