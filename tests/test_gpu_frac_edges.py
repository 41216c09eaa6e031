"""The fractional-delay correction (crsdr_plan_set_frac_apply) per sample, at its edges, on every kernel that runs it, against the
unrounded fp64 model of tests/frac_delay_model.py.

tests/test_gpu_fracdelay.py compares rounded int8 matrices at benign operating points and allows +-1 LSB on 2e-3 of the entries,
anywhere.  Here every output sample of every owned row is held to |q - clip(z)| - 0.5 <= bar, z the model's unrounded value given
the block's own lag, phasor and D: one sample that is wrong by a position, a sign or a bin is many counts over.  The inputs are
those of tests/phase_path_cases.py -- rows steered to every lag class in (-L, L), lag = -L from a zero row, locked full-scale
blocks with -128 and 127 -- with D per row cycled over 0, +-0.25, 0.3, -0.45, +-0.5, +-1, +-7.3, +-64 (override), then
estimate-driven with gain 1, 128, -128 (locked batches use the carried frac).  In the same run: the lags are the steered ones; lag,
mag, frac, phasor, the header, the read counters and the raw row 0 are bit-identical to the same case with the correction off.

Kernels and the shapes that reach them (tests/frac_edge_cases.py):
  generic  k_frac_apply<LOG2N>: B = 16 .. 8192 (one to four radix-16 passes), B = 16384 under CRSDR_FRAC_GENERIC=1, chain cases at 128
  fast14   k_frac_apply14: B = 16384 signed / offset binary, own and 4-byte aligned bound packets, both switched phase paths, chain cases
  long1    k_rows14_cf32p<false, true>: B = 2^15, 2^16 with 37 signal rows (N1 * rows < 1024 lines), enable = 1 and 2
  long2    k_ramp_rowspec + k_rows14_cf32q<true>: B = 2^18 with 64 signal rows (1024 lines), CRSDR_LONG_Q=1; =0 takes long1's kernel
  sharded  G = 4 slab plans against the unsharded plan, bit for bit;   fuzz  32 seeded digital-mode configurations

Bars: 4 x the excess of the fp32 CPU reference (oracle.Engine) on the same family of inputs, computed on the CPU at run time
(frac_edge_cases.reference_excess; tests/test_frac_delay_model.py holds it below 0.1 count), plus, for |D| > 1, the rounding of the
fp32 phase argument 2 pi |D| 2^-24 max|z| (at most 4.3e-3 count here: |D| = 64 on a full-scale row).  Measured on an MI355X, the
largest excess over every sample of the family in counts (reference = oracle.Engine on the CPU; device includes the |D| > 1 rows):

    family                      reference    device      bar without the argument term
    generic                     1.806e-05    2.291e-05   7.223e-05
    fast14                      1.973e-05    3.724e-05   7.892e-05
    long1                       1.669e-05    3.012e-05   6.678e-05
    long2 (CRSDR_LONG_Q=1)      6.899e-06    2.126e-05   2.759e-05
    long2 (CRSDR_LONG_Q=0)      6.899e-06    1.607e-05   2.759e-05
    fuzz                        1.046e-05    1.236e-05   4.184e-05

Which kernel a shape takes was confirmed from a kernel trace of one run per shape (see the table of kernels above).
"""
import importlib
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import frac_edge_cases as fe
import phase_path_cases as pc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def b():
    binding = importlib.import_module("coherent-rtlsdr_amd.binding")
    if binding.device_count() < 1:
        pytest.fail("no HIP device: the product path has no CPU fallback")
    return binding


def _same_bits(a, c, keys, tag):
    for k in keys:
        assert np.array_equal(a[k].view(np.uint8), c[k].view(np.uint8)), (tag, k)


def _check_against_off(case, on, off, tag):
    """The correction only replaces the signal rows: everything else is bit for bit what the plain digital mode gives."""
    mo = 16 + 4 * case.nrows
    assert len(on) == len(off)
    for i, (a, c) in enumerate(zip(on, off)):
        _same_bits(a, c, ("lag", "mag", "frac", "phasor"), (tag, i))
        assert a["packet"].size == c["packet"].size and np.array_equal(a["packet"][:mo + case.B], c["packet"][:mo + case.B]), (tag, i, "header / readcnt / row 0")


def _judge(case, setting, res, family, tag=""):
    ref = fe.reference_excess(family)
    ex, arg = fe.judge(case, setting, res)
    print(f"EXCESS {family} {case.name} {setting.name} {tag}: device {ex.max():.3e} reference(family) {ref:.3e} bar {fe.MARGIN * ref:.3e} + {arg.max():.2e}")
    fe.assert_within(f"{case.name} {setting.name}", ex, arg, ref, tag)


def _run_all(b, case, family, **kw):
    off = fe.run_plan(b, case, None)
    for r, (sub, t) in zip(off, [(s, t) for s in pc.submits(case) for t in range(case.T)]):
        assert np.array_equal(r["matrix"][0], sub.rows[t, 0])                 # the raw reference row (signed)
    runs = {}
    for setting in fe.SETTINGS:
        res = fe.run_plan(b, case, setting, **kw)
        _judge(case, setting, res, family)
        _check_against_off(case, res, off, setting.name)
        runs[setting] = res
    return runs


@pytest.mark.parametrize("case", fe.GENERIC_CASES, ids=lambda c: c.name)
def test_generic_kernel_per_sample(b, case):
    # k_frac_apply<LOG2N>: every shift of the row for B <= 128, shift_set(L) above; one to four passes of the radix-16 network
    _run_all(b, case, "generic")


_CHILD = textwrap.dedent('''
    import importlib, sys, numpy as np
    sys.path[:0] = [%r, %r, %r]
    pkg = importlib.import_module("coherent-rtlsdr_amd")
    b = pkg.binding
    import frac_edge_cases as fe
    out = {}
    if sys.argv[2] == "long2":
        out = fe.run_long2(b, pkg.synth)
    else:
        case = next(c for c in fe.STEERED_CASES if c.name == sys.argv[2])
        for s in (None,) + fe.SETTINGS:
            out.update({(s.name if s else "off") + "_" + k: v for k, v in fe.pack(fe.run_plan(b, case, s)).items()})
    np.savez(sys.argv[1], **out)
''') % (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"))


def _child(tmp_path, what, env):
    out = tmp_path / "child.npz"
    r = subprocess.run([sys.executable, "-c", _CHILD, str(out), what], env=dict(os.environ, **env), capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    return np.load(out)


def test_generic_kernel_at_16384_per_sample(tmp_path):
    # CRSDR_FRAC_GENERIC=1 is read per process: a fresh child; four passes of the radix-16 network at the reference's block size
    case = fe.GENERIC14_CASE
    z = _child(tmp_path, case.name, {"CRSDR_FRAC_GENERIC": "1"})
    off = fe.unpack(z, case.nrows, case.B, "off_")
    for setting in fe.SETTINGS:
        res = fe.unpack(z, case.nrows, case.B, setting.name + "_")
        _judge(case, setting, res, "generic")
        _check_against_off(case, res, off, setting.name)


@pytest.fixture(scope="module")
def fast14_default(b):
    """The default run of the first k_frac_apply14 case, shared with the switched phase paths."""
    return _run_all(b, fe.FAST14_CASES[0], "fast14")


def test_fast14_kernel_per_sample_signed(b, fast14_default):
    case = fe.FAST14_CASES[0]
    for setting, own in fast14_default.items():
        # the dword-store branch: a bound packet whose matrix is only 4-byte aligned holds the same bytes
        bound = fe.run_plan(b, case, setting, bound=True)
        for i, (a, c) in enumerate(zip(own, bound)):
            assert np.array_equal(a["packet"], c["packet"]), (setting.name, i)


def test_fast14_kernel_per_sample_offset_binary(b):
    case = fe.FAST14_CASES[1]
    runs = _run_all(b, case, "fast14")
    for setting in (fe.OVERRIDE, fe.SETTINGS[2]):
        bound = fe.run_plan(b, case, setting, bound=True)
        for i, (a, c) in enumerate(zip(runs[setting], bound)):
            assert np.array_equal(a["packet"], c["packet"]), (setting.name, i)


@pytest.mark.parametrize("env", sorted(pc.CHILD_ENVS))
def test_fast14_kernel_behind_the_switched_phase_paths(tmp_path, fast14_default, env):
    # CRSDR_K2_FUSED=0 (three-kernel phase path) and CRSDR_K2_SPIN=-1 (look-back fallback): only the phase path differs and its
    # phasor is exact, so everything -- the signal rows included -- is bit-identical to the default run
    case = fe.FAST14_CASES[0]
    z = _child(tmp_path, case.name, pc.CHILD_ENVS[env])
    for setting in fe.SETTINGS:
        res = fe.unpack(z, case.nrows, case.B, setting.name + "_")
        for i, (a, c) in enumerate(zip(res, fast14_default[setting])):
            _same_bits(a, c, fe.KEYS, (env, setting.name, i))


@pytest.mark.parametrize("case", fe.CHAIN_CASES, ids=lambda c: c.name)
def test_chain_variants_per_sample(b, case):
    # chain_zeroed: lag = -L rows with D != 0 (a zero row in a tracked batch, then non-zero rows carried at -L through a locked
    # batch: the circular definition brings samples back in from the other end), a held phasor.  chain_refnoise_off: a frozen phasor
    L, T = case.L, case.T
    runs = _run_all(b, case, fe.family_of(case))
    res = runs[fe.OVERRIDE]
    D = fe.d_vector(case.nrows)
    if case.variant == "chain_zeroed":
        assert D[3] != 0 and res[2 * T - 1]["lag"][3] == -L and not res[2 * T - 1]["matrix"][3].any()          # a zero row stays zero
        for r in res[2 * T:]:
            assert r["lag"][3] == -L and r["phasor"][3] == res[2 * T - 1]["phasor"][3] and r["matrix"][3].any()   # samples re-enter
    else:
        ph = np.stack([r["phasor"] for r in res])
        assert np.all(ph[T:3 * T, 1:] == ph[T - 1, 1:]) and all(r["matrix"][1:].any() for r in res[T:3 * T])


@pytest.mark.parametrize("case", fe.LONG1_CASES, ids=lambda c: c.name)
def test_long_blocks_one_line_kernel_per_sample(b, case):
    # k_rows14_cf32p<false, true> + the inverse column pass's quantiser; enable = 2 (no second work area) is bit-identical
    runs = _run_all(b, case, "long1")
    for setting in fe.SETTINGS:
        lean = fe.run_plan(b, case, setting, enable=2)
        for i, (a, c) in enumerate(zip(runs[setting], lean)):
            _same_bits(a, c, fe.KEYS, (setting.name, i))


@pytest.mark.parametrize("q", ["1", "0"])
def test_long_blocks_two_line_kernel_per_sample(tmp_path, synth, q):
    # B = 2^18 with 64 signal rows: 1024 lines, the smallest launch that takes k_ramp_rowspec + k_rows14_cf32q<true> (CRSDR_LONG_Q=1);
    # CRSDR_LONG_Q=0 keeps the one-line kernel at this size.  Synth rows with known lags of both signs and beyond half the row.
    # The two factor the response differently: each meets the bar, they need not agree bit for bit.
    rows, d = fe.long2_blocks(synth)
    n = fe.LONG2_NSIG + 1
    z = _child(tmp_path, "long2", {"CRSDR_LONG_Q": q})
    ref = fe.reference_excess("long2")
    off = fe.unpack(z, n, fe.LONG2_B, "off_")
    mo = 16 + 4 * n
    for setting, nsub in fe.LONG2_RUNS:
        res = fe.unpack(z, n, fe.LONG2_B, setting.name + "_")
        assert len(res) == nsub
        for t, (a, c) in enumerate(zip(res, off)):                                # the correction only replaces the signal rows
            _same_bits(a, c, ("lag", "mag", "frac", "phasor"), (setting.name, t))
            assert np.array_equal(a["packet"][:mo + fe.LONG2_B], c["packet"][:mo + fe.LONG2_B]), (setting.name, t)
        for t, got in enumerate(res):
            assert np.array_equal(got["lag"][1:], d), (setting.name, t)
            ex, arg = fe.judge_block(rows[t], got, fe.block_delays(setting, got, n))
            print(f"EXCESS long2 q={q} {setting.name} block {t}: device {ex.max():.3e} reference(family) {ref:.3e} bar {fe.MARGIN * ref:.3e} + {arg.max():.2e}")
            fe.assert_within(f"long2 q={q} {setting.name}", ex[None], arg[None], ref, f"block {t}")
            assert np.array_equal(got["matrix"][0], rows[t, 0])


@pytest.mark.parametrize("setting", [fe.OVERRIDE, fe.SETTINGS[2]], ids=lambda s: s.name)
@pytest.mark.parametrize("case", fe.SHARD_CASES, ids=lambda c: c.name)
def test_sharded_plans_write_the_unsharded_rows_into_their_slabs(b, case, setting):
    # G = 4 plans of 4 rows each (row_begin = 1, 5, 9, 13) bound with bind_slab_ex: the same kernel on the same bytes, so every slab
    # row equals the unsharded plan's row bit for bit -- B = 2048 (generic kernel) and B = 16384 (k_frac_apply14)
    import torch
    G, n, B, T = 4, case.nrows, case.B, case.T
    per = (n - 1) // G
    dev = torch.device("cuda", 0)
    slot, toff = per * B + 256, per * B
    full = fe.run_plan(b, case, setting)
    _judge(case, setting, full, "generic" if B < 16384 else "fast14", "unsharded")
    plans = [b.Plan(n, B, b.MODE_DIGITAL, row_begin=1 + r * per, row_count=per, max_batch=T) for r in range(G)]
    send = [torch.zeros(T * slot, dtype=torch.uint8, device=dev) for _ in range(G)]
    for r, pl in enumerate(plans):
        pl.set_frac_apply(1, setting.gain, setting.vector(n))
        pl.bind_slab_ex(send[r].data_ptr(), slot, 0, T, toff)
    i = 0
    for sub in pc.submits(case):
        flags = (b.REFNOISE_ENABLED if sub.refnoise else 0) | (b.NO_LAG if sub.kind == "locked" else 0)
        for r, pl in enumerate(plans):
            pl.submit(sub.rows, readcnt=pc.readcnt_for(sub), lag_mask=sub.lag_mask, seq=sub.seq, flags=flags)
            pl.sync()
        for t in range(T):
            for r in range(G):
                slab = send[r][t * slot: t * slot + per * B].cpu().numpy().view(np.int8).reshape(per, B)
                assert np.array_equal(slab, full[i]["matrix"][1 + r * per: 1 + (r + 1) * per]), (sub.kind, t, r)
            i += 1
    for pl in plans:
        pl.close()


@pytest.mark.parametrize("seed", range(fe.FUZZ_SEEDS))
def test_random_digital_configuration_with_the_correction_on(b, synth, seed):
    # the configuration draw of tests/test_gpu_fuzz.py, digital mode only: a slab, a lag mask, a locked batch, the refnoise gate,
    # offset-binary input, read counters, T <= 5; an override drawn from the edge values or a gain of 1, 128, -128.  Rows whose lag
    # has equalled the oracle's in every block so far are judged per sample (sharp-peak data: every owned row).
    cfg = fe.fuzz_config(seed, synth)
    ref = fe.reference_excess("fuzz")
    _, ores = fe.fuzz_reference(seed)
    res = fe.run_fuzz(b, cfg)
    own, n = cfg["own"], cfg["nrows"]
    clean = np.ones(n, dtype=bool)
    hdr, i, worst = 16 + 4 * n, 0, -1.0
    for bt in cfg["batches"]:
        for t in range(cfg["T"]):
            got, exp = res[i], ores[i]
            i += 1
            clean &= got["lag"] == exp["lag"]
            if cfg["L"] >= 256:
                assert clean[own].all(), (seed, i)
            rows_ok = np.flatnonzero(own & clean)
            assert np.array_equal(got["packet"][:hdr + cfg["B"]], exp["packet"][:hdr + cfg["B"]]), (seed, i)
            if rows_ok.size:
                ex, arg = fe.judge_block(bt["blocks"][t], got, fe.fuzz_delays(cfg, got), own=rows_ok)
                worst = max(worst, float(ex.max()))
                fe.assert_within(f"fuzz seed {seed}", ex[None], arg[None], ref, f"block {i - 1} B {cfg['B']} {cfg['setting'].name} rows {cfg['rb']}+{cfg['rcnt']}")
    print(f"EXCESS fuzz seed {seed} B {cfg['B']} {cfg['setting'].name}: device {worst:.3e} reference(family) {ref:.3e}")
