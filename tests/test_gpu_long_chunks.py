"""Long blocks (B = 2^15 .. 2^22) through MORE THAN ONE chunk of the cf32 work area (CRSDR_LONG_CHUNK_MB; crsdr.hip: k1_long and
frac_pass).  Every other long-block shape of the suite is a single chunk, where the row offset r0 of a chunk is always 0; here each
offset the two loops carry is non-zero somewhere -- Y / Z + r0 B, row_begin + r0 into the input rows and the correction's per-row
arguments, d_part + r0 ntiles, d_rowspec + r0 8192, the packet's or the slab's rows + r0 B -- with the per-chunk decisions:
which stage-B kernel a chunk takes (the two-line kernel from N1 cnt >= 1024 lines on, N1 = B / 16384) and the all-or-nothing
`kept_fwd` of the block (the second work area is used only if EVERY chunk takes the two-line kernel).

Every case computes its split from B, the row count and the setting with the plan's own formula (long_chunk_cases.split) and
asserts it: none can pass on a single chunk, and a change of the formula shows up here.  Bars: bit for bit against the unchunked
plan (the chunks run the same kernels on the same rows); injected delays recovered exactly; the oracle / fp64 bars of
test_gpu_plan.py::test_long_block_plan_vs_oracle.  Where a block switches the stage-B kernel between chunks and the correction is
on, a row's bytes are those of the unchunked run that takes THAT row's apply kernel (the two apply kernels factor the response
differently: tests/test_gpu_frac_edges.py, long2)."""
import importlib

import numpy as np
import pytest

import long_chunk_cases as lc
from test_gpu_plan import _compare, _compare_model          # the bars of test_long_block_plan_vs_oracle, unchanged

pytestmark = pytest.mark.gpu

SCALARS = ("lag", "mag", "frac", "phasor")


@pytest.fixture(scope="module")
def b():
    binding = importlib.import_module("coherent-rtlsdr_amd.binding")
    if binding.device_count() < 1:
        pytest.fail("no HIP device: the product path has no CPU fallback")
    return binding


@pytest.mark.parametrize("mode", [0, 1])
def test_one_line_kernel_with_a_ragged_last_chunk(b, oracle, model, synth, monkeypatch, mode):
    # B = 2^15, 1 MB: 4 rows per chunk, 10 signal rows -> 4, 4, 2; two blocks, so that the EMA state carries
    nsig, B = 10, 1 << 15
    L = B // 2
    chunks = lc.split(B, nsig, 1)
    assert chunks == [4, 4, 2] and not any(lc.two_line(B, chunks)) and lc.split(B, nsig, 0) == [nsig]
    seed = 1510 + mode
    params = synth.RowParams(nsig, L, seed)
    chunked, whole = lc.plan(b, monkeypatch, 1, nsig + 1, B, mode), lc.plan(b, monkeypatch, 0, nsig + 1, B, mode)
    orc, mod = oracle.Engine(nsig + 1, B, mode), model.Model(nsig + 1, B, mode)
    for t in range(2):
        rows, _ = synth.make_block(nsig, L, seed, t, params=params)
        got, one, exp = chunked.block(rows, seq=t), whole.block(rows, seq=t), orc.block(rows, seq=t)
        assert np.array_equal(got["lag"][1:], params.d)
        _compare(got, exp, phase_tol=1e-5 if mode == 1 else 2e-4)
        _compare_model(got, mod.block(rows))
        lc.same_bits(got, one, tag=t)
    chunked.close(); whole.close()


def test_a_row_per_chunk(b, synth, monkeypatch):
    # B = 2^17, 1 MB: one row per chunk, five chunks
    nsig, B = 5, 1 << 17
    L = B // 2
    chunks = lc.split(B, nsig, 1)
    assert chunks == [1] * 5 and not any(lc.two_line(B, chunks))
    params = synth.RowParams(nsig, L, 1517)
    rows, _ = synth.make_block(nsig, L, 1517, 0, params=params)
    chunked, whole = lc.plan(b, monkeypatch, 1, nsig + 1, B, b.MODE_DIGITAL), lc.plan(b, monkeypatch, 0, nsig + 1, B, b.MODE_DIGITAL)
    got, one = chunked.block(rows), whole.block(rows)
    assert np.array_equal(got["lag"][1:], params.d)
    lc.same_bits(got, one)
    # and with the correction on (the one-line apply kernel in every chunk, on either side): the plan's own packet rows + r0 B
    for p in (chunked, whole):
        p.set_frac_apply(1, 1.0, lc.d_vector(nsig + 1))
    got, one = chunked.block(rows, seq=1), whole.block(rows, seq=1)
    assert np.array_equal(got["lag"][1:], params.d)
    lc.same_bits(got, one, tag="correction on")
    chunked.close(); whole.close()


def _switched_rows(chunked, q1, q0, nrows, B, chunks, tag):
    """Correction on, a block whose chunks do not all take the two-line kernel: the scalars, the header, the read counters and row 0
    equal both unchunked runs (which agree there); the rows of a chunk equal those rows of the unchunked run under CRSDR_LONG_Q=1
    where the chunk takes the two-line apply kernel, of the run under CRSDR_LONG_Q=0 where it takes the one-line kernel."""
    mo = 16 + 4 * nrows
    for other in (q1, q0):
        lc.same_bits(chunked, other, SCALARS, tag)
        assert np.array_equal(chunked["packet"][:mo + B], other["packet"][:mo + B]), tag
    got, m1, m0 = (lc.matrix(x, nrows, B) for x in (chunked, q1, q0))
    r0 = 1
    for cnt, two in zip(chunks, lc.two_line(B, chunks)):
        assert np.array_equal(got[r0:r0 + cnt], (m1 if two else m0)[r0:r0 + cnt]), (tag, r0, cnt, two)
        r0 += cnt
    assert r0 == nrows
    print(f"{tag}: bytes that differ between the two apply kernels, per row:", [int(np.count_nonzero(m1[r] != m0[r])) for r in range(1, nrows)])


K_B, K_NSIG, K_SWITCH = 1 << 20, 32, 19      # B = 2^20: N1 = 64, 128 MB = 16 rows per chunk, 16 rows = 1024 lines


@pytest.fixture(scope="module")
def two_line_runs(tmp_path_factory, synth):
    """One block of 1 + 32 rows at B = 2^20, generated once; three children: 128 MB chunks and one chunk under CRSDR_LONG_Q=1 (both
    the 32-row block and its first 19 signal rows), one chunk under CRSDR_LONG_Q=0 (the 19 rows)."""
    tmp = tmp_path_factory.mktemp("long_chunks")
    L = K_B // 2
    params = synth.RowParams(K_NSIG, L, 1520)
    rows, _ = synth.make_block(K_NSIG, L, 1520, 0, params=params)
    np.save(tmp / "rows.npy", rows[None])
    both = [f"k3:{K_NSIG + 1}:0,1,2", f"k4:{K_SWITCH + 1}:0,1"]
    return {"d": params.d,
            "chunked": lc.run_child(tmp / "chunked.npz", tmp / "rows.npy", both, 128, 1),
            "whole_q1": lc.run_child(tmp / "whole_q1.npz", tmp / "rows.npy", both, 0, 1),
            "whole_q0": lc.run_child(tmp / "whole_q0.npz", tmp / "rows.npy", both[1:], 0, 0)}


def test_two_line_kernel_in_every_chunk(two_line_runs):
    # 32 signal rows -> 16, 16, both two-line: with set_frac_apply(1) the block keeps stage A's output (kept_fwd) and the second
    # chunk works on d_Z + r0 B and d_rowspec + r0 8192
    chunks = lc.split(K_B, K_NSIG, 128)
    assert chunks == [16, 16] and all(lc.two_line(K_B, chunks)) and lc.split(K_B, K_NSIG, 0) == [K_NSIG]
    for enable in (0, 1, 2):
        got, one = lc.result(two_line_runs["chunked"], "k3", enable), lc.result(two_line_runs["whole_q1"], "k3", enable)
        assert np.array_equal(got["lag"][1:], two_line_runs["d"]), enable
        lc.same_bits(got, one, tag=enable)
    for run in ("chunked", "whole_q1"):
        a, c = lc.result(two_line_runs[run], "k3", 1), lc.result(two_line_runs[run], "k3", 2)
        assert np.array_equal(a["packet"], c["packet"]), run          # with and without the second work area


def test_kernel_switch_inside_a_block(two_line_runs):
    # 19 signal rows -> 16 (two-line) + 3 (one-line): the stage-B kernel changes inside the block and kept_fwd is off for all of it
    n = K_SWITCH + 1
    chunks = lc.split(K_B, K_SWITCH, 128)
    assert chunks == [16, 3] and lc.two_line(K_B, chunks) == [True, False]
    assert lc.two_line(K_B, lc.split(K_B, K_SWITCH, 0)) == [True] and lc.two_line(K_B, [K_SWITCH], long_q=False) == [False]
    runs = {k: {e: lc.result(two_line_runs[k], "k4", e) for e in (0, 1)} for k in ("chunked", "whole_q1", "whole_q0")}
    for e in (0, 1):
        assert np.array_equal(runs["chunked"][e]["lag"][1:], two_line_runs["d"][:K_SWITCH]), e
    # correction off: the two stage-B kernels are bit-identical, so everything equals both unchunked runs
    lc.same_bits(runs["chunked"][0], runs["whole_q1"][0], tag="q1")
    lc.same_bits(runs["chunked"][0], runs["whole_q0"][0], tag="q0")
    _switched_rows(runs["chunked"][1], runs["whole_q1"][1], runs["whole_q0"][1], n, K_B, chunks, "switch at 2^20")


def test_the_default_setting_chunks_at_the_largest_size(tmp_path, synth):
    # no environment variable: 400 MB, B = 2^22 -> 12 rows per chunk; 13 signal rows -> 12 (two-line, N1 = 256) + 1 (one-line)
    nsig, B = 13, 1 << 22
    L, n = B // 2, nsig + 1
    chunks = lc.split(B, nsig)
    assert chunks == [12, 1] and lc.two_line(B, chunks) == [True, False] and lc.two_line(B, lc.split(B, nsig, 0)) == [True]
    params = synth.RowParams(nsig, L, 1522, dmax=5000)
    rows, _ = synth.make_block(nsig, L, 1522, 0, params=params)
    np.save(tmp_path / "rows.npy", rows[None])
    del rows
    default = lc.run_child(tmp_path / "default.npz", tmp_path / "rows.npy", [f"k5:{n}:0,1"], None, None)
    whole_q1 = lc.run_child(tmp_path / "whole_q1.npz", tmp_path / "rows.npy", [f"k5:{n}:0,1"], 0, 1)
    whole_q0 = lc.run_child(tmp_path / "whole_q0.npz", tmp_path / "rows.npy", [f"k5:{n}:1"], 0, 0)
    for e in (0, 1):
        assert np.array_equal(lc.result(default, "k5", e)["lag"][1:], params.d), e
    lc.same_bits(lc.result(default, "k5", 0), lc.result(whole_q1, "k5", 0))
    _switched_rows(lc.result(default, "k5", 1), lc.result(whole_q1, "k5", 1), lc.result(whole_q0, "k5", 1), n, B, chunks, "default at 2^22")


@pytest.mark.parametrize("correction", [False, True], ids=["off", "on"])
def test_a_shard_with_chunks_fills_its_slab(b, synth, monkeypatch, correction):
    # a plan that owns rows 3 .. 9 of 12, 1 MB chunks -> 4, 3: row_begin + r0 into the input rows (and the correction's per-row
    # delays), the slab's rows + r0 B; rows and tails against an unsharded, unchunked plan on the same block
    import torch
    n, B, rb, rc = 12, 1 << 15, 3, 7
    L = B // 2
    chunks = lc.split(B, rc, 1)
    assert chunks == [4, 3] and not any(lc.two_line(B, chunks)) and lc.split(B, n - 1, 0) == [n - 1]
    params = synth.RowParams(n - 1, L, 1526)
    rows, _ = synth.make_block(n - 1, L, 1526, 0, params=params)
    readcnt = np.arange(n, dtype=np.uint32) * 3 + 100
    full = lc.plan(b, monkeypatch, 0, n, B, b.MODE_DIGITAL)
    shard = lc.plan(b, monkeypatch, 1, n, B, b.MODE_DIGITAL, row_begin=rb, row_count=rc)
    if correction:
        for p in (full, shard):
            p.set_frac_apply(1, 1.0, lc.d_vector(n))
    exp = full.block(rows, seq=5, readcnt=readcnt)
    assert np.array_equal(exp["lag"][1:], params.d)
    toff, slot = rc * B, rc * B + 256
    send = torch.full((slot,), 0x5A, dtype=torch.uint8, device=torch.device("cuda", 0))
    shard.bind_slab_ex(send.data_ptr(), slot, 0, 1, toff)
    shard.submit(rows, seq=5, readcnt=readcnt)
    shard.sync()
    raw = send.cpu().numpy()
    own = slice(rb, rb + rc)
    assert np.array_equal(raw[:rc * B].view(np.int8).reshape(rc, B), exp["matrix"][own])
    # the tail (kernels.hpp, k_pack_tails): lag | mag | frac | phasor | read counters of the owned rows
    tail = np.concatenate([exp[k][own].view(np.uint8) for k in SCALARS] + [readcnt[own].view(np.uint8)])
    assert tail.size == 24 * rc and np.array_equal(raw[toff:toff + tail.size], tail)
    full.close(); shard.close()


def test_full_scale_dc_rows_at_the_largest_size(b):
    # test_gpu_plan.py::test_full_scale_dc_rows_do_not_overflow at B = 2^22: every sample -128 - 128j, the largest values the
    # un-scaled transform chain meets.  The correlation peaks at lag 0 with B x the overlap energy: |ifft|^2 = P = (B L 32768)^2 =
    # 2^116 (< FLT_MAX = 2^128) and mag = sqrt(P / L) / 127^2.
    B = 1 << 22
    L = B // 2
    rows = np.full((2, B), -128, dtype=np.int8)
    plan = b.Plan(2, B, b.MODE_DIGITAL)
    got = plan.block(rows)
    assert np.all(np.isfinite(got["mag"])) and np.all(np.isfinite(got["frac"]))
    assert np.all(got["lag"] == 0)
    expect = np.sqrt(2.0 ** 116 / L) / 127.0 ** 2
    assert np.allclose(got["mag"][1:], expect, rtol=1e-4), (got["mag"], expect)
    plan.close()
