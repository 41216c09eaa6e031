"""The two-row K1 (csrc/xcorr14q.hpp, CRSDR_K1_VARIANT=q) against the packed kernel (CRSDR_K1_VARIANT=packed), bit for bit on
lag, mag and frac, at the smallest shapes that reach each path a group of the two-row kernel can take from one row to the next:

  first_only   1 + 5 rows x 3 blocks: 15 items on 8 workgroups -- every group has at most one item (no row before it, none behind)
  steady       rows x blocks between 2 x CUs + 1 and 3 x CUs (read from the device): some groups run two rows and some one, and a
               group's next row often lies in another block (another source pointer and reference spectrum)
  masked       the same shape with a lag mask that clears every third row, then one that clears runs of three consecutive rows
               (xcorr_skip between two rows of a group, and several in a row)
  offset       the same shape as offset-binary input (CRSDR_OFFSET_BINARY)
  run-out      CRSDR_K1_QSPIN=0: every bounded wait of the two-row kernel runs out at once; the kernel terminates by design, the
               error is raised, the plan rolls back, and the resubmitted batch gives the packed kernel's bits

The kernel's twiddles for the middle passes come from a table in LDS that 16 threads build per workgroup with the same tw_load the
packed kernel runs per row, so every case must agree exactly.  B = 16384, input resident on the device.  The variant is read once
per process: one child per variant computes all shapes.
"""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("first_only", "steady", "masked_third", "masked_runs", "offset")

CHILD = textwrap.dedent('''
    import importlib, sys, numpy as np, torch
    sys.path.insert(0, %r)
    pkg = importlib.import_module("coherent-rtlsdr_amd")
    b, synth = pkg.binding, pkg.synth
    L = 8192
    B = 2 * L
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    res = {"cus": np.int64(cus)}

    def on_device(blocks, offset_binary=False):
        u8 = blocks.view(np.uint8) ^ np.uint8(0x80) if offset_binary else blocks.view(np.uint8)
        return torch.from_numpy(np.ascontiguousarray(u8)).to("cuda")

    def fetch_all(plan, T, name):
        outs = [plan.fetch(want_packet=False, block=t) for t in range(T)]
        for key in ("lag", "mag", "frac"):
            res[name + "_" + key] = np.stack([o[key] for o in outs])

    runout = len(sys.argv) > 2 and sys.argv[2] == "runout"      # that child's waits all run out: it only does its own part

    if not runout:
        # every group has at most one item: 15 items, min(CUs, 8) workgroups of two groups
        nsig, T = 5, 3
        params = synth.RowParams(nsig, L, 1501, dmax=1500)
        blocks = np.stack([synth.make_block(nsig, L, 1501, t, params=params)[0] for t in range(T)])
        d_in = on_device(blocks)
        plan = b.Plan(nsig + 1, B, b.MODE_DIGITAL, max_batch=T)
        plan.submit(d_in.data_ptr(), seq=0, nblocks=T, block_stride=(nsig + 1) * B)
        fetch_all(plan, T, "first_only")
        res["first_only_d"] = params.d
        plan.close()

    # between two and three items per workgroup
    nsig = 41
    T = (5 * cus // 2) // nsig
    res["steady_items"] = np.int64(nsig * T)
    params = synth.RowParams(nsig, L, 1502, dmax=2500)
    blocks = np.stack([synth.make_block(nsig, L, 1502, t, params=params)[0] for t in range(T)])
    d_in = on_device(blocks)
    stride = (nsig + 1) * B
    if not runout:
        plan = b.Plan(nsig + 1, B, b.MODE_DIGITAL, max_batch=T)
        plan.submit(d_in.data_ptr(), seq=0, nblocks=T, block_stride=stride)
        fetch_all(plan, T, "steady")
        res["steady_d"] = params.d
        rows = np.arange(nsig + 1)
        third = (rows %% 3 != 0).astype(np.uint8)                 # every third row keeps its carried lag
        runs = ((rows // 3) %% 2 != 0).astype(np.uint8)           # runs of three consecutive rows do
        res["mask_third"], res["mask_runs"] = third, runs
        plan.submit(d_in.data_ptr(), seq=T, nblocks=T, block_stride=stride, lag_mask=third)
        fetch_all(plan, T, "masked_third")
        plan.submit(d_in.data_ptr(), seq=2 * T, nblocks=T, block_stride=stride, lag_mask=runs)
        fetch_all(plan, T, "masked_runs")
        plan.close()
        d_u8 = on_device(blocks, offset_binary=True)
        plan = b.Plan(nsig + 1, B, b.MODE_DIGITAL, max_batch=T)
        plan.submit(d_u8.data_ptr(), seq=0, nblocks=T, block_stride=stride, flags=b.REFNOISE_ENABLED | b.OFFSET_BINARY)
        fetch_all(plan, T, "offset")
        plan.close()

    if runout:
        # the same steady batch on a plan whose waits run out: error, roll-back, resubmission
        plan = b.Plan(nsig + 1, B, b.MODE_DIGITAL, max_batch=T)
        plan.submit(d_in.data_ptr(), seq=0, nblocks=T, block_stride=stride)
        try:
            plan.fetch(want_packet=False, block=0)
            print("NOERROR")
        except b.CrsdrError as e:
            print("ERROR", e)
            plan.submit(d_in.data_ptr(), seq=0, nblocks=T, block_stride=stride)
        fetch_all(plan, T, "resubmitted")
        plan.close()
    np.savez(sys.argv[1], **res)
''') % ROOT


def run_child(out, env, *args):
    r = subprocess.run([sys.executable, "-c", CHILD, str(out), *args], env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return np.load(out), r.stdout


@pytest.fixture(scope="module")
def variants(tmp_path_factory):
    d = tmp_path_factory.mktemp("k1_twshare")
    return {v: run_child(d / f"{v}.npz", {"CRSDR_K1_VARIANT": v})[0] for v in ("packed", "q")}


def test_shapes_reach_their_paths(variants):
    q = variants["q"]
    cus, items = int(q["cus"]), int(q["steady_items"])
    assert 2 * cus + 1 <= items <= 3 * cus, (cus, items)              # two or three items per workgroup: groups with two rows and with one
    assert 3 * 5 <= 2 * min(cus, 8)                                   # first_only: at most one item per group
    for name in ("first_only", "steady"):
        assert np.array_equal(q[name + "_lag"][:, 1:], np.broadcast_to(q[name + "_d"], q[name + "_lag"][:, 1:].shape)), name


@pytest.mark.parametrize("case", CASES)
def test_two_row_kernel_matches_packed_bit_for_bit(variants, case):
    for key in ("lag", "mag", "frac"):
        p, q = variants["packed"][f"{case}_{key}"], variants["q"][f"{case}_{key}"]
        assert p.shape == q.shape and p.size > 0
        assert np.array_equal(p.view(np.uint8), q.view(np.uint8)), (case, key, int(np.count_nonzero(p.view(np.uint8) != q.view(np.uint8))))


def test_masked_rows_keep_their_carried_values(variants):
    # what the masks are for: a cleared row republishes the state the last unmasked batch left (its last block's values)
    q = variants["q"]
    for name, prev in (("masked_third", "steady"), ("masked_runs", "masked_third")):
        keep = q["mask_" + name.split("_")[1]] == 0
        keep[0] = False                          # row 0 is the reference row: K1 has no item for it
        for key in ("lag", "mag", "frac"):
            carried = q[f"{prev}_{key}"][-1][keep]
            got = np.ascontiguousarray(q[f"{name}_{key}"][:, keep])
            assert np.array_equal(got.view(np.uint8), np.broadcast_to(carried, got.shape).copy().view(np.uint8)), (name, key)


def test_offset_binary_input_gives_the_signed_input_s_bits(variants):
    q = variants["q"]
    for key in ("lag", "mag", "frac"):
        assert np.array_equal(q["offset_" + key].view(np.uint8), q["steady_" + key].view(np.uint8)), key


def test_a_wait_that_runs_out_is_reported_and_rolled_back(variants, tmp_path):
    got, stdout = run_child(tmp_path / "runout.npz", {"CRSDR_K1_VARIANT": "q", "CRSDR_K1_QSPIN": "0"}, "runout")
    assert "ERROR" in stdout and "NOERROR" not in stdout, stdout
    assert "bounded wait" in stdout and "rolled back" in stdout, stdout
    for key in ("lag", "mag", "frac"):      # after the roll-back the plan keeps to the packed kernel: the resubmitted batch is the packed kernel's
        assert np.array_equal(got["resubmitted_" + key].view(np.uint8), variants["packed"]["steady_" + key].view(np.uint8)), key
