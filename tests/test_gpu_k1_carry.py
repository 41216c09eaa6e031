"""The carried-chain two-row K1 (k_xcorr_lag14r, CRSDR_K1_VARIANT=r) against the packed kernel (CRSDR_K1_VARIANT=packed), bit for
bit on lag, mag, frac, phasor and the packet bytes.

k_xcorr_lag14r builds a thread's two column twiddle chains once before its row loop; from then on a row's last pass rebuilds them
and the next row's first pass uses what it finds (csrc/xcorr14q.hpp).  The chains are the same function of the same table values
wherever they are built, so every case must agree exactly.  The smallest shapes that reach each way a chain can arrive at a row:

  first_only   1 + 5 rows x 3 blocks: 15 items on 8 workgroups of two groups -- no group has a second row, only the chains built
               before the loop are used
  carried      320 signal rows x enough blocks for six items per workgroup (5 blocks = 1 600 items on 256 workgroups): every group
               runs three rows or more, so a row's chains are those the row before it rebuilt, twice over at least
  masked       the same batch again with a lag mask that clears signal rows 1, 161 and 320.  Item 0 (block 0, row 1) is the FIRST
               item of workgroup 0's group 0: its chains come from before the loop and must survive the skip.  The last item
               overall (last block, row 320) is the last draw that is not empty, so it is the LAST item of the group that draws
               it.  Row 161's items of the blocks in between are drawn in mid-launch: a skip BETWEEN two rows of a group.
  again        the same batch without the mask: a third submit on the plan
  offset       the same shape as offset-binary input (CRSDR_OFFSET_BINARY)
  run-out      CRSDR_K1_QSPIN=0: every bounded wait runs out at once; the kernel terminates by design, the error is raised, the
               plan rolls back, and the resubmitted batch gives the packed kernel's bits

carried, masked and again are three submits on one plan.  B = 16384, input resident on the device.  The variant is read once per
process: one child per variant computes all shapes.
"""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("first_only", "carried", "masked", "again", "offset")
KEYS = ("lag", "mag", "frac", "phasor", "packet")
NSIG = 320
MASKED_ROWS = (1, 161, 320)

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
        outs = [plan.fetch(want_packet=True, block=t) for t in range(T)]
        for key in %r:
            res[name + "_" + key] = np.stack([o[key] for o in outs])

    runout = len(sys.argv) > 2 and sys.argv[2] == "runout"      # that child's waits all run out: it only does its own part

    if not runout:
        # every group has at most one item: 15 items, min(CUs, 8) workgroups of two groups
        nsig, T = 5, 3
        params = synth.RowParams(nsig, L, 1601, dmax=1500)
        blocks = np.stack([synth.make_block(nsig, L, 1601, t, params=params)[0] for t in range(T)])
        d_in = on_device(blocks)
        plan = b.Plan(nsig + 1, B, b.MODE_DIGITAL, max_batch=T)
        plan.submit(d_in.data_ptr(), seq=0, nblocks=T, block_stride=(nsig + 1) * B)
        fetch_all(plan, T, "first_only")
        res["first_only_d"] = params.d
        plan.close()

    # six items per workgroup: three per group
    nsig = %d
    T = -(-6 * cus // nsig)
    res["carried_items"] = np.int64(nsig * T)
    params = synth.RowParams(nsig, L, 1602, dmax=2500)
    blocks = np.stack([synth.make_block(nsig, L, 1602, t, params=params)[0] for t in range(T)])
    d_in = on_device(blocks)
    stride = (nsig + 1) * B
    if not runout:
        plan = b.Plan(nsig + 1, B, b.MODE_DIGITAL, max_batch=T)
        plan.submit(d_in.data_ptr(), seq=0, nblocks=T, block_stride=stride)
        fetch_all(plan, T, "carried")
        res["carried_d"] = res["again_d"] = params.d
        mask = np.ones(nsig + 1, dtype=np.uint8)
        mask[list(%r)] = 0
        plan.submit(d_in.data_ptr(), seq=T, nblocks=T, block_stride=stride, lag_mask=mask)
        fetch_all(plan, T, "masked")
        plan.submit(d_in.data_ptr(), seq=2 * T, nblocks=T, block_stride=stride)
        fetch_all(plan, T, "again")
        plan.close()
        d_u8 = on_device(blocks, offset_binary=True)
        plan = b.Plan(nsig + 1, B, b.MODE_DIGITAL, max_batch=T)
        plan.submit(d_u8.data_ptr(), seq=0, nblocks=T, block_stride=stride, flags=b.REFNOISE_ENABLED | b.OFFSET_BINARY)
        fetch_all(plan, T, "offset")
        plan.close()

    if runout:
        # the carried batch on a plan whose waits run out: error, roll-back, resubmission
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
''') % (ROOT, KEYS, NSIG, MASKED_ROWS)


def run_child(out, env, *args):
    r = subprocess.run([sys.executable, "-c", CHILD, str(out), *args], env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return np.load(out), r.stdout


def same_bits(x, y):
    return x.shape == y.shape and x.size > 0 and np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8))


@pytest.fixture(scope="module")
def variants(tmp_path_factory):
    d = tmp_path_factory.mktemp("k1_carry")
    return {v: run_child(d / f"{v}.npz", {"CRSDR_K1_VARIANT": v})[0] for v in ("packed", "r")}


def test_shapes_reach_their_paths(variants):
    r = variants["r"]
    cus, items = int(r["cus"]), int(r["carried_items"])
    assert 3 * 5 <= 2 * min(cus, 8)                                   # first_only: at most one item per group
    assert items >= 6 * cus                                           # carried: three items per group on the average, all CUs in use
    for name in ("first_only", "carried", "again"):                   # and the lags are the ones the input was made with
        assert np.array_equal(r[name + "_lag"][:, 1:], np.broadcast_to(r[name + "_d"], r[name + "_lag"][:, 1:].shape)), name


@pytest.mark.parametrize("case", CASES)
def test_carried_chain_kernel_matches_packed_bit_for_bit(variants, case):
    for key in KEYS:
        p, r = variants["packed"][f"{case}_{key}"], variants["r"][f"{case}_{key}"]
        assert same_bits(p, r), (case, key, p.shape, r.shape)


def test_masked_rows_keep_their_carried_values(variants):
    # what the mask is for: a cleared row republishes the state the last unmasked batch left (its last block's values)
    r = variants["r"]
    rows = list(MASKED_ROWS)
    for key in ("lag", "mag", "frac"):
        carried = r[f"carried_{key}"][-1][rows]
        got = np.ascontiguousarray(r[f"masked_{key}"][:, rows])
        assert same_bits(got, np.broadcast_to(carried, got.shape).copy()), key
    keep = np.ones(NSIG + 1, dtype=bool)
    keep[rows] = False
    assert same_bits(r["masked_lag"][:, keep], r["carried_lag"][:, keep])      # the rows around a skipped one are computed as ever


def test_offset_binary_input_gives_the_signed_input_s_bits(variants):
    r = variants["r"]
    for key in ("lag", "mag", "frac"):
        assert same_bits(r["offset_" + key], r["carried_" + key]), key


def test_a_wait_that_runs_out_is_reported_and_rolled_back(variants, tmp_path):
    got, stdout = run_child(tmp_path / "runout.npz", {"CRSDR_K1_VARIANT": "r", "CRSDR_K1_QSPIN": "0"}, "runout")
    assert "ERROR" in stdout and "NOERROR" not in stdout, stdout
    assert "bounded wait" in stdout and "rolled back" in stdout, stdout
    for key in KEYS:      # after the roll-back the plan keeps to the packed kernel: the resubmitted batch is the packed kernel's
        assert same_bits(got["resubmitted_" + key], variants["packed"]["carried_" + key]), key
