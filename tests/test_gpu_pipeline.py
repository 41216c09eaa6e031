"""GPU: batches submitted the way bench.py times them, against the same blocks submitted one batch at a time.

bench.py drives a plan with resident device input (flags REFNOISE_ENABLED | INPUT_READY), on a caller stream (set_stream), into
bound device packet buffers, batch after batch with no sync in between, and a last batch of a region that can be shorter than
the rest.  That is the path where the cross-stream ordering of crsdr_plan_submit_batch matters: K0 (the reference spectra) runs on
the aux stream into one of two d_refspec slots, and at B = 16384 a batch whose launch is small folds K0 into K1 on the main stream
instead -- decided per batch, from the batch's length.  Batch lengths on both sides of that threshold, in a period-3 pattern,
put a folded and an unfolded batch on the same slot.

Every block of a run is a distinct synthetic block (its own reference row), so a spectrum of another block gives another answer.
Serialised runs are pinned bit-identical to batched and folded runs by test_gpu_plan.py: any difference here is an ordering bug.
"""
import importlib
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 8128


def _binding():
    return importlib.import_module("coherent-rtlsdr_amd.binding")


@pytest.fixture(scope="module")
def b():
    binding = _binding()
    if binding.device_count() < 1:
        pytest.fail("no HIP device: the product path has no CPU fallback")
    return binding


def fold_lengths(cus):
    """(big, small): batch lengths of 128-row launches that take the two-row kernel with K0 on the aux stream (>= 12 rows per
    CU) and the packed kernel with K0 folded in (below), a few blocks away from the threshold on either side."""
    per = -(-12 * cus // 128)
    return per + 4, max(1, per - 8)


# name: (nsig, L of the synthetic pool, what the plan sees)
POOLS = {"k14": (128, 8192), "generic": (64, 1024), "long": (32, 16384)}


def cases(cus):
    """The runs, as bench.py would issue them.  Every case's blocks are the first sum(batches) blocks of its pool."""
    big, small = fold_lengths(cus)
    return {
        # (a) one rank's slab of the 8-GPU run: 1 + 2R rows, this rank owns the second half (R = 128)
        "slab": dict(pool="k14", nrows=257, row_begin=129, row_count=128, batches=[big, big, small] * 2),
        # (b) the whole matrix, the region's last batch ragged
        "whole_ragged": dict(pool="k14", nrows=129, batches=[big, big, small, big, big, small - 5]),
        # (c) read counters every batch, a lag mask from the second batch on (the aux stream still does not wait for the
        #     main stream: the input is ready)
        "readcnt_mask": dict(pool="k14", nrows=129, batches=[big, small, big, big, small, big], readcnt=True, mask=True),
        # K0 always on the aux stream (generic kernels)
        "generic": dict(pool="generic", nrows=65, batches=[8, 8, 3] * 2),
        # long rows: one block per submit, the reference row's two stages on the aux stream
        "long": dict(pool="long", nrows=33, batches=[1] * 6),
    }


FOLD_CASES = ("slab", "whole_ragged", "readcnt_mask")


def make_pool(synth, name, count):
    nsig, L = POOLS[name]
    params = synth.RowParams(nsig, L, SEED + nsig)
    pool = np.stack([synth.make_block(nsig, L, SEED + nsig, t, params=params)[0] for t in range(count)])
    return pool, params.d


def case_block(case, pool, t):
    """Block t of the case as the plan sees it: the slab case repeats the signal rows, so that rows 129..256 are rows 1..128."""
    blk = pool[t]
    if case["nrows"] == blk.shape[0]:
        return blk
    return np.concatenate([blk[:1], blk[1:], blk[1:]])


def case_inputs(case, nblk):
    """(readcnt per batch, lag mask per batch): deterministic, the same in every process."""
    n, rng = case["nrows"], np.random.default_rng(SEED)
    rc, mk = [], []
    for i, nb in enumerate(case["batches"]):
        rc.append(rng.integers(0, 2 ** 32, size=(nb, n), dtype=np.uint32) if case.get("readcnt") else None)
        mask = None
        if case.get("mask") and i > 0:          # from the second batch on: a skipped row keeps the lag it was given before
            mask = (np.arange(n) % (2 + i % 3) != 1).astype(np.uint8)
        mk.append(mask)
    return rc, mk


def plan_args(case, B):
    return dict(nrows=case["nrows"], blocksize=B, mode=1, row_begin=case.get("row_begin", 0), row_count=case.get("row_count", 0),
                max_batch=max(case["batches"]))


def run_pipelined(b, case, pool):
    """The bench.py pattern: resident input, INPUT_READY, a caller stream, a bound packet region per batch, no sync between
    batches.  Returns every packet of the run and the last batch's scalars."""
    import torch
    B = pool.shape[-1]
    dev = torch.device("cuda", 0)
    batches = case["batches"]
    nblk, nrows = sum(batches), case["nrows"]
    rc, mk = case_inputs(case, nblk)
    plan = b.Plan(**plan_args(case, B))
    d_in = torch.empty((nblk, nrows * B), dtype=torch.uint8, device=dev)
    for t in range(nblk):
        d_in[t].copy_(torch.from_numpy(case_block(case, pool, t).view(np.uint8).reshape(-1)))
    pstride = (plan.packet_bytes + 255) // 256 * 256
    pk = torch.zeros(nblk * pstride + 256, dtype=torch.uint8, device=dev)
    off = (-(pk.data_ptr() + plan.matrix_offset)) % 16
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()                    # INPUT_READY: the caller promises the input is complete
    plan.set_stream(stream.cuda_stream)
    flags = b.REFNOISE_ENABLED | b.INPUT_READY
    first = 0
    for i, nb in enumerate(batches):
        plan.bind_packet(pk.data_ptr() + off + first * pstride, pstride)
        plan.submit(d_in[first].data_ptr(), readcnt=rc[i], lag_mask=mk[i], seq=1000 + first, flags=flags, nblocks=nb,
                    block_stride=nrows * B)
        first += nb
    stream.synchronize()
    last = [plan.fetch(want_packet=False, block=t) for t in range(batches[-1])]
    host = pk.cpu().numpy().view(np.int8)
    packets = np.stack([host[off + t * pstride: off + t * pstride + plan.packet_bytes] for t in range(nblk)])
    plan.close()
    out = {k: np.stack([o[k] for o in last]) for k in ("lag", "mag", "frac", "phasor")}
    out["packets"] = packets
    return out


def run_serialised(b, case, pool):
    """The same blocks and batch lengths from host memory, plan.sync() after every submit; every block's outputs."""
    B = pool.shape[-1]
    batches = case["batches"]
    rc, mk = case_inputs(case, sum(batches))
    plan = b.Plan(**plan_args(case, B))
    outs, first = [], 0
    for i, nb in enumerate(batches):
        rows = np.stack([case_block(case, pool, first + t) for t in range(nb)])
        plan.submit(rows, readcnt=rc[i], lag_mask=mk[i], seq=1000 + first, flags=b.REFNOISE_ENABLED)
        plan.sync()
        outs += [plan.fetch(block=t) for t in range(nb)]
        first += nb
    plan.close()
    return outs


_pools = {}


def pool_for(synth, cus, name):
    if name not in _pools:
        _pools[name] = make_pool(synth, name, max(sum(c["batches"]) for c in cases(cus).values() if c["pool"] == name))
    return _pools[name]


@pytest.fixture(scope="module")
def cus(b):
    return b.device_info(0)["compute_units"]


@pytest.fixture(scope="module")
def nofold(cus, synth, tmp_path_factory):
    """The pipelined runs of the B = 16384 cases in a child process with CRSDR_K1_FOLD=0 (read once per process): K0 on the aux
    stream for every batch."""
    tmp = tmp_path_factory.mktemp("nofold")
    pool, _ = pool_for(synth, cus, "k14")
    np.save(tmp / "pool.npy", pool)
    code = textwrap.dedent('''
        import sys, numpy as np
        sys.path[:0] = [%r, %r]
        import test_gpu_pipeline as m
        b = m._binding()
        pool = np.load(sys.argv[1])
        cs = m.cases(b.device_info(0)["compute_units"])
        res = {}
        for name in m.FOLD_CASES:
            for k, v in m.run_pipelined(b, cs[name], pool).items():
                res[name + "/" + k] = v
        np.savez(sys.argv[2], **res)
    ''') % (ROOT, HERE)
    out = tmp / "nofold.npz"
    r = subprocess.run([sys.executable, "-c", code, str(tmp / "pool.npy"), str(out)], env=dict(os.environ, CRSDR_K1_FOLD="0"),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    return np.load(out)


def _same(x, y):
    return x.shape == y.shape and np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8))


def _check_against_serialised(got, ser, batches, tag):
    nblk = sum(batches)
    assert got["packets"].shape[0] == nblk == len(ser)
    bad = [t for t in range(nblk) if not np.array_equal(got["packets"][t], ser[t]["packet"])]
    assert not bad, (tag, "packets differ from the serialised run", bad)
    last = ser[nblk - batches[-1]:]
    for k in ("lag", "mag", "frac", "phasor"):
        assert _same(got[k], np.stack([o[k] for o in last])), (tag, k)


@pytest.mark.parametrize("name", ["slab", "whole_ragged", "readcnt_mask", "generic", "long"])
def test_bench_submission_pattern_equals_serialised(b, synth, oracle, cus, name, request):
    case = cases(cus)[name]
    pool, d = pool_for(synth, cus, case["pool"])
    B = pool.shape[-1]
    if case["pool"] == "k14":                   # the pattern does cross the fold threshold, and puts both kinds on one slot
        kinds = ["q" if nb * 128 >= 12 * cus else "p" for nb in case["batches"]]
        assert any(kinds[i] != kinds[i + 2] for i in range(len(kinds) - 2)), kinds
    ser = run_serialised(b, case, pool)
    nrows = case["nrows"]
    own = np.zeros(nrows, dtype=bool)
    rb = case.get("row_begin", 1)
    own[rb: rb + case.get("row_count", nrows - 1)] = True
    # the serialised run is right: every signal row of every block finds its synthetic delay ...
    dl = np.concatenate([d, d]) if nrows == 2 * d.size + 1 else d
    for t, o in enumerate(ser):
        assert np.array_equal(o["lag"][own], dl[own[1:]]), (name, t)
    # ... and the first two batches of the slab case match the CPU oracle with the fuzz test's bars
    if name == "slab":
        from test_gpu_fuzz import _check_block
        orc = oracle.Engine(nrows, B, b.MODE_DIGITAL)
        clean = np.ones(nrows, dtype=bool)
        for t in range(sum(case["batches"][:2])):
            exp = orc.block(case_block(case, pool, t), lag_mask=own.astype(np.uint8), seq=1000 + t, nthreads=8)
            _check_block(ser[t], exp, own, True, (name, t), clean)
        orc.close()
    got = run_pipelined(b, case, pool)
    _check_against_serialised(got, ser, case["batches"], name)
    if name in FOLD_CASES:                      # the same pattern with K0 on the aux stream for every batch
        nf = request.getfixturevalue("nofold")
        for k in got:
            assert _same(got[k], nf[name + "/" + k]), (name, "CRSDR_K1_FOLD=0", k)


def test_folded_wait_that_ran_out_rolls_back_and_unfolds(tmp_path):
    # A folded launch's row workgroups wait, with a bounded budget, for their block's reference spectrum (xcorr14p.hpp).
    # CRSDR_K1_REFSPIN=-1@2 makes every row workgroup of the process's third and later folded launches report that wait as run
    # out.  The error must surface at the next status read (fetch, or fetch_wait of the pipelined host loop), name the folded
    # wait, roll back only the batches since the last clean read, and leave the plan unfolded: later batches do not fold (so
    # the switch, still in force, raises nothing more), and resubmitting gives bit for bit what a CRSDR_K1_FOLD=0 run gives.
    root = ROOT
    code = textwrap.dedent('''
        import importlib, sys, numpy as np
        sys.path.insert(0, %r)
        pkg = importlib.import_module("coherent-rtlsdr_amd")
        b, synth = pkg.binding, pkg.synth
        how = sys.argv[2]
        nsig, L, T, NB = 40, 8192, 5, 5                   # 200 rows per launch: the packed kernel, folded
        nrows, B = nsig + 1, 2 * L
        params = synth.RowParams(nsig, L, 515, dmax=1500)
        blocks = np.stack([synth.make_block(nsig, L, 515, t, params=params)[0] for t in range(NB * T)])
        batch = lambda i: blocks[i * T:(i + 1) * T]
        flags = lambda i: b.REFNOISE_ENABLED | (b.NO_LAG if i == NB - 1 else 0)     # the last batch is locked: it shifts by the carried lags
        plan = b.Plan(nrows, B, b.MODE_DIGITAL, max_batch=T)
        res, errors = {}, []
        if how == "sync":
            i = 0
            while i < NB:
                plan.submit(batch(i), seq=i * T, flags=flags(i))
                try:
                    res[i] = [plan.fetch(block=t) for t in range(T)]
                except b.CrsdrError as e:
                    errors.append(str(e))
                    lost = int(str(e).split("the last ")[1].split(" ")[0])
                    print("ERROR at batch", i, "lost", lost)
                    try:
                        plan.fetch(block=0)
                        print("STALE-FETCH-ALLOWED")
                    except b.CrsdrError:
                        pass                              # nothing to fetch until the batch is resubmitted
                    i = i + 1 - lost
                    continue
                i += 1
            res = {i: {k: np.stack([o[k] for o in r]) for k in ("lag", "mag", "frac", "phasor", "packet")} for i, r in res.items()}
        else:
            ps = plan.packet_stride
            rows_pin = [b.PinnedArray((T, nrows, B), np.int8) for _ in range(2)]
            out = [dict(lag=b.PinnedArray((T, nrows), np.int32), mag=b.PinnedArray((T, nrows), np.float32), frac=b.PinnedArray((T, nrows), np.float32),
                        phasor=b.PinnedArray((T, nrows, 2), np.float32), packets=b.PinnedArray((T * ps,), np.int8)) for _ in range(2)]
            def submit(i):
                s = i & 1
                rows_pin[s].array[:] = batch(i)
                plan.submit(rows_pin[s].array, seq=i * T, flags=flags(i))
                o = out[s]
                plan.fetch_batch_async(o["lag"].array, o["mag"].array, o["frac"].array, o["phasor"].array, o["packets"].array, ps)
            def collect(i):
                plan.fetch_wait()
                res[i] = {k: v.array.copy() for k, v in out[i & 1].items()}
            submit(0)
            i = 1
            while i < NB:
                submit(i)
                try:
                    collect(i - 1)
                except b.CrsdrError as e:
                    errors.append(str(e))
                    lost = int(str(e).split("the last ")[1].split(" ")[0])
                    first = i + 1 - lost
                    print("ERROR at collect", i - 1, "lost", lost, "first", first)
                    submit(first)
                    i = first + 1
                    continue
                i += 1
            collect(NB - 1)
        print("NERR", len(errors))
        for e in errors: print(e)
        np.savez(sys.argv[1], **{f"{k}{i}": v for i, r in res.items() for k, v in r.items()}, d=params.d)
    ''') % root
    outs = {}
    for how in ("sync", "async"):
        for name, env, nerr in (("runout", {"CRSDR_K1_REFSPIN": "-1@2"}, 1), ("nofold", {"CRSDR_K1_FOLD": "0"}, 0)):
            out = tmp_path / f"{how}_{name}.npz"
            r = subprocess.run([sys.executable, "-c", code, str(out), how], env=dict(os.environ, **env), capture_output=True, text=True,
                               timeout=300)
            assert r.returncode == 0, r.stdout + r.stderr
            assert f"NERR {nerr}" in r.stdout and "STALE-FETCH-ALLOWED" not in r.stdout, r.stdout + r.stderr
            if nerr:
                assert "bounded wait" in r.stdout and "rolled back" in r.stdout, r.stdout
                assert "folded launch's wait for its reference spectrum" in r.stdout and "two-row" not in r.stdout, r.stdout
                # batches 0 and 1 were read clean; sync: batch 2 alone is lost.  async: batch 3 was submitted behind batch 2 before
                # batch 2's status was read: both, never the clean ones
                assert ("ERROR at batch 2 lost 1" if how == "sync" else "ERROR at collect 2 lost 2 first 2") in r.stdout, r.stdout
            outs[name] = np.load(out)
        assert set(outs["nofold"].files) == set(outs["runout"].files) and len(outs["nofold"].files) == 5 * 5 + 1
        for key in outs["nofold"].files:
            assert _same(outs["nofold"][key], outs["runout"][key]), (how, key)
        assert np.array_equal(outs["runout"]["lag3"][:, 1:], np.broadcast_to(outs["runout"]["d"], (5, 40))), how
