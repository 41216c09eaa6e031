"""Helpers of tests/test_gpu_long_chunks.py: the chunk split of the long-block stages as the plan computes it, plans created under
a chosen CRSDR_LONG_CHUNK_MB, and the child process that runs one block through plans under a chosen CRSDR_LONG_CHUNK_MB /
CRSDR_LONG_Q (the second is read once per process) and saves what they return.

The split (crsdr.hip, plan creation): rows per chunk = (MB << 20) / (8 B), at least 1; MB <= 0: one chunk; default 400 MB.  A chunk
of cnt rows takes the two-line stage-B kernel when CRSDR_LONG_Q is on and N1 * cnt >= 1024, N1 = B / 16384 (two_line())."""
import os
import subprocess
import sys
import textwrap

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_MB = 400
KEYS = ("lag", "mag", "frac", "phasor", "packet")
SWITCHES = ("CRSDR_LONG_CHUNK_MB", "CRSDR_LONG_Q", "CRSDR_K1_VARIANT", "CRSDR_K1_QSPIN")      # what decides the split and the stage-B kernel


def split(B: int, row_count: int, mb=None) -> list:
    """Rows of every chunk, in order; mb None: the default setting."""
    mb = DEFAULT_MB if mb is None else int(mb)
    per = row_count if mb <= 0 else max(1, (mb << 20) // (8 * B))
    return [min(per, row_count - r0) for r0 in range(0, row_count, per)]


def two_line(B: int, chunks: list, long_q: bool = True) -> list:
    """Per chunk: does its launch take the two-line kernel?"""
    return [bool(long_q) and (B // 16384) * cnt >= 1024 for cnt in chunks]


def d_vector(nrows: int) -> np.ndarray:
    """Override delays for the correction: a different one for every row, so that a row corrected with its neighbour's shows."""
    return np.linspace(-0.5, 0.5, nrows).astype(np.float32)


def plan(b, monkeypatch, mb, *args, **kw):
    """b.Plan(...) created under CRSDR_LONG_CHUNK_MB = mb (read at every plan creation)."""
    monkeypatch.setenv("CRSDR_LONG_CHUNK_MB", str(mb))
    return b.Plan(*args, **kw)


def same_bits(a, c, keys=KEYS, tag=""):
    for k in keys:
        assert np.array_equal(a[k].view(np.uint8), c[k].view(np.uint8)), (tag, k)


def child_main(b, argv):
    """argv: out.npz rows.npy job...; job = name:nrows:enable,enable...  Every job runs the first nrows rows of the block(s) in
    rows.npy [nblocks][rows][B] through a fresh digital-mode plan per enable (0: correction off, 1, 2: set_frac_apply(enable) with
    d_vector) and keeps the last block's outputs as name_enable_key."""
    out, blocks = argv[0], np.load(argv[1])
    res = {}
    for job in argv[2:]:
        name, nrows, enables = job.split(":")
        nrows = int(nrows)
        for enable in (int(e) for e in enables.split(",")):
            p = b.Plan(nrows, blocks.shape[2], b.MODE_DIGITAL)
            if enable:
                p.set_frac_apply(enable, 1.0, d_vector(nrows))
            for t in range(blocks.shape[0]):
                got = p.block(np.ascontiguousarray(blocks[t, :nrows]), seq=t)
            res.update({f"{name}_{enable}_{k}": got[k] for k in KEYS})
            p.close()
    np.savez(out, **res)


_CHILD = textwrap.dedent('''
    import importlib, sys
    sys.path[:0] = [%r, %r]
    pkg = importlib.import_module("coherent-rtlsdr_amd")
    import long_chunk_cases as lc
    lc.child_main(pkg.binding, sys.argv[1:])
''') % (ROOT, os.path.join(ROOT, "tests"))


def run_child(out, rows_file, jobs, mb, long_q, timeout=240):
    """One child under CRSDR_LONG_CHUNK_MB = mb (None: not set, the default) and CRSDR_LONG_Q = long_q (None: not set)."""
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    if mb is not None:
        env["CRSDR_LONG_CHUNK_MB"] = str(mb)
    if long_q is not None:
        env["CRSDR_LONG_Q"] = str(long_q)
    r = subprocess.run([sys.executable, "-c", _CHILD, str(out), str(rows_file)] + list(jobs), env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout + r.stderr
    return np.load(out)


def result(z, name, enable) -> dict:
    return {k: z[f"{name}_{enable}_{k}"] for k in KEYS}


def matrix(res, nrows, B):
    return res["packet"][16 + 4 * nrows:].reshape(nrows, B)
