#!/usr/bin/env python3
"""What the reference-noise canceller (crsdr_plan_set_refcancel) costs a submit: 1025 rows x blocksize 16384, T = 20 blocks, device input.

  locked   CRSDR_REFNOISE_ENABLED | CRSDR_NO_LAG (the phase path alone) with the canceller off and with 1, 3 and 9 taps
  track    CRSDR_REFNOISE_ENABLED (cross-correlation + phase path), the same four
  parent   with --parent-lib LIB: the canceller-off submits of another build (e.g. the parent commit's) through CRSDR_LIB in a worker
           process of its own, timed in the same alternation, and beside it
  self     the canceller-off submits of this build in a worker process of the same kind (one plan, nothing else alive): the pair
           to compare -- this build's canceller-off submit must sit inside the run-to-run spread of the parent's

Every figure is the mean of --reps back-to-back submits closed by one sync; --runs rounds alternate all variants in one session (the
plans all alive throughout), medians and ranges are reported.  Per-kernel times come from the plan's event pairs
(crsdr_plan_enable_profiling) in a pass of their own behind the timed rounds: CRSDR_KERNEL_PHASE_DOT is k_phase_dot,
CRSDR_KERNEL_ALIGN_QUANT the rest of the phase path -- with the canceller on: k_align_quant for row 0, then the Gram, dots and apply
kernels.  --json FILE keeps the record."""
import argparse, importlib, json, os, statistics, subprocess, sys, time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NROWS, B, T = 1025, 16384, 20
TAPS = (0, 1, 3, 9)


def _setup(nrows, nblocks):
    sys.path.insert(0, ROOT)
    import torch
    b = importlib.import_module("coherent-rtlsdr_amd.binding")
    rng = np.random.default_rng(1)
    L = B // 2
    rows = np.empty((nblocks, nrows, 2 * L), dtype=np.int8)
    for t in range(nblocks):                   # every row carries the block's reference noise (at lag 0) and noise of its own
        ref = rng.normal(0, 25, 2 * L).astype(np.float32)
        own = rng.standard_normal((nrows, 2 * L), dtype=np.float32) * np.float32(6)
        rows[t] = np.clip(np.rint(0.7 * ref + own), -128, 127)
        rows[t, 0] = np.clip(np.rint(ref), -128, 127)
    d_in = torch.from_numpy(rows.view(np.uint8).reshape(nblocks, -1)).to(torch.device("cuda", 0))
    torch.cuda.synchronize()
    return torch, b, d_in


def _flags(b, kind):
    return b.REFNOISE_ENABLED | (b.NO_LAG if kind == "locked" else 0)


def _time(b, plan, d_in, kind, reps, nrows, nblocks):
    t0 = time.perf_counter()
    for i in range(reps):
        plan.submit(d_in.data_ptr(), seq=i * nblocks, flags=_flags(b, kind), nblocks=nblocks, block_stride=nrows * B)
    plan.sync()
    return (time.perf_counter() - t0) / reps


def worker(nrows, nblocks, reps):
    """the canceller-off plan of whatever build CRSDR_LIB names: 'locked' / 'track' on stdin -> seconds per submit on stdout"""
    torch, b, d_in = _setup(nrows, nblocks)
    plan = b.Plan(nrows, B, b.MODE_DIGITAL, max_batch=nblocks)
    for kind in ("track", "locked"):
        _time(b, plan, d_in, kind, 2, nrows, nblocks)
    print("ready", flush=True)
    for line in sys.stdin:
        print(_time(b, plan, d_in, line.strip(), reps, nrows, nblocks), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=NROWS)
    ap.add_argument("--blocks", type=int, default=T)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--parent-lib")
    ap.add_argument("--json")
    ap.add_argument("--worker", action="store_true")
    a = ap.parse_args()
    if a.worker:
        return worker(a.rows, a.blocks, a.reps)
    workers = {}
    if a.parent_lib:
        for name, env in (("self", dict(os.environ)), ("parent", dict(os.environ, CRSDR_LIB=os.path.abspath(a.parent_lib)))):
            workers[name] = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", "--rows", str(a.rows), "--blocks", str(a.blocks),
                                              "--reps", str(a.reps)], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, env=env)
            assert workers[name].stdout.readline().strip() == "ready"
    torch, b, d_in = _setup(a.rows, a.blocks)
    plans = {}
    for taps in TAPS:
        plans[taps] = b.Plan(a.rows, B, b.MODE_DIGITAL, max_batch=a.blocks)
        if taps:
            plans[taps].set_refcancel(taps)
        for kind in ("track", "locked"):
            _time(b, plans[taps], d_in, kind, 2, a.rows, a.blocks)
    rec = {f"{kind}:{taps}": [] for kind in ("locked", "track") for taps in TAPS}
    for name in workers:
        rec.update({f"locked:{name}": [], f"track:{name}": []})
    for _ in range(a.runs):
        for kind in ("locked", "track"):
            for taps in TAPS:
                rec[f"{kind}:{taps}"].append(_time(b, plans[taps], d_in, kind, a.reps, a.rows, a.blocks))
            for name, w in workers.items():
                w.stdin.write(kind + "\n"); w.stdin.flush()
                rec[f"{kind}:{name}"].append(float(w.stdout.readline()))
    for w in workers.values():
        w.stdin.close(); w.wait(timeout=60)
    out = {"rows": a.rows, "blocksize": B, "blocks": a.blocks, "runs": a.runs, "reps": a.reps, "ms_per_submit": {}, "kernel_ms": {}}
    for key, v in rec.items():
        ms = [1e3 * x for x in v]
        out["ms_per_submit"][key] = {"median": statistics.median(ms), "min": min(ms), "max": max(ms)}
        print(f"{key:>14}: {statistics.median(ms):8.3f} ms per submit of {a.blocks} blocks ({min(ms):.3f} .. {max(ms):.3f}), "
              f"{1e3 * a.blocks / statistics.median(ms):9.0f} blocks/s")
    # per-kernel times from the plan's event pairs, a pass of its own
    for taps in TAPS:
        p = plans[taps]
        p.enable_profiling(16, 0xF)
        for i in range(8):
            p.submit(d_in.data_ptr(), seq=i * a.blocks, flags=_flags(b, "locked"), nblocks=a.blocks, block_stride=a.rows * B)
        p.sync()
        dot, aq = p.kernel_times_ms(b.KERNEL_PHASE_DOT), p.kernel_times_ms(b.KERNEL_ALIGN_QUANT)
        k = {"phase_dot": float(np.median(dot)) if dot.size else 0.0, "align_quant": float(np.median(aq)) if aq.size else 0.0}
        out["kernel_ms"][str(taps)] = k
        print(f"taps {taps}: event pairs per locked submit: phase_dot {k['phase_dot']:.3f} ms, align_quant (+ canceller) {k['align_quant']:.3f} ms")
        p.enable_profiling(0)
        p.close()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
