#!/usr/bin/env python3
"""What a spectra submit (crsdr_spectra) adds behind a plan submit: (21 + 1) and (1024 + 1) rows x blocksize 16384, nfft 256 and 4096,
a batch of T = 64 device-resident blocks, half-overlapping Hann segments.

  plan      plan.submit of the 64 blocks + sync (digital mode, CRSDR_REFNOISE_ENABLED | CRSDR_NO_LAG: the phase path)
  +spectra  plan.submit + spectra.submit_plan + a fetch of the alignment figures only (psd and cross stay on the device)
  alone     spectra.submit on the packets the plan left + the same fetch: the three launches by themselves, and the achieved
            bytes/s over the packet bytes read once (T * nrows * blocksize)
  subband   (22 rows, nfft 256 only) crsdr_doa with crsdr_doa_set_subbands(256, 0, 1, 256, hann) on the same packets, submit + peaks:
            the covariance of all 21 x 21 pairs per bin (strictly more arithmetic per segment) with the subspace and the scan of
            its 64 matrices behind it; `doa` is the same object's submit without subbands, for what that tail costs

`frames` is the smallest power of two for which (T / frames) * nrows * nfft <= 2^24 (the engine's bound on its outputs): 1 for 22 rows,
2 (nfft 256) and 32 (nfft 4096) for 1025.  Every figure is the mean of --reps back-to-back rounds closed by one wait; --runs rounds
alternate all variants in one session, medians and ranges are reported.  --json FILE keeps the record."""
import argparse, importlib, json, os, statistics, sys, time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, T = 16384, 64


def _blocks(nrows, rng):
    """T blocks on the host: every row carries the block's reference noise (at lag 0) and noise of its own"""
    rows = np.empty((T, nrows, B), dtype=np.int8)
    for t in range(T):
        ref = rng.normal(0, 25, B).astype(np.float32)
        own = rng.standard_normal((nrows, B), dtype=np.float32) * np.float32(6)
        rows[t] = np.clip(np.rint(0.7 * ref + own), -128, 127)
        rows[t, 0] = np.clip(np.rint(ref), -128, 127)
    return rows


def _frames(nrows, nfft):
    f = 1
    while (T // f) * nrows * nfft > 1 << 24:
        f *= 2
    return f


def _mean(fn, wait, reps):
    t0 = time.perf_counter()
    for i in range(reps):
        fn(i)
    wait()
    return (time.perf_counter() - t0) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="*", default=[22, 1025])
    ap.add_argument("--nfft", type=int, nargs="*", default=[256, 4096])
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    b = importlib.import_module("coherent-rtlsdr_amd.binding")
    rng = np.random.default_rng(1)
    out = {"blocksize": B, "blocks": T, "runs": a.runs, "reps": a.reps, "shapes": []}
    for nrows in a.rows:
        d_in = torch.from_numpy(_blocks(nrows, rng).view(np.uint8).reshape(T, -1)).to(torch.device("cuda", 0))
        torch.cuda.synchronize()
        plan = b.Plan(nrows, B, b.MODE_DIGITAL, max_batch=T)
        flags = b.REFNOISE_ENABLED | b.NO_LAG
        submit = lambda i: plan.submit(d_in.data_ptr(), seq=i * T, flags=flags, nblocks=T, block_stride=nrows * B)
        variants = {"plan": lambda: _mean(submit, plan.sync, a.reps)}
        objs = []
        for nfft in a.nfft:
            frames = _frames(nrows, nfft)
            sp = b.Spectra(nrows, B, nfft, 1, b.WINDOW_HANN, band=(-(nfft // 10), nfft // 10), max_batch=T, frames=frames)
            objs.append(sp)
            pk = plan.device_buffers()["packet"]

            def with_plan(i, sp=sp):
                submit(i)
                sp.submit_plan(plan)
                sp.fetch(psd=False, cross=False)

            def alone(i, sp=sp):
                sp.submit(pk, plan.packet_stride, plan.matrix_offset, T)
                sp.fetch(psd=False, cross=False)

            variants[f"+spectra:{nfft}"] = lambda f=with_plan: _mean(f, plan.sync, a.reps)
            variants[f"alone:{nfft}"] = lambda f=alone: _mean(f, lambda: None, a.reps)
        if nrows - 1 <= 64 and 256 in a.nfft:
            import math
            mx = max(d for d in range(1, int(math.isqrt(nrows - 1)) + 1) if (nrows - 1) % d == 0)
            doa = b.Doa(nrows, B, 1, 0.5, (nrows - 1) // mx, mx, max_batch=T)
            sub = b.Doa(nrows, B, 1, 0.5, (nrows - 1) // mx, mx, max_batch=T)
            sub.set_subbands(256, 0, 1, 256, b.WINDOW_HANN)
            objs += [doa, sub]
            pk = plan.device_buffers()["packet"]

            def chain(i, d):
                d.submit(pk, plan.packet_stride, plan.matrix_offset, T)
                d.fetch_peaks()

            variants["doa"] = lambda: _mean(lambda i: chain(i, doa), lambda: None, a.reps)
            variants["subband:256"] = lambda: _mean(lambda i: chain(i, sub), lambda: None, a.reps)
        plan.submit(d_in.data_ptr(), seq=0, flags=b.REFNOISE_ENABLED, nblocks=T, block_stride=nrows * B)      # lags and phasors for the locked submits
        plan.sync()
        for fn in variants.values():             # warm-up: code objects, allocations
            fn()
        rec = {k: [] for k in variants}
        for _ in range(a.runs):
            for k, fn in variants.items():
                rec[k].append(fn())
        shape = {"nrows": nrows, "ms": {}}
        base = statistics.median(rec["plan"])
        for k, v in rec.items():
            ms = [1e3 * x for x in v]
            med = statistics.median(ms)
            shape["ms"][k] = {"median": med, "min": min(ms), "max": max(ms)}
            note = ""
            if k.startswith("+spectra"):
                note = f"  (+{med - 1e3 * base:.3f} ms behind the plan; frames {_frames(nrows, int(k.split(':')[1]))})"
            if k.startswith("alone"):
                note = f"  ({T * nrows * B / (med * 1e-3) / 1e9:.1f} GB/s over the packet bytes read once)"
            print(f"rows {nrows:5d} {k:>14}: {med:9.3f} ms ({min(ms):.3f} .. {max(ms):.3f}){note}")
        out["shapes"].append(shape)
        for o in objs:
            o.close()
        plan.close()
        del d_in
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
