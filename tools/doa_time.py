#!/usr/bin/env python3
"""Frames per second of the beamformer chain on the 7 x 3 array (22 rows x 16384, T = 64 device-resident packets), per-op against batched:

  (a) the per-op loop: crsdr_covariance -> crsdr_noisesubspace -> crsdr_pmusic2d with CRSDR_MEM_DEVICE pointers, once per packet
      (pm stays on the device: finding its peak is not even in the figure).  Run in a worker of its own, so that it can load an older
      build of the library (--perop-lib, e.g. the parent commit's) through CRSDR_LIB.
  (b) crsdr_doa_submit of the 64 packets + a fetch of the peaks only,
  (c) the same with the spectra kept and fetched (64 x 40 KB),
  (p) with --peaks COUNT --radius R: crsdr_doa_set_peaks(COUNT, R), then the submit + crsdr_doa_fetch_directions (the local-peak pass).
  (q) with --beams MODE (conventional | mvdr, --loading X) on top of --peaks: crsdr_doa_set_beams, then the submit + a fetch of the beams'
      power only (weights and beams stay on the device), and
  (h) what a caller without beams does to form them on the host: the (p) submit + directions, then the 64 packets and vec copied to
      page-locked host memory (before any host arithmetic).
  (f) with --fb: crsdr_doa_set_smoothing(7, 3, CRSDR_SMOOTH_FB) (forward-backward averaging alone), then the (b) submit + peaks,
  (s) with --smooth SXxSY: crsdr_doa_set_smoothing(SX, SY, CRSDR_SMOOTH_FB if --fb), then the (b) submit + peaks, and
  (o) with --order mdl|aic: crsdr_doa_set_order over k = 1 .. 20, then the (b) submit + peaks (on the unsmoothed covariance).
  (u) with --subbands NFFT:FIRST:COUNT[:WIDTH] [--window rect|hann]: crsdr_doa_set_subbands, then the (b) submit + the peaks of all
      64 x COUNT band matrices + the bands' power; reported with its frames/s and its ratio to (b).
  (v) with --band-beams MODE (conventional | mvdr, --loading X) on top of --subbands [--peaks]: crsdr_doa_set_subband_beams, then the
      submit + a fetch of the band beams' power only (weights and beams stay on the device), and
  (w) what a caller without them does to form the bands' beams on the host: the same object without the beams, submit + directions,
      then the 64 packets and vec of every band matrix copied to page-locked host memory (before any host arithmetic).
  (m) with --spectrum bartlett|capon (--loading X): crsdr_doa_set_spectrum, then the (b) submit + peaks: the power map in the scan's place,
      against the MUSIC submit (b) of the same build and, with --doa-lib, of another (lib:b) in the same alternation.
  (r) with --refine L [--peaks COUNT --radius R]: crsdr_doa_set_refine(L) on an object like (p)'s (or (b)'s without --peaks), then the
      submit + directions (or peaks) + crsdr_doa_fetch_refined: against (p) (or (b)) of the same build in the same alternation.
  (e) with --esprit beside|only [--subbands ...]: crsdr_doa_set_esprit on an object like (b)'s (or (u)'s with --subbands), then the
      submit + crsdr_doa_fetch_esprit of the angles alone (beside: + the peaks): against the MUSIC submit (b) (or (u)) of the same build in the same alternation.
  (g) with --augment VXxVY [--mask BITS]: crsdr_doa_set_augment (the filled VX x VY virtual array from the receivers of BITS, one
      character '0' / '1' per element in element order; without --mask all of them), then the (b) submit + peaks: against (b), the same
      submit without it, in the same alternation; reported with its frames/s.
--array MXxMY runs everything on another array than the 7 x 3 one (8x8: M = 64, the largest).

--runs runs of each, alternating a, b, c in one session (two worker processes, both alive throughout); medians and ranges.
--doa-lib LIB starts a second doa worker on another build (e.g. the parent commit's) through CRSDR_LIB and times its (b) and (c) in
the same alternation, reported as lib:b and lib:c.  --reps N: every (b), (c), (p), (q), (h) figure is the mean of N back-to-back submit + fetch.
Also: what crsdr_doa_submit_plan + the peak fetch add to a 22-row, T = 64 plan batch (plan.submit + sync against
plan.submit + doa.submit_plan + fetch).  --json FILE keeps the record; --once MODE runs three submit + fetch and exits (for a kernel trace): b, c, p, q as above, q64 = the
beams at their largest shape (8 x 8 array, 16 slots: 65 rows x 16384, 64 blocks), s = --smooth / --fb / --order as given, all on one object,
u = --subbands / --window as given, v = u with --peaks and --band-beams as given, m = --spectrum as given, r = --refine with --peaks as given,
e = --esprit (and --subbands) as given."""
import argparse, importlib, json, os, subprocess, sys, time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NROWS, B, T, M = 22, 16384, 64, 21
ARRAY = (7, 3)                             # --array: (mx, my), NROWS = 1 + mx my, M = mx my
SPECTRA = {"bartlett": 1, "capon": 2}
BEAM_MODES = {"conventional": 1, "mvdr": 2}
ORDER_MODES = {"mdl": 1, "aic": 2}
ESPRIT_MODES = {"beside": 1, "only": 2}
WINDOWS = {"rect": 0, "hann": 1}


def _bands(text):
    v = [int(x) for x in text.split(":")]
    if len(v) not in (3, 4):
        raise ValueError("--subbands NFFT:FIRST:COUNT[:WIDTH]")
    return v + [1] * (4 - len(v))


def _sub_array(text):
    sx, sy = text.lower().split("x")
    return int(sx), int(sy)


def _set_array(text):
    """--array MXxMY: the one place the shape constants change, straight after parsing (the workers get the option passed on)."""
    global ARRAY, NROWS, M
    if text:
        ARRAY = _sub_array(text)
        M = ARRAY[0] * ARRAY[1]
        NROWS = M + 1


def _setup(mx=None, my=None):
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    import ura
    b = importlib.import_module("coherent-rtlsdr_amd.binding")
    rng = np.random.default_rng(1)
    dev = torch.device("cuda", 0)
    mx, my = mx or ARRAY[0], my or ARRAY[1]
    nrows = 1 + mx * my
    off = 16 + 4 * nrows
    stride = off + nrows * B
    host = np.zeros((T, stride), dtype=np.int8)
    for t in range(T):
        host[t, off:] = ura.scene(B // 2, [(0.6 + 0.03 * t, 1.2 + 0.02 * t, 1.0)], rng, mx=mx, my=my).reshape(-1)
    pk = torch.from_numpy(host).to(dev)
    return torch, ura, b, dev, pk, off, stride, host


def worker_perop():
    """(a): one line 'ready', then for every line on stdin one timed loop over the 64 packets and its seconds on stdout."""
    import ctypes as C
    torch, ura, b, dev, pk, off, stride, _ = _setup()
    L = b.lib()
    f32p, i8p = C.POINTER(C.c_float), C.POINTER(C.c_int8)
    rxx = torch.zeros(M * M * 2, dtype=torch.float32, device=dev)
    vec = torch.zeros(M * M * 2, dtype=torch.float32, device=dev)
    sv = torch.zeros(M, dtype=torch.float32, device=dev)
    pm = torch.zeros(100 * 100, dtype=torch.float32, device=dev)
    fp = lambda t: C.cast(C.c_void_p(t.data_ptr()), f32p)

    def loop():
        for t in range(T):
            m = C.cast(C.c_void_p(pk.data_ptr() + t * stride + off), i8p)
            b._check(L.crsdr_covariance(fp(rxx), m, NROWS, B, b.MEM_DEVICE))
            b._check(L.crsdr_noisesubspace(fp(vec), fp(sv), fp(rxx), M, b.MEM_DEVICE))
            b._check(L.crsdr_pmusic2d(fp(pm), fp(vec), M, 1, float(ura.D), *ARRAY, 100, 100, b.MEM_DEVICE))
    loop()
    print("ready", flush=True)
    for _ in sys.stdin:
        t0 = time.perf_counter()
        loop()
        print(time.perf_counter() - t0, flush=True)


def worker_doa(npeaks=0, radius=1, reps=1, beams=None, loading=1e-2, smooth=None, fb=False, order=None, subbands=None, window="rect", band_beams=None,
               spectrum=None, refine=0, esprit=None, augment=None, mask=None):
    """(b), (c), (p), (q), (h), (f), (s), (o) and the plan figures: 'b' / 'c' / 'p' / 'q' / 'h' / 'f' / 's' / 'o' / 'plan' / 'plan+doa' on
    stdin -> seconds of one batch of 64 on stdout."""
    torch, ura, b, dev, pk, off, stride, host = _setup()
    peaks = b.Doa(NROWS, B, 1, ura.D, *ARRAY, max_batch=T)
    full = b.Doa(NROWS, B, 1, ura.D, *ARRAY, max_batch=T, flags=b.DOA_KEEP_SPECTRUM)
    plan = b.Plan(NROWS, B, b.MODE_DIGITAL, max_batch=T)
    rows = torch.from_numpy(np.ascontiguousarray(host[:, off:])).to(dev)       # [T][nrows * B], the plan's device input
    pdoa = b.Doa(NROWS, B, 1, ura.D, *ARRAY, max_batch=T)
    dirs = None
    if npeaks:
        dirs = b.Doa(NROWS, B, 1, ura.D, *ARRAY, max_batch=T)
        dirs.set_peaks(npeaks, radius)
    bdoa = None
    if beams:
        bdoa = b.Doa(NROWS, B, 1, ura.D, *ARRAY, max_batch=T)
        if npeaks:
            bdoa.set_peaks(npeaks, radius)
        bdoa.set_beams(BEAM_MODES[beams], loading)
        hdoa = dirs or peaks
        pinned = torch.empty(pk.shape, dtype=torch.int8, pin_memory=True)

    extra = {}
    if fb:
        extra["f"] = b.Doa(NROWS, B, 1, ura.D, *ARRAY, max_batch=T)
        extra["f"].set_smoothing(*ARRAY, b.SMOOTH_FB)
    if smooth:
        extra["s"] = b.Doa(NROWS, B, 1, ura.D, *ARRAY, max_batch=T)
        extra["s"].set_smoothing(*_sub_array(smooth), b.SMOOTH_FB if fb else 0)
    if order:
        extra["o"] = b.Doa(NROWS, B, 1, ura.D, *ARRAY, max_batch=T)
        extra["o"].set_order(ORDER_MODES[order], 1, M - 1)
    if spectrum:
        extra["m"] = b.Doa(NROWS, B, 1, ura.D, *ARRAY, max_batch=T)
        extra["m"].set_spectrum(SPECTRA[spectrum], loading)
    if augment:
        extra["g"] = b.Doa(NROWS, B, 1, ura.D, *ARRAY, max_batch=T)
        extra["g"].set_augment(*_sub_array(augment), mask or 0)
    rdoa = None
    if refine:
        rdoa = b.Doa(NROWS, B, 1, ura.D, *ARRAY, max_batch=T)
        if npeaks:
            rdoa.set_peaks(npeaks, radius)
        rdoa.set_refine(refine)
    udoa = None
    if subbands:
        udoa = b.Doa(NROWS, B, 1, ura.D, *ARRAY, max_batch=T)
        udoa.set_subbands(*_bands(subbands), WINDOWS[window])

    edoa = None
    if esprit:
        edoa = b.Doa(NROWS, B, 1, ura.D, *ARRAY, max_batch=T)
        if subbands:
            edoa.set_subbands(*_bands(subbands), WINDOWS[window])
        edoa.set_esprit(ESPRIT_MODES[esprit])

    def run_e():
        for _ in range(reps):
            edoa.submit(pk.data_ptr(), stride, off, T)
            if esprit == "beside":
                edoa.fetch_peaks()
            edoa.fetch_esprit(want=("angles",))          # like (b): the directions alone, one copy
            if subbands:
                edoa.fetch_subbands()

    vdoa = wdoa = None
    if subbands and band_beams:
        vdoa, wdoa = (b.Doa(NROWS, B, 1, ura.D, *ARRAY, max_batch=T) for _ in range(2))
        for d in (vdoa, wdoa):
            d.set_subbands(*_bands(subbands), WINDOWS[window])
            if npeaks:
                d.set_peaks(npeaks, radius)
        vdoa.set_subband_beams(BEAM_MODES[band_beams], loading)
        wpinned = torch.empty(pk.shape, dtype=torch.int8, pin_memory=True)

    def run_v():
        for _ in range(reps):
            vdoa.submit(pk.data_ptr(), stride, off, T)
            vdoa.fetch_subband_beams(weights=False, beams=False)

    def run_w():
        for _ in range(reps):
            wdoa.submit(pk.data_ptr(), stride, off, T)
            wdoa.fetch_directions() if npeaks else wdoa.fetch_peaks()
            wpinned.copy_(pk, non_blocking=True)
            wdoa.fetch_subspace()
            torch.cuda.synchronize()

    def run_r():
        for _ in range(reps):
            rdoa.submit(pk.data_ptr(), stride, off, T)
            rdoa.fetch_directions() if npeaks else rdoa.fetch_peaks()
            rdoa.fetch_refined()

    def run_u():
        for _ in range(reps):
            udoa.submit(pk.data_ptr(), stride, off, T)
            udoa.fetch_peaks()
            udoa.fetch_subbands()

    def run_extra(d):
        def run():
            for _ in range(reps):
                d.submit(pk.data_ptr(), stride, off, T)
                d.fetch_peaks()
        return run

    def run_q():
        for _ in range(reps):
            bdoa.submit(pk.data_ptr(), stride, off, T)
            bdoa.fetch_beams(weights=False, beams=False)

    def run_h():
        for _ in range(reps):
            hdoa.submit(pk.data_ptr(), stride, off, T)
            hdoa.fetch_directions() if npeaks else hdoa.fetch_peaks()
            pinned.copy_(pk, non_blocking=True)
            hdoa.fetch_subspace()
            torch.cuda.synchronize()

    def run_b():
        for _ in range(reps):
            peaks.submit(pk.data_ptr(), stride, off, T)
            peaks.fetch_peaks()

    def run_c():
        for _ in range(reps):
            full.submit(pk.data_ptr(), stride, off, T)
            full.fetch()

    def run_p():
        for _ in range(reps):
            dirs.submit(pk.data_ptr(), stride, off, T)
            dirs.fetch_directions()

    def run_plan(n=10):
        for i in range(n):
            plan.submit(rows.data_ptr(), nblocks=T, seq=i * T)
        plan.sync()

    def run_plan_doa(n=10):
        for i in range(n):
            plan.submit(rows.data_ptr(), nblocks=T, seq=i * T)
            pdoa.submit_plan(plan)
            pdoa.fetch_peaks()
        plan.sync()
    jobs = {"b": (run_b, reps), "c": (run_c, reps), "plan": (run_plan, 10), "plan+doa": (run_plan_doa, 10)}
    if dirs is not None:
        jobs["p"] = (run_p, reps)
    if bdoa is not None:
        jobs["q"], jobs["h"] = (run_q, reps), (run_h, reps)
    for key, d in extra.items():
        jobs[key] = (run_extra(d), reps)
    if rdoa is not None:
        jobs["r"] = (run_r, reps)
    if udoa is not None:
        jobs["u"] = (run_u, reps)
    if edoa is not None:
        jobs["e"] = (run_e, reps)
    if vdoa is not None:
        jobs["v"], jobs["w"] = (run_v, reps), (run_w, reps)
    for f, _ in jobs.values():
        f()
    print("ready", flush=True)
    for line in sys.stdin:
        f, n = jobs[line.strip()]
        t0 = time.perf_counter()
        f()
        print((time.perf_counter() - t0) / n, flush=True)


def once(mode, npeaks=0, radius=1, beams=None, loading=1e-2, smooth=None, fb=False, order=None, subbands=None, window="rect", band_beams=None, spectrum=None,
         refine=0, esprit=None):
    mx, my = (8, 8) if mode == "q64" else (None, None)
    torch, ura, b, dev, pk, off, stride, _ = _setup(mx, my)
    mx, my = mx or ARRAY[0], my or ARRAY[1]
    d = b.Doa(1 + mx * my, B, 1, ura.D, mx, my, max_batch=T, flags=b.DOA_KEEP_SPECTRUM if mode == "c" else 0)
    if mode == "q64":
        npeaks, radius = 16, 1
    if mode in ("p", "q", "q64", "r") and npeaks:
        d.set_peaks(npeaks, radius)
    if mode == "r":
        d.set_refine(refine or 5)
    if mode in ("q", "q64"):
        d.set_beams(BEAM_MODES[beams or "mvdr"], loading)
    if mode == "s":
        if smooth or fb:
            d.set_smoothing(*(_sub_array(smooth) if smooth else (mx, my)), b.SMOOTH_FB if fb else 0)
        if order:
            d.set_order(ORDER_MODES[order], 1, d.ms - 1)
    if mode == "m":
        d.set_spectrum(SPECTRA[spectrum or "capon"], loading)
    if mode in ("u", "v") or (mode == "e" and subbands):
        d.set_subbands(*_bands(subbands), WINDOWS[window])
    if mode == "e":
        d.set_esprit(ESPRIT_MODES[esprit or "beside"])
    if mode == "v":
        if npeaks:
            d.set_peaks(npeaks, radius)
        d.set_subband_beams(BEAM_MODES[band_beams or "mvdr"], loading)
    for _ in range(3):
        d.submit(pk.data_ptr(), stride, off, T)
        out = d.fetch()
    if mode == "e":
        es = d.fetch_esprit()
        print("esprit angles of the first four, degrees", np.round(np.degrees(es["angles"][:4, 0]), 3).tolist(), "found", es["found"][:4].tolist(), "launches", d.last_launches())
        if esprit == "only":
            return
    if mode in ("u", "v"):
        print("band power of the first estimate", np.round(d.fetch_subbands()[0], 5).tolist())
    print("peaks", out["peak"][:4].tolist(), "launches", d.last_launches())
    if mode == "m":
        print("peak values of the first four, dB", np.round(10 * np.log10(out["peak_value"][:4]), 2).tolist())
    if mode == "s" and order:
        print("k", d.fetch_order()["k"].tolist())
    if mode == "r":
        print("refined offsets of the first", d.fetch_refined()["offsets"][0].tolist())
    if mode in ("p", "q", "q64", "r") and npeaks:
        print("directions of the first", d.fetch_directions()["peaks"][0].tolist())
    if mode == "v":
        print("slots", d.nbandbeams, "band beam power of the first estimate", d.fetch_subband_beams(weights=False, beams=False)["power"][:d.nbands].tolist())
    if mode in ("q", "q64"):
        print("slots", d.nbeams, "beam power of the first", d.fetch_beams(weights=False, beams=False)["power"][0].tolist())


class Worker:
    def __init__(self, mode, lib=None, extra=()):
        env = dict(os.environ)
        if lib:
            env["CRSDR_LIB"] = lib
        self.p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", mode, *extra], stdin=subprocess.PIPE,
                                  stdout=subprocess.PIPE, text=True, env=env)
        line = self.p.stdout.readline().strip()
        if line != "ready":
            raise RuntimeError(f"worker {mode} did not start: {line!r} (exit {self.p.poll()})")

    def run(self, what="go"):
        self.p.stdin.write(what + "\n"); self.p.stdin.flush()
        line = self.p.stdout.readline().strip()
        if not line:
            raise RuntimeError(f"worker died (exit {self.p.wait()})")     # nothing more is started on the device
        return float(line)

    def close(self):
        self.p.stdin.close()
        self.p.wait(timeout=60)


def _stat(xs):
    return {"median": float(np.median(xs)), "min": float(min(xs)), "max": float(max(xs))}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--worker", choices=["perop", "doa"])
    ap.add_argument("--once", choices=["b", "c", "p", "q", "q64", "s", "u", "v", "m", "r", "e"])
    ap.add_argument("--esprit", choices=sorted(ESPRIT_MODES), default=None, help="(e): the directions by 2-D ESPRIT beside the scan or in its place (crsdr_doa_set_esprit)")
    ap.add_argument("--refine", type=int, default=0, metavar="L", help="(r): the directions refined off the grid by L levels (crsdr_doa_set_refine)")
    ap.add_argument("--spectrum", choices=sorted(SPECTRA), default=None, help="(m): this power map in the scan's place (crsdr_doa_set_spectrum, --loading for capon)")
    ap.add_argument("--array", default=None, metavar="MXxMY", help="the array, 2 <= MX MY <= 64 (default 7x3)")
    ap.add_argument("--subbands", default=None, metavar="NFFT:FIRST:COUNT[:WIDTH]", help="(u): a covariance per frequency band (crsdr_doa_set_subbands)")
    ap.add_argument("--window", choices=sorted(WINDOWS), default="rect", help="(u): the segments' window")
    ap.add_argument("--smooth", default=None, metavar="SXxSY", help="(s): sub-arrays of SX x SY elements (crsdr_doa_set_smoothing)")
    ap.add_argument("--fb", action="store_true", help="(f): forward-backward averaging alone; with --smooth: (s) averages backward as well")
    ap.add_argument("--augment", default=None, metavar="VXxVY", help="(g): the covariance of a filled VX x VY virtual array (crsdr_doa_set_augment)")
    ap.add_argument("--mask", default=None, metavar="BITS", help="(g): the receivers that are present, one character 0 / 1 per element (default: all)")
    ap.add_argument("--order", choices=sorted(ORDER_MODES), default=None, help="(o): the source count per estimate (crsdr_doa_set_order)")
    ap.add_argument("--beams", choices=sorted(BEAM_MODES), default=None, help="(q), (h): beams toward the directions, this mode")
    ap.add_argument("--band-beams", choices=sorted(BEAM_MODES), default=None, help="(v), (w): with --subbands, a beam per band toward its directions, this mode")
    ap.add_argument("--loading", type=float, default=1e-2, help="(q), (v): the MVDR diagonal loading")
    ap.add_argument("--perop-lib", default=None, help="library for (a), e.g. a build of the parent commit (default: the current one)")
    ap.add_argument("--doa-lib", default=None, help="a second library whose (b) and (c) are timed in the same alternation (lib:b, lib:c)")
    ap.add_argument("--peaks", type=int, default=0, help="(p): directions per estimate (crsdr_doa_set_peaks count; 0 = no (p))")
    ap.add_argument("--radius", type=int, default=1, help="(p): the local-peak window's radius")
    ap.add_argument("--reps", type=int, default=1, help="submit + fetch pairs per (b), (c), (p), (q), (h) figure")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    _set_array(a.array)                      # first thing: every worker, --once and the record read the shape from the globals
    shape = ["--array", a.array] if a.array else []
    if a.worker:
        return worker_perop() if a.worker == "perop" else worker_doa(a.peaks, a.radius, a.reps, a.beams, a.loading, a.smooth, a.fb, a.order, a.subbands, a.window,
                                                                           a.band_beams, a.spectrum, a.refine, a.esprit, a.augment, a.mask)
    if a.band_beams and not a.subbands:
        ap.error("--band-beams needs --subbands")
    if a.once:
        return once(a.once, a.peaks, a.radius, a.beams, a.loading, a.smooth, a.fb, a.order, a.subbands, a.window, a.band_beams, a.spectrum, a.refine, a.esprit)
    pargs = shape + ["--peaks", str(a.peaks), "--radius", str(a.radius), "--reps", str(a.reps), "--loading", str(a.loading)]
    if a.spectrum:
        pargs += ["--spectrum", a.spectrum]
    if a.beams:
        pargs += ["--beams", a.beams]
    if a.smooth:
        pargs += ["--smooth", a.smooth]
    if a.fb:
        pargs += ["--fb"]
    if a.order:
        pargs += ["--order", a.order]
    if a.subbands:
        pargs += ["--subbands", a.subbands, "--window", a.window]
    if a.band_beams:
        pargs += ["--band-beams", a.band_beams]
    if a.refine:
        pargs += ["--refine", str(a.refine)]
    if a.esprit:
        pargs += ["--esprit", a.esprit]
    if a.augment:
        pargs += ["--augment", a.augment] + (["--mask", a.mask] if a.mask else [])
    legs = (["f"] if a.fb else []) + (["s"] if a.smooth else []) + (["o"] if a.order else []) + (["u"] if a.subbands else []) + (["v", "w"] if a.band_beams else []) + (["m"] if a.spectrum else []) + (["r"] if a.refine else []) + (["e"] if a.esprit else []) + (["g"] if a.augment else [])
    wa, wb = Worker("perop", a.perop_lib, extra=shape), Worker("doa", extra=pargs)
    wl = Worker("doa", a.doa_lib, extra=shape + ["--reps", str(a.reps)]) if a.doa_lib else None
    keys = ["a", "b", "c", "plan", "plan+doa"] + (["lib:b", "lib:c"] if wl else []) + (["p"] if a.peaks else []) + (["q", "h"] if a.beams else []) + legs
    sec = {k: [] for k in keys}
    try:
        for _ in range(a.runs):
            sec["a"].append(wa.run())
            sec["b"].append(wb.run("b"))
            if wl:
                sec["lib:b"].append(wl.run("b"))
            sec["c"].append(wb.run("c"))
            if wl:
                sec["lib:c"].append(wl.run("c"))
            if a.peaks:
                sec["p"].append(wb.run("p"))
            if a.beams:
                sec["q"].append(wb.run("q"))
                sec["h"].append(wb.run("h"))
            for k in legs:
                sec[k].append(wb.run(k))
            sec["plan"].append(wb.run("plan"))
            sec["plan+doa"].append(wb.run("plan+doa"))
    finally:
        wa.close(); wb.close()
        if wl:
            wl.close()
    rec = {"shape": {"nrows": NROWS, "blocksize": B, "blocks": T, "grid": [100, 100]}, "runs": a.runs, "reps": a.reps,
           "perop_lib": a.perop_lib or "current build", "doa_lib": a.doa_lib, "peaks": {"count": a.peaks, "radius": a.radius} if a.peaks else None,
           "beams": {"mode": a.beams, "loading": a.loading} if a.beams else None,
           "smoothing": {"sub_array": a.smooth, "fb": a.fb} if (a.smooth or a.fb) else None, "order": a.order,
           "subbands": dict(zip(("nfft", "first", "nbands", "width"), _bands(a.subbands)), window=a.window) if a.subbands else None,
           "band_beams": {"mode": a.band_beams, "loading": a.loading} if a.band_beams else None,
           "spectrum": {"kind": a.spectrum, "loading": a.loading} if a.spectrum else None, "refine": a.refine or None, "esprit": a.esprit,
           "augment": {"virtual": a.augment, "mask": a.mask} if a.augment else None,
           "ms_per_batch": {k: _stat([1e3 * x for x in v]) for k, v in sec.items()},
           "frames_per_s": {k: _stat([T / x for x in sec[k]]) for k in ("a", "b", "c") + (("u",) if a.subbands else ()) + (("g",) if a.augment else ())}}
    if a.subbands:
        rec["u_over_b_ms"] = rec["ms_per_batch"]["u"]["median"] / rec["ms_per_batch"]["b"]["median"]
    rec["b_faster_than_a_ranges_disjoint"] = rec["ms_per_batch"]["b"]["max"] < rec["ms_per_batch"]["a"]["min"]
    rec["submit_plan_adds_ms_per_batch"] = rec["ms_per_batch"]["plan+doa"]["median"] - rec["ms_per_batch"]["plan"]["median"]
    names = {"a": "per-op loop, device pointers", "b": "doa submit + peaks", "c": "doa submit + peaks + spectra",
             "plan": "plan batch alone", "plan+doa": "plan batch + submit_plan + peaks", "lib:b": "--doa-lib: submit + peaks",
             "lib:c": "--doa-lib: submit + peaks + spectra", "p": f"set_peaks({a.peaks}, {a.radius}): submit + directions",
             "q": f"(p) + {a.beams} beams: submit + power", "h": "(p) + packets and vec to the host",
             "f": "FB alone: submit + peaks", "s": f"{a.smooth}{' + FB' if a.fb else ''}: submit + peaks", "o": f"order {a.order}: submit + peaks",
             "u": f"subbands {a.subbands} {a.window}: submit + peaks + power",
             "v": f"subbands + {a.band_beams} band beams: submit + power", "w": "subbands: packets and vec to the host",
             "m": f"{a.spectrum} map: submit + peaks", "r": f"refine {a.refine}: submit + directions + refined",
             "g": f"augment {a.augment}{' mask ' + a.mask if a.mask else ''}: submit + peaks",
             "e": f"esprit {a.esprit}{' + subbands' if a.subbands else ''}: submit + esprit"}
    for k, s in rec["ms_per_batch"].items():
        fps = f"  {T / (1e-3 * s['median']):10.0f} frames/s" if k in rec["frames_per_s"] else ""
        print(f"({k}) {names[k]:34s} {s['median']:8.3f} ms per 64 blocks  [{s['min']:.3f} .. {s['max']:.3f}]{fps}")
    print(f"(b) faster than (a), ranges disjoint: {rec['b_faster_than_a_ranges_disjoint']};  "
          f"a direction per block adds {rec['submit_plan_adds_ms_per_batch']:.3f} ms to a plan batch of 64")
    if a.subbands:
        print(f"(u) takes {rec['u_over_b_ms']:.2f} x the time of (b) for {_bands(a.subbands)[2]} x the matrices")
    for k in legs:
        rec[f"{k}_adds_ms_per_batch"] = rec["ms_per_batch"][k]["median"] - rec["ms_per_batch"]["b"]["median"]
        print(f"({k}) adds {1e3 * rec[f'{k}_adds_ms_per_batch']:.0f} us to (b)")
    if a.band_beams:
        rec["v_over_w_ms"] = rec["ms_per_batch"]["v"]["median"] / rec["ms_per_batch"]["w"]["median"]
        print(f"(v) takes {rec['v_over_w_ms']:.2f} x the time of (w)")
    if a.refine:
        base = "p" if a.peaks else "b"
        rec["r_adds_ms_per_batch_over"] = base
        rec["r_adds_ms_per_batch"] = rec["ms_per_batch"]["r"]["median"] - rec["ms_per_batch"][base]["median"]
        print(f"(r) adds {1e3 * rec['r_adds_ms_per_batch']:.0f} us to ({base}), the same submit without the refinement")
    if a.esprit:
        base = "u" if a.subbands else "b"
        rec["e_over"] = base
        rec["e_over_base_ms"] = rec["ms_per_batch"]["e"]["median"] / rec["ms_per_batch"][base]["median"]
        rec["e_minus_base_ms"] = rec["ms_per_batch"]["e"]["median"] - rec["ms_per_batch"][base]["median"]
        print(f"(e) takes {rec['e_over_base_ms']:.3f} x the time of ({base}), the MUSIC submit of the same build: {1e3 * rec['e_minus_base_ms']:+.0f} us")
    if a.augment:
        rec["g_over_b_ms"] = rec["ms_per_batch"]["g"]["median"] / rec["ms_per_batch"]["b"]["median"]
        print(f"(g) {rec['frames_per_s']['g']['median']:.0f} frames/s with augmentation, (b) {rec['frames_per_s']['b']['median']:.0f} frames/s without it: "
              f"{rec['g_over_b_ms']:.3f} x the time")
    if a.spectrum:
        rec["m_over_b_ms"] = rec["ms_per_batch"]["m"]["median"] / rec["ms_per_batch"]["b"]["median"]
        print(f"(m) takes {rec['m_over_b_ms']:.3f} x the time of (b), the MUSIC submit at k = 1; the scan's operation count is M / (M - 1) = {M / (M - 1):.3f} x")
        if wl:
            rec["m_over_lib_b_ms"] = rec["ms_per_batch"]["m"]["median"] / rec["ms_per_batch"]["lib:b"]["median"]
            print(f"(m) takes {rec['m_over_lib_b_ms']:.3f} x the time of lib:b")
    if wl:
        rec["b_minus_lib_b_ms"] = rec["ms_per_batch"]["b"]["median"] - rec["ms_per_batch"]["lib:b"]["median"]
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rec, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
