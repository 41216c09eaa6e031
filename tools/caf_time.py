#!/usr/bin/env python3
"""What a range-Doppler submit (crsdr_caf) adds behind a plan submit: (21 + 1) rows x blocksize 16384 at a batch of 64 blocks and
(1024 + 1) rows at a batch of 4; seg 128 and 4 packets a line (nd = 256), Hann over slow time, guard 2.  The 22-row case computes 64
lags; with 1025 rows one line of 256 x 64 cells is 2^14 cells over the engine's bound of 2^24, so that case computes 63.

  plan       plan.submit of the batch + sync (digital mode, CRSDR_REFNOISE_ENABLED | CRSDR_NO_LAG: the phase path)
  +caf       plan.submit + caf.submit_plan + a fetch of the peaks only (chi and map stay on the device)
  caf        caf.submit on the packets the plan left + the same fetch: the three launches by themselves, the achieved bytes/s of the chi
             store (8 bytes a cell) and the int8 complex multiply-adds per second of the range stage
  +spectra   for scale: plan.submit + spectra.submit_plan (nfft 256, half-overlapping Hann segments) + a fetch of its figures
  spectra    the spectra's three launches by themselves
  host       what a user has without the engine: the batch's packets fetched to page-locked host memory
  host+model that fetch and tests/caf_model.py (numpy, fp64) on ONE line of the batch -- measured once, not per round
with --cfar, on a second engine with the CFAR detector set (crsdr_caf_set_cfar: guard 1 x 1, training 3 x 4, alpha for 1e-6 at 90 cells,
16 detections a map):
  caf+cfar   as caf with the detector's two launches behind the three, + a fetch of det, count and snap as well
  get chi    the fetch of chi (pageable host memory, as Caf.fetch returns it) that the detection lists stand in for
  get cfar   the fetch of det + count + snap
and the bytes of P the detector reads per submit (8 a cell of chi, 4 a cell of map), to set against its kernels' time from a profiler.
with --cfar --estimator, on three further engines with the same detector under another noise estimate (crsdr_caf_set_cfar_estimator), each with
the alpha of 1e-6 under its own estimate (crsdr_cfar_alpha_est):
  cfar go    as caf+cfar under greatest-of over lag (42 cells a half)
  cfar so    as caf+cfar under smallest-of over lag
  cfar os    as caf+cfar under the ordered statistic of rank 67 of 90
each against the same build's caf+cfar: the tiles' kernel is the only launch that differs.
with --cancel K[:P], on a further engine with the canceller set (crsdr_caf_set_cancel: K delays of the reference at -P .. P Doppler bins):
  caf+cancel as caf with the canceller's five launches in the place of the rows' one, + a fetch of coef and cinfo as well; beside it the
             fp64 multiply-adds of the subtraction (n complex ones a cell) per second
with --bearing (implies --cfar; shapes whose signal rows are a 7 x 3 array, 22 rows), on three further engines whose detector has the
threshold alpha = 3, so that noise fills every one of the 16 slots of every line, two of them with bearings set (crsdr_caf_set_bearing:
spacing 0.506, a 100 x 100 grid, 5 zoom levels; conventional, and adaptive at loading 1e-2):
  cfar low   as caf+cfar at that threshold: the same build's submit without bearings
  +brg conv  as cfar low with the bearings' three launches behind the detector's, + a fetch of dir as well
  +brg adpt  the same in the adaptive mode
  get dir    the fetch of dir, against "get chi" + "get cfar" (snap among it) that a user's own bearing estimate would need
with --beams NB (shapes of 22 rows; NB a square number up to 64), on four further engines, two of them with a lattice of NB conventional
beams of the 7 x 3 array set (crsdr_caf_set_beams), without the detector and with it (alpha for 1e-6 at 90 cells, 16 detections a map):
  caf b      as caf: the same build's submit without beams
  +beams     as caf b with the beam maps' one launch behind the three; bmap stays on the device
  cfar b     as caf+cfar: the same build's submit with the detector and without beams
  +beams det as cfar b with the beams' four launches behind the detector's, + a fetch of fused and nfused as well
  get fused  the fetch of fused + nfused, against "get chi" that a user's own beamformer would need
and the beam kernel's two bounds for the shape: the bytes it must move, and its MFMAs' cycles.
with --track (22 rows), on two further engines whose detector has the threshold alpha = 3 and 64 detections a map, so that noise fills
the lists -- the tracker's worst case: a 128 x 64 table of d2 every line -- one of them with the tracker set (crsdr_caf_set_track: 128
slots, 3 of 5, gate 9, the array map's list):
  cfar trk   as caf+cfar at that threshold: the same build's submit without the tracker
  +track     as cfar trk with the tracker's one launch behind the detector's, + a fetch of trk and ntrk in the place of det and count
  get trk    the fetch of trk + ntrk, against "get lists", the fetch of det + count that a host tracker would need every submit
with --adapt --beams NB [--cfar], on a further engine with the beams set (with --cfar: and the detector), the same object in turn without
and with the adaptive weights (crsdr_caf_set_beam_adapt: loading 1e-2, the whole map less the zero-Doppler guard):
  adapt off  the submit with the beams alone, + the fetches of "+beams" / "+beams det"
  +adapt     the same with the adaptation's two launches ahead of the beam maps; against m N 8 bytes of chi read once a line, and
             beside "+beams" less "caf b", the beam kernel's own time on the same cells
with --integrate [--beams NB], on a further engine with the integration across lines set (crsdr_caf_set_integrate: forget 1 / 8, coupling
0.05; with --beams on the "+beams" engine's twin as well, array and beam maps):
  integ off  as caf, on the object of the next line with the integration turned off: the same build's submit without.  On and off are
             one object, set in front of every round outside the clock: two objects of one configuration differ by as much as the stage
  +integ     that object with the integration's one launch behind the map; imap stays on the device.  Beside it the stage's bytes (8 a
             cell and line, 16 a cell of state) over the difference, and those bytes against the array-map kernel's, which reads nrows - 1 chi
  integ off bm, +integ bm   the same on an engine with beams: both integration launches
  integ op   crsdr_map_integrate on device memory at the engine's shape: the launch, its wait, and nothing else
  integ big  the same at 64 lines of 16 maps (2^24 cells, 138 MB): the kernel where the launch no longer counts, as bytes / s
with --parent-lib LIB beside it: "caf" -- the integration-off submit -- of another build (e.g. the parent commit's) through CRSDR_LIB in a
worker process, in the same alternation ("caf parent", and "caf self" from a worker of this build).

Every figure is the mean of --reps back-to-back rounds closed by one wait; --runs rounds alternate all variants in one session, medians
and ranges are reported.  --json FILE keeps the record.
with --clean T, and nothing else: a 22-row engine with the canceller (4:1) and the detector, the same object in turn with the second
cancellation stage off, on without picks and on with T picks in every line (crsdr_caf_set_clean; T movers are put into the rows):
  clean off / +clean, no picks / +clean, T picks, and the share of the second pass (rows, map, detector again) in what the stage adds
"""
import argparse, importlib, json, os, statistics, subprocess, sys, time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, SEG, FRAMES, GUARD = 16384, 128, 4, 2
SHAPES = {22: (64, 64), 1025: (4, 63)}           # nrows: (batch, lags)


def _blocks(T, nrows, rng):
    """T blocks on the host: every row carries the block's reference noise (at lag 0) and noise of its own"""
    rows = np.empty((T, nrows, B), dtype=np.int8)
    for t in range(T):
        ref = rng.normal(0, 25, B).astype(np.float32)
        own = rng.standard_normal((nrows, B), dtype=np.float32) * np.float32(6)
        rows[t] = np.clip(np.rint(0.7 * ref + own), -128, 127)
        rows[t, 0] = np.clip(np.rint(ref), -128, 127)
    return rows


def _mean(fn, wait, reps):
    t0 = time.perf_counter()
    for i in range(reps):
        fn(i)
    wait()
    return (time.perf_counter() - t0) / reps


def worker(nrows, reps):
    """the plain submit ("caf") of whatever build CRSDR_LIB names: a line on stdin -> seconds per submit on stdout"""
    sys.path.insert(0, ROOT)
    import torch
    b = importlib.import_module("coherent-rtlsdr_amd.binding")
    T, lags = SHAPES.get(nrows, (FRAMES, 16))
    d_in = torch.from_numpy(_blocks(T, nrows, np.random.default_rng(1)).view(np.uint8).reshape(T, -1)).to(torch.device("cuda", 0))
    plan = b.Plan(nrows, B, b.MODE_DIGITAL, max_batch=T)
    cf = b.Caf(nrows, B, SEG, lags, 0, b.WINDOW_HANN, GUARD, max_batch=T, frames=FRAMES)
    plan.submit(d_in.data_ptr(), seq=0, flags=b.REFNOISE_ENABLED, nblocks=T, block_stride=nrows * B)
    plan.sync()
    pk = plan.device_buffers()["packet"]

    def run(i):
        cf.submit(pk, plan.packet_stride, plan.matrix_offset, T)
        cf.fetch(chi=False, map=False)

    _mean(run, lambda: None, 2)
    print("ready", flush=True)
    for _ in sys.stdin:
        print(_mean(run, lambda: None, reps), flush=True)


def _mover_blocks(T, nrows, picks, rng):
    """_blocks with `picks` movers in every row but the first: the reference delayed by 8 + 6 t samples and rotated by 20.3 + 17 t bins a
    line of FRAMES packets, the phase constant within a segment, at a = 0.5 / (1 + t / 4); complex samples this time"""
    L, J = B // 2, B // 2 // SEG
    rows = np.empty((T, nrows, B), dtype=np.int8)
    cn = lambda *sh: (rng.standard_normal(sh) + 1j * rng.standard_normal(sh)).astype(np.complex64)
    for t0 in range(0, T, FRAMES):
        ref = 25 * cn(FRAMES, L)
        for f in range(FRAMES):
            x = 0.7 * ref[f][None, :] + 6 * cn(nrows, L)
            k = f * J + np.arange(L) // SEG
            for t in range(picks):
                lag, bins = 8 + 6 * t, 20.3 + 17 * t
                d = np.concatenate([np.zeros(lag, dtype=np.complex64), ref[f][:L - lag]])
                x[1:] += (0.5 / (1 + t / 4)) * (d * np.exp(2j * np.pi * bins * k / (FRAMES * J)))[None, :]
            x[0] = ref[f]
            rows[t0 + f, :, 0::2] = np.clip(np.rint(x.real), -128, 127)
            rows[t0 + f, :, 1::2] = np.clip(np.rint(x.imag), -128, 127)
    return rows


def clean_timing(a):
    """--clean T: the submit with canceller (4:1) and detector against the same object's submit with the second stage on, at 22 rows:
    no picks (min_snr out of reach: the second pass alone -- the rows again, their map, the detector), and every line at T picks
    (the sums, the joint solve and the target members' terms on top).  Medians of --runs alternated rounds of --reps submits."""
    sys.path.insert(0, ROOT)
    import torch
    b = importlib.import_module("coherent-rtlsdr_amd.binding")
    nrows, (T, lags) = 22, SHAPES[22]
    rng = np.random.default_rng(1)
    d_in = torch.from_numpy(_mover_blocks(T, nrows, a.clean, rng).reshape(T, -1)).to(torch.device("cuda", 0))
    cf = b.Caf(nrows, B, SEG, lags, 0, b.WINDOW_HANN, GUARD, max_batch=T, frames=FRAMES)
    cf.set_cancel(4, 1)
    cf.set_cfar(b.cfar_desc(alpha=b.cfar_alpha(1e-6, 90), gd=1, gr=1, td=3, tr=4, min_train=20, max_det=16))
    variants = {"clean off": None, "+clean, no picks": b.CleanDesc(a.clean, 1e30, 1, 1), f"+clean, {a.clean} picks": b.CleanDesc(a.clean, 30.0, 1, 1)}

    def run(i):
        cf.submit(d_in.data_ptr(), nrows * B, 0, T)
        cf.fetch(chi=False, map=False)

    ms, info = {k: [] for k in variants}, {}
    for r in range(a.runs + 1):
        for name, desc in variants.items():
            cf.set_clean(desc)
            run(0)
            if desc is not None and r == 0:
                c = cf.fetch_clean(rchi=False, rmap=False)
                info[name] = {"launches": cf.last_launches(), "picks": c["ntgt"].tolist(), "status": sorted(set(c["tinfo"][:, 1:, 1].ravel().tolist())),
                              "rcount": c["rcount"][:, nrows].tolist()}
            if r:
                ms[name].append(1e3 * _mean(run, lambda: None, a.reps))
    cf.set_clean(None)
    cf.close()
    med = {k: statistics.median(v) for k, v in ms.items()}
    off = med["clean off"]
    out = {"rows": nrows, "lines": T // FRAMES, "nd": FRAMES * B // (2 * SEG), "lags": lags, "ms": {k: {"median": med[k], "min": min(v), "max": max(v)} for k, v in ms.items()}, "info": info}
    for k, v in ms.items():
        print(f"  {k:22s} {med[k]:8.4f} ms ({min(v):.4f} ... {max(v):.4f})  {med[k] - off:+.4f} ms  {info.get(k, '')}")
    names = list(variants)
    second, full = med[names[1]] - off, med[names[2]] - off
    print(f"  the second pass alone {second:.4f} ms = {100 * second / max(full, 1e-9):.0f} % of the {full:.4f} ms the stage adds at {a.clean} picks a line")
    if a.json:
        json.dump(out, open(a.json, "w"), indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clean", type=int, default=0, metavar="T", help="the second cancellation stage alone: off, on without picks, on with T picks a line (22 rows)")
    ap.add_argument("--integrate", action="store_true", help="add the variants of the integration across lines (with --beams: the beam maps' too)")
    ap.add_argument("--parent-lib", help="with --integrate: the plain submit of another build, in a worker process")
    ap.add_argument("--worker", type=int, metavar="ROWS", help=argparse.SUPPRESS)
    ap.add_argument("--rows", type=int, nargs="*", default=[22, 1025])
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-model", action="store_true", help="skip the numpy model on one line")
    ap.add_argument("--cfar", action="store_true", help="add the CFAR detector's variants")
    ap.add_argument("--estimator", action="store_true", help="add the detector under greatest-of, smallest-of and the ordered statistic (with --cfar's)")
    ap.add_argument("--cancel", metavar="K[:P]", help="add the canceller's variant")
    ap.add_argument("--bearing", action="store_true", help="add the bearings' variants (with --cfar's)")
    ap.add_argument("--beams", type=int, default=0, metavar="NB", help="add the beam maps' variants: a lattice of NB beams (22 rows)")
    ap.add_argument("--adapt", action="store_true", help="add the adaptive beams' variants (with --beams, 22 rows)")
    ap.add_argument("--track", action="store_true", help="add the tracker's variants (22 rows)")
    ap.add_argument("--json")
    a = ap.parse_args()
    a.cfar = a.cfar or a.bearing or a.estimator
    if a.worker:
        return worker(a.worker, a.reps)
    if a.clean:
        return clean_timing(a)
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    b = importlib.import_module("coherent-rtlsdr_amd.binding")
    rng = np.random.default_rng(1)
    out = {"blocksize": B, "seg": SEG, "frames": FRAMES, "runs": a.runs, "reps": a.reps, "shapes": []}
    for nrows in a.rows:
        T, lags = SHAPES.get(nrows, (FRAMES, 16))
        nd = FRAMES * B // (2 * SEG)
        d_in = torch.from_numpy(_blocks(T, nrows, rng).view(np.uint8).reshape(T, -1)).to(torch.device("cuda", 0))
        torch.cuda.synchronize()
        plan = b.Plan(nrows, B, b.MODE_DIGITAL, max_batch=T)
        flags = b.REFNOISE_ENABLED | b.NO_LAG
        submit = lambda i: plan.submit(d_in.data_ptr(), seq=i * T, flags=flags, nblocks=T, block_stride=nrows * B)
        cf = b.Caf(nrows, B, SEG, lags, 0, b.WINDOW_HANN, GUARD, max_batch=T, frames=FRAMES)
        sp = b.Spectra(nrows, B, 256, 1, b.WINDOW_HANN, band=(-25, 25), max_batch=T, frames=FRAMES)
        pk = plan.device_buffers()["packet"]
        host = b.PinnedArray((T, plan.packet_stride), np.int8)

        def with_caf(i):
            submit(i)
            cf.submit_plan(plan)
            cf.fetch(chi=False, map=False)

        def caf_alone(i):
            cf.submit(pk, plan.packet_stride, plan.matrix_offset, T)
            cf.fetch(chi=False, map=False)

        def with_spectra(i):
            submit(i)
            sp.submit_plan(plan)
            sp.fetch(psd=False, cross=False)

        def spectra_alone(i):
            sp.submit(pk, plan.packet_stride, plan.matrix_offset, T)
            sp.fetch(psd=False, cross=False)

        def to_host(i):
            plan.fetch_batch_async(packets=host.array, host_packet_stride=plan.packet_stride)
            plan.fetch_wait()

        cfd = None
        if a.cfar:
            cfd = b.Caf(nrows, B, SEG, lags, 0, b.WINDOW_HANN, GUARD, max_batch=T, frames=FRAMES)
            cfd.set_cfar(b.cfar_desc(alpha=b.cfar_alpha(1e-6, 90), gd=1, gr=1, td=3, tr=4, max_det=16))

        ests = {}
        if a.estimator:
            for name, ed, n in (("cfar go", b.cfar_est_desc(b.CFAR_GO, b.CFAR_AXIS_LAG), 42), ("cfar so", b.cfar_est_desc(b.CFAR_SO, b.CFAR_AXIS_LAG), 42),
                                ("cfar os", b.cfar_est_desc(b.CFAR_OS, rank=67), 90)):
                e = b.Caf(nrows, B, SEG, lags, 0, b.WINDOW_HANN, GUARD, max_batch=T, frames=FRAMES)
                e.set_cfar(b.cfar_desc(alpha=b.cfar_alpha_est(1e-6, n, ed), gd=1, gr=1, td=3, tr=4, max_det=16))
                e.set_cfar_estimator(ed)
                ests[name] = e

        def caf_est(e):
            def run(i):
                e.submit(pk, plan.packet_stride, plan.matrix_offset, T)
                e.fetch(chi=False, map=False)
                e.fetch_cfar()
            return run

        brg = {}
        if a.bearing and nrows == 22:
            for name, mode in (("cfar low", None), ("+brg conv", b.BEARING_CONVENTIONAL), ("+brg adpt", b.BEARING_ADAPTIVE)):
                e = b.Caf(nrows, B, SEG, lags, 0, b.WINDOW_HANN, GUARD, max_batch=T, frames=FRAMES)
                e.set_cfar(b.cfar_desc(alpha=3.0, gd=1, gr=1, td=3, tr=4, max_det=16))
                if mode is not None:
                    e.set_bearing(b.bearing_desc(7, 3, (1.225 * 1.24) / 3.0, 100, 100, mode, 1e-2, 5))
                brg[name] = e

        def caf_bearing(e):
            def run(i):
                e.submit(pk, plan.packet_stride, plan.matrix_offset, T)
                e.fetch(chi=False, map=False)
                e.fetch_cfar()
                if e is not brg["cfar low"]:
                    e.fetch_bearing()
            return run

        bms = {}
        if a.beams and nrows == 22:
            side = int(round(a.beams ** 0.5))
            xy = np.array([((100.0 * i + 48.0) / side, (100.0 * j + 96.0) / side) for i in range(side) for j in range(side)])
            wts = b.beam_steer(7, 3, (1.225 * 1.24) / 3.0, xy, 100, 100)
            for name, det, on in (("caf b", False, False), ("+beams", False, True), ("cfar b", True, False), ("+beams det", True, True)):
                e = b.Caf(nrows, B, SEG, lags, 0, b.WINDOW_HANN, GUARD, max_batch=T, frames=FRAMES)
                if det:
                    e.set_cfar(b.cfar_desc(alpha=b.cfar_alpha(1e-6, 90), gd=1, gr=1, td=3, tr=4, max_det=16))
                if on:
                    e.set_beams(wts)
                bms[name] = (e, det, on)

        def caf_beams(name):
            e, det, on = bms[name]

            def run(i):
                e.submit(pk, plan.packet_stride, plan.matrix_offset, T)
                e.fetch(chi=False, map=False)
                if det:
                    e.fetch_cfar()
                if det and on:
                    e.fetch_beams(bmap=False, fused_only=True)
            return run

        ads, adapt_engine = {}, None
        if a.adapt and bms:
            e = adapt_engine = b.Caf(nrows, B, SEG, lags, 0, b.WINDOW_HANN, GUARD, max_batch=T, frames=FRAMES)
            if a.cfar:
                e.set_cfar(b.cfar_desc(alpha=b.cfar_alpha(1e-6, 90), gd=1, gr=1, td=3, tr=4, max_det=16))
            e.set_beams(wts)
            ads = {"adapt off": (e, None), "+adapt": (e, b.beam_adapt_desc(1e-2, GUARD + 1, nd - 2 * GUARD - 1, 0, lags))}

        def caf_adapt(e):
            def run(i):
                e.submit(pk, plan.packet_stride, plan.matrix_offset, T)
                e.fetch(chi=False, map=False)
                if a.cfar:
                    e.fetch_cfar()
                    e.fetch_beams(bmap=False, fused_only=True)
            return run

        trs = {}
        if a.track and nrows == 22:
            for name, on in (("cfar trk", False), ("+track", True)):
                e = b.Caf(nrows, B, SEG, lags, 0, b.WINDOW_HANN, GUARD, max_batch=T, frames=FRAMES)
                e.set_cfar(b.cfar_desc(alpha=3.0, gd=1, gr=1, td=3, tr=4, max_det=64))
                if on:
                    e.set_track(b.track_desc(128, m=3, n=5, gate=9.0))
                trs[name] = e

        def caf_track(name):
            e = trs[name]

            def run(i):
                e.submit(pk, plan.packet_stride, plan.matrix_offset, T)
                e.fetch(chi=False, map=False)
                if name == "+track":
                    e.fetch_track()
                else:
                    e.fetch_cfar(snap=False)
            return run

        igs, ops, workers = {}, {}, {}
        if a.integrate:
            idesc = lambda what: b.integrate_desc(1.0 / 8.0, 0.05, what=what)
            e = b.Caf(nrows, B, SEG, lags, 0, b.WINDOW_HANN, GUARD, max_batch=T, frames=FRAMES)
            e.set_integrate(idesc(b.INTEGRATE_ARRAY))
            igs["+integ"] = e
            if bms:
                e = b.Caf(nrows, B, SEG, lags, 0, b.WINDOW_HANN, GUARD, max_batch=T, frames=FRAMES)
                e.set_beams(wts)
                e.set_integrate(idesc(b.INTEGRATE_ARRAY | b.INTEGRATE_BEAMS))
                igs["+integ bm"] = e
            dev = torch.device("cuda", 0)
            for name, (L, n) in (("integ op", (T // FRAMES, 1)), ("integ big", (64, 16))):
                ops[name] = (L, n, torch.rand(L * n * nd * lags, device=dev), torch.zeros(2 + n * nd * lags, device=dev, dtype=torch.float64),
                             torch.empty(L * n * nd * lags, device=dev))
            if a.parent_lib:
                for name, env in (("caf self", dict(os.environ)), ("caf parent", dict(os.environ, CRSDR_LIB=os.path.abspath(a.parent_lib)))):
                    workers[name] = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", str(nrows), "--reps", str(a.reps)], stdin=subprocess.PIPE,
                                                     stdout=subprocess.PIPE, text=True, env=env)
                    assert workers[name].stdout.readline().strip() == "ready"

        def caf_integ(e):
            def run(i):
                e.submit(pk, plan.packet_stride, plan.matrix_offset, T)
                e.fetch(chi=False, map=False)
            return run

        def integ_op(name):
            L, n, maps, state, imap = ops[name]
            return lambda i: b.map_integrate_device(imap.data_ptr(), state.data_ptr(), maps.data_ptr(), L, n, nd, lags, b.integrate_desc(1.0 / 8.0, 0.05))

        def asked(w):
            w.stdin.write("go\n")
            w.stdin.flush()
            return float(w.stdout.readline())

        cfc, basis = None, 0
        if a.cancel:
            taps, dopp = (int(v) for v in (a.cancel + ":0").split(":")[:2])
            cfc = b.Caf(nrows, B, SEG, lags, 0, b.WINDOW_HANN, GUARD, max_batch=T, frames=FRAMES)
            cfc.set_cancel(taps, dopp)
            basis = taps * (2 * dopp + 1)

        def caf_cancel(i):
            cfc.submit(pk, plan.packet_stride, plan.matrix_offset, T)
            cfc.fetch(chi=False, map=False)
            cfc.fetch_cancel()

        def caf_cfar(i):
            cfd.submit(pk, plan.packet_stride, plan.matrix_offset, T)
            cfd.fetch(chi=False, map=False)
            cfd.fetch_cfar()

        variants = {
            "plan": lambda: _mean(submit, plan.sync, a.reps),
            "+caf": lambda: _mean(with_caf, plan.sync, a.reps),
            "caf": lambda: _mean(caf_alone, lambda: None, a.reps),
            "+spectra": lambda: _mean(with_spectra, plan.sync, a.reps),
            "spectra": lambda: _mean(spectra_alone, lambda: None, a.reps),
            "host": lambda: _mean(to_host, lambda: None, a.reps),
        }
        if a.cfar:
            variants["caf+cfar"] = lambda: _mean(caf_cfar, lambda: None, a.reps)
            variants["get chi"] = lambda: _mean(lambda i: cf.fetch(map=False, peak=False), lambda: None, a.reps)
            variants["get cfar"] = lambda: _mean(lambda i: cfd.fetch_cfar(), lambda: None, a.reps)
        for name, e in ests.items():
            variants[name] = lambda e=e: _mean(caf_est(e), lambda: None, a.reps)
        for name, e in brg.items():
            variants[name] = lambda e=e: _mean(caf_bearing(e), lambda: None, a.reps)
        if brg:
            variants["get dir"] = lambda: _mean(lambda i: brg["+brg adpt"].fetch_bearing(), lambda: None, a.reps)
        for name in bms:
            variants[name] = lambda name=name: _mean(caf_beams(name), lambda: None, a.reps)
        if bms:
            variants["get fused"] = lambda: _mean(lambda i: bms["+beams det"][0].fetch_beams(bmap=False, fused_only=True), lambda: None, a.reps)
            if "get chi" not in variants:
                variants["get chi"] = lambda: _mean(lambda i: cf.fetch(map=False, peak=False), lambda: None, a.reps)
        for name in trs:
            variants[name] = lambda name=name: _mean(caf_track(name), lambda: None, a.reps)
        if trs:
            variants["get trk"] = lambda: _mean(lambda i: trs["+track"].fetch_track(), lambda: None, a.reps)
            variants["get lists"] = lambda: _mean(lambda i: trs["cfar trk"].fetch_cfar(snap=False), lambda: None, a.reps)
        if a.cancel:
            variants["caf+cancel"] = lambda: _mean(caf_cancel, lambda: None, a.reps)
        def toggled(e, desc):
            # the setter (it waits, and allocates) and one submit outside the clock: on and off are the SAME object, because two
            # objects of one configuration differ by as much as the stage costs
            def fn():
                e.set_integrate(desc)
                caf_integ(e)(0)
                return _mean(caf_integ(e), lambda: None, a.reps)
            return fn

        def adapted(e, desc):
            # (the same object on and off, as for the integration)
            def fn():
                e.set_beam_adapt(desc)
                caf_adapt(e)(0)
                return _mean(caf_adapt(e), lambda: None, a.reps)
            return fn

        for name, (e, desc) in ads.items():
            variants[name] = adapted(e, desc)
        for name, e in igs.items():
            what = b.INTEGRATE_ARRAY | (b.INTEGRATE_BEAMS if name == "+integ bm" else 0)
            variants[name.replace("+integ", "integ off")] = toggled(e, None)
            variants[name] = toggled(e, idesc(what))
        for name in ops:
            variants[name] = lambda name=name: _mean(integ_op(name), lambda: None, a.reps)
        for name, w in workers.items():
            variants[name] = lambda w=w: asked(w)
        plan.submit(d_in.data_ptr(), seq=0, flags=b.REFNOISE_ENABLED, nblocks=T, block_stride=nrows * B)      # lags and phasors for the locked submits
        plan.sync()
        for fn in variants.values():             # warm-up: code objects, allocations
            fn()
        rec = {k: [] for k in variants}
        for _ in range(a.runs):
            for k, fn in variants.items():
                rec[k].append(fn())
        shape = {"nrows": nrows, "batch": T, "lags": lags, "nd": nd, "ms": {}}
        live = 0
        if brg:                                  # the slots that hold a detection: the others write their zeros and leave
            live = int(np.minimum(brg["+brg adpt"].fetch_cfar(det=False, snap=False)["count"][:, nrows], 16).sum())
            shape["live_slots"] = live
        base = statistics.median(rec["plan"])
        cells = (T // FRAMES) * nrows * nd * lags
        macs = T * nrows * (B // 2) * lags
        for k, v in rec.items():
            ms = [1e3 * x for x in v]
            med = statistics.median(ms)
            shape["ms"][k] = {"median": med, "min": min(ms), "max": max(ms)}
            note = ""
            if k.startswith("+"):
                note = f"  (+{med - 1e3 * base:.3f} ms behind the plan)"
            if k == "caf":
                note = f"  ({8 * cells / (med * 1e-3) / 1e9:.1f} GB/s of chi stored, {macs / (med * 1e-3) / 1e12:.2f} T complex int8 MAC/s)"
            if k == "caf+cfar":
                note = f"  (+{med - shape['ms']['caf']['median']:.3f} ms behind caf; the detector reads {(T // FRAMES) * nd * lags * (8 * nrows + 4) / 1e6:.1f} MB of P)"
            if k in ests:
                note = f"  ({med - shape['ms']['caf+cfar']['median']:+.3f} ms against caf+cfar)"
            if k == "caf+cancel":
                note = f"  (+{med - shape['ms']['caf']['median']:.3f} ms behind caf; {basis} complex fp64 multiply-adds a cell, {basis * cells / (med * 1e-3) / 1e9:.1f} G/s over the submit)"
            if k in brg and k != "cfar low":
                note = f"  (+{med - shape['ms']['cfar low']['median']:.3f} ms behind cfar low; {live} of {(T // FRAMES) * 16} slots hold a detection, 10^4 grid points each)"
            if k == "get dir":
                note = f"  ({(T // FRAMES) * 16 * 32 / 1e3:.1f} kB)"
            if k == "+beams":
                note = f"  (+{med - shape['ms']['caf b']['median']:.3f} ms behind caf b)"
            if k == "+beams det":
                note = f"  (+{med - shape['ms']['cfar b']['median']:.3f} ms behind cfar b)"
            if k == "get fused":
                note = f"  ({(T // FRAMES) * (16 * 32 + 4) / 1e3:.1f} kB)"
            if k == "+track":
                note = f"  (+{med - shape['ms']['cfar trk']['median']:.3f} ms behind cfar trk: {T // FRAMES} lines in one workgroup, {(med - shape['ms']['cfar trk']['median']) / (T // FRAMES) * 1e3:.1f} us a line)"
            if k == "get trk":
                note = f"  ({(T // FRAMES) * (128 * 64 + 16) / 1e3:.1f} kB)"
            if k == "get lists":
                note = f"  ({(T // FRAMES) * (nrows + 1) * (64 * 32 + 4) / 1e3:.1f} kB)"
            if k == "+adapt":
                N, m, over = (nd - 2 * GUARD - 1) * lags, nrows - 1, med - shape["ms"]["adapt off"]["median"]
                bts, beam = (T // FRAMES) * m * N * 8, shape["ms"]["+beams"]["median"] - shape["ms"]["caf b"]["median"]
                shape["adapt"] = {"bytes": bts, "over_ms": over, "beam_kernel_ms": beam}
                note = (f"  ({over:+.4f} ms behind 'adapt off', the same object: {bts / 1e6:.2f} MB of chi read once in two launches, "
                        f"{f'{bts / over / 1e6:.1f} GB/s over the difference' if over > 0.002 else 'a difference inside the spread'}; '+beams' less 'caf b': {beam:+.4f} ms)")
            if k in igs:
                lcells, maps = nd * lags, 1 + (len(wts) if k == "+integ bm" else 0)
                off = k.replace("+integ", "integ off")
                bts, over = maps * lcells * (8 * (T // FRAMES) + 16), med - shape["ms"][off]["median"]
                note = (f"  ({over:+.4f} ms behind '{off}', the same object: {bts / 1e6:.2f} MB in {maps > 1 and 'two launches' or 'one launch'}, "
                        f"{f'{bts / over / 1e6:.1f} GB/s over the difference' if over > 0.002 else 'a difference inside the spread'}; the array-map kernel reads {(T // FRAMES) * (nrows - 1) * lcells * 8 / 1e6:.1f} MB)")
            if k in ops:
                L, n = ops[k][:2]
                bts = n * nd * lags * (8 * L + 16)
                note = f"  ({L} lines of {n} maps, {bts / 1e6:.2f} MB: {bts / (med * 1e-3) / 1e9:.1f} GB/s with the launch and its wait)"
            if k in workers:
                note = f"  ({med - shape['ms']['caf']['median']:+.4f} ms against this process's caf)"
            if k == "get chi":
                note = f"  ({8 * cells / 1e6:.1f} MB)"
            if k == "get cfar":
                note = f"  ({(T // FRAMES) * ((nrows + 1) * (16 * 32 + 4) + 16 * nrows * 8) / 1e3:.1f} kB)"
            if k == "host":
                note = f"  ({T * plan.packet_stride / (med * 1e-3) / 1e9:.1f} GB/s)"
            print(f"rows {nrows:5d} batch {T:2d} {k:>10}: {med:9.3f} ms ({min(ms):.3f} .. {max(ms):.3f}){note}")
        if bms:
            nb, m, lcells = len(wts), nrows - 1, (T // FRAMES) * nd * lags
            mfma = (lcells // 32) * 2 * m * ((nb + 31) // 32)
            shape["beams"] = {"nbeams": nb, "bytes": lcells * (8 * m + 4 * nb), "mfma": mfma}
            print(f"rows {nrows:5d} batch {T:2d} beam maps: {nb} beams, {lcells} cells: {lcells * (8 * m + 4 * nb) / 1e6:.1f} MB to move; {mfma} MFMAs of 64 cycles, "
                  f"{mfma * 64 / 1024 / 2.4e9 * 1e3:.4f} ms over 1024 SIMDs at 2.4 GHz")
        if not a.no_model:
            import caf_model as M
            t0 = time.perf_counter()
            to_host(0)
            off = plan.matrix_offset
            line = [host.array[t, off:off + nrows * B].reshape(nrows, B) for t in range(FRAMES)]
            chi, _ = M.caf(line, SEG, lags, 0, M.WINDOW_HANN)
            M.all_peaks(chi.astype(np.complex64), M.array_map(chi.astype(np.complex64), 0)[0], GUARD)
            dt = 1e3 * (time.perf_counter() - t0)
            shape["ms"]["host+model"] = {"median": dt, "min": dt, "max": dt}
            print(f"rows {nrows:5d} batch {T:2d} host+model: {dt:9.1f} ms for ONE line of {T // FRAMES} (numpy, fp64)")
        out["shapes"].append(shape)
        cf.close()
        if cfd:
            cfd.close()
        if cfc:
            cfc.close()
        for e in list(ests.values()) + list(brg.values()):
            e.close()
        for e, _, _ in bms.values():
            e.close()
        for e in list(trs.values()) + list(igs.values()) + ([adapt_engine] if adapt_engine else []):
            e.close()
        for w in workers.values():
            w.stdin.close()
            w.wait(timeout=60)
        ops.clear()
        sp.close()
        host.close()
        plan.close()
        del d_in
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
