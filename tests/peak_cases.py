"""Inputs whose zero-padded correlation is known in closed form -- helper for test_peak_cases_model.py and test_gpu_peak.py.

The reference row is one impulse (I = 127 at sample q), a signal row a real three-tap pulse TAPS on I at samples p-1, p, p+1 (taps
outside [0, L) dropped).  With B = 2 L the correlation of ccoherent::computelag (oracle/model_fp64.py xcorr_lag) is then three numbers

    m[idx + k] = (B tap_k / 127)^2,  k = -1, 0, 1,   idx = L + p - q,       every other bin zero,

so lag = idx - L, mag = B / sqrt(L) and frac = 0.5 (ym - yp) / (ym - 2 mp + yp) are exact, wherever the peak lands.  q = 0 reaches
idx in [L, 2L-1], q = L-1 reaches idx in [1, L].  Zero, ym, yp and the peak are four distinct values: a neighbour taken from a wrong
lane, wave, half or column changes frac by > 1e-2 (test_peak_cases_model.py proves the margin), against an fp32 error of ~1e-7.
In digital mode the aligned row is the taps at q-1, q, q+1 (clipped at the row's ends) and the EMA phasor stays exactly 1: the dot
product behind the shift is real and positive.
"""
import numpy as np

TAPS = (100, 127, 32)

# ---- the error bar ------------------------------------------------------------------------------------------------------------
# mag: relative 1e-6, the project's bound for K1 against fp64 (BOUNDS in test_gpu_k1_fma.py, test_fft_vs_oracle_and_fp64).
# frac: m = L mag^2, so each of ym, mp, yp carries an absolute error of EPS mp with EPS = 2e-6 (twice the mag bar).  With
# N = ym - yp, D = ym - 2 mp + yp, frac = N / 2D:  |dN| <= 2 EPS mp, |dD| <= 4 EPS mp, so
#     |dfrac| <= |dN| / 2|D| + |frac| |dD| / |D| = EPS mp (1 + 4 |frac|) / |D|
# with ym, mp, yp, frac from the reference (closed form or fp64 model), never from the device.
MAG_RTOL = 1e-6
EPS = 2e-6


def frac_bar(ym, mp, yp, frac):
    ym, mp, yp, frac = (np.asarray(x, dtype=np.float64) for x in (ym, mp, yp, frac))
    den = np.abs(ym - 2.0 * mp + yp)
    with np.errstate(divide="ignore", invalid="ignore"):
        bar = EPS * mp * (1.0 + 4.0 * np.abs(frac)) / den
    return np.where(den > 0, bar, 0.0)                       # no parabola (peak at an end, all ties): frac is 0, exactly


def frac_of(ym, mp, yp):
    """The parabolic estimate of src/ccoherent.cc:206-219 from the three magnitudes (0 where the denominator vanishes)."""
    ym, mp, yp = (np.asarray(x, dtype=np.float64) for x in (ym, mp, yp))
    den = ym - 2.0 * mp + yp
    with np.errstate(divide="ignore", invalid="ignore"):
        f = 0.5 * (ym - yp) / den
    return np.where(den != 0, f, 0.0)


# ---- rows and their closed form -------------------------------------------------------------------------------------------------
def pulse_block(L, q, ps, taps=TAPS):
    """int8 [1 + len(ps)][2 L]: row 0 the impulse at q, row 1 + k the pulse centred on ps[k]."""
    ps = np.asarray(ps, dtype=np.int64)
    rows = np.zeros((1 + ps.size, 2 * L), dtype=np.int8)
    rows[0, 2 * q] = 127
    k = np.arange(ps.size)
    for off, tap in zip((-1, 0, 1), taps):
        s = ps + off
        ok = (s >= 0) & (s < L)
        rows[1 + k[ok], 2 * s[ok]] = tap
    return rows


def closed_form(L, q, ps, taps=TAPS):
    """lag, mag, frac, ym, mp, yp, bar per signal row (fp64; frac = 0 for a peak at idx 0 or B - 1, as computelag has it)."""
    ps = np.asarray(ps, dtype=np.int64)
    B = 2 * L
    idx = L + ps - q
    assert np.all((idx >= 1) & (idx <= B - 1)) and np.all((ps >= 0) & (ps < L))
    val = lambda tap: (B * tap / 127.0) ** 2
    ym = np.where(ps - 1 >= 0, val(taps[0]), 0.0)
    yp = np.where(ps + 1 < L, val(taps[2]), 0.0)
    mp = np.full(ps.size, val(taps[1]))
    inner = (idx > 0) & (idx < B - 1)
    frac = np.where(inner, frac_of(ym, mp, yp), 0.0)
    bar = np.where(inner, frac_bar(ym, mp, yp, frac), 0.0)
    return dict(idx=idx, lag=idx - L, mag=np.sqrt(mp / L), frac=frac, ym=ym, mp=mp, yp=yp, bar=bar, L=L)


def expected_matrix(L, q, ps, taps=TAPS):
    """The digital mode's matrix [1 + len(ps)][2 L]: the reference row verbatim, every signal row shifted by its lag -- the taps that
    survived the source row's ends at q-1, q, q+1, clipped at the destination's ends."""
    ps = np.asarray(ps, dtype=np.int64)
    out = np.zeros((1 + ps.size, 2 * L), dtype=np.int8)
    out[0, 2 * q] = 127
    k = np.arange(ps.size)
    for off, tap in zip((-1, 0, 1), taps):
        if 0 <= q + off < L:
            ok = (ps + off >= 0) & (ps + off < L)
            out[1 + k[ok], 2 * (q + off)] = tap
    return out


def expected_header(seq, nrows, L, readcnt):
    """hdr0 {seq, N, L, 0} + uint32 readcnt[N] (include/crsdr.h: crsdr_plan_fetch) as int8 bytes."""
    return np.concatenate([np.array([seq, nrows, L, 0], dtype=np.uint32), np.asarray(readcnt, dtype=np.uint32)]).view(np.int8)


# ---- positions -------------------------------------------------------------------------------------------------------------
def ref_positions(L):
    return 0, L - 1                                           # q of block 0 (idx in [L, 2L-1]) and of block 1 (idx in [1, L])


def split_by_reference(L, idxs, pad_to=None):
    """Peak indices -> (ps of the q = 0 block, ps of the q = L - 1 block), both padded (by repeating their own entries) to one
    length so that they can ride as the two blocks of one plan.  idx = L is reached by both."""
    idxs = np.unique(np.asarray(idxs, dtype=np.int64))
    assert idxs.size and idxs[0] >= 1 and idxs[-1] <= 2 * L - 1
    p0 = idxs[idxs >= L] - L                                  # q = 0:     idx = L + p
    p1 = idxs[idxs <= L] - 1                                  # q = L - 1: idx = p + 1
    n = max(p0.size, p1.size, 1) if pad_to is None else pad_to
    fill = lambda p, dflt: np.resize(p if p.size else np.array([dflt], dtype=np.int64), n)
    return fill(p0, 0), fill(p1, L - 1)


def full_positions(L):
    """Every idx in 1 .. B - 1 (the generic kernels' sizes: every p in [0, L) under both references)."""
    return np.arange(1, 2 * L)


def sweep_batches(L, n):
    """Every idx 1 .. B - 1 as submits of n signal rows per block: [(q, [ps of submit 0, ps of submit 1, ...])] for the two reference
    positions, each a cut of its L positions into ceil(L / n) slices (a short last slice is padded by repeating its own entries)."""
    out = []
    for q, ps in zip(ref_positions(L), split_by_reference(L, full_positions(L))):
        assert ps.size == L
        out.append((q, [np.resize(ps[s:s + n], n) for s in range(0, L, n)]))
    return out


def gather_by_idx(L, order, res):
    """The rows of a run put in order of their peak index.  order: [(q, ps)] of the fetched blocks in the order they were fetched,
    res: lag, mag, frac [len(order)][1 + len(ps)] (pulse_run of test_gpu_peak.py).  Returns lag, mag, frac [B - 1] for idx 1 .. B - 1
    (idx = L: the q = 0 row), lag_L, mag_L, frac_L [1] (idx = L under q = L - 1), and reached [2][B]: how many rows put their peak
    on an idx under q = 0 / q = L - 1."""
    B = 2 * L
    got = {k: np.zeros(B, dtype=np.asarray(res[k]).dtype) for k in ("lag", "mag", "frac")}
    at_L = {k: np.zeros(1, dtype=np.asarray(res[k]).dtype) for k in ("lag", "mag", "frac")}
    reached = np.zeros((2, B), dtype=np.int64)
    for t, (q, ps) in enumerate(order):
        idx = L + np.asarray(ps, dtype=np.int64) - q
        first = q == 0
        np.add.at(reached[0 if first else 1], idx, 1)
        for k in got:
            vals = np.asarray(res[k][t])[1:]
            keep = np.ones(idx.size, dtype=bool) if first else idx != L
            got[k][idx[keep]] = vals[keep]
            if not first and np.any(~keep):
                at_L[k][0] = vals[~keep][0]
    out = {k: v[1:] for k, v in got.items()}
    out.update({k + "_L": v for k, v in at_L.items()})
    out["reached"] = reached
    return out


def sweep_is_complete(L, reached):
    """Failures (strings) unless the union of the indices reached is exactly {1 .. B - 1} and idx = L was reached under both references."""
    B = 2 * L
    union = np.flatnonzero(reached.sum(axis=0))
    fails = []
    if not np.array_equal(union, np.arange(1, B)):
        missing = np.setdiff1d(np.arange(1, B), union)
        fails.append(f"the sweep reached {union.size} of {B - 1} indices; missing {missing[:16].tolist()}, beyond 1 .. B-1: {np.setdiff1d(union, np.arange(1, B)).tolist()}")
    if not (reached[0, L] >= 1 and reached[1, L] >= 1):
        fails.append(f"idx = L reached {reached[0, L]} times under q = 0 and {reached[1, L]} times under q = L - 1")
    if np.any(reached[0, :L]) or np.any(reached[1, L + 1:]):
        fails.append("a reference position reached an index outside its half")
    return fails


def probe_positions(log2B, seeded=64, seed=41):
    """The indices at which test_peak_cases_model.py proves the closed form for the full sweeps of B = 16384 and 2^15: the ends, the
    centre and `seeded` more, drawn from all of 1 .. B - 1 (most of them no designed position of k1_positions / long_positions)."""
    B = 1 << log2B
    L = B // 2
    return np.unique(np.concatenate([[1, 2, B - 2, B - 1, L - 1, L, L + 1], np.random.default_rng(seed + log2B).integers(1, B, size=seeded)]))


K1_SEEDED, LONG_SEEDED, LONG_MAX_ROWS = 256, 64, 128
K1_SWEEP_ROWS = 2048          # signal rows per block of a submit of the B = 16384 sweep (two blocks: 67 MB of input, as B = 8192's full sweep)
# B = 2^15: 7 submits per reference position.  The plan cuts a block's rows into chunks of 1600 (400 MB of cf32 work area); a chunk
# takes the two-line stage B from 512 rows on (1024 lines).  2048 rows would leave a last chunk of 448; 2341 = ceil(16384 / 7) leaves 741.
LONG_SWEEP_ROWS = 2341


def k1_positions(L=8192, seeded=K1_SEEDED, seed=14):
    """B = 16384 (32 output indices x 512 columns; a wave owns 64 columns): each wave's edge lanes in both halves at every output
    index, the half boundary 255 / 256 and the column wrap 511 -> 0, the block's ends and centre, and `seeded` more.
    (Columns 0, 255, 256 and 511 are wave-edge lanes themselves, so the second set adds no index to the first: it is kept to say what
    is aimed at.  A reference position reaches half of the indices, so the ~1270 positions ride as ~640 rows in each of the two blocks.)"""
    B = 2 * L
    i = np.arange(1, B)
    designed = np.concatenate([i[np.isin(i & 63, (0, 1, 62, 63))], i[np.isin(i & 511, (0, 255, 256, 511))],
                               [1, 2, 3, B - 3, B - 2, B - 1, L - 1, L, L + 1]])
    extra = np.random.default_rng(seed).integers(1, B, size=seeded)
    return np.unique(designed), np.unique(np.concatenate([designed, extra]))


def long_geometry(log2B):
    """csrc/longblock.hpp: B = N1 x N2 with N2 = 16384; stage C works on tiles of TILE = 8192 elements = all N1 rows of C = TILE / N1
    columns, NT = N2 / C tiles per row: tile t holds the indices n1 N2 + t C + c, c < C."""
    N2, TILE = 1 << 14, 1 << 13
    N1 = (1 << log2B) // N2
    C = TILE // N1
    return N1, N2, C, N2 // C


def long_positions(log2B, seeded=LONG_SEEDED, seed=15):
    """Long blocks: n2 in {0, 1, N2-2, N2-1} for every n1 (k_long_finalize's n1 / n2 split of the neighbours), the first and last index
    of every stage-C tile (its smallest and largest natural index: n1 = 0, c = 0 and n1 = N1-1, c = C-1; where the row cap leaves room,
    B = 2^15 and 2^16, its first and last column at every n1 as well), the block's ends and centre, and `seeded` more."""
    B = 1 << log2B
    L = B // 2
    N1, N2, C, NT = long_geometry(log2B)
    n1 = np.arange(N1)[:, None] * N2
    t = np.arange(NT)
    designed = np.concatenate([(n1 + np.array([0, 1, N2 - 2, N2 - 1])[None, :]).ravel(),
                               t * C, (N1 - 1) * N2 + t * C + C - 1,           # a tile's first index (n1 = 0, c = 0) and its last
                               [1, 2, B - 2, B - 1, L - 1, L, L + 1]])
    if 2 * N1 * NT <= LONG_MAX_ROWS // 2:                                       # B = 2^15, 2^16: room for a tile's first and last COLUMN in
        designed = np.concatenate([designed, (n1 + (t * C)[None, :]).ravel(), (n1 + (t * C + C - 1)[None, :]).ravel()])     # every row n1
    designed = np.unique(designed[(designed >= 1) & (designed <= B - 1)])        # (idx 0 is reached only by an all-zero correlation)
    extra = np.random.default_rng(seed + log2B).integers(1, B, size=seeded)
    return designed, extra


def long_blocks(log2B, max_rows=LONG_MAX_ROWS):
    """[(q, ps)] for the two submits of a long block: the designed positions in reach of q, then as many of the seeded ones as
    max_rows signal rows leave room for (the seeded ones are thinned first, the designed ones never)."""
    L = (1 << log2B) // 2
    designed, extra = long_positions(log2B)
    out = []
    for q, lo, hi in ((0, L, 2 * L - 1), (L - 1, 1, L)):
        d = designed[(designed >= lo) & (designed <= hi)]
        e = extra[(extra >= lo) & (extra <= hi)]
        assert d.size <= max_rows, (log2B, q, d.size)
        idx = np.unique(np.concatenate([d, e[:max_rows - d.size]]))
        out.append((q, idx - L + q))
    return out


# ---- comparing an output with its reference ----------------------------------------------------------------------------------------
def compare(got, exp, what=""):
    """got: lag, mag, frac of the signal rows (device or oracle); exp: closed_form() or the same keys from the fp64 model.
    Returns (worst relative mag error, worst absolute frac error, list of failure strings -- empty when all rows lie within the bar).
    A frac off by more than the bar but less than 1e-4 has the right neighbours and lost accuracy: reported as such."""
    lag, mag, frac = np.asarray(got["lag"]), np.asarray(got["mag"], dtype=np.float64), np.asarray(got["frac"], dtype=np.float64)
    fails = []
    bad = np.flatnonzero(lag != exp["lag"])
    if bad.size:
        fails.append(f"{what}: lag wrong in {bad.size} rows, idx {(exp['lag'][bad] + exp['L'])[:16].tolist()}: "
                     f"got {lag[bad][:16].tolist()}, expected {exp['lag'][bad][:16].tolist()}")
    if not (np.all(np.isfinite(mag)) and np.all(np.isfinite(frac))):
        fails.append(f"{what}: non-finite mag or frac")
    with np.errstate(divide="ignore", invalid="ignore"):
        emag = np.where(exp["mag"] > 0, np.abs(mag - exp["mag"]) / exp["mag"], np.abs(mag))
    efrac = np.abs(frac - exp["frac"])
    bad = np.flatnonzero(~(emag <= MAG_RTOL))
    if bad.size:
        fails.append(f"{what}: mag outside {MAG_RTOL:g} in {bad.size} rows, idx {(exp['lag'][bad] + exp['L'])[:16].tolist()}, worst {np.nanmax(emag):.3e}")
    bad = np.flatnonzero(~(efrac <= exp["bar"]))
    if bad.size:
        gross = bad[efrac[bad] >= 1e-4]
        fails.append(f"{what}: frac outside its bar in {bad.size} rows ({gross.size} of them by >= 1e-4: a wrong neighbour; the rest lost "
                     f"accuracy), idx {(exp['lag'][bad] + exp['L']).tolist()[:64]}, worst {np.nanmax(efrac):.3e}")
    return float(np.max(emag)) if emag.size else 0.0, float(np.max(efrac)) if efrac.size else 0.0, fails


def check_pulse_output(out, L, q, ps, seq, readcnt, what=""):
    """One fetched block of a digital-mode plan fed pulse_block(L, q, ps) against the closed form: lag equal, mag and frac within the
    bar, the matrix equal to the expected one (reference row verbatim), the header verbatim, every phasor exactly 1.
    Returns (worst mag error, worst frac error, failures)."""
    exp = closed_form(L, q, ps)
    emag, efrac, fails = compare({k: out[k][1:] for k in ("lag", "mag", "frac")}, exp, what)
    if out["lag"][0] != 0 or out["mag"][0] != 0 or out["frac"][0] != 0 or out["phasor"][0] != 0:
        fails.append(f"{what}: the reference row's own lag, mag, frac and phasor are not zero")
    want = expected_matrix(L, q, ps)
    if not np.array_equal(out["matrix"], want):
        bad = np.flatnonzero(np.any(out["matrix"] != want, axis=1))
        fails.append(f"{what}: matrix rows differ from the expected ones: rows {bad[:16].tolist()} (idx {[int(exp['idx'][r - 1]) if r else 'ref' for r in bad[:16]]})")
    nhdr = out["packet"].size - out["matrix"].size
    if not np.array_equal(out["packet"][:nhdr], expected_header(seq, 1 + len(ps), L, readcnt)):
        fails.append(f"{what}: header differs")
    if not np.all(out["phasor"][1:] == 1.0):
        fails.append(f"{what}: {np.count_nonzero(out['phasor'][1:] != 1.0)} phasors are not exactly 1")
    return emag, efrac, fails


def model_reference(model, rows):
    """lag, mag, frac, ym, mp, yp, bar of every signal row from oracle/model_fp64.py (any rows: the band-limited ones)."""
    L = rows.shape[1] // 2
    B = 2 * L
    ref = model.to_complex(rows[0])
    n = rows.shape[0] - 1
    out = dict(lag=np.zeros(n, dtype=np.int64), mag=np.zeros(n), frac=np.zeros(n), ym=np.zeros(n), mp=np.zeros(n), yp=np.zeros(n), L=L)
    for k in range(n):
        lag, mag, frac, m = model.xcorr_lag(model.to_complex(rows[1 + k]), ref)
        idx = lag + L
        out["lag"][k], out["mag"][k], out["frac"][k], out["mp"][k] = lag, mag, frac, m[idx]
        out["ym"][k] = m[idx - 1] if idx > 0 else 0.0
        out["yp"][k] = m[idx + 1] if idx < B - 1 else 0.0
    inner = (out["lag"] + L > 0) & (out["lag"] + L < B - 1)
    out["bar"] = np.where(inner, frac_bar(out["ym"], out["mp"], out["yp"], out["frac"]), 0.0)
    return out


# ---- rows with real fractional delays -----------------------------------------------------------------------------------------------
FRACTIONAL_DELAYS = (300.25, -7.4, 63.25, -511.7, 1000.4, 37.3)      # no half-sample delay: there the two top bins nearly tie
FRACTIONAL_PHIS = (0.4, -1.1, 2.5, 0.0, 1.9, -2.7)


def _bandlimited_rows(L, total_delays, phis, seed=3, band=0.25, sigma=30.0):
    """ref = low-pass complex Gaussian noise (|f| < band * fs / 2); row k = ref delayed by total_delays[k] samples
    (any real number: the delay is a phase ramp on a 4L-point spectrum of a longer realisation, so nothing wraps into
    the block) and rotated by phis[k]; int8, round half even."""
    rng = np.random.default_rng(seed)
    n = 4 * L
    X = np.fft.fft(rng.standard_normal(n) + 1j * rng.standard_normal(n))
    f = np.fft.fftfreq(n)
    X[np.abs(f) > band / 2] = 0
    base = np.fft.ifft(X)
    base *= sigma / np.sqrt(np.mean(np.abs(base) ** 2) / 2)

    def q(x):
        out = np.empty(2 * L, dtype=np.int8)
        out[0::2] = np.clip(np.rint(x.real), -128, 127)
        out[1::2] = np.clip(np.rint(x.imag), -128, 127)
        return out

    rows = np.zeros((1 + len(total_delays), 2 * L), dtype=np.int8)
    rows[0] = q(base[L:2 * L])
    for k, (tau, phi) in enumerate(zip(total_delays, phis)):
        xs = np.fft.ifft(X * np.exp(-2j * np.pi * f * tau)) * (sigma / np.sqrt(np.mean(np.abs(np.fft.ifft(X)) ** 2) / 2))
        rows[1 + k] = q(xs[L:2 * L] * np.exp(1j * phi))
    return rows


def fractional_rows(L):
    return _bandlimited_rows(L, FRACTIONAL_DELAYS, FRACTIONAL_PHIS)
