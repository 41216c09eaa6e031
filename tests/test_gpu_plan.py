"""GPU parity, plan level: crsdr_plan_{submit,fetch} (the ccoherent::threadf iteration) against
the CPU oracle and the committed golden vectors, through the C ABI.

Bars (SURVEY.md 8c / BASELINE.json north_star):
  lags            bit-exact (equal argmax; test rows have a sharp peak, PAPR >> fp32 noise)
  mag             relative 1e-4 (two different fp32 FFT factorizations)
  phase           <= 1e-5 rad against the fp64 model and the fp32 oracle
  int8 matrix     equal except +-1 LSB at rint boundaries, <= 0.1 % of entries;
                  bit-exact when the oracle is fed the GPU's own phasor (rotate/quantise are
                  single-rounding ops in the same order on both sides)
"""
import importlib
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def b():
    binding = importlib.import_module("coherent-rtlsdr_amd.binding")
    if binding.device_count() < 1:
        pytest.fail("no HIP device: the product path has no CPU fallback")
    return binding


def _compare(got, exp, phase_tol=1e-5):
    """got: HIP path, exp: fp32 C oracle.  phase_tol is 1e-5 rad wherever the phase is well
    conditioned (rows aligned with the reference); rows that are NOT sample-aligned (faithful
    mode with injected delays) correlate to ~noise, the oracle's sequential fp32 accumulator
    (VOLK generic) then carries ~1e-5..1e-4 rad of its own rounding, and the strict 1e-5 bound
    is checked against the fp64 model instead (_compare_model)."""
    assert np.array_equal(got["lag"], exp["lag"]), (got["lag"], exp["lag"])
    assert np.allclose(got["mag"], exp["mag"], rtol=1e-4)
    assert np.allclose(got["frac"], exp["frac"], atol=5e-3)
    gp, ep = got["phasor"][1:], exp["phasor"][1:]
    assert np.abs(np.angle(gp * np.conj(ep))).max() <= phase_tol
    assert np.allclose(np.abs(gp), np.abs(ep), rtol=max(1e-5, phase_tol), atol=1e-7)
    diff = got["matrix"].astype(np.int16) - exp["matrix"].astype(np.int16)
    assert np.abs(diff).max() <= 1
    assert np.count_nonzero(diff) <= 1e-3 * diff.size
    assert np.array_equal(got["packet"][:got["packet"].size - diff.size], exp["packet"][:exp["packet"].size - diff.size])


def _compare_model(got, mod):
    """got: HIP path, mod: (lag, mag, frac, phasor, matrix) of the fp64 numpy model."""
    lag, mag, frac, ph, mat = mod
    assert np.array_equal(got["lag"], lag)
    assert np.allclose(got["mag"], mag, rtol=1e-4)
    assert np.abs(np.angle(got["phasor"][1:] * np.conj(ph[1:]))).max() <= 1e-5
    d = got["matrix"].astype(np.int16) - mat.astype(np.int16)
    assert np.abs(d).max() <= 1 and np.count_nonzero(d) <= 1e-3 * d.size


@pytest.mark.parametrize("name", ["cfg1_faithful", "cfg1_digital", "small_digital", "long_digital"])
def test_plan_matches_golden_and_oracle(b, oracle, golden_dir, name):
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    nblocks, nrows, B = g["rows"].shape
    mode = int(g["mode"])
    plan, orc = b.Plan(nrows, B, mode), oracle.Engine(nrows, B, mode)
    for t in range(nblocks):
        got = plan.block(g["rows"][t], seq=t, readcnt=np.arange(nrows) + 10 * t)
        exp = orc.block(g["rows"][t], seq=t, readcnt=np.arange(nrows) + 10 * t)
        _compare(got, exp, phase_tol=1e-5 if B <= 16384 else 1e-4)    # long rows: the oracle's fp32 accumulator, see _compare
        # committed fp64 golden
        assert np.array_equal(got["lag"], g["lag"][t])
        assert np.allclose(got["mag"], g["mag"][t], rtol=1e-4)
        assert np.abs(np.angle(got["phasor"][1:] * np.conj(g["phasor"][t][1:]))).max() <= 1e-5
        d = got["matrix"].astype(np.int16) - g["matrix"][t].astype(np.int16)
        assert np.abs(d).max() <= 1 and np.count_nonzero(d) <= 1e-3 * d.size
    plan.close()


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("nsig,L", [(21, 8192), (7, 512), (2, 8), (5, 64)])
def test_plan_vs_oracle_synthetic(b, oracle, model, synth, mode, nsig, L):
    # config 2 shape (URA21.cfg: 1 + 21 rows x 8192) and small / minimum block sizes
    seed = synth.config_seed(2) + L
    params = synth.RowParams(nsig, L, seed, dmax=max(1, L // 4))
    plan, orc = b.Plan(nsig + 1, 2 * L, mode), oracle.Engine(nsig + 1, 2 * L, mode)
    mod = model.Model(nsig + 1, 2 * L, mode)
    for t in range(3):
        rows, _ = synth.make_block(nsig, L, seed, t, params=params)
        got, exp = plan.block(rows, seq=t), orc.block(rows, seq=t)
        if L >= 512:
            assert np.array_equal(got["lag"][1:], params.d)       # injected delays recovered
            _compare(got, exp, phase_tol=1e-5 if mode == 1 else 2e-4)
            _compare_model(got, mod.block(rows))                  # strict 1e-5 rad vs fp64
        else:
            # tiny blocks: the peak is not always sharp; lags must still equal the oracle's
            assert np.array_equal(got["lag"], exp["lag"])
    plan.close()


def test_rotate_quantise_bitexact_given_gpu_phasor(b, oracle, synth):
    # per-op parity of a11+a12 inside the fused kernel: feed the GPU's phasor to the oracle ops
    nsig, L = 4, 4096
    rows, _ = synth.make_block(nsig, L, 99, 0, dmax=0, locked=True)
    plan = b.Plan(nsig + 1, 2 * L, b.MODE_FAITHFUL)
    got = plan.block(rows)
    for r in range(1, nsig + 1):
        y = oracle.scalarmul(oracle.convtofloat(rows[r]), got["phasor"][r])
        assert np.array_equal(oracle.convto8bit(y), got["matrix"][r])
    plan.close()


def test_lag_mask_refnoise_gate_and_locked_mode(b, oracle, synth):
    nsig, L = 6, 1024
    params = synth.RowParams(nsig, L, 7, dmax=100)
    rows, _ = synth.make_block(nsig, L, 7, 0, params=params)
    plan, orc = b.Plan(nsig + 1, 2 * L, b.MODE_DIGITAL), oracle.Engine(nsig + 1, 2 * L, oracle.DIGITAL)
    mask = np.zeros(nsig + 1, dtype=np.uint8)
    mask[[2, 5]] = 1
    _compare(plan.block(rows, lag_mask=mask), orc.block(rows, lag_mask=mask))
    _compare(plan.block(rows), orc.block(rows))                                     # all rows now
    # locked steady state: no lag requested, phase path only (CRSDR_NO_LAG), lags are kept
    rows2, _ = synth.make_block(nsig, L, 7, 1, params=params)
    none = np.zeros(nsig + 1, dtype=np.uint8)
    _compare(plan.block(rows2, flags=b.REFNOISE_ENABLED | b.NO_LAG), orc.block(rows2, lag_mask=none))
    # refnoise off: phasor frozen, rotation still applied (src/ccoherent.cc:271-275)
    rows3, _ = synth.make_block(nsig, L, 7, 2, params=params)
    got, exp = plan.block(rows3, flags=0), orc.block(rows3, refnoise_enabled=False)
    _compare(got, exp)
    plan.close()


def test_offset_binary_input_matches_signed(b, synth):
    # a1 fused into the loads: raw librtlsdr uint8 (x ^ 0x80) gives identical results
    nsig, L = 3, 2048
    rows, p = synth.make_block(nsig, L, 11, 0, dmax=300)
    rows_u8 = (rows.view(np.uint8) ^ np.uint8(0x80))
    for mode in (0, 1):
        a = b.Plan(nsig + 1, 2 * L, mode).block(rows)
        c = b.Plan(nsig + 1, 2 * L, mode).block(rows_u8, flags=b.REFNOISE_ENABLED | b.OFFSET_BINARY)
        for k in ("lag", "mag", "phasor", "packet"):
            assert np.array_equal(a[k], c[k]), k


def test_zero_row_holds_phasor_and_reset(b, oracle, synth):
    nsig, L = 2, 512
    rows, _ = synth.make_block(nsig, L, 3, 0, dmax=0, locked=True)
    rows[2] = 0
    plan = b.Plan(nsig + 1, 2 * L, b.MODE_FAITHFUL)
    got = plan.block(rows)
    assert got["phasor"][2] == 1.0 + 0j and not np.any(np.isnan(got["phasor"].view(np.float32)))
    assert np.all(got["matrix"][2] == 0)
    first = plan.block(rows)["phasor"].copy()
    plan.reset()
    again = plan.block(rows)
    assert np.array_equal(again["phasor"], got["phasor"]) and not np.array_equal(first, again["phasor"])
    plan.close()


def test_slab_plans_reassemble_the_full_matrix(b, synth):
    # multi-GPU decomposition on one device: two plans own disjoint slabs of the signal rows;
    # stitching their rows reproduces the single-plan matrix bit for bit (rows are independent
    # given row 0)
    nsig, L = 8, 1024
    rows, _ = synth.make_block(nsig, L, 21, 0, dmax=100)
    full = b.Plan(nsig + 1, 2 * L, b.MODE_DIGITAL).block(rows)
    lo = b.Plan(nsig + 1, 2 * L, b.MODE_DIGITAL, row_begin=1, row_count=4).block(rows)
    hi = b.Plan(nsig + 1, 2 * L, b.MODE_DIGITAL, row_begin=5, row_count=4).block(rows)
    assert np.array_equal(lo["matrix"][:5], full["matrix"][:5])
    assert np.array_equal(hi["matrix"][5:], full["matrix"][5:])
    assert np.array_equal(lo["lag"][1:5], full["lag"][1:5]) and np.array_equal(hi["lag"][5:], full["lag"][5:])
    assert np.array_equal(hi["matrix"][0], full["matrix"][0])       # ref row replicated


def test_full_size_properties_cfg3(b, synth, model):
    # 1 + 256 rows x 8192 (config 3): size-independent properties instead of a CPU re-run:
    #  - every injected delay is recovered exactly,
    #  - after digital alignment each row's xcorr with the ref row peaks at the centre
    #    (matlabclient/seqnum_and_correlation.m:27-43) and the residual phase is ~0,
    #  - the header/readcnt words are what the parser expects (matlabclient/zmqsdr.c:118-144).
    nsig, L = 256, 8192
    seed = synth.config_seed(3)
    params = synth.RowParams(nsig, L, seed)
    plan = b.Plan(nsig + 1, 2 * L, b.MODE_DIGITAL)
    for t in range(8):
        rows, _ = synth.make_block(nsig, L, seed, t, params=params)
        plan.submit(rows, seq=t)
    out = plan.fetch()
    assert np.array_equal(out["lag"][1:], params.d)
    hdr = out["packet"][:16].view(np.uint32)
    assert list(hdr) == [7, nsig + 1, L, 0]
    assert np.all(out["packet"][16:16 + 4 * (nsig + 1)].view(np.uint32) == 7)
    ref = model.to_complex(out["matrix"][0])
    for r in (1, 2, 3, 77, 200, 256):
        y = model.to_complex(out["matrix"][r])
        lag, _, _, _ = model.xcorr_lag(y, ref)
        assert lag == 0
        assert abs(np.angle(np.sum(y * np.conj(ref)))) < 0.03
    # phasors converged to exp(-j phi_k) (EMA, 8 blocks): 2^-8 residual
    assert np.abs(np.angle(out["phasor"][1:] * np.exp(1j * params.phi))).max() < 0.05
    plan.close()


def test_async_pipeline_equals_blockwise(b, synth):
    # submitting several blocks back to back (no host sync) gives the same final state as
    # fetching after every block: EMA state is carried on the device in stream order
    nsig, L = 5, 2048
    params = synth.RowParams(nsig, L, 5, dmax=100)
    blocks = [synth.make_block(nsig, L, 5, t, params=params)[0] for t in range(6)]
    p1, p2 = b.Plan(nsig + 1, 2 * L, b.MODE_FAITHFUL), b.Plan(nsig + 1, 2 * L, b.MODE_FAITHFUL)
    for t, rows in enumerate(blocks):
        last = p1.block(rows, seq=t)
    for t, rows in enumerate(blocks):
        p2.submit(rows, seq=t)
    piped = p2.fetch()
    for k in ("lag", "mag", "phasor", "packet"):
        assert np.array_equal(last[k], piped[k]), k


@pytest.mark.parametrize("mode", [0, 1])
def test_batched_submit_equals_blockwise(b, oracle, synth, mode):
    # crsdr_plan_submit_batch: T blocks in one submit == T submits in a row, bit for bit, for
    # every block of the batch (EMA phasor and last lag are carried block to block), including a
    # lag mask (rows that are not requested keep the lag of an earlier batch) and a second batch.
    nsig, L, T = 6, 2048, 4
    params = synth.RowParams(nsig, L, 31, dmax=300)
    blocks = np.stack([synth.make_block(nsig, L, 31, t, params=params)[0] for t in range(2 * T)])
    one, many = b.Plan(nsig + 1, 2 * L, mode), b.Plan(nsig + 1, 2 * L, mode, max_batch=T)
    orc = oracle.Engine(nsig + 1, 2 * L, mode)
    mask = np.ones(nsig + 1, dtype=np.uint8)
    ref_out = []
    for t in range(2 * T):
        mk = mask if t < T else np.array([0, 1, 0, 1, 0, 1, 0], dtype=np.uint8)
        ref_out.append(one.block(blocks[t], seq=100 + t, lag_mask=mk))
        _compare(ref_out[-1], orc.block(blocks[t], seq=100 + t, lag_mask=mk), phase_tol=1e-5 if mode == 1 else 2e-4)
    for half in range(2):
        mk = mask if half == 0 else np.array([0, 1, 0, 1, 0, 1, 0], dtype=np.uint8)
        many.submit(blocks[half * T:(half + 1) * T], seq=100 + half * T, lag_mask=mk)
        for t in range(T):
            got = many.fetch(block=t)
            exp = ref_out[half * T + t]
            for k in ("lag", "mag", "frac", "phasor", "packet"):
                assert np.array_equal(got[k], exp[k]), (half, t, k)
    one.close(); many.close()


def test_pipelined_async_fetch_equals_blockwise(b, synth):
    # crsdr_plan_fetch_batch_async / crsdr_plan_fetch_wait: batches submitted back to back with their fetches in flight (the
    # next submit's upload shares the link with the previous batch's download; its kernels wait on the device for that
    # download) must hand back, batch by batch, exactly what fetching every block synchronously gives -- packets and scalars.
    nsig, L, T, nb = 40, 8192, 6, 5
    nrows, B = nsig + 1, 2 * L
    params = synth.RowParams(nsig, L, 606, dmax=900)
    blocks = np.stack([synth.make_block(nsig, L, 606, t, params=params)[0] for t in range(nb * T)])
    ref = b.Plan(nrows, B, b.MODE_DIGITAL, max_batch=T)
    exp = []
    for i in range(nb):
        ref.submit(blocks[i * T:(i + 1) * T], seq=i * T)
        exp.append([ref.fetch(block=t) for t in range(T)])
    plan = b.Plan(nrows, B, b.MODE_DIGITAL, max_batch=T)
    pstride = plan.packet_stride
    rows_pin = [b.PinnedArray((T, nrows, B), np.int8) for _ in range(2)]
    out = [dict(lag=b.PinnedArray((T, nrows), np.int32), mag=b.PinnedArray((T, nrows), np.float32), frac=b.PinnedArray((T, nrows), np.float32),
                phasor=b.PinnedArray((T, nrows, 2), np.float32), packets=b.PinnedArray((T * pstride,), np.int8)) for _ in range(2)]

    def submit(i):
        s = i & 1
        rows_pin[s].array[:] = blocks[i * T:(i + 1) * T]
        plan.submit(rows_pin[s].array, seq=i * T)
        o = out[s]
        plan.fetch_batch_async(o["lag"].array, o["mag"].array, o["frac"].array, o["phasor"].array, o["packets"].array, pstride)

    def check(i):
        plan.fetch_wait()
        o = out[i & 1]
        for t in range(T):
            e = exp[i][t]
            assert np.array_equal(o["lag"].array[t], e["lag"]) and np.array_equal(o["mag"].array[t], e["mag"]), (i, t)
            assert np.array_equal(o["frac"].array[t], e["frac"]), (i, t)
            assert np.array_equal(o["phasor"].array[t].reshape(-1).view(np.complex64), e["phasor"]), (i, t)
            assert np.array_equal(o["packets"].array[t * pstride: t * pstride + plan.packet_bytes], e["packet"]), (i, t)

    submit(0)
    for i in range(1, nb):
        submit(i)
        check(i - 1)
    check(nb - 1)
    with pytest.raises(b.CrsdrError):
        plan.fetch_wait()                                        # nothing outstanding any more
    plan.sync()
    for x in rows_pin + [v for o in out for v in o.values()]:
        x.close()
    plan.close(); ref.close()


def test_batch_argument_checks(b):
    plan = b.Plan(3, 1024, max_batch=2)
    with pytest.raises(b.CrsdrError):
        plan.submit(np.zeros((3, 3, 1024), dtype=np.int8))      # more blocks than max_batch
    with pytest.raises(b.CrsdrError):
        b.Plan(3, 1024, max_batch=1000)
    plan.close()


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("log2B", [15, 16, 17, 18, 19, 20])      # N1 = 2 ... 64: every radix split of the column passes (128 and 256: the tests below)
def test_long_block_plan_vs_oracle(b, oracle, model, synth, mode, log2B):
    # blocks longer than the LDS-resident 16384 points: B = N1 x 16384 four-step transform
    # (column FFTs -> row FFTs x conj(ref) -> inverse), chunked phase/rotate kernels
    nsig, B = 3, 1 << log2B
    L = B // 2
    seed = 500 + log2B
    params = synth.RowParams(nsig, L, seed)
    plan, orc = b.Plan(nsig + 1, B, mode), oracle.Engine(nsig + 1, B, mode)
    mod = model.Model(nsig + 1, B, mode)
    for t in range(2):
        rows, _ = synth.make_block(nsig, L, seed, t, params=params)
        got, exp = plan.block(rows, seq=t), orc.block(rows, seq=t)
        assert np.array_equal(got["lag"][1:], params.d)
        _compare(got, exp, phase_tol=1e-5 if mode == 1 else 2e-4)
        _compare_model(got, mod.block(rows))
    plan.close()


def test_cfg5_long_blocks_full_size(b, oracle, model, synth):
    # BASELINE config 5: 1 + 21 rows x 2^20 samples (B = 2^21 = 128 x 16384), digital mode
    nsig, L = 21, 1 << 20
    seed = synth.config_seed(5)
    params = synth.RowParams(nsig, L, seed)
    rows, _ = synth.make_block(nsig, L, seed, 0, params=params)
    plan = b.Plan(nsig + 1, 2 * L, b.MODE_DIGITAL)
    got = plan.block(rows)
    assert np.array_equal(got["lag"][1:], params.d)                       # every injected delay, exactly
    exp = oracle.Engine(nsig + 1, 2 * L, oracle.DIGITAL).block(rows, nthreads=8)
    # over 2^20 terms the oracle's sequential fp32 dot product (VOLK generic) carries ~2e-5 rad of
    # its own rounding; the 1e-5 bar is checked against the fp64 model, whose sum the GPU's exact
    # integer dot product reproduces
    _compare(got, exp, phase_tol=1e-4)
    _compare_model(got, model.Model(nsig + 1, 2 * L, model.DIGITAL).block(rows))
    # second block: EMA state carried, lags re-estimated
    rows2, _ = synth.make_block(nsig, L, seed, 1, params=params)
    got2 = plan.block(rows2, seq=1)
    assert np.array_equal(got2["lag"][1:], params.d)
    assert np.abs(np.angle(got2["phasor"][1:] * np.exp(1j * params.phi))).max() < 0.8   # converging: 1/4 residual after 2 blocks
    plan.close()


def test_full_scale_dc_rows_do_not_overflow(b, oracle):
    # worst case for the un-scaled integer transform chain: every sample -128-128j in every row.  The
    # correlation is a triangle peaking at zero lag; |ifft|^2 reaches (B L 32768)^2 = 2^84 ~ 1.9e25 (< FLT_MAX) before the
    # final 1/127^2 scale (B = 2^22: 2^116, test_gpu_long_chunks.py).  No inf / NaN, lag 0, mag equal to the oracle's.
    nsig, L = 3, 8192
    rows = np.full((nsig + 1, 2 * L), -128, dtype=np.int8)
    got = b.Plan(nsig + 1, 2 * L, b.MODE_DIGITAL).block(rows)
    exp = oracle.Engine(nsig + 1, 2 * L, oracle.DIGITAL).block(rows)
    assert np.all(np.isfinite(got["mag"])) and np.all(np.isfinite(got["frac"]))
    assert np.array_equal(got["lag"], exp["lag"]) and np.all(got["lag"] == 0)
    assert np.allclose(got["mag"], exp["mag"], rtol=1e-4)
    assert np.array_equal(got["matrix"], exp["matrix"])


def test_maximum_block_size_plan(b, synth):
    # largest supported block: B = 2^22 (N1 = 256 column transforms): delays recovered exactly
    nsig, L = 1, 1 << 21
    params = synth.RowParams(nsig, L, 9, dmax=5000)
    rows, _ = synth.make_block(nsig, L, 9, 0, params=params)
    got = b.Plan(nsig + 1, 2 * L, b.MODE_DIGITAL).block(rows)
    assert np.array_equal(got["lag"][1:], params.d)
    with pytest.raises(b.CrsdrError):
        b.Plan(2, 1 << 23)                                        # beyond the supported range
    with pytest.raises(b.CrsdrError):
        b.Plan(2, 1 << 21, max_batch=2)                           # long blocks are submitted one at a time


def _delayed_rows(L, delays, phis, seed=5, sigma=30.0):
    """ref row = seeded complex Gaussian; row k = ref delayed by delays[k] samples and rotated by phis[k]
    (noise-free), the construction of the oracle's known-answer tests (tests/test_oracle_engine.py)."""
    rng = np.random.default_rng(seed)
    pad = L
    r_ext = rng.standard_normal(L + 2 * pad) + 1j * rng.standard_normal(L + 2 * pad)
    rows = np.zeros((1 + len(delays), 2 * L), dtype=np.int8)

    def q(x):
        out = np.empty(2 * L, dtype=np.int8)
        out[0::2] = np.clip(np.rint(x.real), -128, 127)
        out[1::2] = np.clip(np.rint(x.imag), -128, 127)
        return out

    n = np.arange(L)
    rows[0] = q(sigma * r_ext[pad:pad + L])
    for k, (d, phi) in enumerate(zip(delays, phis)):
        rows[1 + k] = q(sigma * r_ext[n - d + pad] * np.exp(1j * phi))
    return rows


@pytest.mark.parametrize("L", [4096, 8192, 1 << 15])
def test_known_delays_give_idx_L_plus_d(b, L):
    # SURVEY 8c known answers, on the HIP path at the reference block size and either side of it:
    # s[n] = r[n - d]  ->  idx = L + d, lag = +d, for d in {0, +-1, +-7, +-1000, -L/2+1, L/2-1}
    delays = [0, 1, -1, 7, -7, 1000, -1000, -L // 2 + 1, L // 2 - 1]
    rows = _delayed_rows(L, delays, [0.0] * len(delays))
    for mode in (b.MODE_FAITHFUL, b.MODE_DIGITAL):
        plan = b.Plan(1 + len(delays), 2 * L, mode)
        out = plan.block(rows)
        assert list(out["lag"][1:]) == delays
        assert np.all(np.abs(out["frac"][1:]) < 0.05)
        # noise-free integer copy: the peak is B x the overlap energy (src/ccoherent.cc:204)
        r = rows[0].astype(np.float64) / 127.0
        e = r[0::2] ** 2 + r[1::2] ** 2
        for k, d in enumerate(delays):
            ov = e[:L - d].sum() if d >= 0 else e[-d:].sum()
            expect = 2 * L * ov / np.sqrt(L)      # unnormalised backward FFT: m[idx] = (B ov)^2, mag = sqrt(m / L)
            assert abs(out["mag"][1 + k] - expect) <= 1e-4 * expect
        plan.close()


def test_pure_rotation_gives_conjugate_phasor_and_ema(b):
    # a10: corr = sum s conj(r) = |.| e^{j phi}; p_raw = e^{-j phi}; EMA from p_prev = 1 (src/csdrdevice.cc:39-40,63-67)
    L = 8192
    phis = [0.3, -1.2, 2.9, -3.0]
    rows = _delayed_rows(L, [0] * 4, phis)
    plan = b.Plan(5, 2 * L, b.MODE_FAITHFUL)
    out = plan.block(rows)
    for k, phi in enumerate(phis):
        assert abs(out["phasor"][1 + k] - (0.5 * np.exp(-1j * phi) + 0.5)) < 2e-3
    for t in range(20):
        out = plan.block(rows, seq=1 + t)
    for k, phi in enumerate(phis):
        assert abs(out["phasor"][1 + k] - np.exp(-1j * phi)) < 2e-3
    frozen = out["phasor"].copy()
    out = plan.block(_delayed_rows(L, [0] * 4, [1.0] * 4), seq=30, flags=0)          # refnoise off: estimate frozen
    assert np.array_equal(out["phasor"], frozen)
    plan.close()


def test_digital_mode_centres_the_correlation_peak(b, model):
    # mirrors matlabclient/seqnum_and_correlation.m:27-43 on the HIP path: after alignment every row of the
    # published matrix correlates with the ref row at the centre (lag 0) with the phase removed
    L = 8192
    delays, phis = [13, -200, 511, -2047], [0.7, -2.0, 3.0, 0.1]
    rows = _delayed_rows(L, delays, phis)
    plan = b.Plan(5, 2 * L, b.MODE_DIGITAL)
    for t in range(12):
        out = plan.block(rows, seq=t)
    ref = model.to_complex(out["matrix"][0])
    for k in range(4):
        y = model.to_complex(out["matrix"][1 + k])
        lag, _, _, _ = model.xcorr_lag(y, ref)
        assert lag == 0
        assert abs(np.angle(np.sum(y * np.conj(ref)))) < 2e-2
    plan.close()



@pytest.mark.parametrize("G,aligned", [(2, True), (4, True), (4, False)])
def test_slab_output_all_to_all_and_assembly_equal_the_single_plan(b, synth, G, aligned):
    # the multi-GPU exchange shape of bench.py on one device: G sharded plans in slab mode (crsdr_plan_bind_slab)
    # write dense [T][per][B] buffers; the all-to-all is emulated by indexing (rank q receives chunk q of every
    # rank's buffer); crsdr_assemble_slabs places the chunks.  Every assembled packet must equal the packet of an
    # unsharded plan bit for bit -- over two consecutive batches (the EMA / lag state is carried per rank).
    import torch
    nsig, L, T = 8, 1024, 4 if G == 4 else 6
    nrows, B = nsig + 1, 2 * L
    per, Tg = nsig // G, T // G
    dev = torch.device("cuda", 0)
    params = synth.RowParams(nsig, L, 77, dmax=200)
    blocks = np.stack([synth.make_block(nsig, L, 77, t, params=params)[0] for t in range(2 * T)])
    full = b.Plan(nrows, B, b.MODE_DIGITAL, max_batch=T)
    plans = [b.Plan(nrows, B, b.MODE_DIGITAL, row_begin=1 + r * per, row_count=per, max_batch=T) for r in range(G)]
    pbytes = full.packet_bytes
    pstride = (pbytes + 255) // 256 * 256
    skew = 0 if aligned else 4                      # 4-byte aligned only: the word-wise (non-16-byte) kernels
    send = [torch.zeros(T * per * B + 64, dtype=torch.uint8, device=dev) for _ in range(G)]
    pk = [torch.zeros(Tg * pstride + 64, dtype=torch.uint8, device=dev) for _ in range(G)]
    off = [(-(p.data_ptr() + full.matrix_offset)) % 16 + skew for p in pk]
    soff = [(-s.data_ptr()) % 16 + skew for s in send]
    for half in range(2):
        d_in = torch.from_numpy(blocks[half * T:(half + 1) * T].view(np.uint8)).to(dev)
        full.submit(d_in.data_ptr(), seq=10 + half * T, nblocks=T, block_stride=nrows * B)
        exp = [full.fetch(block=t)["packet"] for t in range(T)]
        for r, pl in enumerate(plans):
            pl.bind_packet(pk[r].data_ptr() + off[r], pstride)
            pl.bind_slab(send[r].data_ptr() + soff[r], per * B, r * Tg, Tg)
            pl.submit(d_in.data_ptr(), seq=10 + half * T, nblocks=T, block_stride=nrows * B)
            pl.sync()
            with pytest.raises(b.CrsdrError):
                pl.fetch()                             # packets are not assembled by the plan in slab mode
            out = pl.fetch(want_packet=False)
            assert np.array_equal(out["lag"][1 + r * per: 1 + (r + 1) * per], params.d[r * per:(r + 1) * per])
        for q in range(G):                              # root q: chunk q of every rank's send buffer
            recv = torch.stack([send[r][soff[r]: soff[r] + T * per * B].view(G, Tg * per * B)[q] for r in range(G)]).contiguous()
            b.assemble_slabs(pk[q].data_ptr() + off[q], pstride, nrows, B, recv.data_ptr(), G, Tg)
            torch.cuda.synchronize()
            for j in range(Tg):
                got = pk[q][off[q] + j * pstride: off[q] + j * pstride + pbytes].cpu().numpy().view(np.int8)
                assert np.array_equal(got, exp[q * Tg + j]), (half, q, j)
    for pl in plans + [full]:
        pl.close()


@pytest.mark.parametrize("B", [1024, 16384, 1 << 15])
def test_device_input_and_bound_packet_alignments(b, synth, B):
    # caller-owned device memory (CRSDR_MEM_DEVICE + crsdr_plan_bind_packet): 16-byte aligned pointers take the
    # 16-byte vector kernels, 4-byte aligned ones the word kernels, anything else is refused.  Every combination
    # must reproduce the host-buffer result bit for bit, with a block stride larger than one block.
    import torch
    nsig, L, T = 4, B // 2, 1 if B > 16384 else 3
    nrows = nsig + 1
    params = synth.RowParams(nsig, L, 91, dmax=L // 8)
    blocks = np.stack([synth.make_block(nsig, L, 91, t, params=params)[0] for t in range(T)])
    ref = b.Plan(nrows, B, b.MODE_DIGITAL, max_batch=T)
    ref.submit(blocks if T > 1 else blocks[0], seq=5)
    exp = [ref.fetch(block=t) for t in range(T)]
    dev = torch.device("cuda", 0)
    stride = nrows * B + 64
    pstride = (ref.packet_bytes + 3) // 4 * 4 + 32
    for in_off, pk_off in ((0, 0), (4, 0), (0, 8), (12, 4)):
        raw = torch.zeros(T * stride + 64, dtype=torch.uint8, device=dev)
        base = (-raw.data_ptr()) % 16 + in_off
        for t in range(T):
            raw[base + t * stride: base + t * stride + nrows * B] = torch.from_numpy(blocks[t].view(np.uint8).reshape(-1)).to(dev)
        pk = torch.zeros(T * pstride + 64, dtype=torch.uint8, device=dev)
        pbase = (-(pk.data_ptr() + ref.matrix_offset)) % 16 + pk_off
        plan = b.Plan(nrows, B, b.MODE_DIGITAL, max_batch=T)
        plan.bind_packet(pk.data_ptr() + pbase, pstride)
        plan.submit(raw.data_ptr() + base, seq=5, nblocks=T, block_stride=stride)
        plan.sync()
        for t in range(T):
            got = plan.fetch(block=t)
            for k in ("lag", "mag", "frac", "phasor", "packet"):
                assert np.array_equal(got[k], exp[t][k]), (in_off, pk_off, t, k)
            mine = pk[pbase + t * pstride: pbase + t * pstride + ref.packet_bytes].cpu().numpy().view(np.int8)
            assert np.array_equal(mine, exp[t]["packet"]), (in_off, pk_off, t)
        with pytest.raises(b.CrsdrError):
            plan.submit(raw.data_ptr() + base + 1, seq=5, nblocks=T, block_stride=stride)      # not 4-byte aligned
        with pytest.raises(b.CrsdrError):
            plan.bind_packet(pk.data_ptr() + pbase + 2, pstride)
        plan.close()
    ref.close()


def test_k1_variants_agree(tmp_path):
    # CRSDR_K1_VARIANT: packed (xcorr14p.hpp), the two-row kernel q and its carried-chain form r (xcorr14q.hpp; "auto", the default,
    # takes r for launches of >= 12 rows per CU and packed below; q runs only when forced)
    # run the same passes with the same arithmetic: every output agrees bit for bit.  (The two-row kernel's argmax -- per-wave
    # candidates, an edge table, the last wave to arrive finishes -- against the packed kernel's barrier-and-atomicMin form: the
    # first maximum, its parabolic neighbours across wave edges and the lag-mask / skip path included.)  The variant is chosen
    # once per process, so each runs in a child.  (r01's scalar-fp32 twin left the product in r03: tools/xcorr14_scalar.hpp.)
    import subprocess, sys, textwrap
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = textwrap.dedent('''
        import importlib, sys, numpy as np
        sys.path.insert(0, %r)
        pkg = importlib.import_module("coherent-rtlsdr_amd")
        b, synth = pkg.binding, pkg.synth
        nsig, L, T = 37, 8192, 3
        params = synth.RowParams(nsig, L, 4242, dmax=2000)
        blocks = np.stack([synth.make_block(nsig, L, 4242, t, params=params)[0] for t in range(T)])
        plan = b.Plan(nsig + 1, 2 * L, b.MODE_DIGITAL, max_batch=T)
        plan.submit(blocks, seq=3)
        outs = [plan.fetch(block=t) for t in range(T)]
        # a second, larger launch (several rows per workgroup for the persistent two-row kernel) with a lag mask:
        # every third row keeps its carried lag (xcorr_skip), two batches so that there is carried state
        nsig2, T2 = 640, 5
        params2 = synth.RowParams(nsig2, L, 777, dmax=3000)
        blocks2 = np.stack([synth.make_block(nsig2, L, 777, t, params=params2)[0] for t in range(T2)])
        plan2 = b.Plan(nsig2 + 1, 2 * L, b.MODE_DIGITAL, max_batch=T2)
        mask = (np.arange(nsig2 + 1) %% 3 != 0).astype(np.uint8)
        plan2.submit(blocks2, seq=0)
        plan2.submit(blocks2, seq=T2, lag_mask=mask)
        outs2 = [plan2.fetch(block=t) for t in range(T2)]
        np.savez(sys.argv[1], lag=np.stack([o["lag"] for o in outs]), mag=np.stack([o["mag"] for o in outs]),
                 frac=np.stack([o["frac"] for o in outs]), packet=np.stack([o["packet"] for o in outs]), d=params.d,
                 lag2=np.stack([o["lag"] for o in outs2]), mag2=np.stack([o["mag"] for o in outs2]),
                 frac2=np.stack([o["frac"] for o in outs2]), d2=params2.d)
    ''') % root
    res = {}
    # "*_nofold" (CRSDR_K1_FOLD=0): the reference spectra from k_ref_spectrum14p on the aux stream instead of from the launch's own
    # first work items -- the same arithmetic in another place
    for variant in ("packed", "q", "r", "auto", "packed_nofold"):
        out = tmp_path / f"{variant}.npz"
        env = dict(os.environ, CRSDR_K1_VARIANT=variant.split("_")[0], CRSDR_K1_FOLD="0" if variant.endswith("_nofold") else "1")
        r = subprocess.run([sys.executable, "-c", code, str(out)], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        res[variant] = np.load(out)
    for key in res["packed"].files:
        for other in ("packed_nofold",):
            assert np.array_equal(res["packed"][key].view(np.uint8), res[other][key].view(np.uint8)), (other, key)
    for key in ("lag", "mag", "frac", "packet"):
        # q: the packed passes run by one persistent workgroup per CU, two rows in opposite phases (xcorr14q.hpp): identical bits
        assert np.array_equal(res["packed"][key].view(np.uint8), res["q"][key].view(np.uint8)), ("q", key)
        # r: q with the column twiddle chains carried from row to row (k_xcorr_lag14r), a compilation of its own
        assert np.array_equal(res["packed"][key].view(np.uint8), res["r"][key].view(np.uint8)), ("r", key)
    for key in ("lag2", "mag2", "frac2"):      # 3200 items (>= 12 per CU): "auto" takes the two-row kernel r here by itself
        assert np.array_equal(res["packed"][key].view(np.uint8), res["q"][key].view(np.uint8)), ("q", key)
        assert np.array_equal(res["packed"][key].view(np.uint8), res["r"][key].view(np.uint8)), ("r", key)
        assert np.array_equal(res["packed"][key].view(np.uint8), res["auto"][key].view(np.uint8)), ("auto", key)
    assert np.array_equal(res["q"]["lag2"][0, 1:], res["q"]["d2"])


def test_long_block_two_line_stage_b_is_bit_identical(tmp_path):
    # stage B of the long-block path (the 16384-point line transforms x conj(ref)) runs two lines per CU in opposite phases
    # (k_rows14_cf32q) once a launch has >= 1024 lines, the one-line packed kernel otherwise: the same passes on the same
    # data, so lags, magnitudes and packets are equal bit for bit.  CRSDR_LONG_Q is read once per process -> children.
    import subprocess, sys, textwrap
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = textwrap.dedent('''
        import importlib, sys, numpy as np
        sys.path.insert(0, %r)
        pkg = importlib.import_module("coherent-rtlsdr_amd")
        b, synth = pkg.binding, pkg.synth
        res = {}
        for name, nsig, log2B, nblk in (("many", 300, 16, 2), ("odd", 343, 15, 2), ("cfg5", 21, 21, 2)):
            L = (1 << log2B) // 2
            params = synth.RowParams(nsig, L, 31 + log2B)
            plan = b.Plan(nsig + 1, 2 * L, b.MODE_DIGITAL)
            for t in range(nblk):
                rows, _ = synth.make_block(nsig, L, 31 + log2B, t, params=params)
                out = plan.block(rows, seq=t)
                assert np.array_equal(out["lag"][1:], params.d), name
            for key in ("lag", "mag", "frac", "packet"):
                res[name + "_" + key] = out[key]
            plan.close()
        np.savez(sys.argv[1], **res)
    ''') % root
    # (r02 also compared the other work orders of the stages -- lines in memory order, one workgroup per tile in stage A,
    # persistent stage C -- behind switches that were removed in r03 with the measurements that settled them: DESIGN.md section 4.)
    res = {}
    variants = {"0": {"CRSDR_LONG_Q": "0"}, "1": {"CRSDR_LONG_Q": "1"}}
    for q, env in variants.items():
        out = tmp_path / f"longq{q}.npz"
        r = subprocess.run([sys.executable, "-c", code, str(out)], env=dict(os.environ, **env), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        res[q] = np.load(out)
    assert set(res["0"].files) == set(res["1"].files) and len(res["0"].files) == 12
    for key in res["0"].files:
        assert np.array_equal(res["0"][key].view(np.uint8), res["1"][key].view(np.uint8)), key


def test_two_row_kernel_reports_a_wait_that_ran_out(tmp_path):
    # the two-row K1 (xcorr14q.hpp) bounds every wait for the LDS image / its group barriers.  With the bound forced to
    # zero polls (CRSDR_K1_QSPIN=0) waits do run out: the launch must terminate, the next sync / fetch must return an
    # error (never silent garbage), and the plan must be usable again afterwards: the failed batch is ROLLED BACK (carried
    # lag / mag / frac and EMA phase state restored to what they were before it), the plan stays on the packed kernel,
    # and resubmitting the batch -- then a locked batch that shifts by the carried lags -- gives bit for bit what a
    # plan that never used the two-row kernel gives.  Checked in child processes (the variant is read once per process).
    import subprocess, sys, textwrap
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = textwrap.dedent('''
        import importlib, sys, numpy as np
        sys.path.insert(0, %r)
        pkg = importlib.import_module("coherent-rtlsdr_amd")
        b, synth = pkg.binding, pkg.synth
        nsig, L, T1, T2 = 300, 8192, 4, 12
        params = synth.RowParams(nsig, L, 99, dmax=1000)
        blocks = np.stack([synth.make_block(nsig, L, 99, t, params=params)[0] for t in range(T1 + T2 + T1)])
        plan = b.Plan(nsig + 1, 2 * L, b.MODE_DIGITAL, max_batch=T2)
        plan.submit(blocks[:T1], seq=0)                   # 1200 rows: the packed kernel under "auto" -- builds carried state
        res = [plan.fetch(block=t) for t in range(T1)]
        plan.submit(blocks[T1:T1 + T2], seq=T1)           # 3600 rows (>= 12 per CU): "auto" takes the two-row kernel
        try:
            plan.fetch(block=0)
            print("NOERROR")
        except b.CrsdrError as e:
            print("ERROR", e)
            try:
                plan.fetch(block=0)
                print("STALE-FETCH-ALLOWED")
            except b.CrsdrError:
                pass                                      # nothing to fetch until the batch is resubmitted
            plan.submit(blocks[T1:T1 + T2], seq=T1)       # resubmit: rolled back state + packed kernel
        res += [plan.fetch(block=t) for t in range(T2)]
        plan.submit(blocks[T1 + T2:], seq=T1 + T2, flags=b.REFNOISE_ENABLED | b.NO_LAG)     # locked: shifts by the carried lags
        res += [plan.fetch(block=t) for t in range(T1)]
        np.savez(sys.argv[1], lag=np.stack([r["lag"] for r in res]), mag=np.stack([r["mag"] for r in res]),
                 phasor=np.stack([r["phasor"] for r in res]), packet=np.stack([r["packet"] for r in res]), d=params.d)
    ''') % root
    outs = {}
    for name, env, expect in (("runout", {"CRSDR_K1_VARIANT": "auto", "CRSDR_K1_QSPIN": "0"}, "ERROR"),
                              ("packed", {"CRSDR_K1_VARIANT": "packed"}, "NOERROR"),
                              ("auto", {"CRSDR_K1_VARIANT": "auto"}, "NOERROR")):      # the same launches with the normal bound: clean
        out = tmp_path / f"{name}.npz"
        r = subprocess.run([sys.executable, "-c", code, str(out)], env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        assert expect in r.stdout and "STALE-FETCH-ALLOWED" not in r.stdout, r.stdout + r.stderr
        if name == "runout":
            assert "bounded wait" in r.stdout and "rolled back" in r.stdout, r.stdout
        outs[name] = np.load(out)
    for other in ("runout", "auto"):
        for key in ("lag", "mag", "phasor", "packet"):
            assert np.array_equal(outs["packed"][key].view(np.uint8), outs[other][key].view(np.uint8)), (other, key)
    assert np.array_equal(outs["runout"]["lag"][-1, 1:], outs["runout"]["d"])


def test_pipelined_fetch_rolls_back_to_the_last_clean_batch(tmp_path):
    # The host loop of the batched engine never calls sync / fetch: submit, fetch_batch_async, fetch_wait only.  A bounded wait
    # of the two-row kernel that runs out at batch 3 -- after three CLEAN two-row batches (CRSDR_K1_QSPIN=0@3: spin budget zero
    # from the process's fourth two-row launch on) -- must roll the plan back to the state before batch 3, not to the state
    # before batch 0 (r02: the only snapshot was taken at the first two-row launch and a clean fetch_wait never renewed it), and
    # say how many batches to resubmit.  Resubmitting that one batch, then a locked batch that shifts by the carried lags,
    # gives bit for bit what a plan on the packed kernel gives.
    import subprocess, sys, textwrap
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = textwrap.dedent('''
        import importlib, sys, numpy as np
        sys.path.insert(0, %r)
        pkg = importlib.import_module("coherent-rtlsdr_amd")
        b, synth = pkg.binding, pkg.synth
        nsig, L, T, NB = 300, 8192, 12, 5                 # 3600 rows per batch (>= 12 per CU): "auto" takes the two-row kernel
        nrows, B = nsig + 1, 2 * L
        params = synth.RowParams(nsig, L, 77, dmax=1000)
        blocks = np.stack([synth.make_block(nsig, L, 77, t, params=params)[0] for t in range(4 * 4)])      # 16 distinct blocks, cycled
        batch = lambda i: np.stack([blocks[(i * T + t) %% 16] for t in range(T)])
        plan = b.Plan(nrows, B, b.MODE_DIGITAL, max_batch=T)
        ps = plan.packet_stride
        rows_pin = [b.PinnedArray((T, nrows, B), np.int8) for _ in range(2)]
        out = [dict(lag=b.PinnedArray((T, nrows), np.int32), mag=b.PinnedArray((T, nrows), np.float32), frac=b.PinnedArray((T, nrows), np.float32),
                    phasor=b.PinnedArray((T, nrows, 2), np.float32), packets=b.PinnedArray((T * ps,), np.int8)) for _ in range(2)]
        res = {}
        def submit(i, flags=b.REFNOISE_ENABLED):
            s = i & 1
            rows_pin[s].array[:] = batch(i)
            plan.submit(rows_pin[s].array, seq=i * T, flags=flags)
            o = out[s]
            plan.fetch_batch_async(o["lag"].array, o["mag"].array, o["frac"].array, o["phasor"].array, o["packets"].array, ps)
        def collect(i):
            plan.fetch_wait()
            o = out[i & 1]
            res[i] = {k: v.array.copy() for k, v in o.items()}
        errors = []
        submit(0)
        i = 1
        while i < NB:
            fl = b.REFNOISE_ENABLED | (b.NO_LAG if i == NB - 1 else 0)     # the last batch is locked: it shifts by the carried lags
            submit(i, fl)
            try:
                collect(i - 1)
            except b.CrsdrError as e:
                errors.append(str(e))
                # batches i - 1 and i (submitted behind the failed one) are gone: resubmit from the first lost one
                lost = int(str(e).split("the last ")[1].split(" ")[0])
                first = i + 1 - lost
                print("ERROR at collect", i - 1, "lost", lost, "first", first)
                submit(first, b.REFNOISE_ENABLED)
                i = first + 1
                continue
            i += 1
        try:
            collect(NB - 1)
        except b.CrsdrError as e:
            errors.append(str(e))
            lost = int(str(e).split("the last ")[1].split(" ")[0])
            print("ERROR at final collect lost", lost)
            for k in range(NB - lost, NB):
                submit(k, b.REFNOISE_ENABLED | (b.NO_LAG if k == NB - 1 else 0))
                collect(k)
        print("NERR", len(errors))
        for e in errors: print(e)
        np.savez(sys.argv[1], **{f"{k}{i}": v for i, r in res.items() for k, v in r.items()}, d=params.d)
    ''') % root
    outs = {}
    for name, env, nerr in (("runout", {"CRSDR_K1_VARIANT": "auto", "CRSDR_K1_QSPIN": "0@3"}, 1), ("packed", {"CRSDR_K1_VARIANT": "packed"}, 0)):
        out = tmp_path / f"{name}.npz"
        r = subprocess.run([sys.executable, "-c", code, str(out)], env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        assert f"NERR {nerr}" in r.stdout, r.stdout + r.stderr
        if nerr:
            # batch 3 failed; batch 4 had been submitted behind it: two batches to resubmit, never the clean batches 0 .. 2
            assert "rolled back" in r.stdout and "lost 2 first 3" in r.stdout, r.stdout
        outs[name] = np.load(out)
    assert set(outs["packed"].files) == set(outs["runout"].files)
    for key in outs["packed"].files:
        assert np.array_equal(outs["packed"][key].view(np.uint8), outs["runout"][key].view(np.uint8)), key
    assert np.array_equal(outs["runout"]["lag4"][-1, 1:], outs["runout"]["d"])


def test_plan_lifecycle_does_not_leak_device_memory(b, synth):
    # create / submit / destroy in a loop (all three kernel families: generic, 16384, long-block): device memory
    # in use returns to where it started (the plan owns every device allocation, src/ccoherent.cc:100-110)
    import torch
    rows = {B: synth.make_block(2, B // 2, 3, 0, dmax=4)[0] for B in (1024, 16384, 1 << 15)}
    for B in rows:                                   # warm the allocator / code objects first
        b.Plan(3, B, b.MODE_DIGITAL).block(rows[B])
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    for _ in range(40):
        for B in rows:
            p = b.Plan(3, B, b.MODE_DIGITAL, max_batch=1 if B > 16384 else 4)
            p.block(rows[B])
            p.close()
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info()
    assert abs(free0 - free1) <= 8 << 20, (free0, free1)


def test_phase_path_variants_are_bit_identical(tmp_path):
    # the fused phase kernel (default), the same kernel with its look-back budget forced to zero -- every phasor
    # of an earlier block that is not there yet is recomputed by the waiting workgroup itself -- and the
    # three-kernel path (CRSDR_K2_FUSED=0) must agree bit for bit: same integer sums, same EMA order
    import subprocess, sys, textwrap
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = textwrap.dedent('''
        import importlib, sys, numpy as np
        sys.path.insert(0, %r)
        pkg = importlib.import_module("coherent-rtlsdr_amd")
        b, synth = pkg.binding, pkg.synth
        nsig, L, T = 301, 8192, 16
        params = synth.RowParams(nsig, L, 777, dmax=1500)
        blocks = np.stack([synth.make_block(nsig, L, 777, t, params=params)[0] for t in range(T)])
        blocks[3, 7] = 0                                  # a zero row in one block: "hold the previous phasor"
        plan = b.Plan(nsig + 1, 2 * L, b.MODE_DIGITAL, max_batch=T)
        res = []
        for rep in range(2):                              # second batch: state carried across submits
            plan.submit(blocks, seq=rep * T)
            res += [plan.fetch(block=t) for t in range(T)]
        plan.submit(blocks, seq=99, flags=b.REFNOISE_ENABLED | b.NO_LAG)     # locked cadence
        res += [plan.fetch(block=t) for t in range(T)]
        np.savez(sys.argv[1], phasor=np.stack([r["phasor"] for r in res]), packet=np.stack([r["packet"] for r in res]),
                 lag=np.stack([r["lag"] for r in res]), mag=np.stack([r["mag"] for r in res]))
    ''') % root
    outs = {}
    # ("nopoll": one look at the hand-over words and no waiting -- whatever an earlier block has published by then, its chain
    # value or only its unit phasor, is used, everything else recomputed locally: every mix of the three sources in one run)
    for name, env in (("fused", {}), ("fallback", {"CRSDR_K2_SPIN": "-1"}), ("nopoll", {"CRSDR_K2_SPIN": "0"}), ("three", {"CRSDR_K2_FUSED": "0"})):
        out = tmp_path / f"{name}.npz"
        r = subprocess.run([sys.executable, "-c", code, str(out)], env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        outs[name] = np.load(out)
    for other in ("fallback", "nopoll", "three"):
        for key in ("phasor", "packet", "lag", "mag"):
            assert np.array_equal(outs["fused"][key].view(np.uint8), outs[other][key].view(np.uint8)), (other, key)


def test_rotate_quantise_saturates_like_convto8bit(b, oracle):
    # full-scale samples rotated by ~45 degrees exceed the int8 range (127 * sqrt 2): cdsp::convto8bit clamps to
    # [-128, 127] before rounding (src/cdsp.cc:51-54); the phase kernels round and let the byte conversion saturate.
    # Bit-exact against the oracle's ops fed with the GPU's own phasor, including ties at x.5.
    L = 2048
    rng = np.random.default_rng(8)
    rows = np.zeros((4, 2 * L), dtype=np.int8)
    ref = rng.integers(-100, 100, size=2 * L).astype(np.int8)
    rows[0] = ref
    ang = np.pi / 4
    x = (ref[0::2].astype(np.float64) + 1j * ref[1::2]) * np.exp(1j * ang)          # a rotated copy: phasor -> e^{-j pi/4}
    rows[1, 0::2] = np.clip(np.rint(x.real), -128, 127); rows[1, 1::2] = np.clip(np.rint(x.imag), -128, 127)
    rows[2] = rows[1]; rows[2, :64] = 127; rows[2, 64:128] = -128                     # full-scale corners
    rows[3] = rows[1]; rows[3, 0:256:2] = 127; rows[3, 1:256:2] = -128
    plan = b.Plan(4, 2 * L, b.MODE_FAITHFUL)
    for t in range(6):
        got = plan.block(rows, seq=t)
    sat = 0
    for r in range(1, 4):
        y = oracle.scalarmul(oracle.convtofloat(rows[r]), got["phasor"][r])
        exp = oracle.convto8bit(y)
        assert np.array_equal(exp, got["matrix"][r]), r
        sat += int(np.count_nonzero((exp == 127) | (exp == -128)))
    assert sat > 50                                   # the case really saturates
    plan.close()


def test_two_plans_driven_from_two_threads_equal_their_serial_runs(b, synth):
    # the G ranks of a node may be G threads of ONE process, each with its own plan (+ exchange).  Two plans of different
    # shapes on the same device, driven concurrently from two host threads (ctypes releases the GIL inside the library: the calls really
    # overlap), must give bit for bit what each gives alone: no state shared between plans, errors are per thread.
    import threading
    shapes = [(48, 8192, 8, 901), (21, 1024, 5, 902)]          # (nsig, L, T, seed): the 16384-point kernels and a generic size
    data = []
    for nsig, L, T, seed in shapes:
        params = synth.RowParams(nsig, L, seed, dmax=L // 8)
        data.append(np.stack([synth.make_block(nsig, L, seed, t, params=params)[0] for t in range(3 * T)]))

    def run(k, out):
        nsig, L, T, _ = shapes[k]
        plan = b.Plan(nsig + 1, 2 * L, b.MODE_DIGITAL, max_batch=T)
        res = []
        for rep in range(3):
            plan.submit(data[k][rep * T:(rep + 1) * T], seq=rep * T, flags=b.REFNOISE_ENABLED | (b.NO_LAG if rep == 2 else 0))
            res += [plan.fetch(block=t) for t in range(T)]
        plan.close()
        out[k] = res

    serial, conc = {}, {}
    for k in range(2):
        run(k, serial)
    for _ in range(3):                                           # a few rounds: different interleavings
        th = [threading.Thread(target=run, args=(k, conc)) for k in range(2)]
        for t_ in th:
            t_.start()
        for t_ in th:
            t_.join()
        for k in range(2):
            assert len(conc[k]) == len(serial[k])
            for got, exp in zip(conc[k], serial[k]):
                for key in ("lag", "mag", "frac", "phasor", "packet"):
                    assert np.array_equal(got[key].view(np.uint8), exp[key].view(np.uint8)), (k, key)
