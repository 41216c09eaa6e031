"""The exact phase-path model (tests/phase_path_model.py) and the steering rows (tests/phase_path_cases.py), on the CPU.

The GPU tests (tests/test_gpu_phase_path.py) hold the device to this model bit for bit, so the model itself is held here to
the two references the suite already has: the C oracle's single-rounding ops byte for byte, and the fp64 model at that file's own
bars (phase 1e-5 rad, matrix +-1 LSB).  The steering rows are checked in the fp64 model for every (L, d) a GPU case uses: the
reported lag is d, and the correlation peak clears the runner-up by a power ratio of at least 4 (an amplitude ratio of 2: far
above what two fp32 FFT factorisations can move; a condition on the inputs, not a measurement).
"""
import numpy as np
import pytest

import phase_path_cases as pc
import phase_path_model as pm


def test_rotate_quantise_equals_the_oracle_ops_byte_for_byte(oracle):
    # 200 full-scale random rows (-128 and 127 included) at random shifts in [-L, L), rotated by EMA-like phasors (modulus <= 1) and
    # by phasors that drive full-scale samples into the clamp
    rng = np.random.default_rng(41)
    L = 256
    sat = 0
    for k in range(200):
        row = rng.integers(-128, 128, size=2 * L).astype(np.int8)
        y = pm.shift_row(row, int(rng.integers(-L, L)))
        ang, mod = rng.uniform(-np.pi, np.pi), rng.uniform(0.05, 1.0) if k % 4 else 1.0
        p = np.complex64(mod * np.exp(1j * ang))
        got = pm.rotate_quantise(y, (p.real, p.imag))
        exp = oracle.convto8bit(oracle.scalarmul(oracle.convtofloat(y), p))
        assert np.array_equal(got, exp), k
        sat += int(np.count_nonzero((exp == 127) | (exp == -128)))
    assert sat >= 200                                    # the clamp was really reached (on average in every row)


def test_shift_is_the_definition_at_every_shift():
    L = 16
    row = (np.arange(2 * L) + 1).astype(np.int8)
    s = row.reshape(L, 2)
    for d in range(-L, L):
        y = pm.shift_row(row, d).reshape(L, 2)
        for n in range(L):
            exp = s[n + d] if 0 <= n + d < L else (0, 0)
            assert tuple(y[n]) == tuple(exp), (d, n)
    assert not pm.shift_row(row, -L).any()               # lag = -L: everything is shifted out
    for bad in (-L - 1, L):
        with pytest.raises(ValueError):
            pm.shift_row(row, bad)


def test_dot_unit_phasor_and_chain_against_plain_formulas():
    rng = np.random.default_rng(3)
    y, r = rng.integers(-128, 128, size=512).astype(np.int8), rng.integers(-128, 128, size=512).astype(np.int8)
    sr, si = pm.dot_sums(y, r)
    c = np.sum((y[0::2].astype(np.float64) + 1j * y[1::2]) * np.conj(r[0::2].astype(np.float64) + 1j * r[1::2]))
    assert (sr, si) == (int(c.real), int(c.imag))
    assert pm.dot_sums(np.full(4, -128, np.int8), np.full(4, -128, np.int8)) == (4 * 128 * 128, 0)
    assert pm.unit_phasor(0, 0) is None
    u = pm.unit_phasor(sr, si)
    assert abs(complex(u[0], u[1]) - np.conj(c) / abs(c)) < 1e-7
    assert pm.unit_phasor(5, 0) == (1.0, 0.0) and pm.unit_phasor(0, -3) == (0.0, 1.0)
    p = pm.ema((np.float32(1), np.float32(0)), u)
    assert p[0].dtype == np.float32 and p == (np.float32(0.5) * u[0] + np.float32(0.5), np.float32(0.5) * u[1])
    assert pm.to_signed(np.array([0x00, 0x80, 0xFF], dtype=np.uint8), offset_binary=True).tolist() == [-128, 0, 127]


@pytest.mark.parametrize("B", [128, 2048])
def test_model_agrees_with_the_fp64_model_at_its_own_bars(model, B):
    # the exact model must not drift from the fp64 definition: same lags given, phasor within 1e-5 rad and 1e-5 in modulus over a
    # chain of blocks, matrix within +-1 LSB.  Rows: full-scale random, a zero row ("hold"), a refnoise-off block.
    rng = np.random.default_rng(B)
    L, nrows = B // 2, 6
    lags = np.array([0, 0, 3, -5, L - 1, -(L // 2)])
    exact = pm.PhasePathModel(nrows, B)
    fp = model.Model(nrows, B, model.DIGITAL)
    none = np.zeros(nrows, dtype=np.uint8)
    for t in range(6):
        rows = rng.integers(-128, 128, size=(nrows, B)).astype(np.int8)
        if t == 2:
            rows[3] = 0
        fp.lag[:] = lags                                 # the lag is given: no row is requested (the locked cadence)
        refnoise = t != 4
        _, _, _, ph, mat = fp.block(rows, lag_mask=none, refnoise_enabled=refnoise)
        got = exact.block(rows, lag=lags if t == 0 else None, refnoise=refnoise, seq=t)
        assert np.abs(np.angle(got["phasor"][1:] * np.conj(ph[1:]))).max() <= 1e-5
        assert np.abs(np.abs(got["phasor"][1:]) - np.abs(ph[1:])).max() <= 1e-5
        d = got["matrix"].astype(np.int16) - mat.astype(np.int16)
        assert np.abs(d).max() <= 1 and np.count_nonzero(d) <= 1e-3 * d.size
        assert np.array_equal(got["matrix"][0], rows[0])
        hdr = got["packet"][:exact.matrix_offset].view(np.uint32)
        assert hdr.tolist() == [t, nrows, L, 0] + [t] * nrows
        assert np.array_equal(got["packet"][exact.matrix_offset:].reshape(nrows, B), got["matrix"])


def test_model_chain_holds_freezes_and_takes_a_given_phasor():
    B, nrows = 64, 3
    rng = np.random.default_rng(9)
    m = pm.PhasePathModel(nrows, B)
    rows = rng.integers(-128, 128, size=(nrows, B)).astype(np.int8)
    a = m.block(rows, lag=[0, 1, -2])
    assert a["phasor"][0] == 0 and np.all(a["phasor"][1:] != 1)
    z = rows.copy()
    z[1] = 0
    h = m.block(z)                                       # zero row: |corr| = 0 holds the phasor, the row comes out zero
    assert h["phasor"][1] == a["phasor"][1] and h["phasor"][2] != a["phasor"][2] and not h["matrix"][1].any()
    f = m.block(rng.integers(-128, 128, size=(nrows, B)).astype(np.int8), refnoise=False)
    assert np.array_equal(f["phasor"], h["phasor"]) and f["matrix"][1:].any()          # frozen, the rotation still applied
    out = m.block(rows, lag=[0, -B // 2, 0])             # lag = -L: shifted out entirely, held again
    assert not out["matrix"][1].any() and out["phasor"][1] == f["phasor"][1] and out["sums"][1] == (0, 0)
    g = pm.PhasePathModel(nrows, B).block(rows, lag=[0, 1, -2], phasor=np.array([0, 1j, -1], dtype=np.complex64))
    y = pm.shift_row(rows[2], -2)
    neg = np.clip(-y.astype(np.int16), -128, 127).astype(np.int8)       # p = -1: every product exact, -(-128) clamps to 127
    assert np.array_equal(g["matrix"][2], neg)


def _fp64_peak(model, sig_i8, ref_i8):
    lag, _, _, m = model.xcorr_lag(model.to_complex(sig_i8), model.to_complex(ref_i8))
    peak = m[lag + sig_i8.size // 2]
    m = m.copy()
    m[lag + sig_i8.size // 2] = 0.0
    return lag, peak / max(m.max(), 1e-300)


@pytest.mark.parametrize("case", pc.ALL_CASES, ids=lambda c: c.name)
def test_steering_rows_give_the_target_lag_with_a_clear_peak(model, case):
    # every (L, d) of the GPU module, every steering block it submits: lag == d in the fp64 model, peak-to-runner-up power >= 4
    L = case.L
    subs = pc.submits(case)
    covered = set()
    worst = np.inf
    for sub in subs:
        assert sub.rows.shape == (case.T, case.nrows, case.B) and sub.lag.shape == (case.T, case.nrows)
        if sub.kind != "steer":
            continue
        for t in range(case.T):
            for r in sub.steered:
                lag, ratio = _fp64_peak(model, sub.rows[t, r], sub.rows[t, 0])
                assert lag == sub.lag[t, r], (case.name, t, r, lag)
                if not sub.rows[t, r].any():             # a zeroed row (chain_zeroed): the first index of an all-zero correlation
                    assert lag == -L
                    continue
                assert lag == case.shift_list[r - 1], (case.name, t, r, lag)
                assert ratio >= 4.0, (case.name, t, r, ratio)
                worst = min(worst, ratio)
                covered.add(int(lag))
    assert covered == set(case.shift_list)               # every shift of the case is steered by some submit
    if case.variant != "chain_zeroed":
        assert np.array_equal(subs[-1].lag[-1, 1:], case.shift_list)
    else:
        assert list(subs[-1].lag[-1, 1:]) == case.shift_list[:2] + [-L]
    print(f"{case.name}: L = {L}, {len(covered)} shifts, smallest peak-to-runner-up power ratio {worst:.1f}")


@pytest.mark.parametrize("case", pc.CHAIN_CASES + [pc.PATH_CASES[2]], ids=lambda c: c.name)
def test_comparison_passes_on_the_model_and_fails_by_one_bit(case):
    # the GPU module's comparison and its chain properties, on a known answer: the model's own output passes; a copy damaged by one
    # matrix LSB, one phasor bit, one header word or one lag fails, each under its own heading
    res = pc.model_results(case)
    pc.compare(case, res)
    pc.chain_properties(case, res)
    j = len(res) - 1

    def damaged(key, fn):
        out = [dict(r) for r in res]
        out[j] = dict(res[j], **{key: fn(res[j][key].copy())})
        if key == "packet":
            out[j]["matrix"] = out[j]["packet"][16 + 4 * case.nrows:].reshape(case.nrows, case.B)
        return out

    def lsb(m):
        m[case.nrows - 1, case.B - 1] ^= 1
        return m

    def bit(p):
        p.view(np.uint32)[3] ^= 1                        # row 1, imaginary part, last bit
        return p

    def word(p):
        p.view(np.uint32)[5] ^= 1                        # readcnt of row 1
        return p

    def lag(x):
        x[1] += 1
        return x

    for key, fn, text in (("matrix", lsb, "matrix given the device's phasor"), ("phasor", bit, "phasor differs in rows [1]"),
                          ("packet", word, "header"), ("lag", lag, "PRECONDITION")):
        with pytest.raises(AssertionError, match=text.replace("[", r"\[").replace("]", r"\]")):
            pc.compare(case, damaged(key, fn))


def test_shift_sets_cover_what_they_claim():
    for L in (8, 64):
        assert pc.shift_set(L) == list(range(-(L - 1), L))
    for L in (512, 2048, 4096, 8192, 1 << 14, 1 << 15):
        s = pc.shift_set(L)
        assert len(s) == len(set(s)) and all(-L < d < L for d in s)
        for sign in (1, -1):
            assert {(sign * d) % 8 for d in s if sign * d > 0} == set(range(8))           # every residue mod 8, both signs
        for d in (L - 1, -(L - 1), L // 2, -(L // 2), L - 8, -(L - 8)):
            assert d in s
    # steering rows: values outside the overlap are never zero, so a leaked sample is visible
    rows = pc.steering_block(64, [5], [True], 1)
    assert np.all(rows[1, :10] != 0) and np.array_equal(rows[1, 10:], rows[0, :-10])
