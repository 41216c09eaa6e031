"""The unrounded fp64 model of the fractional-delay correction (tests/frac_delay_model.py) and the inputs of the device tests
(tests/frac_edge_cases.py), on the CPU.

tests/test_gpu_frac_edges.py holds every kernel of crsdr_plan_set_frac_apply to this model per sample, so the model is held here
to what the suite already has: the digital mode's zero-filled shift (D = 0), a known answer (a band-limited row delayed by a
non-integer amount comes out aligned), the circular definition beyond |lag + D| = L, and the rounded matrix of
oracle/model_fp64.Model.  The fp32 CPU reference (oracle.Engine) is then measured against the model on every input family of the
device tests: that number, not anything the device gives, is what the device bars are derived from.  Last, the steering blocks of
every new (L, shift) are checked in the fp64 correlation like those of tests/test_phase_path_model.py.
"""
import numpy as np
import pytest

import frac_delay_model as fm
import frac_edge_cases as fe
import phase_path_cases as pc
import phase_path_model as pm
from peak_cases import _bandlimited_rows


def _cplx(row):
    return row[..., 0::2].astype(np.float64) + 1j * row[..., 1::2].astype(np.float64)


@pytest.mark.parametrize("L", [8, 64, 4096])
def test_zero_delay_is_the_zero_filled_integer_shift(L):
    # every shift of shift_set(L), +-(L - 1) included, and lag = -L (all zeros out): 1e-9 of a count on full-scale rows
    rng = np.random.default_rng(L)
    shifts = pc.shift_set(L) + [-L]
    assert L - 1 in shifts and -(L - 1) in shifts
    rows = rng.integers(-128, 128, size=(len(shifts), 2 * L)).astype(np.int8)
    z = fm.unrounded(rows, shifts, np.zeros(len(shifts), np.float32), np.ones(len(shifts), np.complex64))
    exp = np.stack([_cplx(pm.shift_row(r, d)) for r, d in zip(rows, shifts)])
    assert np.abs(z - exp).max() <= 1e-9
    assert np.abs(z[-1]).max() <= 1e-9 and rows[-1].any()
    # a phasor multiplies; the quantised value of an exact shift is the shift
    z2 = fm.unrounded(rows, shifts, np.zeros(len(shifts), np.float32), np.full(len(shifts), -1j, np.complex64))
    assert np.abs(z2 + 1j * exp).max() <= 1e-9
    assert np.array_equal(fm.quantised(z), np.stack([pm.shift_row(r, d) for r, d in zip(rows, shifts)]))


def test_band_limited_row_comes_out_aligned():
    # rows = the reference delayed by a non-integer number of samples and turned by phi, rounded to int8 (peak_cases).  Advanced by
    # that amount and turned back, a row must equal the undelayed reference.  The construction's own error: both int8 roundings
    # are white, uniform in [-0.5, 0.5] per component -- variance 1 / 12 each, and the correction (an all-pass response) keeps the
    # row's -- so the complex difference has an rms of sqrt(4 / 12) = 0.577 count; the zero-padded row's edges ring into the
    # interpolation as sigma / (pi distance), below 0.04 count at L / 16 = 256 samples from an edge.  Allowed: rms 0.577 * 1.1, and
    # 6 standard deviations (sqrt(1 / 6) per component) for the largest component.  A residual misalignment of 0.1 sample would add
    # 1.9 count rms (sigma = 30, band 0.25), one sample 19.
    L = 4096
    total = [37.5, -120.5, 300.25, -7.4, 0.0, 1000.3]
    phis = [0.4, -1.1, 2.5, 0.0, 0.7, -2.0]
    rows = _bandlimited_rows(L, total, phis)
    lag = np.rint(total).astype(np.int64)
    D = (np.array(total) - lag).astype(np.float32)
    z = fm.unrounded(rows[1:], lag, D, np.exp(-1j * np.array(phis)).astype(np.complex64))
    ref = _cplx(rows[0])
    for k, tau in enumerate(total):
        lo, hi = max(0, -int(lag[k]) - 1) + L // 16, min(L, L - int(lag[k]) - 1) - L // 16       # inside the overlap
        err = z[k, lo:hi] - ref[lo:hi]
        rms, big = np.sqrt(np.mean(np.abs(err) ** 2)), max(np.abs(err.real).max(), np.abs(err.imag).max())
        print(f"delay {tau}: rms {rms:.3f} count, largest component {big:.2f}")
        assert rms <= 0.577 * 1.1, (tau, rms)
        assert big <= 6 * np.sqrt(1 / 6), (tau, big)
        # the integer shift alone leaves the fraction in
        if abs(D[k]) >= 0.25:
            plain = fm.unrounded(rows[1 + k:2 + k], lag[k:k + 1], np.zeros(1, np.float32), np.exp(-1j * np.array(phis[k:k + 1])).astype(np.complex64))
            assert np.sqrt(np.mean(np.abs(plain[0, lo:hi] - ref[lo:hi]) ** 2)) > 3.0


def test_beyond_the_row_length_the_advance_wraps_over_two_row_lengths():
    # the shared definition is a CIRCULAR advance of the zero-padded row over 2 L: for |lag + D| > L samples re-enter from the other end
    L = 64
    rng = np.random.default_rng(5)
    row = rng.integers(-128, 128, size=(1, 2 * L)).astype(np.int8)
    s = _cplx(row[0])
    one = np.ones(1, np.complex64)
    z = fm.unrounded(row, [L - 1], np.array([7.0], np.float32), one)[0]          # lag + D = L + 6: z[n] = pad[(n + L + 6) mod 2 L]
    assert np.abs(z[:L - 6]).max() <= 1e-9 and np.abs(z[L - 6:] - s[:6]).max() <= 1e-9
    z = fm.unrounded(row, [-L], np.array([-3.0], np.float32), one)[0]            # lag + D = -(L + 3): the last three samples come in first
    assert np.abs(z[:3] - s[L - 3:]).max() <= 1e-9 and np.abs(z[3:]).max() <= 1e-9
    z = fm.unrounded(row, [-(L - 1)], np.array([-64.0], np.float32), one)[0]     # the largest admitted |D| at the last lag
    assert np.abs(z[:63] - s[1:]).max() <= 1e-9 and abs(z[63]) <= 1e-9
    # and a full turn of 2 L samples is the identity
    a = fm.unrounded(row, [5], np.array([0.3], np.float32), one)
    b = fm.unrounded(row, [5 - 2 * L], np.array([0.3], np.float32), one)
    assert np.abs(a - b).max() <= 1e-9


def test_rounding_agrees_with_the_fp64_model(model):
    # rint(clip(z)) is the matrix of oracle/model_fp64.Model with the correction on, fed the same lags and the same (complex64)
    # phasors: full-scale rows, lags at both ends, every D of the override
    rng = np.random.default_rng(77)
    L, n = 256, 1 + len(fe.D_SET)
    B = 2 * L
    rows = rng.integers(-128, 128, size=(n, B)).astype(np.int8)
    lags = np.array([0] + [int(x) for x in rng.choice(pc.shift_set(L) + [-L], size=n - 1)])
    lags[1:4] = (L - 1, -(L - 1), -L)
    ph = (rng.uniform(0.5, 1.4, n) * np.exp(1j * rng.uniform(-np.pi, np.pi, n))).astype(np.complex64)
    D = fe.d_vector(n)
    mod = model.Model(n, B, model.DIGITAL)
    mod.set_frac_apply(True, 1.0, D)
    mod.lag[:] = lags
    mod.p[:] = ph.astype(np.complex128)
    mat = mod.block(rows, lag_mask=np.zeros(n, np.uint8), refnoise_enabled=False)[4]
    z = fm.unrounded(rows[1:], lags[1:], D[1:], ph[1:])
    assert np.array_equal(fm.quantised(z), mat[1:])
    assert np.count_nonzero((mat[1:] == 127) | (mat[1:] == -128)) > 50          # the clamp is reached
    assert fm.excess(mat[1:], z) <= 0.0
    # the criterion sees one LSB, one position, one sign
    bad = mat[1:].copy()
    bad[3, 11] += 1 if bad[3, 11] < 127 else -1
    assert fm.excess(bad, z) >= 0.0
    assert fm.excess(np.roll(mat[1:], 2, axis=1), z) > 20 and fm.excess((-mat[1:].astype(np.int16)).clip(-128, 127).astype(np.int8), z) > 20
    # D of the estimate-driven form: one fp32 product
    assert fm.delay_of(128.0, np.float32(0.1)).dtype == np.float32 and fm.delay_of(-128.0, np.float32(0.1)) == np.float32(-128.0) * np.float32(0.1)


def test_criterion_sees_small_local_errors_of_the_response():
    # a correctly ROUNDED result of a response that is wrong at the Nyquist bin alone, or at one of the 128 k_hi table entries by
    # 3e-4 rad (18 entries of 16384 move by one count: the rounded-matrix comparison, +-1 LSB on 2e-3 of the entries, lets that
    # through), or a first sample that is off by one count -- each is over the bar of the B = 16384 kernels, 4 x 2e-5 count
    rng = np.random.default_rng(14)
    L = 8192
    B = 2 * L
    row = rng.integers(-128, 128, size=(1, B)).astype(np.int8)
    lag, D, p = 1000, np.float32(0.3), np.complex64(0.6 - 0.7j)
    z = fm.unrounded(row, [lag], [D], [p])
    fs = np.fft.fftfreq(B, d=1.0 / B)
    X = np.fft.fft(np.concatenate([_cplx(row[0]), np.zeros(L)]))
    H = np.exp(2j * np.pi * fs * (lag + float(D)) / B)
    assert np.abs(complex(p) * np.fft.ifft(X * H)[:L] - z[0]).max() < 1e-8
    bar = fe.MARGIN * 2e-5

    def rounded(Hm):
        return fm.quantised((complex(p) * np.fft.ifft(X * Hm)[:L])[None])

    assert fm.excess(rounded(H), z) <= 0.0
    nyq = H.copy()
    nyq[L] = np.exp(2j * np.pi * L * (lag + float(D)) / B)               # k_s = +L instead of -L: differs by cis(2 pi D)
    khi = H.copy()
    khi[37 * 128:38 * 128] *= np.exp(3e-4j)
    for name, Hm in (("nyquist", nyq), ("one k_hi entry", khi)):
        q = rounded(Hm)
        changed = np.count_nonzero(q != rounded(H))
        e = fm.excess(q, z)
        print(f"{name}: {changed} of {q.size} entries move, excess {e:.2e} count")
        assert e > bar and (name == "nyquist" or changed <= 2e-3 * q.size), (name, changed, e)    # (the table entry passes the old criterion)
    q = rounded(H)
    q[0, 0] += 1 if q[0, 0] < 127 else -1
    assert fm.excess(q, z) > bar


@pytest.mark.parametrize("family", sorted(fe.FAMILIES) + ["long2", "fuzz"])
def test_reference_excess_of_every_family_leaves_a_usable_bar(family):
    # oracle.Engine (fp32 FFT, the ramp formed in double) with the correction on, on the inputs of the device tests, against the
    # model fed the oracle's own lag, phasor and frac.  Its lags are the steered ones (asserted inside).  4 x this value is the
    # family's bar on the device: it must stay below 0.1 count, and the reference itself must be a correct rounding to that bar.
    ref = fe.reference_excess(family)
    print(f"{family}: reference excess {ref:.3e} count, bar without the argument term {fe.MARGIN * ref:.3e}")
    assert 0.0 < fe.MARGIN * ref <= fe.MAX_BAR, (family, ref)


def test_argument_term_and_bar_are_what_the_issue_states():
    assert fe.argument_term(np.array([0.5, 1.0, -1.0]), 100.0).tolist() == [0.0, 0.0, 0.0]
    assert np.allclose(fe.argument_term(np.array([64.0, -7.3]), np.array([181.0, 181.0])), 2 * np.pi * np.array([64.0, 7.3]) * 2.0 ** -24 * 181.0)
    assert fe.argument_term(64.0, 182.0) < 0.005                               # full scale at the largest |D|: far below the 0.1 count limit
    ex, arg = np.array([[0.001, 0.5]]), np.array([[0.0, 0.004]])
    with pytest.raises(AssertionError, match="over the bar"):
        fe.assert_within("x", ex, arg, 1e-3)
    fe.assert_within("x", np.array([[0.0039, 0.0079]]), arg, 1e-3)
    with pytest.raises(AssertionError, match="above 0.1"):
        fe.assert_within("x", ex, arg, 0.03)
    D = fe.d_vector(40)
    assert D[0] == 777.0 and set(D[1:].tolist()) == {np.float32(d) for d in fe.D_SET} and np.abs(D[1:]).max() == 64.0


def _fp64_peak(model, sig_i8, ref_i8):
    lag, _, _, m = model.xcorr_lag(model.to_complex(sig_i8), model.to_complex(ref_i8))
    peak = m[lag + sig_i8.size // 2]
    m = m.copy()
    m[lag + sig_i8.size // 2] = 0.0
    return lag, peak / max(m.max(), 1e-300)


@pytest.mark.parametrize("case", fe.STEERED_CASES, ids=lambda c: c.name)
def test_steering_rows_of_the_new_cases_give_the_target_lag_with_a_clear_peak(model, case):
    # as tests/test_phase_path_model.py holds it for its own cases: lag == d in the fp64 correlation and a peak-to-runner-up power
    # ratio of at least 4, for every (L, d) and every steering block the device tests submit
    L, covered, worst = case.L, set(), np.inf
    for sub in pc.submits(case):
        if sub.kind != "steer":
            continue
        for t in range(case.T):
            for r in sub.steered:
                lag, ratio = _fp64_peak(model, sub.rows[t, r], sub.rows[t, 0])
                assert lag == sub.lag[t, r], (case.name, t, r, lag)
                if not sub.rows[t, r].any():
                    assert lag == -L
                    continue
                assert lag == case.shift_list[r - 1] and ratio >= 4.0, (case.name, t, r, lag, ratio)
                worst = min(worst, ratio)
                covered.add(int(lag))
    assert covered == set(case.shift_list)
    print(f"{case.name}: L = {L}, {len(covered)} shifts, smallest peak-to-runner-up power ratio {worst:.1f}")


def test_two_line_rows_have_known_lags_of_both_signs_beyond_half_the_row(synth, model):
    rows, d = fe.long2_blocks(synth)
    L = fe.LONG2_B // 2
    assert rows.shape == (2, fe.LONG2_NSIG + 1, fe.LONG2_B) and (1 << 4) * fe.LONG2_NSIG >= 1024     # N1 = B / 16384 lines per row
    k = int(np.argmax(np.abs(d)))
    lag, ratio = _fp64_peak(model, rows[0, 1 + k], rows[0, 0])                   # the weakest overlap
    assert lag == d[k] and abs(lag) > L // 2 and ratio >= 4.0, (lag, d[k], ratio)


def test_fuzz_draw_reaches_what_it_claims(synth):
    cfgs = [fe.fuzz_config(s, synth) for s in range(fe.FUZZ_SEEDS)]
    bt = [b for c in cfgs for b in c["batches"]]
    assert any(c["rb"] > 1 for c in cfgs) and any(c["offset_binary"] for c in cfgs) and any(c["T"] == 5 for c in cfgs) and max(c["T"] for c in cfgs) <= 5
    assert any(b["mask"] is not None for b in bt) and any(b["locked"] for b in bt) and any(not b["refnoise"] for b in bt) and any(b["readcnt"] is not None for b in bt)
    assert any(c["setting"].override for c in cfgs) and {c["setting"].gain for c in cfgs if not c["setting"].override} == set(fe.GAINS)
    assert {c["B"] for c in cfgs} >= {16384, 1 << 15} and min(c["B"] for c in cfgs) <= 64
