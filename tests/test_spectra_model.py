"""The fp64 model of crsdr_spectra (tests/spectra_model.py) held against what it must agree with without a device: Parseval, the
subband covariance's diagonal, a float32 restatement of the kernel's order, single mistakes that must leave the bar, and the
alignment estimator against rows whose delay, phase and gain are known."""
import numpy as np
import pytest

import doa_subband_model as SB
import peak_cases
import spectra_model as M

LO_HI = lambda N: (-(N // 10), N // 10)


@pytest.mark.parametrize("N,B", [(16, 64), (64, 1024), (256, 2048)])
def test_parseval_rect_without_overlap(N, B):
    """sum_f P_c[f] is the row's mean sample power when the segments tile the row (rect, overlap 0)"""
    mats = [M.gaussian_matrix(4, B, seed) for seed in (1, 2)]
    psd, _ = M.welch(mats, N, 0, M.WINDOW_RECT)
    power = np.mean([np.mean(np.abs(M.samples(m)) ** 2, axis=1) for m in mats], axis=0)
    assert np.allclose(psd.sum(axis=1), power, rtol=1e-12)


@pytest.mark.parametrize("kind", [M.WINDOW_RECT, M.WINDOW_HANN])
@pytest.mark.parametrize("N", [16, 64, 256])
def test_psd_is_the_diagonal_of_the_subband_covariance(N, kind):
    """two routes to the same number: P_c[f] of the signal rows = R_f[c-1][c-1] of doa_subband_model (overlap 0)"""
    mats = [M.gaussian_matrix(5, 4 * N * 2, seed) for seed in (3, 4)]
    psd, cross = M.welch(mats, N, 0, kind)
    Rf = SB.bin_covariances(mats, N, kind)
    assert np.allclose(psd[1:].T, np.einsum("faa->fa", Rf).real, rtol=1e-12, atol=0)
    assert np.array_equal(cross[0], psd[0]) and np.all(cross[0].imag == 0)


@pytest.mark.parametrize("N,B,overlap,kind", [(16, 192, 1, M.WINDOW_HANN), (64, 2048, 0, M.WINDOW_RECT), (64, 16384 + 128, 0, M.WINDOW_HANN),
                                               (256, 4096, 1, M.WINDOW_HANN), (1024, 8192, 1, M.WINDOW_RECT)])
def test_float32_restatement_stays_inside_the_bar(N, B, overlap, kind):
    mats = [M.gaussian_matrix(3, B, seed) for seed in (5, 6)]
    psd, cross = M.welch(mats, N, overlap, kind)
    bp, bc = M.bars(psd, N, M.terms(B, N, overlap))
    p32, c32 = M.welch_f32(mats, N, overlap, kind)
    assert M.worst_ratio(p32, psd, bp) <= 1.0 and M.worst_ratio(c32, cross, bc) <= 1.0


def test_chains_depend_on_the_shape_alone_and_hold_at_most_32_segments():
    for N, B, ov in ((16, 32768, 0), (16, 32768 + 32, 0), (64, 32768, 1), (256, 16384, 1), (4096, 1 << 20, 0), (4096, 16384, 1)):
        ch = M.chains(B, N, ov)
        assert sorted(j for c in ch for j in c) == list(range(M.segments(B, N, ov)))
        assert max(len(c) for c in ch) <= M.CHAIN
    # exactly one full set of chains, and one segment more
    assert [len(c) for c in M.chains(16384, 64, 0)] == [32] * 4 and [len(c) for c in M.chains(16384 + 128, 64, 0)] == [32] * 4 + [1]


@pytest.mark.parametrize("which", M.MUTATIONS)
def test_single_mistakes_leave_the_bar(which):
    N, B = 64, 1024
    mats = [M.gaussian_matrix(3, B, seed) for seed in (7, 8)]
    psd, cross = M.welch(mats, N, 1, M.WINDOW_HANN)
    bp, bc = M.bars(psd, N, M.terms(B, N, 1))
    mp, mc = M.mutated(mats, N, 1, M.WINDOW_HANN, which)
    assert max(M.worst_ratio(mp, psd, bp), M.worst_ratio(mc, cross, bc)) > 1.0, which


def test_unwrapped_negative_bins_leave_the_bar():
    N = 64
    rows = peak_cases._bandlimited_rows(2048, (0.3, -1.5), (0.4, 1.9))
    psd, cross = M.welch([rows], N, 1, M.WINDOW_HANN)
    p32, c32 = psd.astype(np.float32), cross.astype(np.complex64)
    good, bar = M.align(p32, c32, *LO_HI(N))
    bad, _ = M.align(p32, c32, *LO_HI(N), wrap=False)
    assert np.any(M.align_errors(bad, good)[1:] > bar[1:])


# fp64 model against the truth on _bandlimited_rows, L = 8192, Hann, overlap 1, band +-N/10, seeds 3, 4, 5 -- measured worst errors
#   N = 64 :  delay 0.0170 samples, phase 0.00104 rad, gain 0.00999
#   N = 256:  delay 0.0214 samples, phase 0.00054 rad, gain 0.00097
# (finite averaging and the int8 quantiser, not arithmetic); allowed: twice that.
TRUTH_DELAYS, TRUTH_PHIS = (0.3, -0.4, 0.0, 2.25, -1.5, 0.05), (0.4, -1.1, 2.5, 0.0, 1.9, -2.7)
TRUTH_ALLOWED = {64: (2 * 0.0170, 2 * 0.00104, 2 * 0.00999), 256: (2 * 0.0214, 2 * 0.00054, 2 * 0.00097)}


@pytest.mark.parametrize("seed", [3, 4, 5])
@pytest.mark.parametrize("N", [64, 256])
def test_estimator_meets_known_delay_phase_and_gain(N, seed):
    rows = peak_cases._bandlimited_rows(8192, TRUTH_DELAYS, TRUTH_PHIS, seed=seed)
    psd, cross = M.welch([rows], N, 1, M.WINDOW_HANN)
    got, _ = M.align(psd.astype(np.float32), cross.astype(np.complex64), *LO_HI(N))
    truth = np.array([[0.0, 0.0, 1.0, 1.0]] + [[d, p, 1.0, 1.0] for d, p in zip(TRUTH_DELAYS, TRUTH_PHIS)])
    err = M.align_errors(got, truth)
    print(N, seed, err[:, :3].max(axis=0), got[:, 3].min())
    assert np.all(err[:, :3].max(axis=0) <= np.array(TRUTH_ALLOWED[N]))
    assert np.array_equal(got[0], [0.0, 0.0, 1.0, 1.0])


def test_zero_packet_gives_zeros():
    psd, cross = M.welch([np.zeros((3, 256), dtype=np.int8)], 16, 1, M.WINDOW_HANN)
    got, _ = M.align(psd, cross, -4, 4)
    assert not psd.any() and not cross.any() and not got.any()
