"""The fp64 restatement of the beamformer chain (tests/music_model.py) must pass its own bars before the device is held to them: the C
oracle (oracle/beamformer_oracle.c: two-sided Jacobi in fp64, the scan in fp32 in the reference's expression order) is an independent
implementation of the same arithmetic classes, so it has to sit inside every bar, and wrong implementations of the scan (the mutants
below) have to fall outside.  CPU only."""
import numpy as np
import pytest

import music_model as mm
from music_model import SCAN_CASES, case_id

SUBSPACE_M = list(range(2, 65))


# ---- constructors ------------------------------------------------------------------------------------------------------------------

def test_rxx_reference_is_the_definition_and_stacks_frames():
    rng = np.random.default_rng(1)
    blocks = rng.integers(-128, 128, size=(3, 6, 64), dtype=np.int8)
    rows = np.concatenate(list(blocks), axis=1)
    x = rows[1:].astype(np.float64) / 127.0
    X = (x[:, 0::2] + 1j * x[:, 1::2]).T
    X = X - X.mean(axis=0, keepdims=True)
    R = X.conj().T @ X / X.shape[0]                                      # heatmap2d2.cpp:185-199 as written, L = F B / 2 = 96
    assert X.shape[0] == 3 * 64 // 2
    got = mm.rxx_reference_frames(blocks)
    assert got.dtype == np.complex64 and np.array_equal(got, mm.rxx_reference(rows))
    assert np.abs(got - R).max() <= 2e-7 * np.abs(R).max()
    assert np.array_equal(got, got.conj().T)
    # full-scale rows at the length where the int32 sums of a kernel reach 2^30: the reference itself stays exact
    rows = np.zeros((3, 65536), dtype=np.int8)
    rows[1] = -128
    rows[2, 0::2], rows[2, 1::2] = 127, -128
    ref = mm.rxx_reference(rows)
    assert np.all(ref == 0)                                              # constant rows: the covariance of a DC signal is zero, exactly


def test_hermitian32_and_families():
    rng = np.random.default_rng(2)
    z = rng.standard_normal((5, 5)) + 1j * rng.standard_normal((5, 5))
    H = mm.hermitian32(z)
    assert H.dtype == np.complex64 and np.array_equal(H, H.conj().T) and np.all(H.diagonal().imag == 0)
    assert np.array_equal(np.triu(H), np.triu(z.astype(np.complex64), 1) + np.diag(z.diagonal().real.astype(np.float32)))
    for m in (2, 3, 4, 21, 64):
        for name in mm.FAMILIES:
            R, gaps = mm.family(m, name)
            assert R.shape == (m, m) and np.array_equal(R, R.conj().T)
            lam, _ = mm.eigh_by_magnitude(R)
            assert all(0 < k < m and lam[k - 1] - lam[k] > 0.4 * lam[k - 1] for k in gaps), (m, name, gaps)
    lam, _ = mm.eigh_by_magnitude(mm.family(64, "stairs")[0])
    assert np.allclose(lam[:16], 1e3, rtol=1e-5) and np.allclose(lam[16:32], 10, rtol=1e-3) and np.allclose(lam[32:], 1e-2, atol=1e-3)
    assert mm.family(64, "stairs")[1] == [16, 32] and mm.family(64, "clustered")[1] == [1, 2] and mm.family(64, "rank3")[1] == [3]


# ---- subspace bars -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", mm.FAMILIES)
def test_oracle_subspace_meets_the_bars(oracle, name):
    worst = {}
    for m in SUBSPACE_M:
        R, gaps = mm.family(m, name)
        vec, sv = oracle.noisesubspace(R)
        fr = mm.subspace_fractions(R, vec, sv, gaps)
        for key, v in fr.items():
            assert v <= 1.0, (name, m, key, v)
            worst[key] = max(worst.get(key, 0.0), v)
    print(f"oracle subspace, {name}: worst fraction of the bar " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))


def test_subspace_bars_catch_wrong_subspaces():
    # the bars are not vacuous: an eigenvector perturbed by 1e-6, vectors in the wrong order and a projector cut at the wrong column
    # all fail at least one of them
    R, gaps = mm.family(21, "clustered")
    lam, E = mm.eigh_by_magnitude(R)
    good = mm.subspace_fractions(R, E.astype(np.complex64), lam.astype(np.float32), gaps)
    assert max(good.values()) <= 1.0, good
    bad = E.copy()
    bad[:, 1] += 1e-6 * E[:, 5]
    assert max(mm.subspace_fractions(R, bad.astype(np.complex64), lam.astype(np.float32), gaps).values()) > 1.0
    swapped = E[:, [1, 0] + list(range(2, 21))]
    fr = mm.subspace_fractions(R, swapped.astype(np.complex64), lam.astype(np.float32), gaps)
    assert fr["resid"] > 1.0 and fr["proj"] > 1.0
    assert mm.sv_fraction(lam * (1 + 3e-7), lam) > 1.0


# ---- scan --------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def scans(oracle):
    """Per case: the oracle's subspace of the scene's exact covariance, the fp64 scan of it and its bound -- computed once."""
    out = {}
    for c in SCAN_CASES:
        R = mm.hermitian32(mm.rxx_reference(mm.case_scene(c)[0]))
        vec, _ = oracle.noisesubspace(R)
        den, bound = mm.scan(vec, c["k"], _d(), c["mx"], c["my"], c["ncx"], c["ncy"])
        out[case_id(c)] = (vec, den, bound)
    return out


def _d():
    import ura
    return ura.D


@pytest.mark.parametrize("c", SCAN_CASES, ids=case_id)
def test_oracle_scan_is_inside_the_bound_and_the_model_finds_the_sources(oracle, scans, c):
    vec, den, bound = scans[case_id(c)]
    m = c["mx"] * c["my"]
    assert den.shape == bound.shape == (c["ncx"], c["ncy"]) and np.all(bound > 0) and np.all(den > 0)
    pm = oracle.pmusic2d(vec, c["k"], _d(), c["mx"], c["my"], c["ncx"], c["ncy"])
    worst, median = mm.scan_fractions(pm, m, den, bound)
    print(f"oracle scan {case_id(c)}: worst fraction of the bound {worst:.3f}, median |d den| / den {median:.2e}")
    assert worst <= 1.0
    peak = np.unravel_index(np.argmax(pm), pm.shape)
    assert mm.admissible_peak(den, bound, peak)
    if c["flat"]:
        assert np.ptp(den) <= 1e-9 * den.max()                           # one steering vector on the whole grid
        return
    for p in c["src"]:
        assert den[p] <= 1e-2 * np.median(den), (p, den[p], np.median(den))   # sharp: pm there is 1e4 times the median at least
    if c["find"]:
        assert tuple(int(v) for v in np.unravel_index(np.argmin(den), den.shape)) in c["src"]


def test_admissible_peak_tolerates_ties_and_refuses_a_wrong_point():
    den = np.array([[1.0, 1e-3, 2.0], [1.0, 1e-3 + 1e-9, 2.0]])
    bound = np.full_like(den, 1e-6)
    assert mm.admissible_peak(den, bound, (0, 1)) and mm.admissible_peak(den, bound, (1, 1))
    assert not mm.admissible_peak(den, bound, (0, 0))
    assert mm.certain_peak(den, bound) is None
    assert mm.certain_peak(den, np.full_like(den, 1e-10)) == (0, 1)
    assert mm.den_of(np.array([np.inf, 4.0]), 2).tolist() == [0.0, 1.0]


# the places where a scan can be wrong with every kernel-against-kernel test passing
MUTANTS = {
    "index order ix*My + iy": dict(order="col"),
    "Cx / Cy swapped in the grid decomposition": dict(swap=True),
    "col0 = k + 1": dict(dcol=+1),
    "col0 = k - 1": dict(dcol=-1),
    "sign of the iy term": dict(sign_y=-1.0),
}


def _mutant_fraction(c, vec, den, bound, factor, order="row", swap=False, dcol=0, sign_y=1.0):
    k, mx, my, ncx, ncy = c["k"], c["mx"], c["my"], c["ncx"], c["ncy"]
    if swap:
        y, _ = mm._y(vec, k, _d(), mx, my, ncy, ncx)
        wrong = (np.abs(y) ** 2).sum(axis=2).reshape(-1).reshape(ncx, ncy)
    else:
        y, _ = mm._y(vec, k, _d(), mx, my, ncx, ncy, order=order, col0=k + dcol, sign_y=sign_y)
        wrong = (np.abs(y) ** 2).sum(axis=2)
    return float(np.mean(np.abs(wrong - den) > factor * bound))


@pytest.mark.parametrize("name", MUTANTS)
def test_every_mutant_is_caught_by_a_case(scans, name):
    fractions = {}
    for c in SCAN_CASES:
        vec, den, bound = scans[case_id(c)]
        fractions[case_id(c)] = _mutant_fraction(c, vec, den, bound, 1.0, **MUTANTS[name])
    print(f"mutant '{name}': fraction of grid points outside the bound per case: " + ", ".join(f"{k} {v:.2f}" for k, v in fractions.items()))
    assert max(fractions.values()) > 0.5


def test_every_case_is_discriminating(scans):
    # a case on which no mutant leaves the bound at more than half the points would check nothing about the scan's structure
    for c in SCAN_CASES:
        vec, den, bound = scans[case_id(c)]
        best = max(_mutant_fraction(c, vec, den, bound, 1.0, **kw) for kw in MUTANTS.values())
        assert best > 0.5, (case_id(c), best)


def test_structure_mutants_are_caught_wherever_the_shape_can_show_them(scans):
    # the index order at twice the bound on every array that is two-dimensional and not square; the grid swap on every grid that is
    # not square under an array that resolves both angles (the case table has both kinds at several sizes).  More than half the points
    # each; 0.4 where the noise subspace is the complement of a single vector of 64 (den = m - |u_0^H a|^2 only moves where the beam of
    # u_0 is, about half the grid)
    seen = [0, 0]
    for c in SCAN_CASES:
        vec, den, bound = scans[case_id(c)]
        if min(c["mx"], c["my"]) > 1 and c["mx"] != c["my"] and not c["flat"]:
            f = _mutant_fraction(c, vec, den, bound, 2.0, order="col")
            print(f"index order, {case_id(c)}: {f:.2f} of the points beyond twice the bound")
            assert f > 0.5, case_id(c)
            seen[0] += 1
        if min(c["mx"], c["my"]) > 1 and min(c["ncx"], c["ncy"]) > 1 and c["ncx"] != c["ncy"]:
            f = _mutant_fraction(c, vec, den, bound, 1.0, swap=True)
            print(f"grid swap, {case_id(c)}: {f:.2f} of the points beyond the bound")
            assert f > (0.4 if (c["k"], c["mx"] * c["my"]) == (1, 64) else 0.5), case_id(c)
            seen[1] += 1
    assert seen[0] >= 5 and seen[1] >= 7, seen
