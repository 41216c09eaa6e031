"""tests/doa_spectrum_model.py held to itself on the CPU: a float32 numpy restatement of the header's definition meets the model's bound
on every shape the device test runs, single mistakes do not, the maps are what their names say (a^H R a / M^2 and the beams' MVDR
power), and the two scenes the device test uses show what the maps are for: Capon resolves two sources that Bartlett merges, and its
peak values order like the sources' powers."""
import numpy as np
import pytest

import doa_beams_model as bm
import doa_spectrum_model as sm
import music_model as mm
import ura
from music_model import SCAN_CASES, case_id

LOADING = 1e-2
FAMILY_SHAPES = ((2, 1, 12, 9), (7, 3, 12, 9), (8, 8, 12, 9))          # M = 2, 21, 64


def subspace32(R):
    lam, V = mm.eigh_by_magnitude(R)
    return V.astype(np.complex64), lam.astype(np.float32)


def case_subspace(c):
    return subspace32(mm.hermitian32(mm.rxx_reference(mm.case_scene(c, L=1024)[0])))


def steering32(d, mx, my, ncx, ncy):
    """a [ncx ncy][M] as (re, im) float32, every operation a float32 one in the order of music::pmusic2d_point."""
    f = np.float32
    pi = f(3.14159274101257324)
    cx, cy = np.divmod(np.arange(ncx * ncy), ncy)
    alpha, beta = cx.astype(f) * pi / f(ncx), cy.astype(f) * pi / f(ncy)
    ca, sb, cb = np.cos(alpha), np.sin(beta), np.cos(beta)
    ix, iy = mm.element_index(mx, my)
    py = f(2.0) * pi * iy.astype(f)[None, :] * f(d) * cb[:, None]
    px = f(2.0) * pi * ix.astype(f)[None, :] * f(d) * ca[:, None] * sb[:, None]
    sx, cxv, sy, cyv = np.sin(px), np.cos(px), np.sin(py), np.cos(py)
    re, im = cxv * cyv - sx * sy, cxv * sy + sx * cyv
    assert re.dtype == np.float32 and im.dtype == np.float32
    return re, im


def map32(vec, sv, kind, loading, d, mx, my, ncx, ncy, block):
    """pm [ncx][ncy] float32: the definition in float32 without fused operations, `block` columns per pass over the elements."""
    f = np.float32
    M = mx * my
    sv = np.asarray(sv, dtype=f)
    if sv[0] == 0:
        return np.zeros((ncx, ncy), dtype=f)
    w = sm.weights(sv, kind, loading).astype(f)                          # fp64, rounded once
    ar, ai = steering32(d, mx, my, ncx, ncy)
    ur, ui = np.ascontiguousarray(vec.real, dtype=f), np.ascontiguousarray(vec.imag, dtype=f)
    S = np.zeros(ncx * ncy, dtype=f)
    for r0 in range(0, M, block):
        cols = slice(r0, min(r0 + block, M))
        yr = np.zeros((ncx * ncy, cols.stop - r0), dtype=f)
        yi = np.zeros_like(yr)
        for i in range(M):
            yr = yr + ur[i, cols][None, :] * ar[:, i, None] + ui[i, cols][None, :] * ai[:, i, None]
            yi = yi + ur[i, cols][None, :] * ai[:, i, None] - ui[i, cols][None, :] * ar[:, i, None]
        for c in range(cols.stop - r0):
            S = S + w[r0 + c] * (yr[:, c] * yr[:, c] + yi[:, c] * yi[:, c])
    assert S.dtype == f
    return (S if kind == sm.BARTLETT else f(1.0) / S).reshape(ncx, ncy)


def check32(vec, sv, d, mx, my, ncx, ncy, label):
    for name, kind in sm.KINDS.items():
        S, bound = sm.maps(vec, sv, kind, LOADING, d, mx, my, ncx, ncy)
        plain = map32(vec, sv, kind, LOADING, d, mx, my, ncx, ncy, 1)
        blocked = map32(vec, sv, kind, LOADING, d, mx, my, ncx, ncy, 4)
        assert np.array_equal(plain, blocked)                            # columns are independent sums: the blocking changes nothing
        worst, median = sm.fractions(plain, kind, S, bound)
        print(f"float32 {name} {label}: worst fraction of the bound {worst:.3f}, median relative error {median:.2e}, "
              f"worst relative bound {float((bound / S).max()):.1e}")
        assert worst <= 1.0 and np.all(plain > 0)


@pytest.mark.parametrize("c", SCAN_CASES, ids=case_id)
def test_float32_restatement_meets_the_bound_on_every_scan_shape(c):
    vec, sv = case_subspace(c)
    check32(vec, sv, ura.D, c["mx"], c["my"], c["ncx"], c["ncy"], case_id(c))


@pytest.mark.parametrize("name", mm.FAMILIES)
def test_float32_restatement_meets_the_bound_on_the_spectrum_families(name):
    for mx, my, ncx, ncy in FAMILY_SHAPES:
        vec, sv = subspace32(mm.family(mx * my, name)[0])
        check32(vec, sv, ura.D, mx, my, ncx, ncy, f"{name} {mx}x{my}")


def test_all_zero_estimate_is_a_zero_map():
    vec, sv = np.eye(4, dtype=np.complex64), np.zeros(4, dtype=np.float32)
    for kind in sm.KINDS.values():
        assert not map32(vec, sv, kind, LOADING, ura.D, 2, 2, 5, 3, 4).any()
    # the model: Bartlett's S is 0 with a bound of 0; Capon has no S there (pm = 0 is a definition, not 1 / S)
    S, bound = sm.maps(vec, sv, sm.BARTLETT, LOADING, ura.D, 2, 2, 5, 3)
    assert not S.any() and not bound.any()


# ---- single mistakes ----
def _mutant(vec, sv, c, what):
    """(kind, S as the mistaken implementation would report it, in fp64)"""
    mx, my, ncx, ncy, k = c["mx"], c["my"], c["ncx"], c["ncy"], c["k"]
    M = mx * my
    s64 = np.asarray(sv, dtype=np.float64)
    y, _ = sm.y_all(vec, ura.D, mx, my, ncx, ncy)
    p = np.abs(y) ** 2
    wb, wc = sm.weights(sv, sm.BARTLETT, LOADING), sm.weights(sv, sm.CAPON, LOADING)
    if what == "noise columns only":
        return sm.CAPON, (wc[k:] * p[:, :, k:]).sum(axis=2)
    if what == "weights reversed":
        return sm.BARTLETT, (wb[::-1] * p).sum(axis=2)
    if what == "loading from the smallest value":
        return sm.CAPON, ((1.0 / (s64 + float(np.float32(LOADING)) * s64[-1])) * p).sum(axis=2)
    if what == "no 1/M^2":
        return sm.BARTLETT, (wb * M * M * p).sum(axis=2)
    if what == "conjugate lost":
        # sum_i vec[i][r] a[i].  (The conjugate on a instead of on vec is no mistake: it conjugates y_r, and only |y_r| is used.)
        y2, _ = sm.y_all(np.asarray(vec).conj(), ura.D, mx, my, ncx, ncy)
        return sm.BARTLETT, (wb * np.abs(y2) ** 2).sum(axis=2)
    if what == "element order":
        y2, _ = sm.y_all(vec, ura.D, mx, my, ncx, ncy, order="col")
        return sm.CAPON, (wc * np.abs(y2) ** 2).sum(axis=2)
    if what == "Capon not inverted":
        # pm = S is returned; the comparison takes 1 / pm for the S it stands for
        return sm.CAPON, 1.0 / (wc * p).sum(axis=2)
    raise ValueError(what)


MUTANTS = ("noise columns only", "weights reversed", "loading from the smallest value", "no 1/M^2", "conjugate lost", "element order",
           "Capon not inverted")


@pytest.fixture(scope="module")
def subspaces():
    return [(c, *case_subspace(c)) for c in SCAN_CASES]


@pytest.mark.parametrize("what", MUTANTS)
def test_single_mistakes_exceed_the_bound(subspaces, what):
    caught = []
    for c, vec, sv in subspaces:
        kind, wrong = _mutant(vec, sv, c, what)
        S, bound = sm.maps(vec, sv, kind, LOADING, ura.D, c["mx"], c["my"], c["ncx"], c["ncy"])
        if (np.abs(wrong - S) / bound).max() > 1.0:
            caught.append(case_id(c))
    print(f"{what}: outside the bound on {len(caught)} of {len(SCAN_CASES)} shapes")
    assert caught


# ---- what the maps are ----
@pytest.mark.parametrize("c", [SCAN_CASES[2], SCAN_CASES[3], SCAN_CASES[8]], ids=case_id)
def test_identities(c):
    mx, my, ncx, ncy = c["mx"], c["my"], c["ncx"], c["ncy"]
    M = mx * my
    vec, sv = case_subspace(c)
    V, s = vec.astype(np.complex128), sv.astype(np.float64)
    R = (V * s[None, :]) @ V.conj().T
    Sb, _ = sm.maps(vec, sv, sm.BARTLETT, LOADING, ura.D, mx, my, ncx, ncy)
    Sc, _ = sm.maps(vec, sv, sm.CAPON, LOADING, ura.D, mx, my, ncx, ncy)
    rng = np.random.default_rng(0)
    for cx, cy in zip(rng.integers(0, ncx, 8), rng.integers(0, ncy, 8)):
        a = bm.steering(*bm.grid_angles(cx, cy, ncx, ncy), ura.D, mx, my)
        assert np.isclose(Sb[cx, cy] * M * M, np.vdot(a, R @ a).real, rtol=1e-10)
        assert np.isclose(Sb[cx, cy], bm.weights(vec, sv, a, bm.CONVENTIONAL)[1], rtol=1e-10)
        assert np.isclose(1.0 / Sc[cx, cy], bm.weights(vec, sv, a, bm.MVDR, LOADING)[1], rtol=1e-10)


# ---- what they are for ----
def test_capon_resolves_what_bartlett_merges():
    vec, sv = subspace32(mm.hermitian32(mm.rxx_reference(sm.resolution_block())))
    margins = {}
    for name, kind in sm.KINDS.items():
        S, bound = sm.maps(vec, sv, kind, sm.RES_LOADING, ura.D, ura.MX, ura.MY, 100, 100)
        certain, possible, margins[name] = sm.local_peaks_within_bound(S, bound, kind, sm.RES_RADIUS, sm.RES_REGION)
        assert certain == possible                                       # no point of the region is left to the rounding
        assert certain == ([(50, 50)] if kind == sm.BARTLETT else sorted(sm.RES_PEAKS))
        assert sm.region_peaks(sm.power(S, kind)) == certain
    print(f"resolution scene: every comparison that decides a local maximum in the region is at least {margins['bartlett']:.0f} "
          f"(Bartlett) and {margins['capon']:.0f} (Capon) times the bound")
    # measured when the scene was chosen: 93 and 402 bounds; a tenth of that is asked for
    assert margins["bartlett"] >= 9 and margins["capon"] >= 40


def test_capon_peak_values_order_like_the_source_powers():
    # a statement of the fp64 model on the quantised scene: no statistics in it
    vec, sv = subspace32(mm.hermitian32(mm.rxx_reference(sm.power_block())))
    S, bound = sm.maps(vec, sv, sm.CAPON, LOADING, ura.D, ura.MX, ura.MY, 100, 100)
    pm = sm.power(S, sm.CAPON)
    weak, strong = sm.POW_PEAKS
    top = sorted(sm.region_peaks(pm, 2, (slice(0, 100), slice(0, 100))), key=lambda p: -pm[p])[:2]
    assert top == [strong, weak]                                         # the two largest local maxima of the whole map are the sources
    # every map within the bound: the least the strong source's peak can be is above the most the weak one's can be
    assert 1.0 / (S[strong] + bound[strong]) > 1.0 / (S[weak] - bound[weak])
    # the sources' own powers in the map's unit, ((I + jQ) / 127)^2: sigma_s = 25 times the amplitude
    own = [(25.0 * a / 127.0) ** 2 for a in sm.POW_AMPS]
    print(f"Capon at the sources: {pm[weak]:.4f} and {pm[strong]:.4f}, the sources' powers {own[0]:.4f} and {own[1]:.4f}")
