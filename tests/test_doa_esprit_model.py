"""CPU checks of the 2-D ESPRIT model (tests/doa_esprit_model.py, whose docstring states the definition and the two bars): on
tests/ura.py scenes at every (sx, sy, k) the GPU tests run, its two fp64 routes agree within BAR, a complex64 run misses BAR, the
estimated directions lie within one cell of a 100 x 100 grid of the mirrored true ones on arrays >= 7 x 3, and every single planted
mistake misses both bars."""
import numpy as np
import pytest

import doa_esprit_model as em


def _subspace(sx, sy, k, directions=None):
    block, dirs = em.shape_scene(sx, sy, k, directions=directions)
    vec, sv = em.fp64_subspace(block)
    return vec, sv, dirs, em.shape_d(sx, sy)


@pytest.fixture(scope="module")
def results():
    """shape -> (vec, sv, dirs, d, eig route, qr route): computed once"""
    out = {}
    for sx, sy, k in em.SHAPES:
        vec, sv, dirs, d = _subspace(sx, sy, k)
        out[(sx, sy, k)] = (vec, sv, dirs, d, em.esprit(vec, sv, k, d, sx, sy), em.esprit(vec, sv, k, d, sx, sy, route="qr"))
    return out


def pair_error(got, want):
    """largest distance from a wanted (mu, nu) pair to the nearest pair got"""
    def dist(p, q):
        return max(abs((p[i] - q[i] + np.pi) % (2 * np.pi) - np.pi) for i in range(2))
    return max(min(dist(g, w) for g in got) for w in want)


@pytest.mark.parametrize("shape", em.SHAPES, ids=[f"{s[0]}x{s[1]}-k{s[2]}" for s in em.SHAPES])
def test_routes_agree_and_directions_are_found(results, shape):
    sx, sy, k = shape
    vec, sv, dirs, d, a, q = results[shape]
    print(f"{sx}x{sy} k={k}: cond(Gx) {a['cond_gx']:.2f} cond(Gy) {a['cond_gy']:.2f} cond(V) {a['cond_v']:.2f} gap {a['gap']:.3f} QR steps {q['steps']}")
    assert a["found"] == k and q["found"] == k and a["status"] == 0 and q["status"] == 0
    assert q["steps"] <= 40 * k
    err = em.phase_error(a["phases"], q["phases"])
    print(f"  routes differ by {err:.2e} rad")
    # outside the conditioning the bar is stated for, both routes lose digits in proportion
    worst = max(a["cond_gx"], a["cond_gy"], a["cond_v"])
    assert err <= em.BAR * (1.0 if em.well_conditioned(a) else worst / 4.0), err
    for key in ("angles", "modulus", "power"):
        ulp = np.spacing(np.abs(a[key]))
        assert np.all(np.abs(a[key].astype(np.float64) - q[key].astype(np.float64)) <= 4 * ulp), key
    assert np.array_equal(a["flags"], q["flags"]) and not a["flags"].any()
    # slot order: descending power, then ascending mu, then nu
    keys = [(-float(p), float(m), float(n)) for p, (m, n) in zip(a["power"], a["phases"])]
    assert keys == sorted(keys)
    # the scan's convention: the phases of the directions are those the scenes were built from
    want = [em.phases_of(al, be, d) for al, be in dirs]
    if sx >= 7 and sy >= 3:
        derr = em.match_error(a["angles"], dirs)
        print(f"  directions within {derr:.2e} rad")
        assert derr <= em.DIRECTION_BAR, derr
        assert pair_error(a["phases"], want) <= 2 * np.pi * d * em.DIRECTION_BAR * 2
        assert np.all(np.abs(a["modulus"] - 1) < 0.05)


def test_most_scenes_meet_the_bars_conditions(results):
    good = [s for s in em.SHAPES if em.well_conditioned(results[s][4])]
    assert len(good) >= 8 and (8, 8, 16) in good and (2, 2, 1) in good, good


@pytest.mark.parametrize("shape", em.SHAPES, ids=[f"{s[0]}x{s[1]}-k{s[2]}" for s in em.SHAPES])
def test_complex64_misses_the_bar(results, shape):
    sx, sy, k = shape
    vec, sv, dirs, d, a, _ = results[shape]
    for route in ("eig", "qr"):
        c = em.esprit(vec, sv, k, d, sx, sy, route=route, dtype=np.complex64)
        err = pair_error(c["phases"][:k], a["phases"][:k])
        print(f"{sx}x{sy} k={k} {route}: complex64 errs by {err:.2e} rad")
        assert err > em.BAR, (route, err)


@pytest.mark.parametrize("which", ["mu", "nu"])
def test_sources_sharing_a_phase(which):
    """two sources with the same mu, and two with the same nu: gamma pairs them; with gamma = 0 the shared-mu scene loses its nu"""
    sx, sy, k = 7, 3, 2
    vec, sv, dirs, d = _subspace(sx, sy, k, directions=em.shared_directions(which))
    a, q = em.esprit(vec, sv, k, d, sx, sy), em.esprit(vec, sv, k, d, sx, sy, route="qr")
    ph = a["phases"]
    assert abs(ph[0, 0 if which == "mu" else 1] - ph[1, 0 if which == "mu" else 1]) < 0.01
    assert em.match_error(a["angles"], dirs) <= em.DIRECTION_BAR and em.match_error(q["angles"], dirs) <= em.DIRECTION_BAR
    assert em.phase_error(a["phases"], q["phases"]) <= em.BAR
    if which == "mu":
        bad = em.esprit(vec, sv, k, d, sx, sy, mistake="gamma_zero")
        assert em.match_error(bad["angles"], dirs) > em.DIRECTION_BAR and pair_error(bad["phases"], ph) > em.BAR


@pytest.mark.parametrize("mistake", [m for m in em.MISTAKES if m != "gamma_zero"])
def test_single_mistakes_miss_the_bars(results, mistake):
    # five sources, where Gx is far from a multiple of the identity; three that are not their own mirror image for the others
    sx, sy, k = (7, 3, 5) if mistake == "no_inverse" else (7, 3, 3)
    vec, sv, dirs, d, a, _ = results[(sx, sy, k)]
    assert em.match_error(a["angles"], dirs) <= em.DIRECTION_BAR
    for route in ("eig", "qr"):
        bad = em.esprit(vec, sv, k, d, sx, sy, route=route, mistake=mistake)
        derr, perr = em.match_error(bad["angles"], dirs), pair_error(bad["phases"][:k], a["phases"][:k])
        print(f"{mistake} ({route}): directions off by {derr:.3f} rad, phases by {perr:.3f}")
        assert derr > em.DIRECTION_BAR and perr > em.BAR, (mistake, route, derr, perr)


def test_empty_results():
    sx, sy, k = 3, 2, 3
    zero = em.esprit(np.zeros((6, 6)), np.zeros(6), 2, 0.5, sx, sy, slots=3)
    assert zero["found"] == 0 and zero["status"] == 0 and not zero["phases"].any() and np.all(zero["angles"] == -1) and np.all(zero["modulus"] == -1)
    assert np.all(zero["power"] == -1) and not zero["flags"].any()
    # the identity: column 2 is the element (ix = 2, iy = 0), which E1x drops: Gx has an empty column
    for route in ("eig", "qr"):
        flat = em.esprit(np.eye(6), np.ones(6), k, 0.5, sx, sy, route=route)
        assert flat["found"] == 0 and flat["status"] == 2 and np.all(flat["power"] == -1)
    assert em.rank_limit(3, 2) == 3 and em.rank_limit(2, 2) == 2 and em.rank_limit(8, 8) == 16 and em.rank_limit(7, 3) == 14
