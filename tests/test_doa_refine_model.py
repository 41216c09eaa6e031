"""CPU checks of the zoom search's definition (tests/doa_refine_model.py, plain fp64 numpy): on the three scenes of the issue, one emitter
off the grid, the refined direction is at most a fifth of the grid peak's distance from the true cell (measured: 1/17 at worst, so a
fifth is a condition, not a tolerance), and every scene has exactly one reachable final point, which is what makes them fit for the
device's comparison.

Measured and printed, on all nine cases: with vec and sv rounded to fp32 the result moves by 0 lattice steps, and a search on a 3 x 3
or 5 x 5 lattice that halves its spacing (nine levels to the same last lattice) ends on the same point as the definition's 7 x 7
lattice that quarters it: 0 steps.  The assertion is one step: every such search ends on the last lattice's point next to the map's
maximum, and two of them can differ by one where the maximum lies between two points."""
import numpy as np
import pytest

import doa_refine_model as rm

CASES = [(sc, off) for sc in rm.SCENES for off in rm.OFFSETS]
S_LAST = 2.0 ** -(2 * rm.LEVELS - 1)


@pytest.fixture(scope="module")
def solved():
    out = {}
    for sc, off in CASES:
        sv, vec = rm.fp64_subspace(rm.scene_block(sc, off))
        args = (vec, sv, rm.MUSIC, 1, 0.0, sc["d"], sc["mx"], sc["my"], sc["nc"], sc["nc"])
        peak = rm.grid_peak(*args)
        out[rm.scene_id(sc, off)] = (args, peak, rm.refine(*args, peak, rm.LEVELS))
    return out


@pytest.mark.parametrize("sc,off", CASES, ids=[rm.scene_id(*c) for c in CASES])
def test_refined_direction_is_five_times_closer_and_unique(solved, sc, off):
    args, peak, (o, angles, f) = solved[rm.scene_id(sc, off)]
    tx, ty = rm.true_cell(sc, off)
    grid = np.hypot(peak[0] - tx, peak[1] - ty)
    fine = np.hypot(peak[0] + o[0] - tx, peak[1] + o[1] - ty)
    print(f"{rm.scene_id(sc, off)}: grid peak {peak} {grid:.3f} cells off, refined {fine:.4f} cells off (1/{grid / fine:.0f})")
    assert fine <= grid / 5.0
    assert all(abs(v) < 2 and (v / S_LAST) == round(v / S_LAST) for v in o)
    assert np.allclose(angles, ((peak[0] + o[0]) * np.pi / sc["nc"], (peak[1] + o[1]) * np.pi / sc["nc"]), rtol=0, atol=1e-15)
    q, tol, f1 = rm.f_at(*args, peak[0] + o[0], peak[1] + o[1])
    assert abs(rm.q_of(f, rm.MUSIC, sc["mx"] * sc["my"]) - q) <= tol and abs(f - f1) <= 1e-9 * f1      # (numpy sums 49 points and one in different orders)
    assert rm.branches(*args, peak, rm.LEVELS) == {o}


@pytest.mark.parametrize("sc,off", CASES, ids=[rm.scene_id(*c) for c in CASES])
def test_definition_is_not_fragile(solved, sc, off):
    args, peak, (o, _, _) = solved[rm.scene_id(sc, off)]
    steps = lambda other: max(abs(u - v) for u, v in zip(other, o)) / S_LAST
    o32 = rm.refine(args[0].astype(np.complex64), args[1].astype(np.float32), *args[2:], peak, rm.LEVELS)[0]
    o3 = rm.refine(*args, peak, 2 * rm.LEVELS - 1, side=3, shrink=2.0)[0]
    o5 = rm.refine(*args, peak, 2 * rm.LEVELS - 1, side=5, shrink=2.0)[0]
    print(f"{rm.scene_id(sc, off)}: fp32 vec moves the result by {steps(o32):g} steps, a 3 x 3 halving lattice by {steps(o3):g}, 5 x 5 by {steps(o5):g}")
    assert steps(o32) <= 1 and steps(o3) <= 1 and steps(o5) <= 1


def test_search_rules():
    """the centre keeps ties, a zero estimate stays where it is, the lattice is clamped to the grid's range"""
    m = 6
    vec, sv = np.eye(m, dtype=np.complex64), np.zeros(m, dtype=np.float32)
    o, angles, f = rm.refine(vec, sv, rm.BARTLETT, 1, 0.0, 0.5, 3, 2, 10, 7, (3, 4), 5)
    assert o == (0.0, 0.0) and f == 0.0 and np.allclose(angles, (3 * np.pi / 10, 4 * np.pi / 7))
    # a flat map (the identity's Bartlett map with equal values is sum |a_i|^2 / M = 1 everywhere, up to rounding)
    sv = np.ones(m, dtype=np.float32)
    assert (0.0, 0.0) in rm.branches(vec, sv, rm.BARTLETT, 1, 0.0, 0.5, 3, 2, 10, 7, (3, 4), 2)
    px, py = rm.lattice(0.0, 7.0, 0.5, 10, 7)
    assert px.min() == 0.0 and py.max() == 7.0 and len(px) == 49 and (px[24], py[24]) == (0.0, 7.0)
