"""The fp64 statement of the adaptive beams (tests/caf_adapt_model.py) against itself: the enumeration of the training cells, the MVDR
constraint, the special cases with a known answer, the figures, the fallbacks, the scene that the device's end-to-end test runs, and
eight single mistakes, each of which must miss a bar or change the scene's outcome.  No device, no library."""
import numpy as np
import pytest

import caf_adapt_model as A
import caf_beams_model as B
import caf_bearing_model as BM


def _chi(nrows, nd, R, seed, floor=True):
    rng = np.random.default_rng(seed)
    f = np.exp(2j * np.pi * rng.random(nrows)) if floor else None
    return BM.noise_chi(nrows, nd, R, seed, floor=f)


def _w(nb, m, seed):
    rng = np.random.default_rng(seed)
    return ((rng.standard_normal((nb, m)) + 1j * rng.standard_normal((nb, m))) / np.sqrt(2 * m)).astype(np.complex64)


# m 5 with the reference in the middle, a Doppler range that wraps through nd - 1 -> 0, lags that end at R - 1, two tiles
CASE = dict(nrows=6, ref=2, nd=8, R=33, q=A.Desc(1e-2, 6, 4, 1, 32))


@pytest.fixture(scope="module")
def case():
    chi, V = _chi(CASE["nrows"], CASE["nd"], CASE["R"], 11), _w(7, CASE["nrows"] - 1, 12)
    return chi, V, A.adapt(chi, CASE["ref"], V, CASE["q"])


def test_the_covariance_against_a_cell_by_cell_enumeration(case):
    chi, _, r = case
    assert A.tiles_of(CASE["q"].N) == 2 and CASE["q"].d_lo + CASE["q"].d_n > CASE["nd"]
    Q = A.covariance_by_cells(chi, CASE["ref"], CASE["q"])
    assert np.all(np.abs(Q - r["Q"]) <= 2.0 * r["qbar"]) and np.any(Q != 0)
    assert np.allclose(r["Q"], r["Q"].conj().T, rtol=0, atol=float(np.max(r["qbar"])))


def test_the_constraint_and_the_minimum(case):
    _, V, r = case
    for b, v in enumerate(V.astype(np.complex128)):
        w, vv = r["w"][b], float(np.vdot(v, v).real)
        assert abs(np.vdot(w, v) - vv) <= r["dwn"][b] * np.sqrt(vv) + 8 * A.E64 * vv            # w^H v = v^H v
        pw, pv = float(np.vdot(w, r["Ql"] @ w).real), float(np.vdot(v, r["Ql"] @ v).real)
        assert pw <= pv * (1.0 + 1e-12) and pw > 0.0                                           # w^H Q' w <= v^H Q' v
    assert np.any(r["info"][:, 0] < 0.5 * r["info"][:, 1])                                     # (the floor is there to be nulled)


def test_an_identity_covariance_keeps_the_callers_weights():
    m, nd, R = 6, 8, 3
    chi = np.zeros((m + 1, nd, R), dtype=np.complex64)
    q = A.Desc(1e-2, 7, 2, 0, 3)                                                               # N = m = 6 cells, wrapped
    for t, (d, tau) in enumerate(A.train_cells(q, nd, R)):
        chi[1 + t, d, tau] = 0.25 * (1j) ** t                                                  # power-of-two amplitudes: Q = (1 / 96) I exactly
    V = _w(5, m, 3)
    r = A.adapt(chi, 0, V, q)
    assert np.array_equal(r["Q"], np.eye(m) / 96.0)
    aw = r["w"].astype(np.complex64)
    ulp = np.spacing(np.maximum(np.abs(V.real), np.abs(V.imag)))
    assert np.all(np.abs(aw.real - V.real) <= ulp) and np.all(np.abs(aw.imag - V.imag) <= ulp)
    assert np.all(r["wbar"] < 1e-6)


def test_a_power_of_two_scaling_of_chi_leaves_the_weights(case):
    chi, V, r = case
    for s in (2.0 ** -20, 2.0 ** 12):
        r2 = A.adapt((chi * np.float32(s)).astype(np.complex64), CASE["ref"], V, CASE["q"])
        assert np.all(np.abs(r2["w"] - r["w"]) <= r["dwn"][:, None])
        assert np.allclose(r2["info"], r["info"] * s * s, rtol=1e-9, atol=0)


def test_the_figure_is_the_mean_beam_power_over_the_training_cells(case):
    chi, V, r = case
    z, _, _ = B.beam_sums(chi, CASE["ref"], r["w"].astype(np.complex64))                       # (fp64 sums with the published weights)
    P = np.abs(z) ** 2
    for b in range(len(V)):
        mean = A.beam_mean(P[b], CASE["q"])
        assert abs(mean - r["info"][b, 0]) <= A.mean_bar(chi, CASE["ref"], r, b, CASE["q"]), b
        assert A.mean_bar(chi, CASE["ref"], r, b, CASE["q"]) < 1e-5 * r["info"][b, 0]
    zv, _, _ = B.beam_sums(chi, CASE["ref"], V)
    assert np.allclose([A.beam_mean(np.abs(zv[b]) ** 2, CASE["q"]) for b in range(len(V))], r["info"][:, 1], rtol=1e-10)


def test_the_fallbacks(case):
    chi, V, r = case
    q = CASE["q"]
    z = chi.copy()
    for d, tau in A.train_cells(q, CASE["nd"], CASE["R"]):
        z[:, d, tau] = 0
    rz = A.adapt(z, CASE["ref"], V, q)
    assert rz["status"] == A.STATUS_ZERO and np.array_equal(rz["w"], V.astype(np.complex128)) and not rz["info"].any()
    n = chi.copy()
    n[1, 7, 5] = np.nan                                                                        # inside the region
    rn = A.adapt(n, CASE["ref"], V, q)
    assert rn["status"] == A.STATUS_SOLVE and np.array_equal(rn["w"], V.astype(np.complex128)) and not rn["info"].any()
    o = chi.copy()
    o[1, 3, 5] = np.nan                                                                        # outside it (Doppler 3), and at lag 0
    o[4, 7, 0] = np.nan
    ro = A.adapt(o, CASE["ref"], V, q)
    assert ro["status"] == 0 and np.array_equal(ro["w"], r["w"])
    V0 = V.copy()
    V0[3] = 0                                                                                  # a beam that is all zero keeps it
    r0 = A.adapt(chi, CASE["ref"], V0, q)
    assert not r0["w"][3].any() and not r0["info"][3].any() and np.array_equal(r0["w"][2], r["w"][2])
    few = A.adapt(chi, CASE["ref"], V, A.Desc(1e-6, 7, 1, 4, 1))                              # N = 1 < m: the loading alone makes Q' definite
    assert few["status"] == 0 and np.all(np.isfinite(few["w"]))


@pytest.fixture(scope="module")
def scene():
    line, chi32, qa, W, echo = A.scene_line()
    return chi32, W, echo


def test_the_scene(scene):
    """the caller's lattice: no record within one cell of the echo; adaptation on: exactly one record, at the echo's cell, in the beam
    steered nearest to it; both with at least 3 dB to the threshold"""
    chi32, W, (lag, dop) = scene
    thr = 10.0 * np.log10(A.SCENE["alpha"])
    fused, nf, ln, _ = A.scene_fused(chi32, W, adaptive=False)
    assert ln["ambiguous"] == 0
    near = [f for f in fused[:nf] if abs(f[0] - lag) <= 1 and abs(f[1] - dop) <= 1]
    conv = A.scene_ratios(ln["bmap32"], (dop, lag))
    print("conventional: nfused", nf, "largest ratio near the echo %.2f dB, threshold %.2f dB" % (conv[:, 0].max(), thr))
    assert not near and conv[:, 0].max() <= thr - 3.0
    fused, nf, ln, r = A.scene_fused(chi32, W)
    assert ln["ambiguous"] == 0 and r["status"] == 0
    ad = A.scene_ratios(ln["bmap32"], (dop, lag))
    print("adaptive: nfused", nf, "beam", fused[0, 7], "ratio at the echo %.2f dB" % ad[A.SCENE["beam"], 1])
    assert nf == 1 and (fused[0, 0], fused[0, 1], fused[0, 7]) == (lag, dop, A.SCENE["beam"])
    assert ad[A.SCENE["beam"], 1] >= thr + 3.0
    # the floor stands over the noise, and the echo beneath (floor x sidelobe)
    ev = np.linalg.eigvalsh(r["Q"])
    assert ev[-1] > 1000.0 * ev[-2]


@pytest.mark.parametrize("which", A.MUTATIONS)
def test_a_single_mistake_misses_a_bar_or_changes_the_scene(which, case, scene):
    chi, V, r = case
    bad = A.adapt(chi, CASE["ref"], V, CASE["q"], which)
    misses = bool(np.any(np.abs(bad["w"].real - r["w"].real) > r["wbar"]) or np.any(np.abs(bad["w"].imag - r["w"].imag) > r["wbar"]))
    chi32, W, (lag, dop) = scene
    fused, nf, _, _ = A.scene_fused(chi32, W, which=which)
    changes = not (nf == 1 and (fused[0, 0], fused[0, 1], fused[0, 7]) == (lag, dop, A.SCENE["beam"]))
    assert misses or changes
    assert misses                                                                              # (on this case every one of them misses the weights' bar)
