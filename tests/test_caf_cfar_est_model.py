"""The fp64 statement of the greatest-of, smallest-of and ordered-statistic CFAR estimators (tests/caf_cfar_est_model.py) held to the
letter of their definition, on the two scenes that motivate them, against a simulation of the false-alarm rate, and against the
mistakes of MUTATIONS: each must change a detection or miss a bar in some case here.  CPU only."""
import numpy as np
import pytest

import caf_cfar_est_model as E
import caf_cfar_model as C
import caf_model as M

SEED = 7                                                                         # the scenes' floor: default_rng(7).exponential(1.0, (32, 96))
ND, R = 32, 96
ESTS = {"ca": (E.Est(E.CA), 90), "go": (E.Est(E.GO, E.LAG), 42), "so": (E.Est(E.SO, E.LAG), 42), "os": (E.Est(E.OS, 0, 67), 90)}


def _floor():
    return np.random.default_rng(SEED).exponential(1.0, size=(ND, R))


def _scene_params(name, pfa=1e-5):
    est, n = ESTS[name]
    return C.Params(E.cfar_alpha_est(pfa, n, est), 1, 1, 3, 4, max_det=16), est


def _clean(r):
    assert r["ambiguous"] == 0 and r["half_ambiguous"] == 0, (r["ambiguous"], r["half_ambiguous"])
    return r


@pytest.mark.parametrize("guard", [0, 2])
@pytest.mark.parametrize("win", [(1, 1, 2, 3), (0, 0, 1, 2), (2, 0, 1, 0), (0, 3, 0, 2)])
def test_every_cell_against_the_enumeration_by_the_letter(win, guard):
    nd, r = 16, 11
    P = np.random.default_rng(100 + guard).exponential(1.0, size=(nd, r))
    P[3, 4] = P[3, 5] = 0.0                                                      # true zeros take part
    prm = C.Params(5.0, *win)
    Nfull = E.full_count(prm)
    ranks = sorted({1, Nfull // 2 + 1, Nfull})
    os_all = {rank: E.os_values(P, guard, prm, rank) for rank in ranks}
    for axis in (E.LAG, E.DOPPLER):
        zlo, nlo, zhi, nhi = E.half_sums(P, guard, prm, axis)
        for d in range(nd):
            for tau in range(r):
                (wl, cl), (wh, ch) = E.half_cell(P, guard, prm, axis, d, tau)
                if abs(M.signed_bins(nd)[d]) < guard:
                    continue
                assert (nlo[d, tau], nhi[d, tau]) == (cl, ch), (axis, d, tau)
                assert abs(zlo[d, tau] - wl) <= 2 * max(cl, 1) * E.E64 * wl and abs(zhi[d, tau] - wh) <= 2 * max(ch, 1) * E.E64 * wh
                total = C.train_cell(P, guard, prm, d, tau)[1]
                centre = sum(1 for a in range(-prm.Hd, prm.Hd + 1) for b in range(-prm.Hr, prm.Hr + 1)
                             if (b if axis == E.LAG else a) == 0 and not (abs(a) <= prm.gd and abs(b) <= prm.gr) and 0 <= tau + b < r
                             and abs(M.signed_bins(nd)[(d + a) % nd]) >= guard)
                assert cl + ch + centre == total
    for rank, (noise, N) in os_all.items():
        for d in range(nd):
            if abs(M.signed_bins(nd)[d]) < guard:
                continue
            for tau in range(r):
                x, n, k = E.os_cell(P, guard, prm, rank, d, tau)
                assert N[d, tau] == n and (n == 0 or noise[d, tau] == x), (rank, d, tau)
                assert n == 0 or (1 <= k <= n and (rank < Nfull or k == n) and (rank > 1 or k == 1))


def test_os_rank_is_the_integer_ceiling():
    for Nfull in (1, 7, 90, 560):
        for N in (1, Nfull // 3 + 1, Nfull):
            for rank in (1, Nfull // 2 + 1, Nfull):
                want = max(1, int(np.ceil(np.float64(rank * N) / Nfull - 1e-12)))
                assert E.os_rank(rank, N, Nfull) == want and 1 <= E.os_rank(rank, N, Nfull) <= N


def test_the_masking_scene():
    """(10, 44) = 80 stands 19 dB over the floor four lags from (10, 40) = 3000: the mean of all cells, and the greater half, hide it"""
    P = _floor()
    P[10, 40], P[10, 44], P[20, 70] = 3000.0, 80.0, 60.0
    three, two = [10 * R + 40, 10 * R + 44, 20 * R + 70], [10 * R + 40, 20 * R + 70]
    for name, cells in (("ca", two), ("go", two), ("os", three), ("so", three)):
        prm, est = _scene_params(name)
        r = _clean(E.detect(P, 0, prm, est))
        assert r["count"] == len(cells) and sorted(r["cells"]) == cells, (name, r["cells"])
    prm, est = _scene_params("so")
    k = E.detect(P, 0, prm, est)["cells"].index(10 * R + 44)
    assert E.detect(P, 0, prm, est)["det"][k][7] == 42                           # the half away from the interferer, whole


def test_the_edge_scene():
    """the lags from 48 on raised 30 times over a pure-noise floor: nothing is there to detect"""
    P = _floor()
    P[:, 48:] *= 30.0
    for name in ("ca", "go"):
        prm, est = _scene_params(name)
        assert _clean(E.detect(P, 0, prm, est))["count"] == 0, name
    prm, est = _scene_params("so")
    r = _clean(E.detect(P, 0, prm, est))
    assert r["count"] >= 1 and all(48 <= c % R <= 52 for c in r["cells"]), r["cells"]      # (the low half still sees the floor below the step)


def test_go_over_doppler_next_to_the_ridge():
    """guard 3 cuts bins -2 .. 2 out: at bin 3 the lower Doppler half holds bins 1 .. 2 of S only -- none -- and at bin 5 two rows of seven lags"""
    guard, prm, est = 3, C.Params(6.0, 0, 1, 3, 2, max_det=8), E.Est(E.GO, E.DOPPLER)
    P = np.random.default_rng(11).exponential(1.0, size=(ND, 24))
    P[3, 10], P[ND - 5, 6] = 90.0, 70.0
    zlo, nlo, zhi, nhi = E.half_sums(P, guard, prm, E.DOPPLER)
    assert nlo[3, 10] == 0 and nhi[3, 10] == 21 and nlo[5, 10] == 14 and nhi[ND - 3, 10] == 0 and nhi[ND - 5, 6] == 14
    r = _clean(E.detect(P, guard, prm, est))
    assert r["cells"][:2] == [3 * 24 + 10, (ND - 5) * 24 + 6]
    assert r["det"][0][7] == 21 and r["det"][0][1] == 3 and r["det"][1][1] == -5
    # the ridge itself trains nothing: raising it changes no figure
    P2 = P.copy()
    P2[:3], P2[ND - 2:] = 1e6, 1e6
    assert np.array_equal(E.detect(P2, guard, prm, est)["det"], r["det"])


@pytest.mark.parametrize("name", ["os", "go", "so", "ca"])
def test_alpha_against_a_seeded_simulation(name):
    """pfa = 1e-2, M draws: the number of false alarms is binomial(M, pfa) if alpha is right, of standard deviation sqrt(M pfa (1 - pfa)):
    five of them is a bar that a right alpha misses with probability below 1e-6, and a pfa off by 12 % does not pass at M = 200 000"""
    pfa, draws, chunk = 1e-2, 200_000, 25_000
    est, n = {"os": (E.Est(E.OS, 0, 18), 24), "go": (E.Est(E.GO), 12), "so": (E.Est(E.SO), 12), "ca": (E.Est(E.CA), 24)}[name]
    alpha = np.float64(E.cfar_alpha_est(pfa, n, est))
    rng, hits = np.random.default_rng(2024), 0
    for _ in range(draws // chunk):
        x = rng.exponential(1.0, size=chunk)
        if name in ("go", "so"):
            lo, hi = rng.exponential(1.0, size=(chunk, n)).mean(axis=1), rng.exponential(1.0, size=(chunk, n)).mean(axis=1)
            noise = np.maximum(lo, hi) if name == "go" else np.minimum(lo, hi)
        elif name == "os":
            noise = np.sort(rng.exponential(1.0, size=(chunk, n)), axis=1)[:, est.rank - 1]
        else:
            noise = rng.exponential(1.0, size=(chunk, n)).mean(axis=1)
        hits += int(np.sum(x > alpha * noise))
    print(name, float(alpha), hits / draws)
    assert abs(hits - draws * pfa) <= 5.0 * np.sqrt(draws * pfa * (1.0 - pfa)), (name, hits)


def test_alpha_limits():
    # one cell a half: P_SO = 2 / (2 + a), P_GO = 2 / (1 + a) - 2 / (2 + a); OS at N = 1: 1 / (1 + a)
    assert abs(float(E.cfar_alpha_est(0.25, 1, E.Est(E.SO))) - 6.0) <= 6.0 * 2.0 ** -23
    a = float(E.cfar_alpha_est(0.25, 1, E.Est(E.GO)))
    assert abs(2.0 / (1.0 + a) - 2.0 / (2.0 + a) - 0.25) <= 1e-6
    assert abs(float(E.cfar_alpha_est(0.25, 1, E.Est(E.OS, 0, 1))) - 3.0) <= 3.0 * 2.0 ** -23
    assert E.cfar_alpha_est(1e-6, 90, E.Est(E.CA)) == C.cfar_alpha(1e-6, 90) and E.cfar_alpha_est(1e-6, 90, None) == C.cfar_alpha(1e-6, 90)


@pytest.mark.parametrize("guard", [0, 2])
def test_cell_averaging_through_the_new_path(guard):
    P = _floor()
    P[10, 40], P[31, 95], P[0, 0] = 300.0, 80.0, 60.0
    prm = C.Params(C.cfar_alpha(1e-4, 90), 1, 1, 3, 4, max_det=8)
    want = C.detect(P, guard, prm)
    for est in (None, E.Est(E.CA), E.Est(E.CA, 1, 5)):
        got = E.detect(P, guard, prm, est)
        assert got["count"] == want["count"] and got["cells"] == want["cells"] and got["ambiguous"] == want["ambiguous"]
        assert np.array_equal(got["det"], want["det"]) and np.array_equal(got["bar"], want["bar"])


def _mutation_cases():
    """(P, guard, Params, Est): the scenes above and the edges of a small map"""
    cases = []
    P = _floor()
    P[10, 40], P[10, 44], P[20, 70] = 3000.0, 80.0, 60.0
    for name in ("go", "so", "os"):
        prm, est = _scene_params(name)
        cases.append((P, 0, prm, est))
    Q = _floor()
    Q[:, 48:] *= 30.0
    cases.append((Q, 0) + _scene_params("so"))
    S = np.random.default_rng(3).exponential(1.0, size=(16, 9))
    S[0, 0], S[8, 8], S[5, 4] = 40.0, 40.0, 40.0
    cases.append((S, 0, C.Params(4.0, 0, 0, 1, 2, max_det=16), E.Est(E.OS, 0, 12)))         # Nfull = 14: corners hold five cells
    S2 = S.copy()
    S2[4:7, 0], S2[5, 1] = 0.01, 40.0                                            # at lag 1 the lower half is three quiet cells: fewer than min_train
    cases.append((S2, 0, C.Params(4.0, 0, 0, 1, 2, min_train=4, max_det=16), E.Est(E.SO, E.LAG)))
    cases.append((S, 0, C.Params(4.0, 0, 0, 1, 2, max_det=16), E.Est(E.GO, E.DOPPLER)))
    T = np.ones((16, 9))
    T[4, 4], T[9, 2] = 4.0, 5.0                                                  # noise 1, alpha 4: P = 4 sits AT the threshold
    cases.append((T, 0, C.Params(4.0, 0, 0, 1, 2, max_det=16), E.Est(E.OS, 0, 7)))
    return cases


@pytest.mark.parametrize("which", E.MUTATIONS)
def test_every_mutation_is_caught(which):
    caught = 0
    for P, guard, prm, est in _mutation_cases():
        want, got = E.detect(P, guard, prm, est), E.detect(P, guard, prm, est, which)
        same = want["count"] == got["count"] and want["cells"] == got["cells"] and np.all(np.abs(got["det"] - want["det"]) <= want["bar"])
        caught += 0 if same else 1
    assert caught >= 1, which
