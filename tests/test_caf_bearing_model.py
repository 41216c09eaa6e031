"""CPU checks of tests/caf_bearing_model.py, the fp64 statement of crsdr_caf's bearings (include/crsdr.h, section (w), "Bearings"): the
properties of the statistic, the training set against the detector's by enumeration, the polynomial form of a^H W a, the scenes of the
issue with their conditions, the agreement with the MUSIC model, and seven single mistakes that each move a peak or miss a condition
on a named scene.  No device."""
import numpy as np
import pytest

import caf_bearing_model as BM
import caf_cfar_model as C
import caf_model as M
import doa_refine_model as RF
import music_model as mm


def _scene(sc, off=(0.0, 0.0), guard=1, amp=None, seed=None, alpha=BM.ALPHA, cfar=BM.CFAR, direct=0.8):
    """(chi32, det, count, prm, q, truth, the echo's slot) of a scene's line, from the model's own fp32 chi and map"""
    line, q, truth = BM.scene_line(sc, off, amp=amp, seed=seed, direct=direct)
    chi, mp = BM.scene_maps(sc, line)
    prm = C.Params(alpha, max_det=8, **cfar)
    r = C.detect(mp, guard, prm)
    hit = [k for k in range(min(r["count"], 8)) if (r["det"][k][0], r["det"][k][1]) == (sc[9], sc[10])]
    assert len(hit) == 1 and r["ambiguous"] == 0, (r["det"][:4], sc[9], sc[10])
    return chi, r["det"], r["count"], prm, q, truth, hit[0]


@pytest.fixture(scope="module")
def scenes():
    return [_scene(sc) for sc in BM.SCENES]


def test_the_statistic_lies_in_0_1_and_is_1_at_a_steering_vector():
    rng = np.random.default_rng(3)
    for mx, my, nc in ((1, 2, 8), (2, 1, 8), (3, 2, 16), (7, 3, 24), (8, 8, 12)):
        q = BM.Desc(mx, my, 0.5, nc, nc)
        gx, gy = BM.grid_points(q)
        a = BM.steer(q, gx, gy)
        u = rng.standard_normal(q.m) + 1j * rng.standard_normal(q.m)
        A = rng.standard_normal((q.m, q.m)) + 1j * rng.standard_normal((q.m, q.m))
        for W in (np.eye(q.m), np.linalg.inv(A @ A.conj().T + 0.1 * np.eye(q.m))):
            T = BM.stat(W, u, a)
            assert T.min() >= 0.0 and T.max() <= 1.0 + 1e-12
        for p in (0, len(gx) // 3, len(gx) - 1):
            T = BM.stat(np.eye(q.m), (0.3 - 0.2j) * a[p], a)
            assert abs(T[p] - 1.0) <= 8 * q.m * BM.E64 and T.max() <= 1.0 + 8 * q.m * BM.E64


def test_adaptive_with_white_training_tends_to_conventional():
    q = BM.Desc(3, 2, 0.5, 16, 16, BM.ADAPTIVE, 1e-2)
    gx, gy = BM.grid_points(q)
    a = BM.steer(q, gx, gy)
    rng = np.random.default_rng(5)
    u = rng.standard_normal(q.m) + 1j * rng.standard_normal(q.m)
    conv = BM.stat(np.eye(q.m), u, a)
    gap = []
    for n in (100, 10000, 1000000):
        Ut = (rng.standard_normal((n, q.m)) + 1j * rng.standard_normal((n, q.m))) / np.sqrt(2.0)
        Q = Ut.T @ Ut.conj() / n
        W = np.linalg.inv(Q + q.loading * np.trace(Q).real / q.m * np.eye(q.m))
        gap.append(np.max(np.abs(BM.stat(W, u, a) - conv)))
    assert gap[0] > gap[1] > gap[2] and gap[2] < 0.01, gap                       # like 1 / sqrt(n)


@pytest.mark.parametrize("nd,R,guard,cf", [(8, 6, 0, dict(gd=1, gr=1, td=2, tr=3)), (16, 10, 2, dict(gd=1, gr=1, td=3, tr=4)), (8, 5, 4, dict(gd=0, gr=0, td=1, tr=0)),
                                           (16, 3, 1, dict(gd=2, gr=0, td=5, tr=8))])
def test_the_training_set_is_the_detectors_for_every_cell(nd, R, guard, cf):
    """N against caf_cfar_model.train_cell and train_sums by enumeration over the whole map: lag 0, lag R - 1, the bins beside the guard
    and the wrap among them"""
    prm = C.Params(1.0, **cf)
    _, N = C.train_sums(np.ones((nd, R)), guard, prm)
    ok = M.in_set(nd, guard)
    for d in range(nd):
        if not ok[d]:
            continue
        for tau in range(R):
            cells = BM.train_cells(nd, R, guard, prm, d, tau)
            z, n, want = C.train_cell(np.ones((nd, R)), guard, prm, d, tau)
            assert cells == want and len(cells) == n == N[d, tau] == len(set(cells)), (d, tau)
            assert all(ok[dq] and 0 <= tq < R and not (min(abs(dq - d), nd - abs(dq - d)) <= prm.gd and abs(tq - tau) <= prm.gr) for dq, tq in cells)


def test_the_polynomial_form_equals_the_quadratic_form():
    rng = np.random.default_rng(11)
    for mx, my, nc in ((1, 2, 8), (2, 1, 8), (3, 2, 16), (7, 3, 20), (8, 8, 10), (64, 1, 6), (1, 64, 6)):
        q = BM.Desc(mx, my, 0.5, nc, nc + 1)
        A = rng.standard_normal((q.m, q.m)) + 1j * rng.standard_normal((q.m, q.m))
        W = np.linalg.inv(A @ A.conj().T / q.m + 0.05 * np.eye(q.m))
        gx, gy = BM.grid_points(q)
        gx, gy = gx + 0.37, gy - 0.21
        a = BM.steer(q, gx, gy)
        quad = np.einsum("pe,ef,pf->p", a.conj(), W, a).real
        poly = BM.awa_polynomial(W, q, gx, gy)
        assert np.max(np.abs(poly - quad) / quad) <= 1e-12, (mx, my)
        assert BM.coefficients(W, mx, my).shape == (mx, 2 * my - 1)


@pytest.mark.parametrize("mode", [BM.CONVENTIONAL, BM.ADAPTIVE])
def test_the_echo_is_on_its_cell_and_the_leaks_at_broadside(scenes, mode):
    for sc, (chi, det, count, prm, q, truth, k) in zip(BM.SCENES, scenes):
        q.mode = mode
        r = BM.bearing(chi, det, count, 0, 1, prm, q)
        assert r["ambiguous"] == 0
        assert (r["dir"][k][0], r["dir"][k][1]) == sc[8], (BM.scene_id(sc), r["dir"][k])
        leaks = [j for j in range(min(count, 8)) if det[j][0] == 0 and abs(det[j][1]) == 1]
        assert len(leaks) == 2 and all((r["dir"][j][0], r["dir"][j][1]) == (q.ncx // 2, q.ncy // 2) for j in leaks), (BM.scene_id(sc), r["dir"][:count])
        T = r["spec"][k]
        second = np.sort(T.reshape(-1))[-2]
        assert second <= 0.999 * T.max()                                         # the runner-up is orders of magnitude outside any fp64 bar
        if mode == BM.ADAPTIVE:
            assert np.all(r["N"][:count] == det[:count, 7])                      # N is the ntrain the detection reports


@pytest.mark.parametrize("off", BM.OFFSETS)
def test_off_the_grid(off):
    """guard 2, levels 5: within 0.15 cell of the truth conventional, within 0.02 adaptive at loading 1e-2"""
    for sc in BM.OFF_SCENES:
        chi, det, count, prm, q, (x, y), k = _scene(sc, off, guard=2)
        q.levels = 5
        for mode, bound in ((BM.CONVENTIONAL, 0.15), (BM.ADAPTIVE, 0.02)):
            q.mode = mode
            d, tau = BM.cell_of(det[k], chi.shape[1])
            f = BM.one(chi, 0, 2, prm, q, d, tau)["dir"]
            err = max(abs(f[0] + f[3] - x), abs(f[1] + f[4] - y))
            print(BM.scene_id(sc), off, mode, f[:5], err)
            assert err <= bound, (BM.scene_id(sc), off, mode, f)


def _weak(seed, which=None, mode=BM.ADAPTIVE):
    w = BM.WEAK
    sc = BM.SCENES[w["scene"]]
    chi, det, count, prm, q, _, k = _scene(sc, guard=w["guard"], amp=w["amp"], seed=seed, alpha=w["alpha"], cfar=w["cfar"])
    q.mode, q.loading = mode, float(np.float32(w["loading"]))
    d, tau = BM.cell_of(det[k], chi.shape[1])
    return BM.one(chi, 0, w["guard"], prm, q, d, tau, which)["dir"], sc


@pytest.mark.parametrize("seed", BM.WEAK["seeds"])
def test_the_weak_echo(seed):
    f, sc = _weak(seed)
    g, _ = _weak(seed, mode=BM.CONVENTIONAL)
    print(seed, f[:3], g[:3])
    assert (f[0], f[1]) == sc[8] and f[2] >= 0.99
    assert g[2] <= 0.9


def test_agreement_with_the_music_model():
    """one emitter and no direct path: music_model's MUSIC peak (k = 1) of the element rows and the bearing of the echo's detection are
    the same cell"""
    for sc in BM.SCENES[:2]:
        line, q, _ = BM.scene_line(sc, amp=0.5, direct=0.0)
        chi, det, count, prm, q, _, k = _scene(sc, amp=0.5, direct=0.0)
        d, tau = BM.cell_of(det[k], chi.shape[1])
        f = BM.one(chi, 0, 1, prm, q, d, tau)["dir"]
        block = np.concatenate(line, axis=1)
        sv, vec = RF.fp64_subspace(block)
        den, _ = mm.scan(vec, 1, q.d, q.mx, q.my, q.ncx, q.ncy)
        peak = np.unravel_index(np.argmin(den), den.shape)
        assert tuple(int(v) for v in peak) == (int(f[0]), int(f[1])) == sc[8], (peak, f)


# ---- single mistakes: each moves a peak or misses a condition on a named scene ----
def _strong(which, mode, scene=0):
    chi, det, count, prm, q, _, k = _scene(BM.SCENES[scene])
    q.mode = mode
    d, tau = BM.cell_of(det[k], chi.shape[1])
    return BM.one(chi, 0, 1, prm, q, d, tau, which)["dir"], BM.SCENES[scene]


def test_mistake_no_conjugate():
    f, sc = _strong("no_conj", BM.CONVENTIONAL)
    assert (f[0], f[1]) != sc[8]                                                 # the mirrored direction


def test_mistake_reference_row_counted():
    f, sc = _strong("ref_counts", BM.CONVENTIONAL)
    assert (f[0], f[1]) != sc[8] or f[2] < 0.9


def test_mistake_ix_iy_swapped():
    f, sc = _strong("xy_swapped", BM.CONVENTIONAL)
    assert (f[0], f[1]) != sc[8]


def test_mistake_guard_cells_train():
    """the target in its own training set nulls itself: the fit of the weak echo drops under the condition"""
    for seed in BM.WEAK["seeds"][:2]:
        f, sc = _weak(seed, "guard_trains")
        assert f[2] < 0.99 or (f[0], f[1]) != sc[8], f


def test_mistake_denominator_left_out():
    """without a^H W a the weighting's own gain decides: the weak echo's peak leaves its cell"""
    moved = 0
    for seed in BM.WEAK["seeds"]:
        f, sc = _weak(seed, "no_denominator")
        moved += (f[0], f[1]) != sc[8] or not f[2] <= 1.0
    assert moved >= 1


def test_mistake_loading_left_out():
    """N < m without loading: Q is singular; what an inverse of it gives is not finite, elsewhere, or far outside the bar"""
    sc = BM.SCENES[2]                                                            # 8 x 8: m = 64 above N = 26 .. 54
    chi, det, count, prm, q, _, k = _scene(sc)
    q.mode = BM.ADAPTIVE
    d, tau = BM.cell_of(det[k], chi.shape[1])
    good = BM.one(chi, 0, 1, prm, q, d, tau)
    assert good["N"] < q.m and (good["dir"][0], good["dir"][1]) == sc[8]
    with np.errstate(all="ignore"):
        f = BM.one(chi, 0, 1, prm, q, d, tau, "no_loading")["dir"]
    assert not np.all(np.isfinite(f)) or (f[0], f[1]) != sc[8] or abs(f[2] - good["dir"][2]) > 1e3 * good["tbar"], (f, good["dir"])


def test_mistake_doppler_not_wrapped():
    """a cell whose window crosses the wrap loses training cells: N no longer equals the detector's ntrain"""
    nd, R, guard = 16, 10, 1
    prm = C.Params(1.0, gd=1, gr=1, td=3, tr=4)
    d, tau = 14, 5
    right, wrong = BM.train_cells(nd, R, guard, prm, d, tau), BM.train_cells(nd, R, guard, prm, d, tau, "doppler_nowrap")
    assert len(right) == C.train_cell(np.zeros((nd, R)), guard, prm, d, tau)[1] > len(wrong)
    q = BM.Desc(3, 2, 0.5, 16, 16, BM.ADAPTIVE, 1e-2)
    floor = np.insert(BM.steer(q, [8], [8])[0], 0, 1.0)
    chi = BM.plant(BM.noise_chi(7, nd, R, 8, floor), 0, q, d, tau, 5, 9, amp=0.004)
    a, bb = BM.one(chi, 0, guard, prm, q, d, tau), BM.one(chi, 0, guard, prm, q, d, tau, "doppler_nowrap")
    assert a["N"] != bb["N"] and np.max(np.abs(a["spec"] - bb["spec"])) > 1e3 * a["tbar"]
