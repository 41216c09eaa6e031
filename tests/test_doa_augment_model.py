"""CPU checks of the numpy restatement of co-array augmentation (tests/doa_augment_model.py) that the GPU tests compare against: the
population identity it is defined by, its structure, that it ignores absent receivers, that single mistakes miss the bar, and the 24
scenes of the 7 x 3 array (full, two dead receivers, a 12-of-21 thinning, and a 5 x 2 virtual array) in fp64."""
import numpy as np
import pytest

import doa_augment_model as model
import doa_peaks_model as peaks_model
import doa_smooth_model as smooth_model
import ura


def _population(mx, my, dirs, powers, noise):
    """R = A P A^H + noise I in the X^H X convention (conjugated steering vectors), fp64"""
    A = np.stack([ura.steering(a, b, ura.D, mx, my).conj() for a, b in dirs], axis=1)
    return A @ np.diag(powers) @ A.conj().T + noise * np.eye(mx * my)


def _random_hermitian(m, rng):
    x = rng.standard_normal((m, 3 * m)) + 1j * rng.standard_normal((m, 3 * m))
    r = x @ x.conj().T / (3 * m)
    return ((r + r.conj().T) / 2).astype(np.complex64)      # Hermitian to the bit


def test_population_identity():
    dirs = [(a, b) for a, b, _ in model.SOURCES]
    powers = [1.0, 0.8, 0.6]
    R = _population(7, 3, dirs, powers, 0.4)
    worst = 0.0
    for name, mask, vx, vy in model.CONFIGS:
        want = _population(vx, vy, dirs, powers, 0.4)
        err = np.abs(model.augment(R, 7, 3, vx, vy, mask) - want).max()
        worst = max(worst, err)
        assert err < 1e-13, (name, err)
    print(f"population identity: largest error {worst:.2e}")


def test_block_toeplitz_input_comes_back_and_output_is_hermitian():
    rng = np.random.default_rng(5)
    R = _population(7, 3, [(1.0, 1.2), (2.0, 1.9)], [1.0, 0.5], 0.3).astype(np.complex64)      # block-Toeplitz up to fp32 rounding
    T = model.augment(R, 7, 3, 7, 3)                                                           # ... and exactly, as fp64 numbers
    assert np.abs(model.augment(T, 7, 3, 7, 3) - T).max() < 1e-14                                # (means of equal fp64 numbers: a few ulp)
    for mx, my, vx, vy, mask in ((7, 3, 7, 3, 0), (7, 3, 5, 2, model.dead(21, (4, 16))), (8, 8, 4, 4, 0), (7, 1, 7, 1, model.mask_of(model.RULER, 7))):
        ra = model.augment(_random_hermitian(mx * my, rng), mx, my, vx, vy, mask)
        assert np.array_equal(ra, ra.conj().T) and not ra.imag.diagonal().any(), (mx, my, vx, vy)
        # block-Toeplitz: an entry depends on the lag alone
        for a in range(vx * vy - 1):
            if (a + 1) % vx:
                assert ra[a, a + 1] == ra[0, 1]


def test_absent_rows_and_columns_are_never_read():
    rng = np.random.default_rng(6)
    for name, mask, vx, vy in model.CONFIGS[1:]:
        r = _random_hermitian(21, rng)
        ref = model.augment(r, 7, 3, vx, vy, mask)
        gone = [i for i in range(21) if i not in model.present(mask, 21)]
        r[gone, :] = np.nan
        r[:, gone] = np.nan
        assert np.array_equal(model.augment(r, 7, 3, vx, vy, mask), ref), name
        assert np.isfinite(model.readable_top(r, 7, 3, mask))


def _mistaken(rxx, mx, my, vx, vy, mask, which):
    """augment() with one mistake"""
    r = np.asarray(rxx).astype(np.complex128)
    m, mv = mx * my, vx * vy
    full = (1 << m) - 1
    vw = mx if which == "mx_for_vx" else vx

    def mean(ux, uy):
        if uy < 0 or (uy == 0 and ux < 0):
            return np.conj(mean(-ux, -uy))
        summed = model.pairs(mx, my, ux, uy, full if which == "masked_element" else mask)
        counted = model.pairs(mx, my, ux, uy, full if which in ("unmasked_count", "masked_element") else mask)
        return sum(r[p, q] for p, q in summed) / max(len(counted), 1)

    out = np.zeros((mv, mv), dtype=np.complex128)
    for a in range(mv):
        for b in range(a, mv):
            ux, uy = b % vw - a % vw, b // vw - a // vw
            v = mean(-ux if which == "ux_sign" else ux, uy)
            if which == "wrong_triangle":
                v = np.conj(v)
            if a == b:
                v = complex(v.real, 0.0)
            out[a, b], out[b, a] = v, np.conj(v)
    return out


@pytest.mark.parametrize("which", ["none", "unmasked_count", "wrong_triangle", "ux_sign", "mx_for_vx", "masked_element"])
def test_single_mistakes_miss_the_bar(which):
    rng = np.random.default_rng(7)
    r = _random_hermitian(21, rng)
    mask, vx, vy = model.dead(21, (4, 16)), 5, 2
    want = model.augment(r, 7, 3, vx, vy, mask)
    dev = _mistaken(r, 7, 3, vx, vy, mask, which).astype(np.complex64)
    ok, worst = model.within_bar(dev, want, model.readable_top(r, 7, 3, mask))
    print(f"{which}: largest error / bar {worst:.3g}")
    assert ok == (which == "none"), (which, worst)


def _music(ra, k, vx, vy):
    s, pm = smooth_model.spectrum(ra, k, vx, vy)
    n, found, _ = peaks_model.directions(pm.astype(np.float32), k, 2)
    return s, n, found


@pytest.mark.parametrize("name,mask,vx,vy", model.CONFIGS, ids=[c[0] for c in model.CONFIGS])
def test_every_scene_is_resolved_by_the_model(name, mask, vx, vy):
    scenes = model.scenes()
    assert len(scenes) == 24
    low = 0.0
    for seed, k, blk in scenes:
        r = model.scene_covariance(blk, mask)
        ra = model.augment(r, 7, 3, vx, vy, mask)
        s, n, found = _music(ra, k, vx, vy)
        assert n == k and smooth_model.all_within(found, model.SOURCES[:k], tol=1.0), (name, seed, k, found.tolist())
        ev = np.linalg.eigvalsh(ra)[0] / s[k - 1]
        low = min(low, ev)
        assert ev > -0.05, (name, seed, k, ev)
    print(f"{name}: 24 / 24, smallest eigenvalue / sv[k-1] {low:.4f}")
