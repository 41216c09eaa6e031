"""CPU checks of the reference-noise canceller's definition (tests/refcancel_model.py) and of the bars the device tests hold the kernels
to (tests/refcancel_cases.py): the least-squares properties of the solution, the edge terms of the Gram, what the filter buys
against a residual timing offset, the conditioning the coefficient tolerance rests on, and that single mistakes miss the bars."""
import numpy as np
import pytest

import refcancel_cases as cases
import refcancel_model as M


def db(x):
    return 10.0 * np.log10(x)


@pytest.mark.parametrize("taps", [1, 3, 5, 9])
def test_residual_is_orthogonal_to_every_tap(taps):
    block, lag, ph = cases.perop_case(256)
    for r in (3, 5, 6, 9):
        m = M.cancel_row(block, r, int(lag[r]), ph[r], taps)
        z = m["y"] - m["g"] @ m["R"]
        dots = m["R"].conj() @ z
        assert np.abs(dots).max() <= 1e-9 * np.abs(m["c"]).max(), (taps, r, np.abs(dots).max())


@pytest.mark.parametrize("taps", [1, 3, 9])
def test_residual_identity(taps):
    block, lag, ph = cases.perop_case(256)
    for r in range(1, block.shape[0]):
        m = M.cancel_row(block, r, int(lag[r]), ph[r], taps)
        z = m["y"] - m["g"] @ m["R"]
        if m["E"] == 0:
            assert m["residual"] == 1.0
            continue
        g, res, _ = M.solve(m["G"], m["c"], m["E"])
        assert abs(res - np.sum(np.abs(z) ** 2) / m["E"]) <= 1e-12, (taps, r)


def test_gram_has_its_edge_terms_at_L32():
    block, _ = M.noise_scene(3, 32, 0.5)
    ri, rq = M.to_ints(block[0])
    r = ri + 1j * rq
    R = M.tap_rows(r, 4)
    _, G, _ = M.sums(r, R)
    T = M.toeplitz_gram(r, 4)
    assert np.allclose(G, G.conj().T) and np.abs(G - T).max() >= 1.0
    assert G[4, 4] == T[4, 4] == np.sum(np.abs(r) ** 2)                    # the centre entry has no edge term
    assert G[0, 0].real < T[0, 0].real and G[8, 8].real < T[8, 8].real      # the outer taps lose samples at the edges
    # by hand: G_ij = sum over n with both n - i and n - j inside the row
    for (i, j) in ((-4, 3), (0, 1), (2, 2), (-1, -3)):
        want = sum(np.conj(r[n - i]) * r[n - j] for n in range(32) if 0 <= n - i < 32 and 0 <= n - j < 32)
        assert G[i + 4, j + 4] == want, (i, j)


def scene_residuals(taps, seed):
    block, share = M.noise_scene(seed, 512, 0.5, gain=1.0)       # noise sigma 25 against receiver noise sigma 4: a share of -16 dB
    m = M.cancel_row(block, 1, 0, 1.0, taps)
    return float(m["residual"]), float(share[0]), m["cond"]


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_depth_against_half_a_sample_of_offset(seed):
    """band-limited noise (0.8 of the band), L = 512, D = 0.5: nine taps reach the receiver-noise share of the scene within 1 dB, one
    tap stays at least 10 dB above it"""
    r9, share, _ = scene_residuals(9, seed)
    r1, _, _ = scene_residuals(1, seed)
    print(f"seed {seed}: share {db(share):.2f} dB, 9 taps {db(r9):.2f} dB, 1 tap {db(r1):.2f} dB")
    assert abs(db(r9) - db(share)) <= 1.0, (db(r9), db(share))
    assert db(r1) - db(share) >= 10.0, (db(r1), db(share))


def test_gram_condition_number_of_these_rows():
    """the coefficient tolerance of the device tests has a term 1e-12 cond(G): it is only a tolerance while cond(G) stays small"""
    worst = 0.0
    for seed in (1, 2, 3):
        worst = max(worst, scene_residuals(9, seed)[2])
    for B in cases.BLOCKSIZES:
        m = cases.perop_model(B, 9)
        worst = max(worst, m["cond"][1:].max())
    print(f"largest cond(G): {worst:.1f}")
    assert worst <= 100.0, worst


def test_solver_refuses_deficient_reference_rows():
    for kind, status in (("zero", 1), ("single", 1), ("constant", 0)):
        block, lag, ph = cases.failure_case(kind)
        want = M.cancel_block(block, lag, ph, 3)
        assert (want["status"][1:] == status).all(), (kind, want["status"])
        if status:
            assert not want["coef"].any() and (want["residual"][1:] == 1.0).all()
            # with g = 0 the row is the plain rotation of the shifted row
            y, R = M.row_parts(block, 5, int(lag[5]), 1)
            assert np.array_equal(want["out"][5], M.quantise(np.complex64(ph[5]).astype(np.complex128) * y))


def test_restated_excess_is_small():
    """the float32 restatement's own rounding excess -- the device tests allow four times this -- is far below one count"""
    e = cases.reference_excess()
    print(f"e_ref = {e:.3e}")
    assert cases.EXCESS_FLOOR <= e < 1e-3, e


@pytest.mark.parametrize("mutation", ["tapdir", "noconj", "toeplitz", "pconj"])
def test_single_mistakes_miss_the_bars_at_L32(mutation):
    """a device that made one of these mistakes, judged as the device tests judge: it must miss a bar"""
    B = 64
    block, lag, ph = cases.perop_case(B)
    want = cases.perop_model(B, 3)
    got = dict(out=np.zeros_like(want["out"]), coef=np.zeros_like(want["coef"]), residual=want["residual"].copy(), status=want["status"].copy())
    got["out"][0] = block[0]
    for r in range(1, block.shape[0]):
        m = M.cancel_row(block, r, int(lag[r]), ph[r], 3, mutation=mutation)
        got["out"][r], got["coef"][r] = m["out"], m["g32"]
    miss = cases.check_block(block, lag, ph, 3, got, want, mutation)
    assert miss, mutation
    if mutation in ("tapdir", "pconj"):                       # these two are caught by the bytes themselves
        assert any("byte excess" in x for x in miss), miss
    # and the unmutated answer passes
    assert cases.check_block(block, lag, ph, 3, want, want) == []
