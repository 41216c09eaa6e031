"""CPU: the closed form of tests/peak_cases.py against the fp64 model and the fp32 C oracle, and the margin that keeps
test_gpu_peak.py from passing a wrong neighbour.

  - closed form == oracle/model_fp64.py xcorr_lag: lag exactly, mag and frac to 1e-12 (relative / absolute), the aligned matrix and the
    phasors of model_fp64.Model equal to the expected ones -- over every peak position of B = 16 .. 1024 and the designed positions
    of B = 16384 and 2^15, and at those two sizes the ends, the centre and 64 seeded indices from anywhere in 1 .. B - 1 (what the
    full sweeps of test_gpu_peak.py rest on); the sweeps' slices reach every index;
  - the C oracle (fp32, another FFT) lies within the error bar the GPU tests use; its worst errors are printed for scale;
  - the confusion margin: putting any other value that occurs (0, the other neighbour, the peak) in place of ym or yp moves frac by at
    least 100 x the largest error bar used anywhere, the band-limited rows' bars included.
"""
import numpy as np
import pytest

import peak_cases as pc

FULL = [4, 5, 6, 7, 8, 9, 10]
DESIGNED = [14, 15]


def _blocks(log2B):
    """[(q, ps)] of one size: every position for the small sizes, the designed ones for 16384 and 2^15."""
    L = (1 << log2B) // 2
    if log2B in FULL:
        idxs = pc.full_positions(L)
    elif log2B == 14:
        idxs = pc.k1_positions(L)[0]
    else:
        return [(q, ps) for q, ps in pc.long_blocks(log2B)]
    return list(zip(pc.ref_positions(L), pc.split_by_reference(L, idxs)))


def _probe_blocks(log2B):
    """[(q, ps)] of the full sweeps' proof: the ends, the centre and 64 seeded indices anywhere in 1 .. B - 1."""
    L = (1 << log2B) // 2
    idxs = pc.probe_positions(log2B)
    return [(q, idxs[(idxs >= lo) & (idxs <= hi)] - L + q) for q, lo, hi in ((0, L, 2 * L - 1), (L - 1, 1, L))]


def test_the_sweeps_reach_every_index_once_per_reference():
    for L, n in ((8192, pc.K1_SWEEP_ROWS), (1 << 14, pc.LONG_SWEEP_ROWS)):
        order = [(q, ps) for q, slices in pc.sweep_batches(L, n) for ps in slices]
        assert all(len(ps) == n for _, ps in order) and len(order) == 2 * -(-L // n)
        exp = [pc.closed_form(L, q, ps) for q, ps in order]
        res = {k: [np.concatenate([[0], e[k]]) for e in exp] for k in ("lag", "mag", "frac")}      # a fetched block: row 0 is the reference
        g = pc.gather_by_idx(L, order, res)
        assert not pc.sweep_is_complete(L, g["reached"])
        assert np.array_equal(g["lag"], np.arange(1, 2 * L) - L) and g["lag_L"][0] == 0 and g["mag_L"][0] == g["mag"][L - 1]
        assert g["frac"][0] != g["frac"][1] and g["frac"][-1] == 0                                   # idx 1 has no ym, idx B - 1 no parabola
        if L % n == 0:
            assert g["reached"].sum() == 2 * L                                                       # every idx once, idx = L twice
        g["reached"][0, L + 5] = 0
        assert pc.sweep_is_complete(L, g["reached"])                                                 # a hole is seen


@pytest.mark.parametrize("log2B", [14, 15])
def test_closed_form_equals_fp64_model_off_the_designed_positions(model, log2B):
    # the full sweeps of test_gpu_peak.py hold the device to the closed form at every idx: prove it away from the wave edges and tile ends
    L = (1 << log2B) // 2
    designed = pc.k1_positions(L)[0] if log2B == 14 else pc.long_positions(log2B)[0]
    idxs = pc.probe_positions(log2B)
    assert np.isin([1, 2, 2 * L - 2, 2 * L - 1, L - 1, L, L + 1], idxs).all() and np.count_nonzero(~np.isin(idxs, designed)) >= 48
    blocks = _probe_blocks(log2B)
    assert sum(len(ps) for _, ps in blocks) == idxs.size + 1                                         # idx = L under both references
    for q, ps in blocks:
        _check_against_model(model, L, q, ps)


@pytest.mark.parametrize("log2B", FULL + DESIGNED)
def test_closed_form_equals_fp64_model(model, log2B):
    L = (1 << log2B) // 2
    for q, ps in _blocks(log2B):
        _check_against_model(model, L, q, ps)


def _check_against_model(model, L, q, ps):
    rows, exp = pc.pulse_block(L, q, ps), pc.closed_form(L, q, ps)
    ref = pc.model_reference(model, rows)
    assert np.array_equal(ref["lag"], exp["lag"])
    assert np.max(np.abs(ref["mag"] - exp["mag"]) / exp["mag"]) <= 1e-12
    assert np.max(np.abs(ref["frac"] - exp["frac"])) <= 1e-12
    for key in ("ym", "mp", "yp"):
        assert np.max(np.abs(ref[key] - exp[key]) / exp["mp"]) <= 1e-12, key
    mod = model.Model(rows.shape[0], 2 * L, model.DIGITAL)
    for _ in range(2):                                         # the second block runs on the carried EMA state
        lag, mag, frac, phasor, matrix = mod.block(rows)
        assert np.array_equal(matrix, pc.expected_matrix(L, q, ps))
        assert np.all(phasor[1:] == 1.0)


@pytest.mark.parametrize("log2B", FULL + DESIGNED)
def test_oracle_lies_within_the_bar(oracle, log2B):
    L = (1 << log2B) // 2
    worst_mag = worst_frac = 0.0
    for q, ps in _blocks(log2B):
        rows, exp = pc.pulse_block(L, q, ps), pc.closed_form(L, q, ps)
        orc = oracle.Engine(rows.shape[0], 2 * L, oracle.DIGITAL)
        for t in range(2):
            got = orc.block(rows, seq=t)
            emag, efrac, fails = pc.compare({k: got[k][1:] for k in ("lag", "mag", "frac")}, exp, f"B = 2^{log2B}, q = {q}")
            assert not fails, "\n".join(fails)
            assert np.array_equal(got["matrix"], pc.expected_matrix(L, q, ps))
            assert np.all(got["phasor"][1:] == 1.0)
            worst_mag, worst_frac = max(worst_mag, emag), max(worst_frac, efrac)
        orc.close()
    print(f"oracle, B = 2^{log2B}: worst mag rel err {worst_mag:.3e}  worst frac abs err {worst_frac:.3e}")


@pytest.fixture(scope="module")
def fractional(model):
    """{L: (rows, fp64 reference)} of the band-limited rows test_gpu_peak.py uses."""
    out = {}
    for L in (2048, 8192, 1 << 15):
        rows = pc.fractional_rows(L)
        out[L] = (rows, pc.model_reference(model, rows))
    return out


def test_fractional_rows_have_large_fractions_and_the_oracle_is_well_inside(fractional, oracle):
    for L, (rows, ref) in fractional.items():
        assert np.all(np.abs(ref["lag"] - np.array(pc.FRACTIONAL_DELAYS)) <= 0.5)
        assert np.all((np.abs(ref["frac"]) > 0.15) & (np.abs(ref["frac"]) < 0.45)), ref["frac"]     # clear of 0 and of the half-sample tie
        orc = oracle.Engine(rows.shape[0], 2 * L, oracle.DIGITAL)
        got = orc.block(rows)
        orc.close()
        emag, efrac, fails = pc.compare({k: got[k][1:] for k in ("lag", "mag", "frac")}, ref, f"L = {L}")
        assert not fails, "\n".join(fails)
        print(f"band-limited rows, L = {L}: |frac| {np.abs(ref['frac']).min():.3f} .. {np.abs(ref['frac']).max():.3f}, bar {ref['bar'].min():.2e} .. "
              f"{ref['bar'].max():.2e}, oracle worst mag rel err {emag:.3e}, frac abs err {efrac:.3e} ({(ref['bar'] / np.maximum(np.abs(got['frac'][1:] - ref['frac']), 1e-300)).min():.0f} x inside)")


def test_a_wrong_neighbour_moves_frac_by_100_bars(fractional):
    largest_bar = max(ref["bar"].max() for _, ref in fractional.values())
    smallest_move = np.inf
    for log2B in FULL + [14, 15, 16, 18]:
        L = (1 << log2B) // 2
        blocks = _blocks(log2B) if log2B != 14 else list(zip(pc.ref_positions(L), pc.split_by_reference(L, pc.k1_positions(L)[1])))
        if log2B in (14, 15):                                               # the full sweeps of test_gpu_peak.py: every idx 1 .. B - 1
            blocks = blocks + list(zip(pc.ref_positions(L), pc.split_by_reference(L, pc.full_positions(L))))
        for q, ps in blocks:
            exp = pc.closed_form(L, q, ps)
            largest_bar = max(largest_bar, exp["bar"].max())
            inner = (exp["idx"] > 0) & (exp["idx"] < 2 * L - 1)             # (a peak at B - 1 has no parabola: frac is 0 whatever is read)
            ym, mp, yp, frac = (exp[k][inner] for k in ("ym", "mp", "yp", "frac"))
            for wrong in (np.zeros_like(mp), mp, None):
                for side in (0, 1):
                    a, b = ym.copy(), yp.copy()
                    sub = wrong if wrong is not None else (yp if side == 0 else ym)      # None: the other neighbour
                    changed = sub != (a if side == 0 else b)                # a row whose dropped tap already reads 0: no replacement
                    (a if side == 0 else b)[:] = sub
                    move = np.abs(pc.frac_of(a, mp, b) - frac)[changed]
                    if move.size:
                        smallest_move = min(smallest_move, move.min())
    print(f"smallest change of frac by a wrong neighbour {smallest_move:.3e}, largest error bar {largest_bar:.3e}: factor {smallest_move / largest_bar:.0f}")
    assert smallest_move >= 100 * largest_bar
