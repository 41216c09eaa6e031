"""GPU checks of the k_caf<LG, MODE> instantiations, lag-tile widths and lag reaches that tests/test_gpu_caf*.py do not run: nd = 128, 512
and 1024 (the radix-8, radix-2 and radix-4 remainder passes of sp_pass behind one or two radix-16 passes; tiles of T = 16, 8 and 4 lags),
the canceller's passes at T = 16 above nd = 32 and at T = 8, 4 and 2 with the taps crossing a tile, up to 64 tiles a row, nlags = 1024
with 512 staged words in front of a chunk, every lag parity at one lag a tile, and the smallest packet.

The models and the bars are tests/caf_model.py's and tests/caf_cancel_model.py's, the checks the functions of tests/test_gpu_caf.py and
tests/test_gpu_caf_cancel.py themselves: nothing here is measured and no tolerance is added."""
import importlib

import numpy as np
import pytest

import caf_cancel_model as X
import caf_model as M
from test_gpu_caf import HANN, RECT, _check_line, _run
from test_gpu_caf_cancel import KEYS, _bits, _engine, _hold, _same_line

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def b():
    binding = importlib.import_module("coherent-rtlsdr_amd.binding")
    if binding.device_count() < 1:
        pytest.fail("no HIP device: the product path has no CPU fallback")
    return binding


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


# (nrows, B, seg, frames, nlags, ref, pad), nd = frames B / (2 seg), a tile is T = min(16, 4096 / nd) lags:
#   nd 128   LG 7: the radix-8 remainder behind one radix-16 pass; T = 16, and the tile's tail (13 lags) ends on an even lag
#   nd 512   T = 8: two full tiles and a tail of 5
#   nd 512   even nrows (the matrix only 4-byte aligned) and a padded stride
#   nd 1024  T = 4: two full tiles and a tail of 3; two chunks of 1024 words per packet
#   nd 512   16 tiles of 8 (the last of 5), pre up to 63 words
#   nd 1024  32 tiles of 4 (the last of 3), eight chunks per packet
#   nd 4096  one lag a tile, both parities, up to lag 62
#   nd 8     nlags = seg = 1024: 64 tiles, pre = 512, the reach crosses the chunk boundary and the zero prefix of both packets
#   nd 8     the smallest packet: B = 32, one piece of eight words
CASES = [(3, 1024, 16, 4, 13, 2, 0), (3, 4096, 32, 8, 21, 1, 0), (4, 4096, 32, 8, 16, 0, 4), (2, 8192, 32, 8, 11, 0, 0), (2, 16384, 128, 8, 125, 1, 0),
         (2, 32768, 128, 8, 127, 0, 0), (2, 65536, 64, 8, 63, 0, 0), (2, 8192, 1024, 2, 1024, 1, 0), (2, 32, 16, 8, 16, 0, 0)]
_Y = {}


def _model(case, line, kind):
    """the model of a case's line; the exact range stage is computed once per case and shared by the windows"""
    nrows, B, seg, frames, nlags, ref, pad = case
    if case not in _Y:
        _Y[case] = M.range_stage(line, seg, nlags, ref)
    return M.caf_from_y(*_Y[case], seg, kind)


@pytest.mark.parametrize("kind", [RECT, HANN])
@pytest.mark.parametrize("case", CASES)
def test_chi_map_and_peaks_against_the_model(b, torch, case, kind):
    nrows, B, seg, frames, nlags, ref, pad = case
    line = [M.random_matrix(nrows, B, 7 * B + seg + t) for t in range(frames)]
    want, bar = _model(case, line, kind)
    nd = frames * B // (2 * seg)
    guard = min(2, nd // 2)
    out = _run(b, torch, np.stack(line), seg, nlags, ref, kind, guard, frames, pad)
    _check_line(out["chi"][0], out["map"][0], out["peak"][0], want, bar, ref, guard, f"case {case} window {kind}")


@pytest.mark.parametrize("case", CASES)
def test_exact_cells_at_zero_and_half_doppler(b, torch, case):
    """test_gpu_caf's test_exact_cells_at_zero_doppler at every tile width and lag reach, and at bin nd / 2 beside bin 0.  Rect, rows of
    bytes in -3 .. 3: y converts to fp32 exactly and the window is 1.0f.  Bin 0 leaves every pass of sp_pass as output 0 of its butterfly,
    bin nd / 2 as output 0 of every pass but the last and output R / 2 of the last (digit_reverse<LG>: the last pass makes the index's top
    digit, and nd / 2 sets that digit's top bit alone).  Read in fft_lds.hpp: output 0 of dft2 / dft4 / dft8 / dft16 is a tree of cadd
    alone; output R / 2 is a - b (dft2), (a + c) - (b + d) (dft4), e0 - o0 with both an output 0 of dft4 (dft8), and output 2 of the row
    dft4 over the four untwiddled s = 0 column sums (dft16); sp_pass multiplies the outputs k >= 1 by twiddles, never output 0, and
    nothing behind a last pass (M = 1).  So either cell is a signed sum of the y[k], each partial sum a signed sum of a subset of them:
    with sum_k |y| < 2^24 every one is exact in fp32, whatever the order, and the cell is the exact integer times the fp32 scale: two
    roundings (the scale's own and the product's).  A single wrong product of the range stage shows here; bin nd / 2 sets even k
    against odd k, which bin 0 cannot."""
    nrows, B, seg, frames, nlags, ref, pad = case
    rng = np.random.default_rng(5 + B + nlags)
    line = [rng.integers(-3, 4, size=(nrows, B)).astype(np.int8) for _ in range(frames)]
    yr, yi = M.range_stage(line, seg, nlags, ref)
    nd = frames * B // (2 * seg)
    sr, si = yr.sum(axis=1), yi.sum(axis=1)                                       # [nrows][R], exact
    alt = np.where(np.arange(nd) % 2, -1, 1)[None, :, None]
    ar, ai = (yr * alt).sum(axis=1), (yi * alt).sum(axis=1)
    assert max(np.abs(sr).max(), np.abs(si).max()) < 2 ** 24 and np.abs(si).max() > 0 and np.abs(ai).max() > 0
    assert max(np.abs(yr).sum(axis=1).max(), np.abs(yi).sum(axis=1).max()) < 2 ** 24      # every partial sum of either cell
    print(f"case {case}: largest |sum_k y| {max(np.abs(sr).max(), np.abs(si).max())}, largest sum_k |y| {max(np.abs(yr).sum(axis=1).max(), np.abs(yi).sum(axis=1).max())}")
    out = _run(b, torch, np.stack(line), seg, nlags, ref, RECT, 0, frames, pad)
    sc = M.scale_of(seg, nd, RECT)
    for d, wr, wi in ((0, sr, si), (nd // 2, ar, ai)):
        got = out["chi"][0][:, d, :].astype(np.complex128)
        for g, s in ((got.real, wr), (got.imag, wi)):
            exact = s.astype(np.float64) * sc
            assert np.all(np.abs(g - exact) <= 2.0 * M.U * (1.0 + M.U) * np.abs(exact)), (d, np.max(np.abs(g - exact) / np.maximum(np.abs(exact), 1e-300)))


# (name, nrows, B, frames, seg, R, ref, window, guard, K, P): k_caf<LG, 1> and k_caf<LG, 2> where test_gpu_caf_cancel.py (nd 8, 16, 32 and
# 4096: T = 16 and 1) does not run them.  The taps crossing a tile: MODE 1's Y [nd][taps] store at lag0 > 0 with the `tile != 0` return in
# front of the energy tree, and MODE 2's G [nd][taps][nlags] reads at lag0 > 0.
CANCEL_CASES = [
    ("T 16 at nd 128", 3, 1024, 4, 16, 16, 1, HANN, 1, 5, 1),                    # one tile, above nd 32
    ("K 9 over tiles of 8", 3, 4096, 8, 32, 21, 2, RECT, 0, 9, 0),               # nd 512
    ("K 5 over tiles of 4", 2, 8192, 8, 32, 11, 0, HANN, 2, 5, 1),               # nd 1024
    ("K 3 over tiles of 2", 2, 8192, 8, 16, 5, 1, HANN, 1, 3, 1),                # nd 2048
    # the two nd left at which no test holds the canceller's passes against the model (nd 64 runs only in the end-to-end scenes)
    ("nd 64, three Doppler offsets", 3, 1024, 2, 16, 16, 0, RECT, 1, 4, 2), ("nd 256, a tail of 12", 2, 4096, 2, 16, 12, 1, HANN, 2, 6, 0),
]


def _scene(case):
    """the recipe of test_gpu_caf_cancel.test_against_the_model"""
    name, nrows, B, frames, seg, R, ref, kind, guard, K, P = case
    return M.echo_scene(B, frames, [(c, 3 % R, 2, 0.2) for c in range(nrows) if c != ref], nrows=nrows, ref=ref, seed=len(name))


@pytest.mark.parametrize("case", CANCEL_CASES, ids=[c[0] for c in CANCEL_CASES])
def test_the_canceller_against_the_model(b, torch, case):
    name, nrows, B, frames, seg, R, ref, kind, guard, K, P = case
    line = _scene(case)
    out = _engine(b, torch, np.stack(line), seg, R, ref, kind, guard, frames, K, P)
    got = tuple(out[k][0] for k in KEYS)
    r = _hold(got, line, seg, R, ref, kind, guard, K, P, name)
    others = [c for c in range(nrows) if c != ref]
    assert np.all(r["share"][others] < 0.5)                                      # the direct path went, so the check is of a cancelled row
    # row r is bit for bit the canceller-off submit's of the same packets, every other row is not
    off = _run(b, torch, np.stack(line), seg, R, ref, kind, guard, frames)["chi"][0]
    assert np.array_equal(_bits(off[ref]), _bits(got[0][ref])) and not any(np.array_equal(_bits(off[c]), _bits(got[0][c])) for c in others)


def test_a_cancelled_line_at_tiles_of_8_has_its_bits_anywhere(b, torch):
    """a line alone, and at positions 0 and 3 of a batch of four lines (32 packets) at a padded stride"""
    name, nrows, B, frames, seg, R, ref, kind, guard, K, P = CANCEL_CASES[1]
    blocks = np.concatenate([np.stack(M.echo_scene(B, frames, [(0, 6, 3, 0.2)], nrows=nrows, ref=ref, seed=700 + e)) for e in range(4)])
    blocks[3 * frames:] = blocks[:frames]
    alone = _engine(b, torch, blocks[:frames], seg, R, ref, kind, guard, frames, K, P, max_batch=4 * frames)
    batch = _engine(b, torch, blocks, seg, R, ref, kind, guard, frames, K, P, pad=40)
    assert _same_line(alone, 0, batch, 0) and _same_line(alone, 0, batch, 3) and not _same_line(alone, 0, batch, 1)
    _hold(tuple(batch[k][2] for k in KEYS), list(blocks[2 * frames:3 * frames]), seg, R, ref, kind, guard, K, P, "line 2 of 4")
