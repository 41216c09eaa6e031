"""Inputs and bars shared by the CPU and the device tests of the reference-noise canceller (tests/refcancel_model.py is the definition).

A per-op case is one block: row 0 band-limited noise, one signal row per lag of LAGS (the row carries the noise so that its shifted
form lines up with row 0, plus receiver noise), and a full-scale row (every byte 127 or -128) that drives the output into the clamp.

Bars of check_block (got = what a device, or a mutated model, answered; want = cancel_block of the model):
  coefficients  max |g_got - g_model| <= 2^-23 max|g_model| + 1e-12 cond(G) max|g_model|   (the rounding to fp32 + the fp64 solve)
  residual      |got - model| <= 2^-23 model + 1e-9
  status        exact
  bytes         |out - clip(w64, -128, 127)| - 0.5 <= 4 e_ref for every byte, w64 the fp64 output sample from the answer's OWN published
                coefficients and the given phasor, e_ref = reference_excess(): the largest such excess of the float32 restatement
                (refcancel_model.output32: one rounding per operation) over every row of every case of the family, floored at the
                rounding of one fp32 operation on a full-scale sample (2^-24 * 256): a restatement that happens to cross no tie has a
                negative excess, which says nothing about the arithmetic's error.
"""
import functools

import numpy as np

import refcancel_model as M

BLOCKSIZES = (64, 256, 4096, 16384)
TAPS = (1, 3, 9)
EXCESS_FLOOR = 2.0 ** -24 * 256.0
MARGIN = 4.0


def lags(L):
    return (-L, -L + 1, -3, -1, 0, 1, 2, L - 1)


@functools.lru_cache(maxsize=None)
def perop_case(B, seed=5):
    """(block int8 [10][B] signed, lag int32 [10], phasor complex64 [10])"""
    L = B // 2
    lg = lags(L)
    scene, _ = M.noise_scene(seed + B, L, 0.5, nsig=len(lg))
    rng = np.random.default_rng(seed)
    block = np.zeros((len(lg) + 2, B), dtype=np.int8)
    block[0] = scene[0]
    for k, d in enumerate(lg):                                   # s = the scene's row moved so that s[n + d] lines up again
        si, sq = M.to_ints(scene[1 + k])
        s = M.shift(si + 1j * sq, -d)
        block[1 + k] = M.to_i8(s)
    block[-1] = np.where(rng.random(B) < 0.5, 127, -128).astype(np.int8)
    lag = np.array((0,) + lg + (0,), dtype=np.int32)
    ph = (0.95 * np.exp(2j * np.pi * rng.random(len(lg) + 2))).astype(np.complex64)
    ph[0] = 0
    block.setflags(write=False)
    return block, lag, ph


@functools.lru_cache(maxsize=None)
def perop_model(B, taps):
    block, lag, ph = perop_case(B)
    return M.cancel_block(block, lag, ph, taps)


def failure_case(kind, B=256):
    """(block, lag, phasor): the reference row all zero ("zero"), or nonzero in its first sample alone ("single": r_{-1} is then the zero
    row and the Gram rank-deficient), or constant ("constant": with the zero-filled edges its Gram is full rank, badly conditioned)."""
    block, lag, ph = perop_case(B)
    block = block.copy()
    block[0] = 0
    if kind == "single":
        block[0, :2] = (90, -35)
    elif kind == "constant":
        block[0, 0::2], block[0, 1::2] = 57, -21
    return block, lag, ph


class ArrayScene:
    """The 7 x 3 array (tests/ura.py steering) with its calibration noise ON: every signal row c is
        delay_{d_c + D_c}(emitter * a_c + 0.7 * noise) * e^{j phi_c} + receiver noise (sigma 4 per component)
    with a 0.1-band emitter (sigma 10) from (alpha, beta), 0.8-band noise (sigma 25), d_c in -3 .. 3, |D_c| <= 0.5, all fixed over the
    blocks; row 0 is the noise alone."""

    def __init__(self, seed, L, alpha=33 * np.pi / 100, beta=39 * np.pi / 100, m=21):
        import ura
        self.rng = np.random.default_rng(seed)
        self.L, self.m = L, m
        self.a = ura.steering(alpha, beta)[:m]
        self.d = self.rng.integers(-3, 4, m)
        self.D = self.rng.uniform(-0.5, 0.5, m)
        self.phi = self.rng.uniform(-np.pi, np.pi, m)

    def block(self):
        rng, L = self.rng, self.L
        nz = M.band_noise(rng, L, 0.8, 25.0)
        em = M.band_noise(rng, L, 0.1, 10.0)
        blk = np.zeros((self.m + 1, 2 * L), dtype=np.int8)
        blk[0] = M.to_i8(nz)
        for c in range(self.m):
            x = M.delay(em * self.a[c] + 0.7 * nz, self.d[c] + self.D[c]) * np.exp(1j * self.phi[c])
            x = x + 4.0 * (rng.standard_normal(L) + 1j * rng.standard_normal(L))
            blk[1 + c] = M.to_i8(x)
        return blk

    def blocks(self, n):
        return np.stack([self.block() for _ in range(n)])


def restated_excess(block, lag, ph, taps, coef):
    """largest excess of the float32 restatement over the signal rows of one block, against fp64 on the same coefficients"""
    K = (taps - 1) // 2
    worst = -1.0
    for r in range(1, block.shape[0]):
        y, R = M.row_parts(block, r, int(lag[r]), K)
        worst = max(worst, M.excess(M.quantise(M.output32(y, R, coef[r], ph[r])), M.output64(y, R, coef[r], ph[r])))
    return worst


@functools.lru_cache(maxsize=None)
def reference_excess():
    """e_ref of the family: every per-op case, with the model's published coefficients"""
    worst = EXCESS_FLOOR
    for B in BLOCKSIZES:
        for taps in TAPS:
            block, lag, ph = perop_case(B)
            worst = max(worst, restated_excess(block, lag, ph, taps, perop_model(B, taps)["coef"]))
    return worst


def device_excess(block, lag, ph, taps, got):
    """per signal row: the excess of the answer's bytes against fp64 on its own published coefficients"""
    K = (taps - 1) // 2
    ex = np.zeros(block.shape[0])
    for r in range(1, block.shape[0]):
        y, R = M.row_parts(block, r, int(lag[r]), K)
        ex[r] = M.excess(got["out"][r], M.output64(y, R, got["coef"][r], ph[r]))
    return ex


def check_block(block, lag, ph, taps, got, want, tag=""):
    """Every bar of the module docstring; returns the list of misses (empty: the answer passes)."""
    miss = []
    if not np.array_equal(got["status"], want["status"]):
        miss.append(f"{tag} status {got['status']} != {want['status']}")
    if not np.array_equal(got["out"][0], block[0]):
        miss.append(f"{tag} row 0 is not the reference row")
    for r in range(1, block.shape[0]):
        gm = np.abs(want["g64"][r]).max()
        cond = want["cond"][r] if np.isfinite(want["cond"][r]) else 0.0
        bar = 2.0 ** -23 * gm + 1e-12 * cond * gm
        err = np.abs(got["coef"][r].astype(np.complex128) - want["g64"][r]).max()
        if not err <= bar:
            miss.append(f"{tag} row {r}: coefficients off by {err:.3g}, bar {bar:.3g} (cond {cond:.3g})")
        rw = float(want["residual"][r])
        if not abs(float(got["residual"][r]) - rw) <= 2.0 ** -23 * rw + 1e-9:
            miss.append(f"{tag} row {r}: residual {got['residual'][r]!r} against {rw!r}")
    ex = device_excess(block, lag, ph, taps, got)
    bar = MARGIN * reference_excess()
    for r in np.flatnonzero(ex > bar):
        miss.append(f"{tag} row {r}: byte excess {ex[r]:.4g} over the bar {bar:.4g}")
    return miss
