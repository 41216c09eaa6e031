"""Exact model of the digital-mode phase path (K2) -- TEST INFRASTRUCTURE ONLY.

Plain numpy, no FFT: the four steps as the kernels of csrc/kernels.hpp define them, GIVEN the lag (the lag itself is K1's, pinned
by tests/test_gpu_peak.py).  Every step is either integer arithmetic or a fixed sequence of IEEE operations that round once, so a
device result is compared with this model bit for bit and byte for byte (tests/test_gpu_phase_path.py):

  shift    y[n] = s[n + d] for 0 <= n + d < L, zero elsewhere; d any integer in [-L, L - 1]          (shifted_word / shifted_vec)
  dot      sr = sum(yI rI + yQ rQ), si = sum(yQ rI - yI rQ) over signed int8 values, in int64          (dot_word3, k_phase_dot)
  unit     sr == si == 0: hold.  Else in float64 inv = 1 / sqrt(cr cr + ci ci), u = (float32(cr inv), float32(-ci inv))
                                                                                                       (unit_bits, k_phase_chain)
  chain    p <- (0.5f u.x + 0.5f p.x, 0.5f u.y + 0.5f p.y), each product and sum one float32 rounding, in block order, carried
           across submits, from (1, 0); frozen while the reference noise is off
  rotate   x = int8 * (1.0f / 127.0f); (I px - Q py, Q px + I py): four products and two sums, each rounded once; * 127.0f;
           round half to even; clamp to [-128, 127]                                                    (rotq_word)
  header   hdr0 {seq, nrows, L, 0}, the readcnt words (seq where none are given), row 0 = the reference row verbatim

Offset-binary input is `^ 0x80` first.  numpy's float32 array operations round once per operation (no contraction), which is what
the device code does under -ffp-contract=off.
"""
from __future__ import annotations

import math

import numpy as np

F32 = np.float32
INV127 = F32(1.0) / F32(127.0)          # the kernels' constant 1.0f / 127.0f: one float32 rounding of 1 / 127


def to_signed(rows: np.ndarray, offset_binary: bool = False) -> np.ndarray:
    """int8 view of the input bytes; offset binary (raw librtlsdr uint8) is ^ 0x80 first."""
    u = np.ascontiguousarray(rows).view(np.uint8)
    if offset_binary:
        u = u ^ np.uint8(0x80)
    return u.view(np.int8)


def shift_row(row: np.ndarray, d: int) -> np.ndarray:
    """One int8 row [2 L] of interleaved (I, Q) shifted by d complex samples: y[n] = s[n + d], zero outside [0, L)."""
    L = row.size // 2
    d = int(d)
    if not -L <= d <= L - 1:
        raise ValueError(f"shift {d} outside [-L, L - 1] for L = {L}")
    s = row.reshape(L, 2)
    y = np.zeros_like(s)
    lo, hi = max(0, -d), min(L, L - d)
    if hi > lo:
        y[lo:hi] = s[lo + d:hi + d]
    return y.reshape(-1)


def dot_sums(y: np.ndarray, r: np.ndarray):
    """(sr, si) = sum y conj(r) over signed int8 samples, exact (Python ints from int64 sums)."""
    yI, yQ = y[0::2].astype(np.int64), y[1::2].astype(np.int64)
    rI, rQ = r[0::2].astype(np.int64), r[1::2].astype(np.int64)
    return int(np.sum(yI * rI + yQ * rQ)), int(np.sum(yQ * rI - yI * rQ))


def unit_phasor(sr: int, si: int):
    """conj(corr) / |corr| from the integer sums, in the kernels' operation order; None = "|corr| == 0, hold"."""
    if sr == 0 and si == 0:
        return None
    cr, ci = float(sr), float(si)                        # int64 -> float64, round to nearest even (|sums| < 2^53 here: exact)
    inv = 1.0 / math.sqrt(cr * cr + ci * ci)             # three roundings, a correctly rounded sqrt and a correctly rounded divide
    return F32(cr * inv), F32(-ci * inv)                 # float64 product, then one rounding to float32


def ema(p, u):
    """One step of the alpha = 0.5 chain on float32 pairs: (0.5f u + 0.5f p) per component."""
    h = F32(0.5)
    return F32(F32(h * F32(u[0])) + F32(h * F32(p[0]))), F32(F32(h * F32(u[1])) + F32(h * F32(p[1])))


def rotate_quantise(y: np.ndarray, p) -> np.ndarray:
    """rotq_word on a whole int8 row (or rows, along the last axis): the float32 operations of csdrdevice::phasecorrect and
    cdsp::convto8bit in the oracle's order."""
    px, py = F32(p[0]), F32(p[1])
    xI = y[..., 0::2].astype(F32) * INV127
    xQ = y[..., 1::2].astype(F32) * INV127
    re = (xI * px - xQ * py) * F32(127.0)                # every * and -/+ is its own float32 array operation: one rounding each
    im = (xQ * px + xI * py) * F32(127.0)
    out = np.empty(y.shape, dtype=np.int8)
    out[..., 0::2] = np.clip(np.rint(re), -128.0, 127.0).astype(np.int8)
    out[..., 1::2] = np.clip(np.rint(im), -128.0, 127.0).astype(np.int8)
    return out


def phasor_bits(p) -> np.ndarray:
    """uint32 [.., 2] view of complex64 phasors (or float32 pairs): what "bit for bit" compares."""
    a = np.ascontiguousarray(p)
    if a.dtype == np.complex64:
        return a.view(np.uint32).reshape(a.shape + (2,))
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


class PhasePathModel:
    """Stateful model of one plan's phase path: the EMA phasor and the lag of every row, carried from block to block."""

    def __init__(self, nrows: int, B: int, digital: bool = True):
        self.nrows, self.B, self.L, self.digital = nrows, B, B // 2, digital
        self.matrix_offset = 16 + 4 * nrows
        self.packet_bytes = self.matrix_offset + nrows * B
        self.p = np.zeros((nrows, 2), dtype=F32)
        self.p[:, 0] = 1.0
        self.lag = np.zeros(nrows, dtype=np.int64)

    def block(self, rows, lag=None, refnoise: bool = True, offset_binary: bool = False, seq: int = 0, readcnt=None, phasor=None):
        """One block.  lag [nrows]: the lags K1 reported for this block (None: a locked block, the carried lags shift).
        phasor [nrows] complex64: rotate by these instead of the model's own chain (the device's phasor bits given).
        Returns {phasor complex64 [nrows] (row 0: 0), matrix int8 [nrows][B], packet int8, sums [(sr, si)] per row}."""
        rows = to_signed(np.asarray(rows).reshape(self.nrows, self.B), offset_binary)
        if lag is not None:
            self.lag[:] = np.asarray(lag, dtype=np.int64)
        ref = rows[0]
        matrix = np.empty((self.nrows, self.B), dtype=np.int8)
        matrix[0] = ref
        sums = [(0, 0)]
        for r in range(1, self.nrows):
            y = shift_row(rows[r], self.lag[r]) if self.digital else rows[r]
            s = dot_sums(y, ref)
            sums.append(s)
            if refnoise:
                u = unit_phasor(*s)
                if u is not None:
                    self.p[r] = ema(self.p[r], u)
            prot = self.p[r] if phasor is None else (np.complex64(phasor[r]).real, np.complex64(phasor[r]).imag)
            matrix[r] = rotate_quantise(y, prot)
        ph = self.p.copy().view(np.complex64).reshape(self.nrows)
        ph[0] = 0
        hdr = np.empty(4 + self.nrows, dtype=np.uint32)
        hdr[:4] = (seq & 0xFFFFFFFF, self.nrows, self.L, 0)
        hdr[4:] = (seq & 0xFFFFFFFF) if readcnt is None else np.asarray(readcnt, dtype=np.uint32)
        packet = np.concatenate([hdr.view(np.int8), matrix.reshape(-1)])
        return dict(phasor=ph, matrix=matrix, packet=packet, sums=sums, lag=self.lag.copy())
