"""Unrounded fp64 model of the fractional-delay correction (crsdr_plan_set_frac_apply) -- TEST INFRASTRUCTURE ONLY
(tests/test_frac_delay_model.py, tests/test_gpu_frac_edges.py).

The definition oracle/model_fp64.py and oracle/coherent_oracle.c share, BEFORE rint / clip, in int8 counts: row k of the matrix is

    z = p * ifft(fft(pad_2L(I + jQ)) * exp(2j pi f_s (lag + D) / (2L)))[:L],     f_s = 0 .. L-1, -L .. -1 (the signed bin index)

-- a circular advance of the zero-padded row by lag + D samples over 2L (|lag + D| > L wraps: samples re-enter from the other end),
rotated by the phasor.  The 1 / 127 of convtofloat and the x 127 of convto8bit cancel.  The lag, the phasor (complex64, as fetched)
and D are INPUTS, so the kernels that form the response are judged on their own: a device result is held to this value per sample
(excess), not to another rounded matrix.
"""
from __future__ import annotations

from concurrent.futures import ThreadPoolExecutor

import numpy as np


def delay_of(gain, frac) -> np.ndarray:
    """D of the estimate-driven correction: the single fp32 product gain * frac the kernels (and the C oracle) form."""
    return (np.float32(gain) * np.asarray(frac, dtype=np.float32)).astype(np.float32)


def unrounded(rows_i8_signed, lag, D, phasor, chunk: int = 16) -> np.ndarray:
    """complex128 [nrows][L] for signed int8 rows [nrows][2 L] of interleaved (I, Q); lag, D, phasor: one per row."""
    rows = np.asarray(rows_i8_signed)
    assert rows.dtype == np.int8 and rows.ndim == 2
    n, B = rows.shape
    L = B // 2
    lg = np.asarray(lag, dtype=np.float64).reshape(n)
    Dd = np.asarray(D, dtype=np.float32).astype(np.float64).reshape(n)
    p = np.asarray(phasor, dtype=np.complex64).astype(np.complex128).reshape(n)
    fs = np.fft.fftfreq(B, d=1.0 / B)                                   # 0 .. L-1, -L .. -1
    out = np.empty((n, L), dtype=np.complex128)

    def part(r0):
        r1 = min(n, r0 + chunk)
        a = np.zeros((r1 - r0, B), dtype=np.complex128)
        a[:, :L] = rows[r0:r1, 0::2].astype(np.float64) + 1j * rows[r0:r1, 1::2].astype(np.float64)
        # f_s lag is an integer (exact in float64) and is reduced mod B before the exponential: the argument keeps its precision at |lag| ~ L
        rev = (np.mod(fs[None, :] * lg[r0:r1, None], float(B)) + fs[None, :] * Dd[r0:r1, None]) / B
        out[r0:r1] = p[r0:r1, None] * np.fft.ifft(np.fft.fft(a, axis=1) * np.exp(2j * np.pi * rev), axis=1)[:, :L]

    if n * B >= 1 << 21:                                                # long rows: the chunks on a few threads (numpy's FFT releases the GIL)
        chunk = max(1, min(chunk, (1 << 19) // B))
        with ThreadPoolExecutor(max_workers=8) as pool:
            list(pool.map(part, range(0, n, chunk)))
    else:
        for r0 in range(0, n, chunk):
            part(r0)
    return out


def _flat(z) -> np.ndarray:
    q = np.empty(z.shape[:-1] + (2 * z.shape[-1],), dtype=np.float64)
    q[..., 0::2], q[..., 1::2] = z.real, z.imag
    return q


def quantised(z) -> np.ndarray:
    """int8 [..][2 L]: cdsp::convto8bit of the unrounded value (clamp, round half to even)."""
    return np.rint(np.clip(_flat(z), -128.0, 127.0)).astype(np.int8)


def excess_rows(q_i8, z) -> np.ndarray:
    """float64 [nrows]: per row, the largest |q - clip(z, -128, 127)| - 0.5 over the I and Q of every sample."""
    q = np.asarray(q_i8)
    assert q.dtype == np.int8 and q.shape == z.shape[:-1] + (2 * z.shape[-1],), (q.dtype, q.shape, z.shape)
    return np.abs(q.astype(np.float64) - np.clip(_flat(z), -128.0, 127.0)).max(axis=-1) - 0.5


def excess(q_i8, z) -> float:
    """Largest |q - clip(z, -128, 127)| - 0.5 over every entry: <= 0 for a correctly rounded matrix, 0 at a tie, many counts for a
    sample that is wrong by one position, sign or bin."""
    return float(np.max(excess_rows(q_i8, z)))
