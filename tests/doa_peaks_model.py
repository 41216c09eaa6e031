"""Test helper: a numpy restatement of crsdr_doa_set_peaks / crsdr_doa_fetch_directions (include/crsdr.h (iv)), from the definition
alone: no tiles, no separable maximum, every window position compared.

Grid point g = cx * ncy + cy of a spectrum pm [ncx][ncy] has the key (bits(pm) << 32) | (0xFFFFFFFF - g), bits = the float32's bit
pattern with a NaN canonicalised to 0x7FC00000.  It is a local peak if its key is strictly larger than the key of every other grid point
(cx', cy') with |cx' - cx| <= r and |cy' - cy| <= r, the window clipped at the grid's edges (no wrap-around).  The result is the `count`
largest local peaks in descending key order; the slots after the last one hold (-1, -1) and -1.0."""
import numpy as np

_LOW = np.uint64(0xFFFFFFFF)


def keys(pm):
    """uint64 keys [ncx][ncy] of one spectrum."""
    pm = np.ascontiguousarray(pm, dtype=np.float32)
    bits = pm.view(np.uint32).astype(np.uint64)
    bits[np.isnan(pm)] = 0x7FC00000
    g = np.arange(pm.size, dtype=np.uint64).reshape(pm.shape)
    return (bits << np.uint64(32)) | (_LOW - g)


def is_local_peak(pm, radius):
    """bool [ncx][ncy]: the key beats every other key of its clipped window."""
    k = keys(pm)
    ncx, ncy = k.shape
    r = int(radius)
    pad = np.zeros((ncx + 2 * r, ncy + 2 * r), dtype=np.uint64)      # 0: no grid point there (every real key is above 0)
    pad[r:r + ncx, r:r + ncy] = k
    peak = np.ones(k.shape, dtype=bool)
    for dx in range(-r, r + 1):
        for dy in range(-r, r + 1):
            if dx or dy:
                peak &= k > pad[r + dx:r + dx + ncx, r + dy:r + dy + ncy]
    return peak


def directions(pm, count, radius):
    """found, peaks [count][2] int32 (cx, cy), values [count] float32 of one spectrum."""
    ncy = pm.shape[1]
    k = np.sort(keys(pm)[is_local_peak(pm, radius)])[::-1][:count]
    n = len(k)
    peaks = np.full((count, 2), -1, dtype=np.int32)
    values = np.full(count, -1.0, dtype=np.float32)
    g = (_LOW - (k & _LOW)).astype(np.int64)
    peaks[:n, 0], peaks[:n, 1] = g // ncy, g % ncy
    values[:n] = (k >> np.uint64(32)).astype(np.uint32).view(np.float32)
    return n, peaks, values


def batch_directions(pm, count, radius):
    """{"found" [nest], "peaks" [nest][count][2], "values" [nest][count]} of spectra pm [nest][ncx][ncy], as Doa.fetch_directions."""
    res = [directions(p, count, radius) for p in pm]
    return {"found": np.array([r[0] for r in res], dtype=np.int32), "peaks": np.stack([r[1] for r in res]),
            "values": np.stack([r[2] for r in res])}
