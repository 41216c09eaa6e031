"""The beamformer chain on the device against the fp64 model of tests/music_model.py, at the array shapes, scan grids and spectra the
other GPU modules do not reach: crsdr_noisesubspace at every m from 2 to 64 on five spectrum families, crsdr_pmusic2d point by point
against the fp64 scan and its derived error bound, crsdr_doa end to end against exact covariances and fp64 rather than against the per-op
chain (both are the same device functions), and the covariance shapes no other test launches.

Every bar is derived in music_model's docstring; tests/test_music_model.py shows on the CPU that the C oracle meets them and that a
scan with a wrong element order, grid decomposition, column offset or sign does not.  Each test prints the device's worst fraction of
each bar."""
import importlib

import numpy as np
import pytest

import music_model as mm
import ura
from music_model import SCAN_CASES, case_id

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


def _report(title, worst):
    print(f"{title}: worst fraction of the bar " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))


def _check_subspace(b, R, gaps, label, worst, failures):
    try:
        vec, sv = b.noisesubspace(R)                                     # CRSDR_ESTATE (not converged in 30 sweeps) raises
    except b.CrsdrError as e:
        failures.append((label, f"error {e.code}: {e}"))
        return
    for key, v in mm.subspace_fractions(R, vec, sv, gaps).items():
        worst[key] = max(worst.get(key, 0.0), v)
        if not v <= 1.0:
            failures.append((label, key, v))


# ---- subspace ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", mm.FAMILIES)
def test_subspace_at_every_size(b, name):
    # every m: odd sizes seat a dummy player in the tournament, m <= 32 leaves pairs idle, m = 64 fills the LDS.  The families are the
    # spectra MUSIC meets: strong eigenvalues over a clustered floor, six decades of range, exact rank deficiency, plateaus
    worst, failures = {}, []
    for m in range(2, 65):
        R, gaps = mm.family(m, name)
        _check_subspace(b, R, gaps, f"{name} m={m}", worst, failures)
    _report(f"device subspace, {name}, m = 2..64", worst)
    assert not failures, failures


def test_subspace_of_rank_one_and_zero_matrices(b):
    worst, failures = {}, []
    for m in range(2, 65):
        a = ura.steering(0.7, 1.9, mx=m, my=1)
        _check_subspace(b, mm.hermitian32(np.outer(a, a.conj())), [1], f"rank one m={m}", worst, failures)
        vec, sv = b.noisesubspace(np.zeros((m, m), dtype=np.complex64))
        if not (np.all(sv == 0) and np.abs(vec.conj().T @ vec - np.eye(m)).max() <= 2.0 ** -22):
            failures.append((f"zero m={m}", float(np.abs(sv).max())))
    _report("device subspace, rank one from a steering vector, m = 2..64", worst)
    assert not failures, failures


# ---- scan --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", SCAN_CASES, ids=case_id)
def test_scan_against_fp64_at_every_point(b, oracle, c):
    mx, my, k, ncx, ncy = c["mx"], c["my"], c["k"], c["ncx"], c["ncy"]
    m = mx * my
    R = mm.hermitian32(mm.rxx_reference(mm.case_scene(c)[0]))
    vec, _ = b.noisesubspace(R)
    den, bound = mm.scan(vec, k, ura.D, mx, my, ncx, ncy)
    pm = b.pmusic2d(vec, k, ura.D, mx, my, ncx, ncy)
    assert pm.shape == (ncx, ncy)
    worst, median = mm.scan_fractions(pm, m, den, bound)
    o_worst, o_median = mm.scan_fractions(oracle.pmusic2d(vec, k, ura.D, mx, my, ncx, ncy), m, den, bound)
    print(f"device scan {case_id(c)}: worst fraction of the bound {worst:.3f} (oracle {o_worst:.3f}), median |d den| / den {median:.2e} "
          f"(oracle {o_median:.2e}, ratio {median / o_median:.2f})")
    assert worst <= 1.0                                                  # every point, peaks and infs included
    # what a worst-case bound cannot see: an error that is systematic but small.  A different sincosf, fused multiply-adds and another
    # summation order may cost a factor; four times the typical error of the reference's own fp32 arithmetic on the same vec is the bar
    assert median <= 4.0 * o_median
    peak = np.unravel_index(np.argmax(pm), pm.shape)
    assert mm.admissible_peak(den, bound, peak)
    certain = mm.certain_peak(den, bound)
    if certain is not None:
        assert tuple(int(v) for v in peak) == certain
    if c["find"]:
        assert tuple(int(v) for v in np.unravel_index(np.argmin(den), den.shape)) in c["src"]


# ---- crsdr_doa end to end ----------------------------------------------------------------------------------------------------------

class _Packets:
    """nblocks packet-shaped slots on the device as a plan lays them out: packet t at ptr + t * stride, its matrix [nrows][B] at
    + 16 + 4 nrows (4-byte aligned only), headers and gaps holding something that is not zero."""

    def __init__(self, torch, blocks):
        blocks = np.ascontiguousarray(blocks)
        self.T, nrows, B = blocks.shape
        self.offset = 16 + 4 * nrows
        self.stride = self.offset + nrows * B + 64
        host = np.full((self.T, self.stride), 0x55, dtype=np.int8)
        host[:, self.offset: self.offset + nrows * B] = blocks.reshape(self.T, -1)
        self.buf = torch.from_numpy(host).to(torch.device("cuda", 0))
        self.ptr = self.buf.data_ptr()


_DOA_GRIDS = {(2, 1): (24, 36), (3, 7): (33, 17), (11, 3): (30, 20), (16, 4): (24, 36), (8, 8): (33, 17), (64, 1): (30, 20)}


@pytest.mark.parametrize("frames", [1, 4])
@pytest.mark.parametrize("mx,my,k", [(mx, my, k) for mx, my in _DOA_GRIDS for k in (1, 3) if k < mx * my])
def test_doa_end_to_end_against_fp64(b, torch, mx, my, k, frames):
    m = mx * my
    ncx, ncy = _DOA_GRIDS[(mx, my)]                                      # none a multiple of 64 points: the last workgroup is ragged
    assert ncx != ncy and (ncx * ncy) % 64
    c = mm.scan_case(mx, my, k, ncx, ncy)
    nest, L = 2, 1024
    blocks = np.concatenate([mm.case_scene(c, L=L, frames=frames, seed=e) for e in range(nest)])
    pk = _Packets(torch, blocks)
    doa = b.Doa(m + 1, 2 * L, k, ura.D, mx, my, ncx, ncy, max_batch=nest * frames, frames=frames,
                flags=b.DOA_KEEP_SPECTRUM | b.DOA_KEEP_RXX)
    doa.submit(pk.ptr, pk.stride, pk.offset, nest * frames)
    out = doa.fetch()
    vecs = doa.fetch_subspace()
    doa.close()
    assert out["rxx"].shape == (nest, m, m) and out["pm"].shape == (nest, ncx, ncy) and vecs.shape == (nest, m, m)
    worst, sure = {}, 0
    for e in range(nest):
        assert out["status"][e] == 0
        rxx = out["rxx"][e]
        ref = mm.rxx_reference_frames(blocks[e * frames: (e + 1) * frames])
        assert np.abs(rxx - ref).max() <= 2e-7 * np.abs(ref).max()       # exact integer sums, one fp32 rounding
        assert np.array_equal(rxx, rxx.conj().T)
        fr = mm.subspace_fractions(rxx, vecs[e], out["sv"][e])
        den, bound = mm.scan(vecs[e], k, ura.D, mx, my, ncx, ncy)
        fr["scan"], _ = mm.scan_fractions(out["pm"][e], m, den, bound)
        for key, v in fr.items():
            worst[key] = max(worst.get(key, 0.0), v)
        assert fr["sv"] <= 1.0 and fr["orth"] <= 1.0 and fr["resid"] <= 1.0, fr
        assert fr["scan"] <= 1.0, fr
        peak = tuple(int(v) for v in out["peak"][e])
        assert mm.admissible_peak(den, bound, peak)
        assert out["peak_value"][e] == out["pm"][e][peak]
        certain = mm.certain_peak(den, bound)                            # the source's own grid point wherever the model is sure of it
        if certain is not None:
            assert peak == certain
        # several sources of one strength: which of them is strongest may be inside the bound, that it is one of them is not
        # (a line array along x sees sin(beta) only: the point mirrored in beta has the same steering vector, an exact tie)
        allowed = list(c["src"]) + [(cx, ncy - cy) for cx, cy in c["src"] if my == 1 and 0 < cy < ncy]
        elsewhere = den - bound
        elsewhere[tuple(zip(*allowed))] = np.inf
        if min((den + bound)[p] for p in allowed) < elsewhere.min():
            assert peak in allowed
            sure += 1
    _report(f"doa {mx}x{my} k={k} F={frames} grid {ncx}x{ncy} ({sure} of {nest} peaks pinned to the sources by the model)", worst)


@pytest.mark.parametrize("B", [65536, 66048])
@pytest.mark.parametrize("mx,my", [(11, 3), (8, 8)])
def test_doa_covariance_at_the_int32_bound(b, torch, mx, my, B):
    # k_doa_cov keeps a K slice's sums in int32: one slice of exactly 65536 bytes (a full-scale row sums to 2^30 there), two slices
    # just above; m = 33 has one live row in its second 32-row operand block, m = 64 fills both
    m = mx * my
    rng = np.random.default_rng(m + B)
    blocks = rng.integers(-128, 128, size=(2, m + 1, B), dtype=np.int8)
    blocks[:, 1] = -128
    blocks[:, 2, 0::2], blocks[:, 2, 1::2] = 127, -128
    blocks[1, m] = -128                                                  # the last live row too
    pk = _Packets(torch, blocks)
    doa = b.Doa(m + 1, B, 1, ura.D, mx, my, 5, 7, max_batch=2, flags=b.DOA_KEEP_SPECTRUM | b.DOA_KEEP_RXX)
    doa.submit(pk.ptr, pk.stride, pk.offset, 2)
    out = doa.fetch()
    doa.close()
    for e in range(2):
        ref = mm.rxx_reference(blocks[e])
        assert np.abs(out["rxx"][e] - ref).max() <= 2e-7 * np.abs(ref).max()
        assert np.array_equal(out["rxx"][e], out["rxx"][e].conj().T)
        assert out["status"][e] == 0
        assert mm.sv_fraction(out["sv"][e], mm.eigh_by_magnitude(out["rxx"][e])[0]) <= 1.0


# ---- covariance shapes -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B", [96, 8224, 65536])
@pytest.mark.parametrize("nsig", [33, 63, 65, 100, 130])
def test_covariance_shapes_nobody_runs(b, torch, nsig, B):
    # B % 512 != 0, or fewer than 64 channels, takes k_covariance (one 64 x 64 tile per workgroup): grids of one to nine workgroups,
    # mirror stores from the tiles above the diagonal, padded tiles (33, 65, 100, 130).  B = 65536 is the longest row whose int32 sums
    # are exact (2^30 for the full-scale rows); from 64 channels on it runs the LDS-tiled kernel at ragged channel counts
    rng = np.random.default_rng(nsig * 11 + B)
    rows = rng.integers(-128, 128, size=(nsig + 1, B), dtype=np.int8)
    rows[3] = -128
    rows[nsig, 0::2], rows[nsig, 1::2] = 127, -128                       # the last row: in the padded tile wherever there is one
    rxx = b.covariance(rows)
    ref = mm.rxx_reference(rows)
    assert rxx.shape == ref.shape
    assert np.abs(rxx - ref).max() <= 2e-7 * np.abs(ref).max()
    assert np.array_equal(rxx, rxx.conj().T)
    dev = torch.device("cuda", 0)
    off = 16 + 4 * (nsig + 1)                                            # where a packet holds the matrix: 4-byte aligned only
    off += 4 if off % 16 == 0 else 0
    buf = torch.zeros(off + rows.size + 256, dtype=torch.int8, device=dev)
    buf[off: off + rows.size].copy_(torch.from_numpy(rows.reshape(-1)))
    out = torch.zeros((nsig, nsig, 2), dtype=torch.float32, device=dev)
    assert (buf.data_ptr() + off) % 16 != 0 and (buf.data_ptr() + off) % 4 == 0
    b.covariance_device(out.data_ptr(), buf.data_ptr() + off, nsig + 1, B)
    got = out.cpu().numpy().view(np.complex64).reshape(nsig, nsig)
    assert np.array_equal(got, rxx)
