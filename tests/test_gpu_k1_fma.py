"""K1's FMA-form transforms (csrc/cpk.hpp fnet, csrc/xcorr14p.hpp dft32s / dft32s_pruned / tw_dft32_inv<true>).

  (a) tools/fma_bfly_check.hip: the one-instruction a + i^K r b every butterfly and twiddle bracket is made of gives the bits of
      the scalar fmaf formula it claims, and each FMA-form transform is exact to fp32 rounding against a double DFT;
  (b) the K1 outputs against the fp64 model (oracle/model_fp64.py) at the config-4 shape (1 + 1024 rows x 8192) and at a
      low-SNR shape: every lag equal, and the worst relative mag error and absolute frac error within the bounds the
      product-form kernels had (measured on the parent commit at the same shapes and seeds).
"""
import importlib
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (name, nsig, L, seed, gain or None) -- gain None: the generator's own 0.5 .. 1
SHAPES = {
    "cfg4": (1024, 8192, 0xC0FFEE + 4, None),
    "low_snr": (256, 8192, 0x5A17, 0.03),
}
# worst errors of the product-form kernels at these shapes, rounded up: |mag - mag64| / mag64, |frac - frac64|.
# Measured: product form cfg4 4.5e-7 / 7.0e-11, low_snr 4.2e-7 / 7.2e-9; FMA form cfg4 3.2e-7 / 7.8e-11, low_snr 3.1e-7 / 9.3e-9
BOUNDS = {
    "cfg4": (1e-6, 1e-10),
    "low_snr": (1e-6, 1e-8),
}


def k1_errors(b, synth, model, nsig, L, seed, gain):
    """(share of rows whose lag equals the fp64 model's, worst relative mag error, worst absolute frac error) of one block."""
    params = synth.RowParams(nsig, L, seed)
    if gain is not None:
        params.g = np.full(nsig, float(gain))
    rows, _ = synth.make_block(nsig, L, seed, 0, params=params)
    plan = b.Plan(nsig + 1, 2 * L, b.MODE_DIGITAL)
    got = plan.block(rows, seq=0)
    plan.close()
    ref = model.to_complex(rows[0])
    lag = np.zeros(nsig, dtype=np.int64)
    mag = np.zeros(nsig)
    frac = np.zeros(nsig)
    for k in range(nsig):
        lag[k], mag[k], frac[k], _ = model.xcorr_lag(model.to_complex(rows[k + 1]), ref)
    same = got["lag"][1:] == lag
    emag = float(np.max(np.abs(got["mag"][1:][same] - mag[same]) / mag[same]))
    efrac = float(np.max(np.abs(got["frac"][1:][same] - frac[same])))
    return float(same.mean()), emag, efrac


@pytest.fixture(scope="module")
def b():
    binding = importlib.import_module("coherent-rtlsdr_amd.binding")
    if binding.device_count() < 1:
        pytest.fail("no HIP device: the product path has no CPU fallback")
    return binding


def test_fma_primitives_round_like_their_scalar_formulas(tmp_path):
    exe = str(tmp_path / "fma_bfly_check")
    subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-slp-vectorize",
                    "-w", "-o", exe, os.path.join(ROOT, "tools", "fma_bfly_check.hip")], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "mismatches 0" in r.stdout and "accuracy ok" in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_k1_against_fp64_model(b, synth, model, shape):
    nsig, L, seed, gain = SHAPES[shape]
    same, emag, efrac = k1_errors(b, synth, model, nsig, L, seed, gain)
    print(f"{shape}: lags equal {same:.4f}  worst mag rel err {emag:.3e}  worst frac abs err {efrac:.3e}")
    assert same == 1.0
    bmag, bfrac = BOUNDS[shape]
    assert emag <= bmag and efrac <= bfrac
