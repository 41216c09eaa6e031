"""The beams of the bands through the C++ host layer: coherent_demo --bench --music --subbands --band-beams
(cbeamformer::batch::set_subband_beams over crsdr_doa_set_subband_beams) prints each band's beam power beside its direction."""
import importlib
import os
import re
import subprocess

import pytest

HOST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "coherent-rtlsdr_amd", "host")


@pytest.fixture(scope="module")
def host_build():
    importlib.import_module("coherent-rtlsdr_amd.binding").build()
    subprocess.run(["make", "-C", HOST, "all", "libcsynth.so"], check=True, stdout=subprocess.DEVNULL)
    return HOST


@pytest.mark.gpu
def test_host_demo_prints_a_beam_power_per_band(host_build):
    r = subprocess.run([os.path.join(host_build, "coherent_demo"), "--bench", "--music", "--subbands", "16:0:16", "--peaks", "2", "--band-beams", "mvdr",
                        "--nsig", "21", "--batch", "8", "--blocks", "32"], capture_output=True, text=True, timeout=300)
    print(r.stdout[-4000:], r.stderr)
    assert r.returncode == 0 and "DEMO OK" in r.stdout, r.stdout + r.stderr
    lines = re.findall(r"doa: batch (\d+): estimate (\d+) band (\d+) \(bins \d+\.\.\d+ of 16\): \(\d+, \d+\) power ([0-9.eE+-]+) beam power ([0-9.eE+-]+)", r.stdout)
    assert len(lines) == 4 * 8 * 16, len(lines)                                  # 32 blocks in batches of 8, 16 bands each
    for _, _, _, band_power, beam_power in lines:
        # the Capon estimate of the loaded covariance is at most the conventional one, a^H (R + delta I) a / m^2 <= (1 + loading)
        # lambda_max / m <= 1.01 trace(R) / m; both are printed with four digits
        assert 0.0 < float(beam_power) <= 1.02 * float(band_power), (band_power, beam_power)


@pytest.mark.gpu
def test_host_demo_refuses_band_beams_without_subbands(host_build):
    r = subprocess.run([os.path.join(host_build, "coherent_demo"), "--bench", "--music", "--band-beams", "mvdr", "--nsig", "21", "--batch", "8", "--blocks", "32"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "DEMO FAILED" in r.stdout and "--band-beams" in r.stdout, r.stdout + r.stderr
