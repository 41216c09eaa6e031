"""The subband covariance through the C++ host layer: coherent_demo --bench --music --subbands (cbeamformer::batch::set_subbands over
crsdr_doa_set_subbands) prints a direction and a power for every band of every estimate."""
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
def test_host_demo_prints_sixteen_bands_per_estimate(host_build):
    r = subprocess.run([os.path.join(host_build, "coherent_demo"), "--bench", "--music", "--subbands", "16:0:16", "--nsig", "21", "--batch", "8", "--blocks", "32"],
                       capture_output=True, text=True, timeout=300)
    print(r.stdout[-4000:], r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "DEMO OK" in r.stdout
    lines = re.findall(r"doa: batch (\d+): estimate (\d+) band (\d+) \(bins (\d+)\.\.(\d+) of 16\): \((\d+), (\d+)\) power ([0-9.eE+-]+)", r.stdout)
    batches = sorted({int(l[0]) for l in lines})
    assert batches == [0, 1, 2, 3], batches                                      # 32 blocks in batches of 8
    for bt in batches:
        for e in range(8):
            bands = [l for l in lines if int(l[0]) == bt and int(l[1]) == e]
            assert [int(l[2]) for l in bands] == list(range(16)) and [int(l[3]) for l in bands] == list(range(16)), (bt, e)
            assert all(0 <= int(l[5]) < 100 and 0 <= int(l[6]) < 100 and float(l[7]) >= 0.0 for l in bands)
    # the synthetic channels all carry the aligned reference noise, white over the band: every band sees it at broadside
    assert sum(l[5] == "50" and l[6] == "50" for l in lines) >= len(lines) // 2
    assert re.search(r"doa: batch 3: 128 directions", r.stdout)                  # the summary counts estimates x bands
