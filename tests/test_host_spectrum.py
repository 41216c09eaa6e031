"""The power maps through the C++ host layer: coherent_demo --bench --music --spectrum capon (cbeamformer::batch::set_spectrum over
crsdr_doa_set_spectrum) prints every direction with the map's value in dB beside the MVDR beam's power toward it: the same quantity,
once from the fp32 scan and once from the fp64 weights kernel."""
import importlib
import math
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
def test_host_demo_prints_the_capon_value_beside_the_beam_power(host_build):
    r = subprocess.run([os.path.join(host_build, "coherent_demo"), "--bench", "--music", "--spectrum", "capon", "--peaks", "2", "--beams", "mvdr", "--nsig", "21",
                        "--batch", "8", "--blocks", "32"], capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:], r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "DEMO OK" in r.stdout
    lines = re.findall(r"doa: batch (\d+): 8 estimates, peaks of the first:((?: \(\d+, \d+\) value [0-9.eE+-]+ dB power [0-9.eE+-]+)+)", r.stdout)
    assert sorted(int(l[0]) for l in lines) == [0, 1, 2, 3], r.stdout               # 32 blocks in batches of 8
    for _, dirs in lines:
        found = re.findall(r"\((\d+), (\d+)\) value ([0-9.eE+-]+) dB power ([0-9.eE+-]+)", dirs)
        assert 1 <= len(found) <= 2
        # the synthetic channels all carry the aligned reference noise: the strongest direction is broadside
        assert found[0][:2] == ("50", "50")
        for _, _, db, power in found:
            assert abs(float(db) - 10.0 * math.log10(float(power))) <= 0.02        # two decimals of a dB and four digits of the power, as printed
