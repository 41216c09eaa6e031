"""The gridless directions through the C++ host layer: coherent_demo --bench --music --esprit [only] (cbeamformer::batch::set_esprit over
crsdr_doa_set_esprit) prints every estimate's ESPRIT angles in degrees and power beside the grid direction; they lie within one cell of
it.  With `only` no scan runs and the line carries no grid direction."""
import importlib
import os
import re
import subprocess

import pytest

HOST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "coherent-rtlsdr_amd", "host")
CELL = 180.0 / 100                         # the demo's grid is 100 x 100 over 180 degrees
LINE = r"doa: batch (\d+): esprit (\d+):(?: grid \((\d+), (\d+)\))? found (\d+) status (\d+):((?: \([0-9.eE+-]+, [0-9.eE+-]+\) deg power [0-9.eE+-]+)*)"


@pytest.fixture(scope="module")
def host_build():
    importlib.import_module("coherent-rtlsdr_amd.binding").build()
    subprocess.run(["make", "-C", HOST, "all", "libcsynth.so"], check=True, stdout=subprocess.DEVNULL)
    return HOST


def _demo(host_build, *extra):
    r = subprocess.run([os.path.join(host_build, "coherent_demo"), "--bench", "--music", "--esprit", *extra, "--nsig", "21", "--batch", "8", "--blocks", "32"],
                       capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:], r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "DEMO OK" in r.stdout
    lines = re.findall(LINE, r.stdout)
    assert len(lines) == 4 * 8, r.stdout                                              # 32 blocks in batches of 8, an estimate per block
    return lines, r.stdout


@pytest.mark.gpu
def test_host_demo_prints_the_esprit_angles_beside_the_grid_direction(host_build):
    lines, out = _demo(host_build)
    for batch, e, cx, cy, found, status, slots in lines:
        assert (found, status) == ("1", "0"), (batch, e)
        (alpha, beta, power), = re.findall(r"\(([0-9.eE+-]+), ([0-9.eE+-]+)\) deg power ([0-9.eE+-]+)", slots)
        # the synthetic channels all carry the aligned reference noise: one source at broadside
        assert (cx, cy) == ("50", "50")
        assert abs(float(alpha) - int(cx) * CELL) <= CELL and abs(float(beta) - int(cy) * CELL) <= CELL, (batch, e, alpha, beta)
        assert float(power) > 0
    assert "at broadside" in out                                                      # the grid's own report is still there


@pytest.mark.gpu
def test_host_demo_esprit_only_runs_without_the_scan(host_build):
    lines, out = _demo(host_build, "only")
    for batch, e, cx, cy, found, status, slots in lines:
        assert (cx, cy, found, status) == ("", "", "1", "0"), (batch, e)
        (alpha, beta, power), = re.findall(r"\(([0-9.eE+-]+), ([0-9.eE+-]+)\) deg power ([0-9.eE+-]+)", slots)
        assert abs(float(alpha) - 90.0) <= CELL and abs(float(beta) - 90.0) <= CELL, (batch, e, alpha, beta)
    assert "estimates by ESPRIT alone" in out and "at broadside" not in out
