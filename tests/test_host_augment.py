"""Co-array augmentation through the C++ host layer: coherent_demo --bench --music --augment VXxVY [--mask BITS]
(cbeamformer::batch::set_augment over crsdr_doa_set_augment) prints the receivers used and the virtual array beside the directions, and
refuses a mask that leaves a lag of the virtual array without a pair of receivers, naming the lag."""
import importlib
import os
import re
import subprocess

import pytest

import doa_augment_model as model

HOST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "coherent-rtlsdr_amd", "host")


@pytest.fixture(scope="module")
def host_build():
    importlib.import_module("coherent-rtlsdr_amd.binding").build()
    subprocess.run(["make", "-C", HOST, "all", "libcsynth.so"], check=True, stdout=subprocess.DEVNULL)
    return HOST


def _demo(host_build, *extra):
    r = subprocess.run([os.path.join(host_build, "coherent_demo"), "--bench", "--music", *extra, "--nsig", "21", "--batch", "8", "--blocks", "16"],
                       capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:], r.stderr)
    return r


@pytest.mark.gpu
def test_host_demo_prints_the_receivers_and_the_virtual_array(host_build):
    r = _demo(host_build, "--augment", "7x3", "--mask", model.THINNED)
    assert r.returncode == 0 and "DEMO OK" in r.stdout, r.stdout + r.stderr
    assert "doa: augment: 12 receivers of 21 -> 7 x 3 virtual array" in r.stdout
    beside = re.findall(r"doa: batch (\d+): the directions below are from 12 receivers on the 7 x 3 virtual array\ndoa: batch (\d+): 8 directions, first \((\d+), (\d+)\)", r.stdout)
    assert beside and all(a == c for a, c, _, _ in beside), r.stdout
    # the synthetic channels all carry the aligned reference noise: one source at broadside, on the virtual array as on the filled one
    assert all((cx, cy) == ("50", "50") for _, _, cx, cy in beside), beside


@pytest.mark.gpu
def test_host_demo_refuses_an_uncovered_mask_and_names_the_lag(host_build):
    first_row_only = "1110011" + "0" * 14                                           # no pair of receivers one row apart
    r = _demo(host_build, "--augment", "7x3", "--mask", first_row_only)
    assert r.returncode != 0 and "DEMO FAILED" in r.stdout, r.stdout + r.stderr
    assert "refused" in r.stdout and "lag (ux, uy) = (-6, 1)" in r.stdout, r.stdout
    r = _demo(host_build, "--augment", "7x3", "--mask", "101")                      # not one character per receiver
    assert r.returncode != 0 and "DEMO FAILED" in r.stdout
