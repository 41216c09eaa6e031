"""The digital-mode phase path (K2: shift, integer dot product, phasor chain, rotate + quantise, header) against the exact model
of tests/phase_path_model.py: the phasor bit for bit, the matrix rows byte for byte, the packet header byte for byte -- given the
lag, at every shift class and on every K2 dispatch path.

The other plan tests compare this path with the oracle and the fp64 model under tolerances (1e-5 rad, +-1 LSB on 0.1 % of the
entries: the share of a row that one wrongly patched 16-byte vector damages) or compare the paths with one another, where a
mistake in shifted_word / shifted_vec / dot_word3 / rotq_word / align_shift is common to all of them and cancels.  Here the
reference is exact, so a kernel that is subtly wrong fails by a bit.

Each case (tests/phase_path_cases.py) steers the rows of one plan to its shift set with steering blocks (PRECONDITION: the
reported lag equals the target; a failure of that is K1's or the input's, not K2's), compares those blocks, then runs locked
blocks of full-scale random int8 that the carried lags shift.  phase_path_cases.compare checks every block four ways and reports
them separately: phasor bits, the matrix given the device's own phasor bits (a shift / rotate / quantise defect alone), the matrix
with the model's chain, and the header + reference row.  tests/test_phase_path_model.py runs the same comparison on the CPU
against the model's own output and against a damaged copy of it.
"""
import importlib
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import phase_path_cases as pc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def b():
    binding = importlib.import_module("coherent-rtlsdr_amd.binding")
    if binding.device_count() < 1:
        pytest.fail("no HIP device: the product path has no CPU fallback")
    return binding


@pytest.mark.parametrize("case", pc.PATH_CASES, ids=lambda c: c.name)
def test_phase_path_is_exact_on_the_default_paths(b, case):
    # 16-byte aligned host rows: the fused kernel's three instantiations for B <= 16384 (FULL signed / FULL offset binary / generic
    # with one vector in the row, one per thread, two of four slots live), the three-kernel path with chunks for longer rows
    # (k_phase_dot<true, 8> with chunks / 2 z-slices and atomic partial sums, k_align_quant's inline chain)
    pc.compare(case, pc.run_plan(b, case))


@pytest.mark.parametrize("case", pc.WORD_CASES, ids=lambda c: c.name)
def test_phase_path_is_exact_on_the_word_kernels(b, case):
    # device input at a 4-byte offset: k_phase_dot<false, 4> / k_align_quant<false>, shifted_word for every word of every row
    pc.compare(case, pc.run_plan(b, case, in_off=4))


_CHILD = textwrap.dedent('''
    import importlib, sys, numpy as np
    sys.path[:0] = [%r, %r]
    b = importlib.import_module("coherent-rtlsdr_amd").binding
    import phase_path_cases as pc
    out = {}
    for case in pc.CHILD_CASES:
        res = pc.run_plan(b, case)
        for k in ("lag", "phasor", "packet"):
            out[case.name + "_" + k] = np.stack([r[k] for r in res])
    np.savez(sys.argv[1], **out)
''')


@pytest.mark.parametrize("env", sorted(pc.CHILD_ENVS))
def test_phase_path_is_exact_on_the_switched_paths(tmp_path, env):
    # CRSDR_K2_FUSED=0 (the three-kernel path at B <= 16384: k_phase_dot<true, 4>, k_phase_chain, k_align_quant<true>) and
    # CRSDR_K2_SPIN=-1 (the fused kernel forms every earlier block's dot product itself) are read once per process: a fresh
    # child each, compared against the MODEL, not against each other
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = tmp_path / f"{env}.npz"
    r = subprocess.run([sys.executable, "-c", _CHILD % (root, os.path.join(root, "tests")), str(out)], env=dict(os.environ, **pc.CHILD_ENVS[env]),
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    z = np.load(out)
    for case in pc.CHILD_CASES:
        lag, ph, pk = (z[case.name + "_" + k] for k in ("lag", "phasor", "packet"))
        mo = 16 + 4 * case.nrows
        pc.compare(case, [dict(lag=lag[i], phasor=ph[i], packet=pk[i], matrix=pk[i][mo:].reshape(case.nrows, case.B)) for i in range(lag.shape[0])])


@pytest.mark.parametrize("case", pc.CHAIN_CASES, ids=lambda c: c.name)
def test_phasor_chain_is_exact_over_full_batches(b, case):
    # B = 1024, 3 signal rows, T = 64 = kMaxBatch on the fused path: lane t = 63 is the last lane of the folding wave.  Two tracked
    # batches and locked ones, the chain carried across the submits and compared at every block.  chain_zeroed: a zero row
    # reports lag = -L and holds its phasor; carried into the locked batch, lag = -L shifts a non-zero row out entirely (the output
    # row is all zero, the phasor held again).  chain_refnoise_off: the phasor is frozen, the rotation still applied.
    res = pc.run_plan(b, case)
    pc.compare(case, res)
    pc.chain_properties(case, res)
