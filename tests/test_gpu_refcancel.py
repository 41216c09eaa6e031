"""GPU checks of the reference-noise canceller (include/crsdr.h: crsdr_plan_set_refcancel, crsdr_refcancel; csrc/refcancel.hpp).

The per-op call is held against the definition in numpy (tests/refcancel_model.py) with the bars of tests/refcancel_cases.py
(check_block): coefficients within the rounding to fp32 plus the fp64 solve's 1e-12 cond(G), residual within 2^-23 relative plus
1e-9, status exact, every output byte within 0.5 + 4 e_ref of the fp64 output sample formed from the device's OWN published
coefficients, e_ref the float32 restatement's excess on the family (tests/test_refcancel_model.py prints it; DESIGN.md holds the
device's).  The plan is held against the per-op call byte for byte, a sharded plan against the unsharded one, and the
direction-of-arrival engine on a plan's cancelled packets against the fp64 model's direction.

One departure from the cases as first listed: a constant reference row is NOT rank-deficient under the definition -- the
zero-filled edges make its delayed copies differ in their first and last samples, the smallest Cholesky pivot is of the order of one
sample's power, 2^27 times the floor -- so its status is 0, as the model says, with a badly conditioned Gram (the coefficient bar's
cond(G) term covers it).  The rank-deficient case here is a reference row that is zero but for its first sample (its copy r_{-1} is
the zero row): status 1, like the all-zero row."""
import importlib

import numpy as np
import pytest

import refcancel_cases as cases
import refcancel_model as M
import ura

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


def on_device(torch, b, rows, lag, ph, taps, flags, skew):
    """the per-op call on device memory; rows and out 16-byte aligned plus skew bytes"""
    dev = torch.device("cuda", 0)
    n, B = rows.shape
    raw_in = torch.zeros(n * B + 64, dtype=torch.uint8, device=dev)
    raw_out = torch.zeros(n * B + 64, dtype=torch.uint8, device=dev)
    i0, o0 = (-raw_in.data_ptr()) % 16 + skew, (-raw_out.data_ptr()) % 16 + skew
    raw_in[i0:i0 + n * B] = torch.from_numpy(np.array(rows).view(np.uint8).reshape(-1)).to(dev)
    d_lag = torch.from_numpy(lag).to(dev)
    d_ph = torch.from_numpy(ph.view(np.float32).copy()).to(dev)
    d_coef = torch.full((n * taps * 2,), 7.0, dtype=torch.float32, device=dev)
    d_res = torch.full((n,), 7.0, dtype=torch.float32, device=dev)
    d_st = torch.full((n,), 7, dtype=torch.int32, device=dev)
    b.refcancel_device(raw_out.data_ptr() + o0, d_coef.data_ptr(), d_res.data_ptr(), d_st.data_ptr(), raw_in.data_ptr() + i0, n, B, d_lag.data_ptr(),
                       d_ph.data_ptr(), taps, flags)
    assert not raw_out[:o0].any() and not raw_out[o0 + n * B:].any()                  # nothing written outside the rows
    return dict(out=raw_out[o0:o0 + n * B].cpu().numpy().view(np.int8).reshape(n, B), coef=d_coef.cpu().numpy().view(np.complex64).reshape(n, taps),
                residual=d_res.cpu().numpy(), status=d_st.cpu().numpy())


def every_way(torch, b, block, lag, ph, taps):
    """(tag, answer) of the per-op call on signed and offset-binary input, in host memory and in device memory at both alignments"""
    for obin in (False, True):
        rows = (block.view(np.uint8) ^ np.uint8(0x80)) if obin else block
        flags = b.OFFSET_BINARY if obin else 0
        yield f"host obin={obin}", b.refcancel(rows, lag, ph, taps, flags)
        for skew in (0, 4):
            yield f"device+{skew} obin={obin}", on_device(torch, b, rows, lag, ph, taps, flags, skew)


@pytest.mark.parametrize("taps", cases.TAPS)
@pytest.mark.parametrize("B", cases.BLOCKSIZES)
def test_per_op_against_the_model(b, torch, B, taps):
    block, lag, ph = cases.perop_case(B)
    want = cases.perop_model(B, taps)
    assert (np.abs(block[-1].astype(np.int16)) >= 127).all() and np.abs(want["out"][-1].astype(np.int16)).max() >= 127      # the clamp is hit
    first, worst = None, -1.0
    for tag, got in every_way(torch, b, block, lag, ph, taps):
        worst = max(worst, cases.device_excess(block, lag, ph, taps, got)[1:].max())
        miss = cases.check_block(block, lag, ph, taps, got, want, f"B={B} taps={taps} {tag}")
        assert not miss, "\n".join(miss[:8])
        assert not got["coef"][0].any() and got["residual"][0] == 0 and got["status"][0] == 0
        if first is None:
            first = got
        for key in ("out", "coef", "residual", "status"):                  # one arithmetic, whatever the memory and the input's form
            assert np.array_equal(got[key], first[key]), (tag, key)
    print(f"B={B} taps={taps}: device byte excess {worst:.3e}, e_ref {cases.reference_excess():.3e}")


@pytest.mark.parametrize("kind", ["zero", "single", "constant"])
def test_deficient_reference_rows(b, torch, kind):
    block, lag, ph = cases.failure_case(kind)
    want = M.cancel_block(block, lag, ph, 3)
    status = 0 if kind == "constant" else M.STATUS_SINGULAR
    assert (want["status"][1:] == status).all()
    for tag, got in every_way(torch, b, block, lag, ph, 3):
        miss = cases.check_block(block, lag, ph, 3, got, want, f"{kind} {tag}")
        assert not miss, "\n".join(miss[:8])
        if status:
            assert not got["coef"].any() and (got["residual"][1:] == 1.0).all() and (got["status"][1:] == 1).all()


NROWS, B22, T22 = 22, 4096, 3


@pytest.fixture(scope="module")
def batches():
    sc = cases.ArrayScene(11, B22 // 2)
    return [sc.blocks(T22) for _ in range(4)]


FLAGS = lambda b: (b.REFNOISE_ENABLED, b.REFNOISE_ENABLED | b.NO_LAG, 0)      # measured lags; lags from the carried state; the gate closed


def run_plan(b, batches, taps, **kw):
    """three submits (flags above): list over (submit, block) of fetch dicts (+ cancel: fetch_refcancel)"""
    plan = b.Plan(NROWS, B22, b.MODE_DIGITAL, max_batch=T22, **kw)
    if taps:
        plan.set_refcancel(taps)
    out = []
    for i, flags in enumerate(FLAGS(b)):
        plan.submit(batches[i], seq=100 * i, flags=flags)
        for t in range(T22):
            got = plan.fetch(block=t)
            if taps:
                got["cancel"] = plan.fetch_refcancel(block=t)
            out.append(got)
        plan.sync()
    return plan, out


@pytest.mark.parametrize("taps", [9, 3])
def test_plan_against_the_per_op_call(b, batches, taps):
    off_plan, off = run_plan(b, batches, 0)
    plan, on = run_plan(b, batches, taps)
    mo = plan.matrix_offset
    for i in range(3):
        for t in range(T22):
            got, ref = on[i * T22 + t], off[i * T22 + t]
            for key in ("lag", "mag", "frac"):
                assert np.array_equal(got[key], ref[key]), (i, t, key)
            assert np.array_equal(got["phasor"].view(np.uint32), ref["phasor"].view(np.uint32)), (i, t)
            assert np.array_equal(got["packet"][:mo], ref["packet"][:mo]) and np.array_equal(got["matrix"][0], ref["matrix"][0])
            if i == 2:                                                        # submitted without the flag: today's bits, status 2
                assert np.array_equal(got["packet"], ref["packet"]), t
                assert (got["cancel"]["status"][1:] == M.STATUS_IDLE).all() and got["cancel"]["status"][0] == 0 and not got["cancel"]["coef"].any()
                continue
            per = b.refcancel(batches[i][t], got["lag"], got["phasor"], taps)
            assert np.array_equal(got["matrix"], per["out"]), (i, t, np.count_nonzero(got["matrix"] != per["out"]))
            for key in ("coef", "residual", "status"):
                assert np.array_equal(got["cancel"][key], per[key]), (i, t, key)
            assert not np.array_equal(got["matrix"][1:], ref["matrix"][1:])    # and the pass did change the rows
        if i == 1:
            assert np.array_equal(on[T22]["lag"], on[T22 - 1]["lag"])          # CRSDR_NO_LAG: the lags of the first submit's last block
    # off again: today's bits
    plan.set_refcancel(0)
    with pytest.raises(b.CrsdrError) as e:
        plan.fetch_refcancel()
    assert e.value.code == -5
    for p in (plan, off_plan):
        p.submit(batches[3], seq=900, flags=b.REFNOISE_ENABLED)
    for t in range(T22):
        assert np.array_equal(plan.fetch(block=t)["packet"], off_plan.fetch(block=t)["packet"]), t
    plan.close()
    off_plan.close()


def test_sharded_plan_writes_the_unsharded_rows_into_its_slab(b, torch, batches):
    full, on = run_plan(b, batches, 9)
    full.close()
    first, count = 8, 7
    plan = b.Plan(NROWS, B22, b.MODE_DIGITAL, row_begin=first, row_count=count, max_batch=T22)
    plan.set_refcancel(9)
    slot, toff = count * B22 + 256, count * B22
    send = torch.zeros(T22 * slot, dtype=torch.uint8, device=torch.device("cuda", 0))
    plan.bind_slab_ex(send.data_ptr(), slot, 0, T22, toff)
    for i, flags in enumerate(FLAGS(b)):
        plan.submit(batches[i], seq=100 * i, flags=flags)
        plan.sync()
        for t in range(T22):
            slab = send[t * slot: t * slot + count * B22].cpu().numpy().view(np.int8).reshape(count, B22)
            assert np.array_equal(slab, on[i * T22 + t]["matrix"][first:first + count]), (i, t)
            c = plan.fetch_refcancel(block=t)
            for key in ("coef", "residual", "status"):
                assert np.array_equal(c[key][first:first + count], on[i * T22 + t]["cancel"][key][first:first + count]), (i, t, key)
                assert not c[key][:first].any() and not c[key][first + count:].any()           # rows outside the slab hold zeros
    plan.close()


def test_exclusions(b):
    plan = b.Plan(4, 1024, b.MODE_DIGITAL)
    for taps in (2, 4, 11, -1):
        with pytest.raises(b.CrsdrError) as e:
            plan.set_refcancel(taps)
        assert e.value.code == -1
    plan.set_frac_apply(1, 1.0)
    with pytest.raises(b.CrsdrError) as e:
        plan.set_refcancel(3)
    assert e.value.code == -5
    plan.set_frac_apply(0)
    plan.set_refcancel(3)
    with pytest.raises(b.CrsdrError) as e:
        plan.set_frac_apply(1, 1.0)
    assert e.value.code == -5
    plan.set_frac_apply(0)                                      # turning the other one off is always allowed
    assert plan.refcancel_buffers()["taps"] == 3
    plan.set_refcancel(0)
    with pytest.raises(b.CrsdrError) as e:
        plan.refcancel_buffers()
    assert e.value.code == -5
    plan.set_frac_apply(1, 1.0)
    plan.close()
    for args in ((4, 1024, b.MODE_FAITHFUL), (4, 32768, b.MODE_DIGITAL)):
        plan = b.Plan(*args)
        with pytest.raises(b.CrsdrError) as e:
            plan.set_refcancel(3)
        assert e.value.code == -1, args
        plan.close()


def test_directions_with_the_noise_on(b):
    """calibrate and measure on the same blocks: without the canceller the MUSIC peak is the all-ones steering vector of the calibrated
    noise, (50, 50), whatever the emitter's direction; with nine taps it is the fp64 model's peak on the model's cancelled rows"""
    L, T = 2048, 16
    rows = cases.ArrayScene(7, L).blocks(T)
    found = {}
    for taps in (0, 9):
        plan = b.Plan(NROWS, 2 * L, b.MODE_DIGITAL, max_batch=T)
        doa = b.Doa(NROWS, 2 * L, 1, ura.D, ura.MX, ura.MY, 100, 100, max_batch=T)
        if taps:
            plan.set_refcancel(taps)
        plan.submit(rows, seq=0, flags=b.REFNOISE_ENABLED)
        doa.submit_plan(plan)
        out = doa.fetch()
        last = plan.fetch(block=T - 1)
        found[taps] = (tuple(int(x) for x in out["peak"][T - 1]), float(out["sv"][T - 1][1] / out["sv"][T - 1][0]), last)
        assert not out["status"].any()
        doa.close()
        plan.close()
    assert found[0][0] == (50, 50), found[0][0]
    last = found[9][2]
    assert np.array_equal(last["lag"], found[0][2]["lag"]) and np.array_equal(last["phasor"], found[0][2]["phasor"])
    model = {}
    for taps in (1, 9):
        m = M.cancel_block(rows[T - 1], last["lag"], last["phasor"], taps)
        _, _, s, pm = ura.music_fp64(m["out"], 1)
        model[taps] = (tuple(int(x) for x in np.unravel_index(np.argmax(pm), pm.shape)), float(s[1] / s[0]))
    print(f"device: off {found[0][:2]}, 9 taps {found[9][:2]}; model: 1 tap {model[1]}, 9 taps {model[9]}")
    assert model[1][1] >= 10.0 * model[9][1], model                       # the precondition: one tap leaves the noise in the rows
    assert model[9][0] != (50, 50)
    assert found[9][0] == model[9][0], (found[9][0], model[9][0])
    assert found[9][1] <= 2.0 * model[9][1], (found[9][1], model[9][1])
