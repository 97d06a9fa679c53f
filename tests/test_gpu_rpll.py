"""idsp_rpll_i32 on the GPU, through the C ABI, against the specification (tests/_rpll_spec.py, rpll_np — held to the Python-integer
restatement and to the reference's own limits in tests/test_rpll_spec.py), the reference's test harness on the device's own
output, and the chain timestamps -> RPLL -> batch LO -> lock-in with nothing returning to the host in between.

Every output word and every written-back state word is compared with array_equal; outputs start poisoned, states start random
(ff = u32::MAX on every fifth lane), every buffer sits between guard bands (tests/_guard.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

from idsp_amd import _abi
from idsp_amd._abi import RPLL  # the feature's prototype table
from tests import _harness as H
from tests import _rpll_chain as CH
from tests import _rpll_spec as S
from tests import _stream_proc_cases as SP
from tests._guard import Guards

pytestmark = pytest.mark.gpu
DEV, POISON, _ptr = SP.DEV, SP.POISON, SP._ptr

# the shape list of tests/test_gpu_phase.py: every dispatch limit of launch_stream
SHAPES = [(1, 4096), (63, 1000), (64, 33), (65, 2), (1000, 4096), (16384, 1000), (24577, 31), (65536, 32), (65537, 1), (65536, 1000), (65537, 33)]
KERNELS = {}  # (layout, lanes, frames) -> idsp_last_kernel()


def gpu_run(gpu, cfg, st, ts, layout, chunks=None):
    """ts [frames, lanes, 2] int32; st [4, lanes] uint32, updated; chunks: frame counts of consecutive calls on one state
    (the runner: tests/_stream_proc_cases.py)"""
    frames, lanes = ts.shape[:2]
    return SP.run_form(gpu, "rpll", cfg, st, ts, frames, layout, chunks=chunks, record=lambda n, k: KERNELS.__setitem__((layout, lanes, n), k))


def check_case(gpu, cfg, st, ts, density=None):
    ss = st.copy()
    want = S.rpll_np(cfg, ss, ts)
    frames, lanes = ts.shape[:2]
    for layout in (H.FM, H.LM):
        sg = st.copy()
        got = gpu_run(gpu, cfg, sg, ts, layout)
        k = KERNELS[(layout, lanes, frames)]
        assert np.array_equal(got, want), (cfg, layout, lanes, frames, density, k)
        assert np.array_equal(sg, ss), (cfg, layout, lanes, frames, density, k)
        assert k.startswith("stream_frame_major" if layout == H.FM else "stream_lane_major") and "RpllProc" in k, k


@pytest.mark.parametrize("lanes,frames", SHAPES)
def test_equals_the_spec(gpu, lanes, frames):
    rng = np.random.default_rng(lanes % 997 + frames)
    cfg = S.CONFIGS[(lanes + frames) % len(S.CONFIGS)]
    check_case(gpu, cfg, S.random_state(rng, lanes), S.adversarial_ts(rng, frames, lanes))


@pytest.mark.parametrize("cfg", S.CONFIGS)
def test_every_configuration(gpu, cfg):
    """the smallest and largest of every shift; at one shape also the all-`None` and the all-`Some` input"""
    rng = np.random.default_rng(sum(cfg))
    for density in (1 / 3, 0.0, 1.0):
        check_case(gpu, cfg, S.random_state(rng, 1000), S.adversarial_ts(rng, 257, 1000, density), density)


def test_uneven_chunks_equal_one_call(gpu):
    for lanes, frames, chunks in ((1000, 333, [1, 7, 100, 225]), (16384, 130, [33, 1, 64, 32]), (65, 4096, [4000, 95, 1])):
        rng = np.random.default_rng(lanes)
        cfg = (8, 23, 22)
        ts, st = S.adversarial_ts(rng, frames, lanes), S.random_state(rng, lanes)
        ss = st.copy()
        want = S.rpll_np(cfg, ss, ts)
        for layout in (H.FM, H.LM):
            s1, s2 = st.copy(), st.copy()
            whole = gpu_run(gpu, cfg, s1, ts, layout)
            parts = gpu_run(gpu, cfg, s2, ts, layout, chunks=chunks)
            assert np.array_equal(whole, parts) and np.array_equal(s1, s2), (layout, lanes)
            assert np.array_equal(whole, want) and np.array_equal(s1, ss), (layout, lanes)


def test_zero_state_is_default(gpu):
    """all-zero words are `RPLL::default()`; `phase()` / `frequency()` after the call are state words 3 and 2"""
    rng = np.random.default_rng(9)
    ts = S.adversarial_ts(rng, 200, 300)
    ss, sg = np.zeros((4, 300), np.uint32), np.zeros((4, 300), np.uint32)
    want = S.rpll_np((8, 9, 8), ss, ts)
    got = gpu_run(gpu, (8, 9, 8), sg, ts, H.FM)
    assert np.array_equal(got, want) and np.array_equal(sg, ss)
    assert np.array_equal(got[-1, :, 0].view(np.uint32), sg[3]) and np.array_equal(got[-1, :, 1].view(np.uint32), sg[2])


def test_rejected_calls_write_nothing(gpu):
    """ts == accu, overlapping and misaligned calls: IDSP_EINVAL, and no byte of any buffer moves"""
    lanes, frames = 64, 16
    rng = np.random.default_rng(2)
    c = _abi.Rpll(8, 9, 8)
    g = Guards(DEV)
    sd = g.upload("state", S.random_state(rng, lanes), readonly=True)
    td = g.upload("ts", S.adversarial_ts(rng, frames + 1, lanes), readonly=True)
    ad = g.full("accu", (frames + 1) * lanes * 2, torch.int32, POISON)
    g.freeze("accu")
    for layout in (H.FM, H.LM):
        for ts_p, accu_p in ((td.data_ptr(), td.data_ptr()), (td.data_ptr(), td.data_ptr() + 8), (td.data_ptr() + 4, ad.data_ptr()),
                             (td.data_ptr(), ad.data_ptr() + 4)):
            rc = gpu.fn["rpll_i32"](C.byref(c), _ptr(sd), C.c_void_p(ts_p), C.c_void_p(accu_p), lanes, frames, layout, None)
            assert rc == _abi.IDSP_EINVAL and gpu.err(), (layout, ts_p - td.data_ptr(), accu_p - ad.data_ptr())
    torch.cuda.synchronize()
    g.check("rejected idsp_rpll_i32 calls")


def test_reference_harness_on_the_device(gpu):
    """src/rpll.rs:105-206 over 1024 lanes, FrameMajor, in calls of 4096 updates on one state.  Lane 0 is the `default` case
    (:208-213) and meets its four limits on the device's own output; the other lanes take periods, offsets and noise amplitudes
    from the seven cases (under the one configuration of the call: the periods the reference's harness would not accept for it —
    :136-137 — do not lock, they are compared all the same).  Every lane is bit-equal to the spec."""
    kat = S.kat()
    cases = kat["cases"]
    lanes, cfg = 1024, tuple(cases[0]["cfg"])
    pick = np.arange(lanes) % len(cases)
    period = np.array([c["period"] for c in cases], np.int64)[pick]
    nxt = np.array([c["next"] for c in cases], np.int64)[pick]
    noise = np.array([c["noise"] for c in cases], np.int64)[pick]
    assert (period[0], nxt[0], noise[0]) == (333, 111, 0)
    h = S.Harness(cfg, period, nxt, noise, seed=kat["seed"])
    assert h.lockable()[0]
    c = _abi.Rpll(*cfg)
    ss = np.zeros((4, lanes), np.uint32)
    gs = Guards(DEV)
    sd = gs.upload("state", ss)
    settle, n, chunk = S.t_settle(cfg), kat["n"], 4096
    y0, f0 = [], []
    for count, measured in [(settle, False)] + [(chunk, True)] * (n // chunk):
        ts, book = h.timestamps(count)
        want = S.rpll_np(cfg, ss, ts)
        g = Guards(DEV)
        td = g.upload("ts", ts, readonly=True)
        ad = g.full("accu", count * lanes * 2, torch.int32, POISON)
        assert gpu.fn["rpll_i32"](C.byref(c), _ptr(sd), _ptr(td), _ptr(ad), lanes, count, H.FM, None) == 0, gpu.err()
        torch.cuda.synchronize()
        g.check(("harness", count))
        gs.check(("harness", count))
        got = ad.cpu().numpy().reshape(count, lanes, 2)
        assert np.array_equal(got, want), count
        if measured:
            y, f = h.errors(got, book)
            y0.append(y[:, 0]), f0.append(f[:, 0])
    assert np.array_equal(sd.cpu().numpy().view(np.uint32), ss)
    assert gpu.last_kernel().startswith("stream_frame_major"), gpu.last_kernel()
    m = S.Harness.stats(np.concatenate(y0)[:, None], np.concatenate(f0)[:, None])[:, 0]
    rel = np.abs(m) / np.array(cases[0]["limits"], np.float32)
    print("default case on the device: measured", m, "relative", rel)
    assert (rel <= 1.0).all(), (m, rel)
    assert np.allclose(m, cases[0]["measured"], rtol=1e-6, atol=0.0)


def test_chain_on_the_device(gpu):
    """256 lanes with their own periods, phases and harmonics, k = 3: timestamps -> idsp_rpll_i32 -> idsp_accu_lo_i32 ->
    idsp_lockin_i32_lo_process, nothing returns to the host in between.  Bit-equal to the spec's LO fed to the checker library's
    lock-in; atan2(mean Q, mean I) over the last quarter within 1e-2 rad of -phi on every lane (3e-3 on components of 0.5, times
    sqrt 2, rounded up).  The CPU form of the assertion: tests/test_rpll_spec.py, test_chain_through_the_lock_in."""
    case = CH.chain()
    lanes, updates, frames = CH.LANES, CH.UPDATES, case["frames"]
    lc = CH.lockin_cfg()
    worst = 0.0
    for hh in CH.HARMONICS:
        g = Guards(DEV)
        td = g.upload("ts", case["ts"], readonly=True)
        xd = g.upload("x", case["x"], readonly=True)
        rd = g.full("rpll state", 4 * lanes, torch.int32, 0)
        ld = g.full("arm state", 4 * lanes, torch.int32, 0)
        ad = g.full("accu", updates * lanes * 2, torch.int32, POISON)
        lod = g.full("lo", frames * lanes * 2, torch.int32, POISON)
        yd = g.full("y", frames * lanes * 2, torch.int32, POISON)
        assert gpu.fn["rpll_i32"](C.byref(_abi.Rpll(*CH.CFG)), _ptr(rd), _ptr(td), _ptr(ad), lanes, updates, H.FM, None) == 0, gpu.err()
        assert gpu.fn["accu_lo_i32"](C.byref(_abi.AccuLo(CH.K, hh, 0)), _ptr(ad), _ptr(lod), lanes, updates, H.FM, None) == 0, gpu.err()
        assert "accu_lo" in gpu.last_kernel(), gpu.last_kernel()
        assert gpu.fn["lockin_i32_lo_process"](C.byref(lc), _ptr(ld), _ptr(xd), _ptr(lod), _ptr(yd), lanes, frames, H.FM, None) == 0, gpu.err()
        torch.cuda.synchronize()
        g.check(("rpll_i32 -> accu_lo_i32 -> lockin_i32_lo_process", hh))
        assert np.array_equal(ad.cpu().numpy().reshape(updates, lanes, 2), case["accu"])
        assert np.array_equal(rd.cpu().numpy().view(np.uint32).reshape(4, lanes), case["rpll_state"])
        y = yd.cpu().numpy().reshape(frames, lanes, 2)
        assert np.array_equal(y, case["want"][hh]), hh
        assert np.array_equal(ld.cpu().numpy().view(np.uint32).reshape(4, lanes), case["arms"][hh])
        worst = max(worst, CH.phase_error(case, hh, y).max())
    print("chain on the device: worst |arg + phi|", worst)
    assert worst <= 1e-2, worst


def test_dispatch(gpu):
    if not KERNELS:
        rng = np.random.default_rng(0)
        check_case(gpu, (8, 9, 8), S.random_state(rng, 1000), S.adversarial_ts(rng, 17, 1000))
    assert "rpll_i32" in RPLL
    for key in sorted(KERNELS):
        print(key, KERNELS[key])
