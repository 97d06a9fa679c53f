"""idsp_sweep_i32 on the GPU, through the C ABI, against the specification (tests/_sweep_spec.py, osc_np — held to the big-integer
restatement and to the reference's figures in tests/test_sweep_spec.py).

Every output word and every written-back state word is compared with array_equal; outputs start poisoned, every buffer sits
between guard bands.  Lane populations mix fit-derived sweeps, random (state, rate), the corner states of
tests/golden/sweep_kat.json and lanes placed by the spec so that they end at a chosen frame; every case asserts, against the spec,
that a lane ends strictly inside the call, one had ended before it and one never ends (tests/_sweep_gpu.py, assert_mixed: over
three one-lane populations where there is one lane; in a one-frame call "inside" is a lane that emits its last sample there)."""
import numpy as np
import pytest

from idsp_amd._abi import SWEEP  # the feature's prototype table
from tests import _harness as H
from tests import _sweep_gpu as G
from tests import _sweep_spec as S

pytestmark = pytest.mark.gpu

# 63 / 64 / 65: the ragged last wave; 1000: the 4-lane piece of the staged kernels; 40960 / 40961: kSplitMaxLanes
SHAPES = [(lanes, frames) for lanes in (1, 63, 64, 65, 1000) for frames in (1, 3, 16, 17, 257, 1000)] + \
         [(lanes, frames) for lanes in (40960, 40961) for frames in (1, 17, 33)]


@pytest.mark.parametrize("lanes,frames", SHAPES)
def test_equals_the_spec(gpu, lanes, frames):
    cases = []
    for variant in G.variants_for(lanes):
        st, after, want = G.osc_case(lanes, frames, 0, variant)
        cases.append((st, after))
        for layout in (H.FM, H.LM):
            sg = st.copy()
            got = G.run(gpu, sg, frames, layout)
            k = G.KERNELS[("sweep_i32", layout, lanes, frames)]
            assert np.array_equal(got, want), (layout, lanes, frames, k)
            assert np.array_equal(sg, after), (layout, lanes, frames, k)
            assert k.startswith("stream_frame_major" if layout == H.FM else "stream_lane_major") and "SweepProc" in k, k
    G.assert_mixed(cases, frames)


@pytest.mark.parametrize("lanes,frames", [(65, 257), (1000, 257), (1, 17), (40961, 33)])
def test_uneven_chunks_equal_one_call(gpu, lanes, frames):
    """(1, F - 1), (F - 1, 1) and a three-way split on one state; in each, the lanes of kind `boundary` emit their last sample in
    the last frame of the first chunk"""
    for chunks in ([1, frames - 1], [frames - 1, 1], [frames // 3, 1, frames - frames // 3 - 1]):
        cases = []
        for variant in G.variants_for(lanes):
            st, after, want = G.osc_case(lanes, frames, chunks[0], variant)
            cases.append((st, after))
            if lanes >= 8:  # the `boundary` lanes: chunks[0] samples left, so the chunk ends on their last emitted frame
                b = np.arange(lanes) % len(S.KINDS) == S.KINDS.index("boundary")
                e = (S.emitted_of(after) - S.emitted_of(st)).astype(np.int64)
                assert b.any() and (e[b] == chunks[0]).all() and want[chunks[0] - 1][b].any(axis=1).all() and not want[chunks[0]:, b].any()
            for layout in (H.FM, H.LM):
                sg = st.copy()
                got = G.run(gpu, sg, frames, layout, chunks=chunks)
                assert np.array_equal(got, want) and np.array_equal(sg, after), (layout, lanes, frames, chunks)
        G.assert_mixed(cases, frames)


def test_an_ended_lane_stays_ended(gpu):
    """further calls on the written-back state: (0, 0) and no word moves on every lane that has ended, `emitted` says where"""
    st, after, _ = G.osc_case(1000, 257)
    gone = S.ended_np(after)
    assert gone.any() and not gone.all()
    sg = after.copy()
    want_state = after.copy()
    want = S.osc_np(want_state, 40)
    got = G.run(gpu, sg, 40, H.FM)
    assert np.array_equal(got, want) and np.array_equal(sg, want_state)
    assert not got[:, gone].any() and np.array_equal(sg[:, gone], after[:, gone])
    assert got[:, ~gone].any(axis=2)[0].all()  # a live lane never writes (0, 0)


def test_the_reference_sweep_to_its_end(gpu):
    """the reference test's sweep (src/sweptsine.rs:199-202) from 1000 samples before its end, beside lanes further back:
    `emitted` of lane 0 stops at the 1000 it had left"""
    rate, tail = S.kat_tail()
    st = S.pack([tail[1000], tail[2000], tail[1], tail[0]], rate)
    ss = st.copy()
    want = S.osc_np(ss, 1500)
    got = G.run(gpu, st, 1500, H.LM)
    assert np.array_equal(got, want) and np.array_equal(st, ss)
    assert [int(v) for v in S.emitted_of(st)] == [1000, 1500, 1, 0]
    assert got[999, 0].any() and not got[1000:, 0].any()


@pytest.mark.parametrize("layout", [H.FM, H.LM])
def test_into_the_lock_in(gpu, layout):
    """the swept lock-in as the library offers it: idsp_sweep_i32 into an LO buffer into idsp_lockin_i32_lo_process, against the
    checker library's lock-in fed the spec's LO (an ended lane's LO is (0, 0): its arms go on filtering zeros)"""
    import ctypes as C

    import torch

    from tests._guard import Guards

    lanes, frames = 1000, 257
    st, after, lo = G.osc_case(lanes, frames)
    cfg = H.lockin_cfg([[1 << 24, -(1 << 21)], [1 << 22, 12345]])
    rng = np.random.default_rng(3)
    x = rng.integers(-(1 << 31), 1 << 31, (frames, lanes)).astype(np.int32)
    arms = rng.integers(0, 1 << 32, (16, lanes), dtype=np.uint64).astype(np.uint32)
    so, want = arms.copy(), np.empty((frames, lanes, 2), np.int32)
    assert H.oracle().fn["lockin_i32_lo_process"](C.byref(cfg), H._ptr(so), H._ptr(np.ascontiguousarray(x)), H._ptr(np.ascontiguousarray(lo)),
                                                  H._ptr(want), lanes, frames, H.FM) == 0
    g = Guards(G.DEV)
    sd, ad = g.upload("sweep state", st), g.upload("arm state", arms)
    xd = g.upload("x", G.to_layout(x, layout), readonly=True)
    lod = g.full("lo", lanes * frames * 2, torch.int32, G.POISON)
    yd = g.full("y", lanes * frames * 2, torch.int32, G.POISON)
    assert gpu.fn["sweep_i32"](G._ptr(sd), G._ptr(lod), lanes, frames, layout, None) == 0, gpu.err()
    assert gpu.fn["lockin_i32_lo_process"](C.byref(cfg), G._ptr(ad), G._ptr(xd), G._ptr(lod), G._ptr(yd), lanes, frames, layout, None) == 0, gpu.err()
    torch.cuda.synchronize()
    g.check(("sweep_i32 -> lockin_i32_lo_process", layout))
    assert np.array_equal(G.from_layout(lod.cpu().numpy(), layout, frames, lanes, 2), lo)
    assert np.array_equal(G.from_layout(yd.cpu().numpy(), layout, frames, lanes, 2), want)
    assert np.array_equal(ad.cpu().numpy().view(np.uint32), so) and np.array_equal(sd.cpu().numpy().view(np.uint32), after)


def test_dispatch(gpu):
    if not G.KERNELS:
        st, _, _ = G.osc_case(1000, 17)
        for layout in (H.FM, H.LM):
            G.run(gpu, st.copy(), 17, layout)
    assert "sweep_i32" in SWEEP
    for key in sorted(G.KERNELS):
        print(key, G.KERNELS[key])
