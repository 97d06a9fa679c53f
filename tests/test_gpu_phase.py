"""The phase consumers on the GPU, through the C ABI, against the numpy specification (tests/_phase_spec.py): idsp_pll_i32 in its
three output forms, idsp_unwrap_i32, idsp_unwrap_i32_phase and idsp_clamp_wrap_i32.

Every output element and every written-back state word is compared with array_equal — all integer, no tolerance, nothing sampled.
Outputs start poisoned, states start random (the `Wrap` word in {-1, 0, 1}).

Figures of the convergence tests on the specification (tests/test_phase_spec.py prints them; the reference's bounds in brackets):
converge_pll worst |step + frequency| 0 [1], worst |x + y| 0 [4]; converge_narrow 2 [65536] and 1747 [65536]."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from idsp_amd import _abi
from idsp_amd._abi import PHASE  # the feature's prototype table
from tests import _harness as H
from tests import _phase_spec as S
from tests import _stream_proc_cases as SP
from tests._guard import Guards

pytestmark = pytest.mark.gpu
DEV, POISON, _ptr = SP.DEV, SP.POISON, SP._ptr

FORMS = ["pll0", "pll1", "pll2", "unwrap0", "unwrap1", "clamp"]
WORDS = {f: SP.TRAITS[f].words for f in FORMS}
FOUR_BYTE = [f for f in FORMS if f in SP.FOUR_BYTE]  # forms whose output element is 4 bytes: y == x allowed
KAT = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "phase_kat.json")))

# every lane count of {1, 63, 64, 65, 1000, 16384, 24577, 65536, 65537} and every frame count of {1, 2, 31, 32, 33, 1000, 4096}
# appears, with each layout and each form (the tests below run every pair in both layouts for all six forms)
SHAPES = [(1, 4096), (63, 1000), (64, 33), (65, 2), (1000, 4096), (16384, 1000), (24577, 31), (65536, 32), (65537, 1), (65536, 1000), (65537, 33)]

KERNELS = {}  # (form, layout, lanes, frames) -> idsp_last_kernel()


def spec_run(form, ba, st, x):
    """x [frames, lanes] int32; st updated; returns [frames, lanes(, 2)]"""
    return SP.spec_run(form, ba, st, x)


def gpu_call(gpu, form, ba, sd, xd, yd, lanes, frames, layout):
    rc = SP.call_form(gpu, form, ba, _ptr(sd), _ptr(xd), _ptr(yd), lanes, frames, layout)
    assert rc == 0, gpu.err()


def gpu_run(gpu, form, ba, st, x, layout, inplace=False, chunks=None):
    """x [frames, lanes] int32 (numpy); st [words, lanes] uint32, updated; returns the output as [frames, lanes(, 2)].
    chunks: frame counts of consecutive calls on one state (their sum = frames).  (The runner: tests/_stream_proc_cases.py.)"""
    frames, lanes = x.shape
    return SP.run_form(gpu, form, ba, st, x, frames, layout, inplace=inplace, chunks=chunks,
                       record=lambda n, k: KERNELS.__setitem__((form, layout, lanes, n), k))


def case(form, lanes, frames, seed):
    rng = np.random.default_rng(seed)
    ba = S.random_ba(rng)
    x = S.adversarial_phases(rng, frames, lanes)
    st = S.random_state(rng, WORDS[form], lanes)
    return ba, x, st


@pytest.mark.parametrize("lanes,frames", SHAPES)
@pytest.mark.parametrize("form", FORMS)
def test_equals_the_spec(gpu, form, lanes, frames):
    ba, x, st = case(form, lanes, frames, 1000 * FORMS.index(form) + lanes % 997 + frames)
    ss = st.copy()
    want = spec_run(form, ba, ss, x)
    for layout in (H.FM, H.LM):
        sg = st.copy()
        got = gpu_run(gpu, form, ba, sg, x, layout)
        assert got.dtype == want.dtype and np.array_equal(got, want), (form, layout, lanes, frames, KERNELS[(form, layout, lanes, frames)])
        assert np.array_equal(sg, ss), (form, layout, lanes, frames)
        k = KERNELS[(form, layout, lanes, frames)]
        assert k.startswith("stream_"), k
        assert k.startswith("stream_frame_major" if layout == H.FM else "stream_lane_major"), k
        assert {"pll": "PllProc", "unw": "UnwrapProc", "cla": "ClampWrapProc"}[form[:3]] in k, k


@pytest.mark.parametrize("form", FORMS)
def test_uneven_chunks_equal_one_call(gpu, form):
    for lanes, frames, chunks in ((1000, 333, [1, 7, 100, 225]), (16384, 130, [33, 1, 64, 32]), (65, 4096, [4000, 95, 1])):
        ba, x, st = case(form, lanes, frames, 77 + FORMS.index(form))
        ss = st.copy()
        want = spec_run(form, ba, ss, x)
        for layout in (H.FM, H.LM):
            s1, s2 = st.copy(), st.copy()
            whole = gpu_run(gpu, form, ba, s1, x, layout)
            parts = gpu_run(gpu, form, ba, s2, x, layout, chunks=chunks)
            assert np.array_equal(whole, parts) and np.array_equal(s1, s2), (form, layout, lanes)
            assert np.array_equal(whole, want) and np.array_equal(s1, ss), (form, layout, lanes)


@pytest.mark.parametrize("form", FOUR_BYTE)
def test_in_place(gpu, form):
    for lanes, frames in ((1000, 1000), (16384, 64), (65536, 33), (65537, 40), (3, 500), (24577, 31)):
        ba, x, st = case(form, lanes, frames, 5 + FORMS.index(form))
        ss = st.copy()
        want = spec_run(form, ba, ss, x)
        for layout in (H.FM, H.LM):
            sg = st.copy()
            got = gpu_run(gpu, form, ba, sg, x, layout, inplace=True)
            assert np.array_equal(got, want) and np.array_equal(sg, ss), (form, layout, lanes, frames, KERNELS[(form, layout, lanes, frames)])


def test_zero_state_is_default(gpu):
    """all-zero words are `PLLState::default()`, `Unwrapper::default()`, `ClampWrap::default()`"""
    rng = np.random.default_rng(9)
    x = S.adversarial_phases(rng, 200, 300)
    for form in FORMS:
        ba = S.random_ba(rng)
        ss, sg = np.zeros((WORDS[form], 300), np.uint32), np.zeros((WORDS[form], 300), np.uint32)
        want = spec_run(form, ba, ss, x)
        assert np.array_equal(gpu_run(gpu, form, ba, sg, x, H.FM), want) and np.array_equal(sg, ss), form


def _abs32(v):
    """`W<i32>::abs()` of int64-held i32 values: wrapping (|i32::MIN| = i32::MIN)"""
    v = ((v + (1 << 31)) % (1 << 32)) - (1 << 31)
    a = np.abs(v)
    return np.where(a == (1 << 31), -(1 << 31), a)


@pytest.mark.parametrize("name,chunk", [("converge_pll", 512), ("converge_narrow", 4096)])
def test_reference_convergence_tests(gpu, name, chunk):
    """src/pll.rs:117-150 over 4096 lanes: lane 0 carries the reference's accumulator step and must meet the reference's bounds;
    every other lane has a step of its own; every lane is bit-equal to the spec.  {phase, frequency} pairs, FrameMajor, the
    long run in calls of `chunk` frames on one state."""
    k = KAT[name]
    lanes, n = 4096, k["n"]
    rng = np.random.default_rng(42)
    step = rng.integers(0, 1 << 32, size=lanes, dtype=np.uint64)
    step[0] = k["accu_step"]
    ba = S.pll_from_bandwidth(k["bandwidth"], k["split"])
    lib_ba = (C.c_int32 * 3)()
    assert gpu.fn["pll_from_bandwidth"](k["bandwidth"], k["split"], lib_ba) == 0 and list(lib_ba) == ba
    ss, sg = np.zeros((9, lanes), np.uint32), np.zeros((9, lanes), np.uint32)
    gs = Guards(DEV)
    sd = gs.upload("state", sg)
    worst_f = worst_p = 0
    for f0 in range(0, n, chunk):
        idx = np.arange(f0 + 1, f0 + chunk + 1, dtype=np.uint64)[:, None]  # Accu: pre-increment (src/accu.rs:34-37)
        x = ((idx * step[None, :] + np.uint64(k["accu_state"])) & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32)
        want = S.pll_np(ba, ss, x, output=2)
        g = Guards(DEV)
        xd = g.upload("x", x, readonly=True)
        yd = g.full("y", chunk * lanes * 2, torch.int32, POISON)
        gpu_call(gpu, "pll2", ba, sd, xd, yd, lanes, chunk, H.FM)
        torch.cuda.synchronize()
        g.check((name, f0))
        gs.check((name, f0))
        got = yd.cpu().numpy().reshape(chunk, lanes, 2)
        assert np.array_equal(got, want), (name, f0)
        sel = np.arange(f0, f0 + chunk) > k["bounds_apply_for_i_greater_than"]
        if sel.any():
            df = _abs32(int(step[0]) + got[sel, 0, 1].astype(np.int64))
            dp = _abs32(x[sel, 0].astype(np.int64) + got[sel, 0, 0].astype(np.int64))
            worst_f, worst_p = max(worst_f, int(df.max())), max(worst_p, int(dp.max()))
            assert (df <= k["frequency_bound"]).all() and (dp <= k["phase_bound"]).all(), (name, f0, worst_f, worst_p)
    assert np.array_equal(sd.cpu().numpy().view(np.uint32), ss)
    assert gpu.last_kernel().startswith("stream_frame_major"), gpu.last_kernel()
    print(name, "lane 0: worst |step + frequency|", worst_f, "worst |x + y|", worst_p)


def test_lockin_arg_into_pll_frequency(gpu):
    """The chain the phase consumers exist for: idsp_lockin_i32_arg on a tone offset from the lock-in's LO, its phase output handed
    on the device to idsp_pll_i32(output = frequency).  Equals the spec PLL fed the checker library's `arg` stream."""
    lanes, frames = 256, 4096
    lc = H.lockin_cfg([[1 << 24]])
    rng = np.random.default_rng(1)
    lo_step = rng.integers(1 << 26, 1 << 29, size=lanes, dtype=np.int64)
    offset = rng.integers(-(1 << 22), 1 << 22, size=lanes, dtype=np.int64)
    n = np.arange(frames, dtype=np.float64)[:, None]
    tone = (np.cos(2 * np.pi * ((lo_step + offset)[None, :] / 2.0 ** 32) * n + rng.uniform(0, 6.28, size=lanes)[None, :]) * (1 << 28)).astype(np.int32)
    st = np.zeros((6, lanes), np.uint32)
    st[1] = lo_step.astype(np.uint32)
    so = st.copy()
    arg_o = np.empty((frames, lanes), np.int32)
    assert H.oracle().cfgcall("lockin_i32_arg", lc, so, np.ascontiguousarray(tone), arg_o, lanes, frames, H.FM) == 0
    ba = S.pll_from_bandwidth(1e-2, 4.0)
    ps = np.zeros((9, lanes), np.uint32)
    want = S.pll_np(ba, ps, arg_o, output=1)

    g = Guards(DEV)
    sd = g.upload("lock-in state", st)
    xd = g.upload("x", tone, readonly=True)
    ad = g.full("arg", frames * lanes, torch.int32, POISON)
    assert gpu.cfgcall("lockin_i32_arg", lc, sd, xd, ad, lanes, frames, H.FM) == 0, gpu.err()
    pd = g.full("pll state", 9 * lanes, torch.int32, 0).reshape(9, lanes)
    fd = g.full("y", frames * lanes, torch.int32, POISON)
    gpu_call(gpu, "pll1", ba, pd, ad, fd, lanes, frames, H.FM)
    torch.cuda.synchronize()
    g.check("lockin_i32_arg -> pll_i32")
    assert np.array_equal(ad.cpu().numpy().reshape(frames, lanes), arg_o)
    got = fd.cpu().numpy().reshape(frames, lanes)
    assert np.array_equal(got, want) and np.array_equal(pd.cpu().numpy().view(np.uint32), ps)
    # and it does what a PLL is for: the phase of this lock-in's output advances by minus the tone's offset from the LO per sample,
    # and the loop settles to the complement of its input's increment (src/pll.rs:28-31) — the frequency estimate is the offset,
    # to 5 % of the offsets' range (+-2^22)
    settled = got[frames // 2:].astype(np.float64).mean(axis=0)
    assert np.abs(settled - offset).max() < (1 << 22) * 0.05, np.abs(settled - offset).max()


def test_dispatch_per_shape_class(gpu):
    """which stream kernel each shape class took (recorded by the tests above when they ran first; run here when alone)"""
    if not KERNELS:
        for form in FORMS:
            ba, x, st = case(form, 1000, 64, 1)
            for layout in (H.FM, H.LM):
                gpu_run(gpu, form, ba, st.copy(), x, layout)
    assert "pll_i32" in PHASE
    assert KERNELS and all(k.startswith("stream_") for k in KERNELS.values()), sorted(set(KERNELS.values()))
    for key in sorted(KERNELS):
        print(key, KERNELS[key])
