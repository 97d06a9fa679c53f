"""idsp_pfb_f32_process on the GPU, through the C ABI, against the numpy specification (tests/_pfb_spec.py).

Every case compares all of y and every state word with `assert_same_float` (NaN at the same positions, everything else
bit-identical, signed zeros and subnormals included), asserts the kernel's name, allocates through tests/_guard.py (bands
checked; x unchanged when not in place) and starts y from a finite poison.

Time tiles: the FRAME_MAJOR kernel cuts the time axis into segments of 256 frames, the LANE_MAJOR kernel into tiles of 256 frames
(both in the kernel's name); `2 * T + 3` frames cross two boundaries and end ragged."""
import ctypes as C

import numpy as np
import pytest
import torch

from idsp_amd import _abi
from idsp_amd._abi import PFB  # noqa: F401  (the feature's prototype table)
from tests import _float_special as F
from tests import _harness as H
from tests import _pfb_spec as S
from tests._guard import Guards

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
TAPS = [1, 3, 8, 16]
LANES = [1, 29, 64, 65, 200]
NAMES = {
    (H.FM, False): "pfb_frame_major[segment {T} frames]<taps {taps}>",
    (H.FM, True): "pfb_frame_major[unsegmented, in place]<taps {taps}>",
    (H.LM, False): "pfb_lane_major[tile {T} frames]<taps {taps}>",
    (H.LM, True): "pfb_lane_major[tile {T} frames, one workgroup per lane, in place]<taps {taps}>",
}
T = 256  # segment / tile of both kernels, asserted against the names below


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def make_cfg(coeff, dft):
    cfg = _abi.PfbF32()
    cfg.taps, cfg.dft = coeff.shape[0], dft
    for t in range(coeff.shape[0]):
        for m in range(4):
            cfg.coeff[t][m] = float(coeff[t, m])
    return cfg


def to_layout(a, layout):
    """[frames, lanes, 4, 2] -> the flat tensor of `layout`"""
    return np.ascontiguousarray(a if layout == H.FM else np.swapaxes(a, 0, 1)).reshape(-1)


def from_layout(a, layout, frames, lanes):
    a = a.reshape(frames, lanes, 4, 2) if layout == H.FM else np.swapaxes(a.reshape(lanes, frames, 4, 2), 0, 1)
    return np.ascontiguousarray(a)


def gpu_run(gpu, cfg, st, x, layout, inplace=False, chunks=None):
    """x float32 [frames, lanes, 4, 2]; st uint32 [8*taps + 1, lanes], updated; returns y in x's shape.
    chunks: frame counts of consecutive calls on one state (their sum = frames)."""
    frames, lanes = x.shape[:2]
    gs = Guards(DEV)
    sd = gs.upload("state", st)
    outs, f0 = [], 0
    for n in chunks or [frames]:
        g = Guards(DEV)
        xd = g.upload("x", to_layout(x[f0:f0 + n], layout), readonly=not inplace)
        yd = xd if inplace else g.upload("y", F.poison(lanes * n * 8, F32))
        rc = gpu.fn["pfb_f32_process"](C.byref(cfg), _ptr(sd), _ptr(xd), _ptr(yd), lanes, n, layout, None)
        assert rc == 0, gpu.err()
        torch.cuda.synchronize()
        name = gpu.last_kernel()
        what = (name, "dft", cfg.dft, lanes, n, "in place" if inplace else "")
        g.check(what)
        gs.check(what)
        assert name == NAMES[(layout, inplace)].format(T=T, taps=cfg.taps), what
        outs.append(from_layout(yd.cpu().numpy(), layout, n, lanes))
        f0 += n
    assert f0 == frames
    st[...] = sd.cpu().numpy().view(np.uint32)
    return np.concatenate(outs)


def same(want, got, sw, sg, what):
    frames, lanes = want.shape[:2]
    F.assert_same_float(want, got, ("y",) + what, where=lambda i: f"(frame {i // (lanes * 8)}, lane {i // 8 % lanes}, element {i % 8})")
    nt = sw.shape[0] - 1
    F.assert_same_float(sw[:nt].view(F32), sg[:nt].view(F32), ("hist",) + what, where=lambda i: f"(word {i // lanes}, lane {i % lanes})")
    assert np.array_equal(sw[nt], sg[nt]), ("head",) + what


@pytest.mark.parametrize("layout", [H.FM, H.LM])
@pytest.mark.parametrize("taps", TAPS)
def test_equals_the_spec(gpu, taps, layout):
    """lanes 1, 29, 64, 65, 200 x frames 1, taps - 1, taps, taps + 1, 2 * T + 3, dft 0 / 1; random `hist`, every possible head"""
    rng = np.random.default_rng(1000 * taps + layout)
    for frames in sorted({1, max(taps - 1, 1), taps, taps + 1, 2 * T + 3}):
        for lanes in LANES:
            coeff = rng.standard_normal((taps, 4)).astype(F32)
            st = S.random_state(rng, taps, lanes)
            x = rng.standard_normal((frames, lanes, 4, 2)).astype(F32)
            for dft in (0, 1):
                sw, sg = st.copy(), st.copy()
                want = S.bank_np(coeff, dft, sw, x)
                got = gpu_run(gpu, make_cfg(coeff, dft), sg, x, layout)
                same(want, got, sw, sg, (taps, layout, lanes, frames, dft))


@pytest.mark.parametrize("layout", [H.FM, H.LM])
@pytest.mark.parametrize("taps", TAPS)
def test_chunks_equal_one_call(gpu, taps, layout):
    """5 + 1 + 13 + rest, the rest crossing a tile boundary"""
    rng = np.random.default_rng(taps)
    lanes, frames = 65, 19 + T + 7
    coeff = rng.standard_normal((taps, 4)).astype(F32)
    st = S.random_state(rng, taps, lanes)
    x = rng.standard_normal((frames, lanes, 4, 2)).astype(F32)
    sw, s1, s2 = st.copy(), st.copy(), st.copy()
    want = S.bank_np(coeff, 1, sw, x)
    cfg = make_cfg(coeff, 1)
    whole = gpu_run(gpu, cfg, s1, x, layout)
    parts = gpu_run(gpu, cfg, s2, x, layout, chunks=[5, 1, 13, frames - 19])
    same(want, whole, sw, s1, (taps, layout, "one call"))
    same(want, parts, sw, s2, (taps, layout, "5 + 1 + 13 + rest"))


@pytest.mark.parametrize("layout", [H.FM, H.LM])
@pytest.mark.parametrize("taps", TAPS)
def test_in_place(gpu, taps, layout):
    """y == x equals the out-of-place call; 2 * T + 3 frames are more than one time segment of the out-of-place kernels"""
    rng = np.random.default_rng(50 + taps)
    for lanes, frames in ((65, 2 * T + 3), (200, taps + 1), (1, T + 1), (29, 1)):
        coeff = rng.standard_normal((taps, 4)).astype(F32)
        st = S.random_state(rng, taps, lanes)
        x = rng.standard_normal((frames, lanes, 4, 2)).astype(F32)
        for dft in (0, 1):
            sw, s1, s2 = st.copy(), st.copy(), st.copy()
            want = S.bank_np(coeff, dft, sw, x)
            cfg = make_cfg(coeff, dft)
            got = gpu_run(gpu, cfg, s1, x, layout, inplace=True)
            same(want, got, sw, s1, (taps, layout, lanes, frames, dft, "in place"))
            out = gpu_run(gpu, cfg, s2, x, layout)
            same(out, got, s2, s1, (taps, layout, lanes, frames, dft, "in place against out of place"))


@pytest.mark.parametrize("layout", [H.FM, H.LM])
@pytest.mark.parametrize("taps", TAPS)
def test_special_values(gpu, taps, layout):
    """one kind of data per lane (kind = lane % 8): signed zeros, subnormals, huge values, inf, NaN; over a tile boundary"""
    rng = np.random.default_rng(9 * taps)
    coeff = S.coeff_of(S.prototype(taps))
    for lanes, frames, inplace in ((200, T + 9, False), (72, taps + 2, False), (72, T + 9, True)):
        x, kind = F.special_chunks(rng, frames, lanes, 8, F32)
        x = x.reshape(frames, lanes, 4, 2)
        st = np.concatenate([F.special_state(rng, 8 * taps, lanes, kind, F32), (np.arange(lanes) % taps).astype(np.uint32)[None]])
        for dft in (0, 1):
            sw, sg = st.copy(), st.copy()
            want = S.bank_np(coeff, dft, sw, x)
            F.assert_poison_absent(want, (taps, layout, dft))
            assert np.isnan(want).mean() <= 0.5, "at least half of the output elements must be non-NaN"
            got = gpu_run(gpu, make_cfg(coeff, dft), sg, x, layout, inplace=inplace)
            same(want, got, sw, sg, (taps, layout, lanes, frames, dft, "special values", inplace))


def test_head_beyond_taps_is_reduced(gpu):
    """a head >= taps (caller error) is taken modulo taps: no lane reaches outside its own state words"""
    rng = np.random.default_rng(3)
    taps, lanes, frames = 3, 200, 10
    coeff = rng.standard_normal((taps, 4)).astype(F32)
    st = S.random_state(rng, taps, lanes, heads=rng.integers(0, 1 << 32, size=lanes, dtype=np.uint64).astype(np.uint32))
    x = rng.standard_normal((frames, lanes, 4, 2)).astype(F32)
    for layout in (H.FM, H.LM):
        sw, sg = st.copy(), st.copy()
        want = S.bank_np(coeff, 1, sw, x)
        got = gpu_run(gpu, make_cfg(coeff, 1), sg, x, layout)
        same(want, got, sw, sg, ("head >= taps", layout))


def test_argument_errors(gpu):
    """every row returns IDSP_EINVAL with a message and writes nothing (guard bands and poisoned contents)"""
    lanes, frames, taps = 8, 4, 8
    coeff = S.coeff_of(S.prototype(taps))
    g = Guards(DEV)
    sd = g.upload("state", np.zeros((8 * taps + 1, lanes), np.uint32), readonly=True)
    xd = g.upload("x", np.ones(lanes * frames * 8 + 8, F32), readonly=True)
    yd = g.upload("y", F.poison(lanes * frames * 8 + 8, F32), readonly=True)
    ok = make_cfg(coeff, 1)

    def cfg_with(**kw):
        c = make_cfg(coeff, 1)
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    x, y, s = xd.data_ptr(), yd.data_ptr(), sd.data_ptr()
    rows = [
        ("taps 0", cfg_with(taps=0), s, x, y, H.FM), ("taps 17", cfg_with(taps=17), s, x, y, H.FM), ("taps -1", cfg_with(taps=-1), s, x, y, H.LM),
        ("dft 2", cfg_with(dft=2), s, x, y, H.FM), ("dft -1", cfg_with(dft=-1), s, x, y, H.LM),
        ("layout 2", ok, s, x, y, 2), ("layout -1", ok, s, x, y, -1),
        ("state NULL", ok, None, x, y, H.FM), ("x NULL", ok, s, None, y, H.FM), ("y NULL", ok, s, x, None, H.LM),
        ("x off 16-byte grid", ok, s, x + 4, y, H.FM), ("y off 16-byte grid", ok, s, x, y + 8, H.LM),
        ("partial overlap", ok, s, x, x + 32, H.FM), ("partial overlap, y in front", ok, s, x + 32, x, H.LM),
    ]
    for what, cfg, sp, xp, yp, layout in rows:
        rc = gpu.fn["pfb_f32_process"](C.byref(cfg), C.c_void_p(sp), C.c_void_p(xp), C.c_void_p(yp), lanes, frames, layout, None)
        assert rc == _abi.IDSP_EINVAL and gpu.err(), (what, rc)
    assert gpu.fn["pfb_f32_process"](None, C.c_void_p(s), C.c_void_p(x), C.c_void_p(y), lanes, frames, H.FM, None) == _abi.IDSP_EINVAL
    # empty calls launch nothing and succeed, as idsp_fir_sym_f32_process
    assert gpu.fn["pfb_f32_process"](C.byref(ok), C.c_void_p(s), C.c_void_p(x), C.c_void_p(y), lanes, 0, H.FM, None) == 0
    assert gpu.fn["pfb_f32_process"](C.byref(ok), None, None, None, 0, frames, H.LM, None) == 0
    torch.cuda.synchronize()
    g.check("argument errors")


@pytest.mark.parametrize("layout", [H.FM, H.LM])
def test_reference_routing_test(gpu, layout):
    """`routes_center_tones_to_expected_bins` (examples/polyphase_channelizer.rs:166-178) on the device: 256 lanes, the tone chosen
    by lane % 4, the library's prototype, `BankState::default()`; bit-equal to the specification, and the reference's two assertions
    hold in every lane"""
    lanes = 256
    cfg = _abi.PfbF32()
    assert gpu.fn["pfb_prototype_f32"](8, C.byref(cfg)) == 0
    coeff = np.array([[cfg.coeff[t][m] for m in range(4)] for t in range(8)], F32)
    tones = [S.frames_of(S.tone(freq, 4096)) for freq, _ in S.ROUTING]
    x = np.ascontiguousarray(np.stack([tones[lane % 4] for lane in range(lanes)], axis=1))
    sw, sg = np.zeros((65, lanes), np.uint32), np.zeros((65, lanes), np.uint32)
    want = S.bank_np(coeff, 1, sw, x)
    got = gpu_run(gpu, cfg, sg, x, layout)
    same(want, got, sw, sg, ("routing", layout))
    p = S.channel_powers(got)
    for lane in range(lanes):
        S.assert_routed(p[lane], S.ROUTING[lane % 4][1])

