"""The polyphase channelizer's specification (tests/_pfb_spec.py) held against itself and against the reference's own test, plus
the host-side entries of the library that need no GPU (idsp_pfb_prototype_f32, idsp_pfb_state_words).

The two restatements (per-lane scalar with the circular bank; all lanes with direct indexing) must agree under
`assert_same_float` in y and in every state word.  The pin is `routes_center_tones_to_expected_bins`
(examples/polyphase_channelizer.rs:166-178).

Not checked here: bit equality of the prototype with the reference's own libm (`f32::sin` / `f32::cos` of the Rust build) — there
is no Rust toolchain to run it; the prototype is held to its defining properties instead (sum, symmetry, routing)."""
import ctypes as C

import numpy as np
import pytest

from idsp_amd import _abi
from idsp_amd._abi import PFB  # the feature's prototype table
from tests import _float_special as F
from tests import _pfb_spec as S

F32 = np.float32


def both(coeff, dft, st, x):
    """y and the new state from both restatements, compared; returns (y, state)"""
    s1, s2 = st.copy(), st.copy()
    y2 = S.bank_np(coeff, dft, s2, x)
    y1 = np.empty_like(x)
    for lane in range(x.shape[1]):
        y1[:, lane] = S.bank_scalar(coeff, dft, s1, lane, np.ascontiguousarray(x[:, lane]))
    F.assert_same_float(y1, y2, "y, scalar against vectorised")
    nt = 8 * coeff.shape[0]
    F.assert_same_float(s1[:nt].view(F32), s2[:nt].view(F32), "hist, scalar against vectorised")
    assert np.array_equal(s1[nt], s2[nt]), "head"
    return y2, s2


@pytest.mark.parametrize("dft", [0, 1])
@pytest.mark.parametrize("taps", [1, 3, 8, 16])
def test_restatements_agree_on_random_data(taps, dft):
    rng = np.random.default_rng(100 * taps + dft)
    lanes, frames = 2 * taps + 1, 2 * taps + 5
    coeff = rng.standard_normal((taps, 4)).astype(F32)
    st = S.random_state(rng, taps, lanes)  # every possible head
    x = rng.standard_normal((frames, lanes, 4, 2)).astype(F32)
    both(coeff, dft, st, x)


@pytest.mark.parametrize("dft", [0, 1])
@pytest.mark.parametrize("taps", [1, 3, 8, 16])
def test_restatements_agree_on_special_values(taps, dft):
    rng = np.random.default_rng(7 * taps + dft)
    lanes, frames = 16, taps + 9
    x, kind = F.special_chunks(rng, frames, lanes, 8, F32)
    st = np.concatenate([F.special_state(rng, 8 * taps, lanes, kind, F32), (np.arange(lanes) % taps).astype(np.uint32)[None]])
    coeff = S.coeff_of(S.prototype(taps))
    y, _ = both(coeff, dft, st, x.reshape(frames, lanes, 4, 2))
    census = F.classes(y)
    print(taps, dft, census)
    assert census["nan"] <= F.NAN_CAP and census["-0"] + census["+0"] > 0 and census["subnormal"] > 0, census


@pytest.mark.parametrize("taps", [1, 3, 8, 16])
def test_chunks_equal_one_call(taps):
    rng = np.random.default_rng(taps)
    lanes, frames = 5, 40
    coeff = rng.standard_normal((taps, 4)).astype(F32)
    st = S.random_state(rng, taps, lanes)
    x = rng.standard_normal((frames, lanes, 4, 2)).astype(F32)
    s1, s2 = st.copy(), st.copy()
    whole = S.bank_np(coeff, 1, s1, x)
    parts, f0 = [], 0
    for n in (5, 1, 13, frames - 19):
        parts.append(S.bank_np(coeff, 1, s2, x[f0:f0 + n]))
        f0 += n
    F.assert_same_float(whole, np.concatenate(parts), "5 + 1 + 13 + rest")
    assert np.array_equal(s1, s2)
    s3 = st.copy()
    y3 = np.concatenate([S.bank_scalar(coeff, 1, s3, 2, x[:6, 2]), S.bank_scalar(coeff, 1, s3, 2, x[6:, 2])])
    F.assert_same_float(whole[:, 2], y3, "scalar, 6 + rest")
    assert np.array_equal(s3[:, 2], s1[:, 2])


def routing(coeff):
    """:166-178 through the specification: one lane per tone, 4096 samples, the first 128 output frames dropped"""
    x = np.stack([S.frames_of(S.tone(freq, 4096)) for freq, _ in S.ROUTING], axis=1)  # [1024, 4, 4, 2]
    st = np.zeros((8 * coeff.shape[0] + 1, len(S.ROUTING)), np.uint32)  # `BankState::default()`
    y = S.bank_np(coeff, 1, st, x)
    p = S.channel_powers(y)
    for lane, (_, want) in enumerate(S.ROUTING):
        S.assert_routed(p[lane], want)
    return x, y, p


def test_reference_routing_test_on_the_specification():
    coeff = S.coeff_of(S.prototype(8))
    x, y, p = routing(coeff)
    print("channel powers per tone:", p.tolist())
    st = np.zeros((65, 4), np.uint32)
    y1 = S.bank_scalar(coeff, 1, st, 1, np.ascontiguousarray(x[:, 1]))  # the scalar restatement on the 0.25 tone
    F.assert_same_float(y1, y[:, 1], "routing, scalar against vectorised")


# ------------------------------------------------------------------------------------------- the library's host-side entries
@pytest.fixture(scope="module")
def fn():
    from idsp_amd._lib import load

    return load()[0]


def lib_prototype(fn, taps):
    cfg = _abi.PfbF32()
    assert fn["pfb_prototype_f32"](taps, C.byref(cfg)) == 0
    assert cfg.taps == taps and cfg.dft == 1
    return cfg, np.array([[cfg.coeff[t][m] for m in range(4)] for t in range(_abi.PFB_MAX_TAPS)], F32)


def test_library_prototype(fn):
    assert set(PFB) == {"pfb_state_words", "pfb_prototype_f32", "pfb_f32_process"}
    cfg, c = lib_prototype(fn, 8)
    h = c[:8].reshape(-1)
    s = F32(0)
    for v in h:
        s = F32(s + v)
    print("sum", float(s), "asymmetry", float(np.abs(h - h[::-1]).max()), "against numpy f32", float(np.abs(h - S.prototype(8)).max()))
    assert abs(float(s) - 1.0) <= 2.0 ** -22
    assert np.all(np.abs(h - h[::-1]) <= 1e-7)
    assert np.array_equal(c[:8], S.coeff_of(h)) and not c[8:].any()  # coeff[tap][m] == h[4*tap + m]
    assert np.abs(h - S.prototype(8)).max() <= 2.0 ** -22  # two libms, a few ulp of the largest coefficient (0.22)
    routing(np.ascontiguousarray(c[:8]))
    for taps in (1, 3, 16):
        _, c = lib_prototype(fn, taps)
        assert np.abs(c[:taps].reshape(-1) - S.prototype(taps)).max() <= 2.0 ** -21 and not c[taps:].any(), taps
    for taps in (0, 17, -1):
        assert fn["pfb_prototype_f32"](taps, C.byref(_abi.PfbF32())) == _abi.IDSP_EINVAL
        assert b"taps" in fn["last_error"]()
    assert fn["pfb_prototype_f32"](8, None) == _abi.IDSP_EINVAL


def test_library_state_words(fn):
    cfg = _abi.PfbF32()
    for taps in range(1, 17):
        cfg.taps = taps
        assert fn["pfb_state_words"](C.byref(cfg)) == 8 * taps + 1
    for taps in (0, 17):
        cfg.taps = taps
        assert fn["pfb_state_words"](C.byref(cfg)) == 0
    assert fn["pfb_state_words"](None) == 0
    assert C.sizeof(_abi.PfbF32) == 8 + 4 * 4 * 16


def test_rust_struct_matches_ctypes():
    """rust/idsp-hip-sys/src/pfb.rs is what tools/gen_rust_sys.py generates, and its `#[repr(C)]` field list implies ctypes' size"""
    import os
    import re
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "rust", "idsp-hip-sys", "src", "pfb.rs")).read()
    gen = subprocess.run([sys.executable, "-c", "import sys; sys.path.insert(0, 'tools'); import gen_rust_sys as g; sys.stdout.write(g.generate_side('pfb'))"],
                         cwd=root, capture_output=True, text=True, check=True).stdout
    assert gen == src, "rust/idsp-hip-sys/src/pfb.rs is stale: run python tools/gen_rust_sys.py"
    (name, body), = re.findall(r"pub struct (\w+) \{\n(.*?)\n\}", src, flags=re.S)
    assert name == "IdspPfbF32"
    fields = re.findall(r"pub (\w+): (.+),", body)
    assert fields == [("taps", "i32"), ("dft", "i32"), ("coeff", "[[f32; 4]; 16]")]
    assert 4 + 4 + 4 * 4 * 16 == C.sizeof(_abi.PfbF32)
    lib = open(os.path.join(root, "rust", "idsp-hip-sys", "src", "lib.rs")).read()
    assert "mod pfb;\npub use pfb::*;" in lib and "cfg: *const IdspPfbF32" in lib
