"""The host side of idsp_biquad_i16_df1 / _df1_clamp / _from_sos without a GPU: every call here returns before a launch (the pointers
are numbers that are only compared, never followed).  Needs the built library (`make all`)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from idsp_amd import _abi
from tests import _biquad_i16_spec as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FM, LM = _abi.FRAME_MAJOR, _abi.LANE_MAJOR
X, Y, ST = 0x10000, 0x20000, 0x30000  # three far-apart "device" addresses


@pytest.fixture(scope="module")
def fn():
    from idsp_amd._lib import load

    return load()[0]


def _cfg(n, clamped=False, frac=13):
    arr = ((_abi.BiquadClampI16 if clamped else _abi.BiquadI16) * max(n, 1))()
    for a in arr:
        a.ba[:] = [553, 1105, 553, 9363, -3382]
        a.frac = frac
        if clamped:
            a.u, a.min, a.max = 7, 100, -100
    return arr


def _call(fn, n, st, x, xp, y, yp, lanes, frames, layout, clamped=False, cfg="own"):
    cfg = _cfg(n, clamped) if cfg == "own" else cfg
    return fn["biquad_i16_df1_clamp" if clamped else "biquad_i16_df1"](cfg, n, C.c_void_p(st) if st else None, C.c_void_p(x) if x else None, xp,
                                                                       C.c_void_p(y) if y else None, yp, lanes, frames, layout, None)


def _einval(fn, *args, **kw):
    rc = _call(fn, *args, **kw)
    return rc == _abi.IDSP_EINVAL and len(fn["last_error"]()) > 0


def test_prototypes_and_struct_sizes():
    assert set(_abi.BIQUAD_I16) == {"biquad_i16_from_sos", "biquad_i16_state_words", "biquad_i16_df1", "biquad_i16_df1_clamp"}
    assert set(_abi.BIQUAD_I16) <= set(_abi.UTILS)
    assert not set(_abi.BIQUAD_I16) & (set(_abi.PROCESSING) | set(_abi.HELPERS))  # those promise a twin in the checker library
    assert C.sizeof(_abi.BiquadI16) == 12 and C.sizeof(_abi.BiquadClampI16) == 18
    assert _abi.ABI_VERSION == 4


def test_state_words(fn):
    assert [fn["biquad_i16_state_words"](n) for n in (0, 1, 2, 9, 64)] == [0, 4, 8, 36, 256]
    assert fn["version"]() == 4


def test_from_sos_equals_the_specification(fn):
    """2000 random rows, among them saturating, tying, NaN and inf ones and a0 = 0, at four F"""
    sos = S.sos_rows(np.random.default_rng(2), 2000)
    out = _abi.BiquadI16()
    seen = set()
    for frac in (0, 13, 15, 31):
        want = S.from_sos_np(sos, frac)
        for row, w in zip(sos, want):
            assert fn["biquad_i16_from_sos"]((C.c_double * 6)(*row), frac, C.byref(out)) == 0
            assert list(out.ba) == w.tolist() and out.frac == frac, (row, frac)
            seen |= set(w.tolist())
    assert {S.I16_MIN, S.I16_MAX, 0} <= seen
    lp = [0.06745527388907189, 0.13491054777814377, 0.06745527388907189, 1.0, -1.1429805025399011, 0.4128015980961886]
    assert fn["biquad_i16_from_sos"]((C.c_double * 6)(*lp), 13, C.byref(out)) == 0 and list(out.ba) == [553, 1105, 553, 9363, -3382]
    for bad in ((None, 13, C.byref(out)), ((C.c_double * 6)(*lp), 13, None), ((C.c_double * 6)(*lp), -1, C.byref(out)),
                ((C.c_double * 6)(*lp), 32, C.byref(out))):
        assert fn["biquad_i16_from_sos"](*bad) == _abi.IDSP_EINVAL and fn["last_error"]()


@pytest.mark.parametrize("clamped", [False, True])
@pytest.mark.parametrize("args", [
    (2, ST, X, 0, Y, 0, 4, 4, 2), (2, ST, X, 0, Y, 0, 4, 4, -1),            # layout
    (65, ST, X, 0, Y, 0, 4, 4, FM),                                         # n > IDSP_MAX_SECTIONS
    (2, ST, None, 0, Y, 0, 4, 4, FM), (2, ST, X, 0, None, 0, 4, 4, LM),     # NULL x / y
    (2, None, X, 0, Y, 0, 4, 4, FM),                                        # NULL state with n > 0
    (2, ST, X, 3, Y, 0, 4, 9, FM), (2, ST, X, 0, Y, 3, 4, 9, FM),           # pitch < row (FrameMajor: row = lanes)
    (2, ST, X, 8, Y, 0, 4, 9, LM), (2, ST, X, 0, Y, 8, 4, 9, LM),           # (LaneMajor: row = frames)
    (2, ST, X + 1, 0, Y, 0, 4, 4, FM), (2, ST, X, 0, Y + 1, 0, 4, 4, LM),   # an odd address
    (2, ST, X + 3, 0, X + 3, 0, 4, 4, FM), (0, ST, X + 1, 0, Y, 0, 4, 4, FM),
    (2, ST, X, 0, X, 5, 4, 4, FM), (2, ST, X, 6, X, 0, 4, 4, LM),           # y == x with two pitches
    (2, ST, X, 4, X, 5, 4, 4, FM),
    (2, ST, X, 0, X + 2, 0, 4, 4, FM), (2, ST, X, 0, X + 30, 0, 4, 4, LM),  # y one element into x / on its last element
    (2, ST, X + 30, 0, X, 0, 4, 4, FM),                                     # x starts on the last element of y
    (2, ST, X, 8, X + 8, 8, 4, 4, FM),                                      # y rows in the gaps of a pitched x: the EXTENTS overlap
    (0, ST, X, 0, X + 2, 0, 4, 4, FM),                                      # ... also for the copy of n == 0
    (2, ST, X, 1 << 62, Y, 0, 4, 4, FM),                                    # an extent past size_t
])
def test_einval(fn, args, clamped):
    assert _einval(fn, *args, clamped=clamped), args


def test_einval_frac_and_cfg(fn):
    for clamped in (False, True):
        for frac in (-1, 32, 1000, -32768):
            cfg = _cfg(3, clamped)
            cfg[2].frac = frac
            assert _einval(fn, 3, ST, X, 0, Y, 0, 4, 4, FM, clamped=clamped, cfg=cfg), frac
            assert "frac" in fn["last_error"]().decode()
            assert _call(fn, 2, ST, X, 0, Y, 0, 0, 4, FM, clamped=clamped, cfg=cfg) == 0  # the section with it does not run
        assert _einval(fn, 1, ST, X, 0, Y, 0, 4, 4, FM, clamped=clamped, cfg=None)       # NULL cfg with n > 0
        for frac in (0, 31):
            assert _call(fn, 1, ST, X, 0, Y, 0, 0, 0, FM, clamped=clamped, cfg=_cfg(1, clamped, frac)) == 0


def test_inplace_rule_accepts_one_pitch(fn):
    """y == x passes the checks when both pitches name one pitch, 0 counting as the row length: seen on calls with nothing to launch
    (lanes = 0 ends a call before the overlap test, so the accepted side is held on the device: tests/test_gpu_biquad_i16.py)"""
    assert _call(fn, 2, ST, X, 0, X, 0, 0, 4, FM) == 0 and _call(fn, 2, ST, X, 9, X, 9, 4, 0, LM) == 0


def test_empty_calls(fn):
    assert _call(fn, 2, ST, X, 0, Y, 0, 0, 4, FM) == 0 and _call(fn, 2, ST, X, 0, Y, 0, 4, 0, LM, clamped=True) == 0
    assert _call(fn, 0, None, None, 0, None, 0, 0, 0, FM, cfg=None) == 0
    assert _call(fn, 2, None, X, 0, Y, 0, 0, 5, FM) == 0   # no lanes: no state
    assert _call(fn, 2, ST, X, 7, Y, 1, 0, 5, FM) == 0     # FrameMajor row = lanes = 0: any pitch covers it
    assert _call(fn, 2, ST, X + 1, 0, Y + 1, 0, 0, 5, LM) == 0  # nothing would be touched


def test_python_mirror_without_device():
    from idsp_amd import process as P

    assert "BiquadQ16" in P.__all__ and "BiquadQ16Lanes" in P.__all__ and "Biquad<Q16<F>>" in P.__doc__
    for bad in (-1, 32, 2.0, "3", None, True):
        with pytest.raises(ValueError):
            P.BiquadQ16([1, 2, 3, 4, 5], bad)
    with pytest.raises(ValueError):
        P.BiquadQ16([1, 2, 3, 4], 13)
    with pytest.raises(ValueError):
        P.BiquadQ16([1, 2, 3, 4, 32768], 13)
    with pytest.raises(ValueError):
        P.BiquadQ16([1, 2, 3, 4, 5], 13, u=-32769)
    q = P.BiquadQ16([1, 2, 3, 4, -32768], 31)
    assert not q.clamp and (q.u, q.min, q.max) == (0, -32768, 32767)
    k = P.BiquadQ16([1, 2, 3, 4, 5], 0, max=5)
    assert k.clamp and (k.u, k.min, k.max) == (0, -32768, 5)
    assert P.BiquadQ16.from_sos([0.06745527388907189, 0.13491054777814377, 0.06745527388907189, 1.0, -1.1429805025399011, 0.4128015980961886],
                                13).ba == [553, 1105, 553, 9363, -3382]
    with pytest.raises(ValueError):
        q.lanes(4, device="cpu")
    with pytest.raises(ValueError):
        q.lanes(-1)
    with pytest.raises(ValueError):
        P.BiquadQ16Lanes([q, k], 4)  # plain and clamped mixed
    with pytest.raises(ValueError):
        P.BiquadQ16Lanes([q] * 65, 4)


def test_cpp_host_program():
    """tests/cpp/test_biquad_i16_host.cpp: the same table through the C ABI and `BiquadI16Lanes` of include/idsp_hip.hpp, before anything
    touches a device (plain g++ against the C ABI)"""
    exe = os.path.join(ROOT, "build", "test_biquad_i16_host")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Iinclude", "tests/cpp/test_biquad_i16_host.cpp", "-Lidsp_amd/lib", "-lidsp_hip",
                    "-Wl,-rpath,$ORIGIN/../idsp_amd/lib", "-o", exe], cwd=ROOT, check=True)
    r = subprocess.run([exe], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "biquad i16 host tests passed" in r.stdout


def test_rust_structs_match_ctypes():
    """rust/idsp-hip-sys/src/biquad_i16.rs is what tools/gen_rust_sys.py generates, and its `#[repr(C)]` field lists imply ctypes' sizes"""
    import re
    import sys

    src = open(os.path.join(ROOT, "rust", "idsp-hip-sys", "src", "biquad_i16.rs")).read()
    gen = subprocess.run([sys.executable, "-c", "import sys; sys.path.insert(0, 'tools'); import gen_rust_sys as g; sys.stdout.write(g.generate_side('biquad_i16'))"],
                         cwd=ROOT, capture_output=True, text=True, check=True).stdout
    assert gen == src, "rust/idsp-hip-sys/src/biquad_i16.rs is stale: run python tools/gen_rust_sys.py"
    found = {name: re.findall(r"pub (\w+): (.+),", body) for name, body in re.findall(r"pub struct (\w+) \{\n(.*?)\n\}", src, flags=re.S)}
    assert found == {"IdspBiquadI16": [("ba", "[i16; 5]"), ("frac", "i16")],
                     "IdspBiquadClampI16": [("ba", "[i16; 5]"), ("frac", "i16"), ("u", "i16"), ("min", "i16"), ("max", "i16")]}
    assert [f[0] for f in _abi.BiquadI16._fields_] == [f[0] for f in found["IdspBiquadI16"]]
    assert [f[0] for f in _abi.BiquadClampI16._fields_] == [f[0] for f in found["IdspBiquadClampI16"]]
    lib = open(os.path.join(ROOT, "rust", "idsp-hip-sys", "src", "lib.rs")).read()
    assert "mod biquad_i16;\npub use biquad_i16::*;" in lib and "cfg: *const IdspBiquadI16" in lib and "cfg: *const IdspBiquadClampI16" in lib
    assert "pub fn idsp_biquad_i16_df1_clamp(" in lib and '"idsp_biquad_i16_from_sos",' in lib
