"""The host side of idsp_biquad_i16_df1_bylane / _df1_clamp_bylane / idsp_biquad_i16_bank_from_sos without a GPU: every call here returns
before a launch (the device pointers are numbers that are only compared, never followed; the planes bank_from_sos writes are host memory).
Needs the built library (`make all`)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from idsp_amd import _abi
from tests import _biquad_i16_spec as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FM, LM = _abi.FRAME_MAJOR, _abi.LANE_MAJOR
X, Y, ST, CF = 0x10000, 0x20000, 0x30000, 0x40000  # four far-apart "device" addresses
FRAMES = "biquad_i16_bylane_frame_major"
DWORDS, HALVES = "biquad_i16_bylane_lane_major[dword runs]", "biquad_i16_bylane_lane_major[half runs]"
A = 0x7F0000001000


@pytest.fixture(scope="module")
def fn():
    from idsp_amd._lib import load

    return load()[0]


def _p(v):
    return C.c_void_p(v) if v else None


def _call(fn, coef, frac, n, st, x, xp, y, yp, lanes, frames, layout, clamped=False):
    return fn["biquad_i16_df1_clamp_bylane" if clamped else "biquad_i16_df1_bylane"](_p(coef), frac, n, _p(st), _p(x), xp, _p(y), yp, lanes, frames,
                                                                                     layout, None)


def _einval(fn, *args, **kw):
    return _call(fn, *args, **kw) == _abi.IDSP_EINVAL and len(fn["last_error"]()) > 0


def _bank(fn, sos, frac, cv):
    """sos [lanes, n, 6] -> (status, coef [n, cv, lanes] int16)"""
    lanes, n = sos.shape[:2]
    sos = np.ascontiguousarray(sos, np.float64)
    coef = np.full((n, cv, lanes), 12345, np.int16)
    rc = fn["biquad_i16_bank_from_sos"](sos.ctypes.data_as(C.c_void_p), lanes, n, frac, cv, coef.ctypes.data_as(C.c_void_p))
    return rc, coef


def test_prototypes():
    assert set(_abi.BIQUAD_I16_BYLANE) == {"biquad_i16_df1_bylane", "biquad_i16_df1_clamp_bylane", "biquad_i16_bank_from_sos"}
    assert set(_abi.BIQUAD_I16_BYLANE) <= set(_abi.UTILS)
    assert not set(_abi.BIQUAD_I16_BYLANE) & (set(_abi.PROCESSING) | set(_abi.HELPERS))  # those promise a twin in the checker library
    assert _abi.ABI_VERSION == 4


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("lanes", [1, 3, 64])
def test_bank_from_sos_equals_the_specification(fn, lanes, n):
    """random rows, among them saturating, tying, NaN and inf ones and a0 = 0, at EVERY frac, element by element in the plane layout"""
    sos = S.sos_rows(np.random.default_rng(10 * lanes + n), max(lanes * n, 40))[:lanes * n].reshape(lanes, n, 6)
    sos[0, 0] = [4.0, -4.0 - 1.0 / 8192, np.nan, 1.0, np.inf, 3.9998779296875]  # saturates both ways at F = 13, NaN -> 0
    seen = set()
    for frac in range(32):
        for cv in (5, 8):
            rc, coef = _bank(fn, sos, frac, cv)
            assert rc == 0, fn["last_error"]()
            flat = coef.reshape(-1)
            for l in range(lanes):
                for k in range(n):
                    if sos[l, k, 3] == 0.0:  # 1 / 0 raises in S.from_sos's Python floats: those rows are held by S.from_sos_np below
                        continue
                    want = S.from_sos(sos[l, k].tolist(), frac)
                    got = [int(flat[(k * cv + v) * lanes + l]) for v in range(5)]  # coef[(k*CV + v)*lanes + l]
                    assert got == want, (lanes, n, frac, cv, l, k)
                    seen |= set(want)
            assert np.array_equal(coef[:, :5].transpose(2, 0, 1).reshape(-1, 5), S.from_sos_np(sos.reshape(-1, 6), frac))
            if cv == 8:  # BiquadClamp::default
                assert (coef[:, 5] == 0).all() and (coef[:, 6] == S.I16_MIN).all() and (coef[:, 7] == S.I16_MAX).all()
    assert {S.I16_MIN, S.I16_MAX, 0} <= seen


def test_bank_from_sos_is_from_sos(fn):
    """the same function as idsp_biquad_i16_from_sos: every section of a bank equals the one-section entry's answer"""
    sos = S.sos_rows(np.random.default_rng(5), 600).reshape(200, 3, 6)
    out = _abi.BiquadI16()
    for frac in (0, 13, 31):
        rc, coef = _bank(fn, sos, frac, 5)
        assert rc == 0
        for l in range(200):
            for k in range(3):
                assert fn["biquad_i16_from_sos"]((C.c_double * 6)(*sos[l, k]), frac, C.byref(out)) == 0
                assert coef[k, :, l].tolist() == list(out.ba), (frac, l, k)


def test_bank_from_sos_einval(fn):
    sos = np.ones((2, 2, 6))
    coef = np.full(2 * 8 * 2, 12345, np.int16)
    s, c = sos.ctypes.data_as(C.c_void_p), coef.ctypes.data_as(C.c_void_p)
    bank = fn["biquad_i16_bank_from_sos"]
    for bad in ((None, 2, 2, 13, 5, c), (s, 2, 2, 13, 5, None), (s, 2, 2, -1, 5, c), (s, 2, 2, 32, 5, c), (s, 2, 2, 13, 0, c), (s, 2, 2, 13, 6, c),
                (s, 2, 2, 13, 7, c), (s, 2, 2, 13, 9, c), (s, 1, _abi.MAX_SECTIONS + 1, 13, 5, c)):
        assert bank(*bad) == _abi.IDSP_EINVAL and fn["last_error"](), bad
    assert (coef == 12345).all()  # nothing written
    assert bank(None, 0, 2, 13, 5, None) == 0 and bank(None, 2, 0, 13, 8, None) == 0  # an empty bank
    assert bank(s, 2, 2, 0, 5, c) == 0 and bank(s, 2, 2, 31, 8, c) == 0


@pytest.mark.parametrize("clamped", [False, True])
@pytest.mark.parametrize("args", [
    (None, 13, 2, ST, X, 0, Y, 0, 4, 4, FM), (None, 13, 1, ST, X, 0, Y, 0, 1, 1, LM),   # NULL coef with n > 0 and lanes > 0
    (CF + 1, 13, 2, ST, X, 0, Y, 0, 4, 4, FM), (CF + 3, 13, 2, ST, X, 0, Y, 0, 4, 4, LM),  # an odd coef address
    (CF + 1, 13, 0, ST, X, 0, Y, 0, 4, 4, FM),
    (CF, -1, 2, ST, X, 0, Y, 0, 4, 4, FM), (CF, 32, 2, ST, X, 0, Y, 0, 4, 4, LM),       # frac
    (CF, 13, 2, ST, X, 0, Y, 0, 4, 4, 2), (CF, 13, 2, ST, X, 0, Y, 0, 4, 4, -1),        # layout
    (CF, 13, 65, ST, X, 0, Y, 0, 4, 4, FM),                                             # n > IDSP_MAX_SECTIONS
    (CF, 13, 2, ST, None, 0, Y, 0, 4, 4, FM), (CF, 13, 2, ST, X, 0, None, 0, 4, 4, LM),  # NULL x / y
    (CF, 13, 2, None, X, 0, Y, 0, 4, 4, FM),                                            # NULL state with n > 0
    (CF, 13, 2, ST, X, 3, Y, 0, 4, 9, FM), (CF, 13, 2, ST, X, 0, Y, 3, 4, 9, FM),       # pitch < row
    (CF, 13, 2, ST, X, 8, Y, 0, 4, 9, LM), (CF, 13, 2, ST, X, 0, Y, 8, 4, 9, LM),
    (CF, 13, 2, ST, X + 1, 0, Y, 0, 4, 4, FM), (CF, 13, 2, ST, X, 0, Y + 1, 0, 4, 4, LM),  # an odd x / y address
    (CF, 13, 2, ST, X, 0, X, 5, 4, 4, FM), (CF, 13, 2, ST, X, 6, X, 0, 4, 4, LM),       # y == x with two pitches
    (CF, 13, 2, ST, X, 0, X + 2, 0, 4, 4, FM), (CF, 13, 2, ST, X + 30, 0, X, 0, 4, 4, FM),  # partial overlaps
    (CF, 13, 2, ST, X, 8, X + 8, 8, 4, 4, FM),                                          # y rows in the gaps of a pitched x
    (CF, 13, 0, ST, X, 0, X + 2, 0, 4, 4, FM),                                          # ... also for the copy of n == 0
    (CF, 13, 2, ST, X, 1 << 62, Y, 0, 4, 4, FM),                                        # an extent past size_t
])
def test_einval(fn, args, clamped):
    assert _einval(fn, *args, clamped=clamped), args


def test_empty_calls_and_the_inplace_rule(fn):
    assert _call(fn, CF, 13, 2, ST, X, 0, Y, 0, 0, 4, FM) == 0 and _call(fn, CF, 13, 2, ST, X, 0, Y, 0, 4, 0, LM, clamped=True) == 0
    assert _call(fn, None, 0, 0, None, None, 0, None, 0, 0, 0, FM) == 0
    assert _call(fn, None, 31, 2, None, X, 0, Y, 0, 0, 5, FM) == 0   # no lanes: no planes, no state
    assert _call(fn, CF, 13, 2, ST, X, 7, Y, 1, 0, 5, FM) == 0       # FrameMajor row = lanes = 0: any pitch covers it
    assert _call(fn, CF, 13, 2, ST, X, 0, X, 0, 0, 4, FM) == 0 and _call(fn, CF, 13, 2, ST, X, 9, X, 9, 4, 0, LM) == 0  # y == x, one pitch
    assert _call(fn, CF + 2, 13, 2, ST, X, 0, Y, 0, 4, 0, LM) == 0   # coef on the 2-byte grid, off the 4-byte one


@pytest.fixture(scope="module")
def cli():
    exe = os.path.join(ROOT, "build", "biquad_i16_bylane_plan_cli")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Iinclude", "tests/cpp/biquad_i16_bylane_plan_cli.cpp", "-o", exe], cwd=ROOT, check=True)

    def ask(*cases):
        text = "".join(" ".join(str(v) for v in c) + "\n" for c in cases)
        r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60, check=True)
        out = []
        for ln in r.stdout.splitlines():
            name, shared, rest = ln.split("\t")
            out.append((name, shared, dict((k, int(v)) for k, v in (kv.split("=") for kv in rest.split()))))
        assert len(out) == len(cases), r.stdout
        return out

    return ask


def test_kernel_names_follow_the_form_rule(cli):
    """`plan_biquad_i16_bylane` (idsp_amd/csrc/biquad_i16_plan.h) on the CPU: the by-lane names, on the form, grid and block of the shared
    entry's plan for the same addresses and pitches — all 2 x 4 x 4 x 2 x 2 x 2 residues, the FrameMajor workgroup step, the switch"""
    cases, want = [], []
    for layout in ("FM", "LM"):
        for xo in (0, 2, 4, 6):
            for yo in (0, 2, 4, 6):
                for xl in (1000, 1001):
                    for yl in (1000, 1003):
                        for lanes in (998, 999):
                            cases.append((layout, lanes, A + xo, A + 0x10000 + yo, xl, yl))
                            grid4 = xo % 4 == 0 and yo % 4 == 0 and xl % 2 == 0 and yl % 2 == 0
                            want.append(((DWORDS if grid4 else HALVES) if layout == "LM" else FRAMES, -(-lanes // 64)))
    for (name, shared, p), w, c in zip(cli(*cases), want, cases):
        assert (name, p["grid"]) == w and p["same"] == 1, c
        assert name == shared.replace("biquad_i16_", "biquad_i16_bylane_"), c
    got = cli(("FM", 65535, A, A + 64, 65535, 65535), ("FM", 65536, A, A, 65536, 65536), ("FM", 65537, A + 2, A + 6, 65538, 65539),
              ("FM", 16384, A, A, 16384, 16384, "fm_block=256"), ("LM", 65537, A, A, 4098, 4098), ("LM", 65, A + 2, A + 4, 4096, 4096))
    assert [(g[0], g[2]["form"], g[2]["grid"], g[2]["block"], g[2]["same"]) for g in got] == [
        (FRAMES, 1, 1024, 64, 1), (FRAMES, 1, 256, 256, 1), (FRAMES, 1, 257, 256, 1), (FRAMES, 1, 64, 256, 1), (DWORDS, 2, 1025, 64, 1), (HALVES, 3, 2, 64, 1)]


def test_python_mirror_without_device():
    from idsp_amd import process as P

    assert "BiquadQ16ByLane" in P.__all__ and "BiquadQ16ByLane" in P.__doc__
    a, b = P.BiquadQ16([1, 2, 3, 4, 5], 13), P.BiquadQ16([5, 4, 3, 2, 1], 13)
    k = P.BiquadQ16([1, 2, 3, 4, 5], 13, u=7)
    for bad in ([], [[]], [[a, b], [a]], [a, k], [[a, k]], [a, P.BiquadQ16([1, 2, 3, 4, 5], 14)], [[a] * (_abi.MAX_SECTIONS + 1)], [3]):
        with pytest.raises(ValueError):
            P.BiquadQ16ByLane(bad)
    with pytest.raises(ValueError):
        P.BiquadQ16ByLane([a, b], device="cpu")
    for bad in (dict(sos=np.ones((2, 6)), frac=13), dict(sos=np.ones((2, 1, 5)), frac=13), dict(sos=np.ones((2, 1, 6)), frac=32),
                dict(sos=np.ones((0, 1, 6)), frac=13), dict(sos=np.ones((2, 0, 6)), frac=13), dict(sos=np.ones((2, 1, 6)), frac=13, device="cpu")):
        with pytest.raises(ValueError):
            P.BiquadQ16ByLane.from_sos(**bad)
    planes = P.BiquadQ16ByLane._planes([a, b], 2, False, 13)
    assert planes.tolist() == [[1, 2, 3, 4, 5], [5, 4, 3, 2, 1]]
    assert P.BiquadQ16ByLane._planes([k], 1, True, 13).tolist() == [[1, 2, 3, 4, 5, 7, -32768, 32767]]


def test_cpp_host_program():
    """tests/cpp/test_biquad_i16_bylane_host.cpp: the same table through the C ABI and `BiquadI16ByLane` of include/idsp_hip.hpp, before
    anything touches a device (plain g++ against the C ABI)"""
    exe = os.path.join(ROOT, "build", "test_biquad_i16_bylane_host")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Iinclude", "tests/cpp/test_biquad_i16_bylane_host.cpp", "-Lidsp_amd/lib", "-lidsp_hip",
                    "-Wl,-rpath,$ORIGIN/../idsp_amd/lib", "-o", exe], cwd=ROOT, check=True)
    r = subprocess.run([exe], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "biquad i16 by-lane host tests passed" in r.stdout


def test_rust_sys_declares_the_entries():
    lib = open(os.path.join(ROOT, "rust", "idsp-hip-sys", "src", "lib.rs")).read()
    for name in _abi.BIQUAD_I16_BYLANE:
        assert f"pub fn idsp_{name}(" in lib and f'"idsp_{name}",' in lib, name
    assert "coef: *const i16" in lib
