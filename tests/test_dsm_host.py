"""The host side of idsp_dsm_u32 without a GPU: every call here returns before a launch (the pointers are numbers that are only
compared, never followed).  Needs the built library (`make all`)."""
import ctypes as C
import os
import subprocess

import pytest

from idsp_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FM, LM = _abi.FRAME_MAJOR, _abi.LANE_MAJOR
X, Y, ST = 0x10000, 0x20000, 0x30000  # three far-apart "device" addresses


@pytest.fixture(scope="module")
def fn():
    from idsp_amd._lib import load

    return load()[0]


def _call(fn, order, st, x, xp, y, yp, lanes, frames, layout):
    return fn["dsm_u32"](order, C.c_void_p(st), C.c_void_p(x), xp, C.c_void_p(y), yp, lanes, frames, layout, None)


def _einval(fn, *args):
    rc = _call(fn, *args)
    return rc == _abi.IDSP_EINVAL and len(fn["last_error"]()) > 0


def test_prototypes():
    assert set(_abi.DSM) == {"dsm_state_words", "dsm_u32"} and set(_abi.DSM) <= set(_abi.UTILS)
    assert not set(_abi.DSM) & (set(_abi.PROCESSING) | set(_abi.HELPERS))
    assert _abi.DSM_MAX_ORDER == 8 and _abi.ABI_VERSION == 4


def test_state_words(fn):
    assert [fn["dsm_state_words"](k) for k in range(-1, 10)] == [0, 0, 2, 4, 6, 8, 10, 12, 14, 16, 0]


@pytest.mark.parametrize("args", [
    (-1, ST, X, 0, Y, 0, 4, 4, FM), (9, ST, X, 0, Y, 0, 4, 4, FM),          # order
    (3, ST, X, 0, Y, 0, 4, 4, 2), (3, ST, X, 0, Y, 0, 4, 4, -1),            # layout
    (3, ST, None, 0, Y, 0, 4, 4, FM), (3, ST, X, 0, None, 0, 4, 4, LM),     # NULL x / y
    (3, None, X, 0, Y, 0, 4, 4, FM),                                        # NULL state with order > 0
    (3, ST, X, 3, Y, 0, 4, 9, FM), (3, ST, X, 0, Y, 3, 4, 9, FM),           # pitch < row (FrameMajor: row = lanes)
    (3, ST, X, 8, Y, 0, 4, 9, LM), (3, ST, X, 0, Y, 8, 4, 9, LM),           # (LaneMajor: row = frames)
    (3, ST, X + 2, 0, Y, 0, 4, 4, FM),                                      # x not 4-byte aligned
    (3, ST, X, 0, X, 0, 4, 4, FM), (3, ST, X, 0, X + 63, 0, 4, 4, LM),      # y inside x / on its last byte
    (3, ST, X + 16, 0, X + 1, 0, 4, 4, FM),                                 # x starts on the last byte of y
    (3, ST, X, 8, X + 16, 32, 4, 4, FM),                                    # y in the gaps of a pitched x: the EXTENTS overlap
    (3, ST, X, 1 << 62, Y, 0, 4, 4, FM),                                    # an extent past size_t
])
def test_einval(fn, args):
    assert _einval(fn, *args), args


def test_empty_calls(fn):
    assert _call(fn, 3, ST, X, 0, Y, 0, 0, 4, FM) == 0 and _call(fn, 3, ST, X, 0, Y, 0, 4, 0, LM) == 0
    assert _call(fn, 0, None, X, 0, Y, 0, 0, 0, FM) == 0  # K = 0 has no state
    assert _call(fn, 8, ST, X, 7, Y, 1, 0, 5, FM) == 0     # FrameMajor row = lanes = 0: any pitch covers it


def test_python_mirror_without_device():
    from idsp_amd import process as P

    assert "Dsm" in P.__all__ and "Dsm<K>" in P.__doc__
    for bad in (-1, 9, 2.0, "3", None, True):
        with pytest.raises(ValueError):
            P.Dsm(bad)
    assert [P.Dsm(k).order for k in range(9)] == list(range(9))
    with pytest.raises(ValueError):
        P.Dsm(3).lanes(4, device="cpu")
    with pytest.raises(ValueError):
        P.Dsm(3).lanes(-1)


def test_cpp_host_mirror():
    """tests/cpp/test_dsm_host.cpp: `Dsm` / `DsmLanes` of include/idsp_hip.hpp — the same validation — and the argument errors and
    empty calls of the entry, before anything touches a device (plain g++ against the C ABI)"""
    exe = os.path.join(ROOT, "build", "test_dsm_host")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Iinclude", "tests/cpp/test_dsm_host.cpp", "-Lidsp_amd/lib", "-lidsp_hip",
                    "-Wl,-rpath,$ORIGIN/../idsp_amd/lib", "-o", exe], cwd=ROOT, check=True)
    r = subprocess.run([exe], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "dsm host tests passed" in r.stdout
