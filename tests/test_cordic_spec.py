"""The CORDIC specification (tests/_cordic_spec.py) against itself, the reference's test data (tests/golden/cordic_kat.json:
src/cordic.rs:163-263, build.rs:69-119) and the committed tables.  No test here needs a GPU; the last two
(`test_gains_and_prototypes`, `test_cpp_argument_validation`) call the library's host side, so they need the built
`idsp_amd/lib/libidsp_hip.so` (`make all`), as the host-side test of `tests/test_gpu_pfb_host_mirror.py` does.

The reference's random values come from `StdRng::seed_from_u64(42)`, which cannot be reproduced here; `S.test_values` draws the
same COUNT of values (50 and 300) from a seeded numpy generator and appends the reference's 17 fixed values unchanged.
The quickcheck limits 22 and 29 (:253, :262) are not asserted: over 115,000 random in-domain cases the rotation maximum was 22.0,
on the first of them."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

from idsp_amd import _abi
from idsp_amd._abi import CORDIC  # noqa: F401  (the feature's prototype table)
from tests import _cordic_spec as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KAT = json.load(open(os.path.join(ROOT, "tests", "golden", "cordic_kat.json")))
SEED = 42


def corner_triples():
    v = np.array(KAT["fixed_values"], np.int64)
    return [g.reshape(-1) for g in np.meshgrid(v, v, v, indexing="ij")]


def test_fixed_values_are_the_reference_list():
    assert KAT["fixed_values"] == S.FIXED_VALUES and len(S.FIXED_VALUES) == 17


@pytest.mark.parametrize("name", list(S.FUNCTIONS))
def test_restatements_agree_on_the_corner_triples(name):
    """all 17^3 triples of the fixed values — i32::MIN, +-0x7fffffff, +-2^30, ... — bit for bit"""
    vectoring, coord, _ = S.FUNCTIONS[name]
    x, y, z = corner_triples()
    a, b = S.cordic_np(vectoring, coord, x, y, z)
    for i in range(x.size):
        assert S.cordic_int(vectoring, coord, int(x[i]), int(y[i]), int(z[i])) == (int(a[i]), int(b[i])), (name, int(x[i]), int(y[i]), int(z[i]))


@pytest.mark.parametrize("name", list(S.FUNCTIONS))
def test_restatements_agree_on_random_triples(name):
    vectoring, coord, pair = S.FUNCTIONS[name]
    rng = np.random.default_rng(5)
    x, y, z = rng.integers(S.I32_MIN, 1 << 31, size=(3, 2000), dtype=np.int64)
    a, b = S.cordic_np(vectoring, coord, x, y, z)
    for i in range(x.size):
        assert S.cordic_int(vectoring, coord, int(x[i]), int(y[i]), int(z[i])) == (int(a[i]), int(b[i])), (name, i)
    out = S.function_np(name, np.stack([x, y], axis=-1).astype(np.int32), z.astype(np.int32))
    assert np.array_equal(out, np.stack([a, b], axis=-1) if pair else b)
    zero = S.function_np(name, np.stack([x, y], axis=-1).astype(np.int32))
    a0, b0 = S.cordic_np(vectoring, coord, x, y, 0)
    assert np.array_equal(zero, np.stack([a0, b0], axis=-1) if pair else b0)


@pytest.mark.parametrize("name", list(S.FUNCTIONS))
def test_recorded_outputs(name):
    for row in KAT["outputs"][name]:
        r = S.function_int(name, *row["xyz"])
        assert (list(r) if isinstance(r, tuple) else r) == row["out"], (name, row)


def test_negation_of_i32_min_wraps():
    """`-x` of i32::MIN is i32::MIN (release build): the flip leaves x = i32::MIN < 0 in place, and the shifts see it"""
    x, z = S.cordic_int(S.DEROTATE, S.LINEAR, S.I32_MIN, 0, 0)
    assert x == S.I32_MIN  # linear mode leaves x untouched after the flip


def test_schedule():
    assert len(S.schedule(S.CIRCULAR)) == 30 and len(S.schedule(S.LINEAR)) == 30 and len(S.schedule(S.HYPERBOLIC)) == 32
    assert [s for s, _ in S.schedule(S.HYPERBOLIC)].count(4) == 2 and [s for s, _ in S.schedule(S.HYPERBOLIC)].count(13) == 2
    assert S.schedule(S.LINEAR)[0] == (0, S.I32_MIN) and S.schedule(S.LINEAR)[29] == (29, 4)
    assert S.schedule(S.HYPERBOLIC)[0][0] == 1 and S.schedule(S.HYPERBOLIC)[-1][0] == 30


def test_basic_rot_and_tables():
    """`basic_rot`'s gain assertion (:165); the tables of the specification, of tools/gen_cordic_table.py, of the golden file and
    of idsp_amd/csrc/cordic_table.h (parsed as text) are the same numbers"""
    b = KAT["bounds"]
    assert abs(S.circular_gain() - b["circular_gain"]) < b["circular_gain_tolerance"]
    from tools import gen_cordic_table as G

    assert G.circular() == S.CORDIC_CIRCULAR == KAT["circular_table"] and G.hyperbolic() == S.CORDIC_HYPERBOLIC == KAT["hyperbolic_table"]
    assert G.circular_gain() == S.circular_gain() == KAT["circular_gain"] and G.hyperbolic_gain() == S.hyperbolic_gain() == KAT["hyperbolic_gain"]
    assert S.CORDIC_CIRCULAR[:4] == [536870912, 316933406, 167458907, 85004756] and S.CORDIC_CIRCULAR[-3:] == [5, 3, 1]
    assert S.CORDIC_HYPERBOLIC[:3] == [1179625963, 548494837, 269846813] and S.CORDIC_HYPERBOLIC[-3:] == [8, 4, 2]
    text = open(os.path.join(ROOT, "idsp_amd", "csrc", "cordic_table.h")).read()
    assert text == G.text()

    def ints(name):
        return [int(v) for v in re.search(name + r"\[30\] = \{([^}]*)\}", text).group(1).split(",")]

    assert ints("kCordicCircular") == S.CORDIC_CIRCULAR and ints("kCordicHyperbolic") == S.CORDIC_HYPERBOLIC
    assert float(re.search(r"kCordicCircularGain = ([0-9.e+-]+);", text).group(1)) == S.circular_gain()
    assert float(re.search(r"kCordicHyperbolicGain = ([0-9.e+-]+);", text).group(1)) == S.hyperbolic_gain()


def test_basic_rot_calls():
    """the seven `cos_sin_err` calls of `basic_rot` (:167-173) run; each stays under `meanmax_rot`'s maximum"""
    for x, y, z in ((0.50, 0.2, 0.123), (0.01, 0.0, -0.35), (0.605, 0.0, 0.35), (-0.3, 0.4, 0.55), (-0.3, -0.4, -0.55), (-0.3, -0.4, 0.8), (-0.3, -0.4, -0.8)):
        f = 1.0 / S.circular_gain()
        x, y, z = (np.array([v]) for v in (x, y, z))
        out = S.function_np("cos_sin", np.stack([S.f2i(x * f), S.f2i(y * f)], axis=-1), S.f2i(z))
        assert S.rot_errors(out, x, y, z)[0] < KAT["bounds"]["meanmax_rot"]["max"]


def test_meanmax_rot():
    """`meanmax_rot` (:201-223): 50 + 17 values cubed, mean over ALL cases (skipped ones included) < 5, max < 24.
    This seed: mean 4.04, max 21.4."""
    b = KAT["bounds"]["meanmax_rot"]
    total, x, y, z, xy, zi = S.rot_cases(S.test_values(b["random"], SEED))
    assert total == 67 ** 3
    e = S.rot_errors(S.function_np("cos_sin", xy, zi), x, y, z)
    mean, mx = e.sum() / total, e.max()
    print(f"meanmax_rot: mean {mean:.4f} max {mx:.4f} over {e.size} of {total} cases")
    assert mean < b["mean"] and mx < b["max"]


def test_meanmax_vect():
    """`meanmax_vect` (:225-245): 300 + 17 values squared, mean over ALL cases < 8, max < 30.  This seed: mean 6.41, max 29.0005
    (the maximum comes from the fixed values, not the random ones)."""
    b = KAT["bounds"]["meanmax_vect"]
    total, x, y, xy = S.vect_cases(S.test_values(b["random"], SEED))
    assert total == 317 ** 2
    e = S.vect_errors(S.function_np("sqrt_atan2", xy), x, y)
    mean, mx = e.sum() / total, e.max()
    print(f"meanmax_vect: mean {mean:.4f} max {mx:.4f} over {e.size} of {total} cases")
    assert mean < b["mean"] and mx < b["max"]


# ---- mul, div, cosh_sinh, sqrt_atanh2: the reference asserts no values (`check_hyp_vect` returns true whatever happens, :265-277),
# so bit equality with the specification is the rule.  One sanity check each against f64 on the convergence domain catches a wrong
# table or shift in BOTH restatements; the bound is twice the maximum measured on these very 200,000 cases (seeded, so the figure is reproducible).
N_SANITY = 200000


def test_mul_against_f64():
    """|x|, |y| <= 2^29, |z| <= 2^30 (beyond +-2^30 the pre-rotation flips and the result diverges): y + x z / 2^31.
    Measured maximum 15.9 counts; bound 31.8."""
    rng = np.random.default_rng(7)
    x, y = rng.integers(-(1 << 29), (1 << 29) + 1, (2, N_SANITY))
    z = rng.integers(-(1 << 30), (1 << 30) + 1, N_SANITY)
    got = S.function_np("mul", np.stack([x, y], -1), z).astype(np.float64)
    assert np.abs(got - (y + x * (z / S.Q31))).max() < 31.8


def test_div_against_f64():
    """2^29 <= x <= 2^30, |y| <= x / 2, |z| <= 2^29: z + y / x * 2^31.  Measured maximum 48.4 counts (the truncated `x >> i`
    terms, relative to an x of 2^29); bound 96.8."""
    rng = np.random.default_rng(8)
    x = rng.integers(1 << 29, (1 << 30) + 1, N_SANITY)
    y = (rng.uniform(-0.5, 0.5, N_SANITY) * x).astype(np.int64)
    z = rng.integers(-(1 << 29), (1 << 29) + 1, N_SANITY)
    got = S.function_np("div", np.stack([x, y], -1), z).astype(np.float64)
    assert np.abs(got - (z + y / x * S.Q31)).max() < 96.8


def test_cosh_sinh_against_f64():
    """|x|, |y| <= 2^29, |z| < 2^30 = 0.5 (the pre-rotation of rotating mode flips beyond, which has no hyperbolic meaning):
    gain * (x cosh z + y sinh z), gain * (x sinh z + y cosh z) with gain = CORDIC_HYPERBOLIC_GAIN.  Measured maximum 15.5; bound 31."""
    rng = np.random.default_rng(9)
    x, y = rng.integers(-(1 << 29), (1 << 29) + 1, (2, N_SANITY))
    z = rng.integers(-(1 << 30) + 1, 1 << 30, N_SANITY)
    got = S.function_np("cosh_sinh", np.stack([x, y], -1), z).astype(np.float64)
    g, zf = S.hyperbolic_gain(), z / S.Q31
    want = np.stack([g * (x * np.cosh(zf) + y * np.sinh(zf)), g * (x * np.sinh(zf) + y * np.cosh(zf))], -1)
    assert np.abs(got - want).max() < 31


def test_sqrt_atanh2_against_f64():
    """2^28 <= x <= 2^30, |y| <= 0.75 x (atanh 0.75 = 0.97, inside the convergence range 1.1 of :271), |z| <= 2^20:
    gain * sqrt(x^2 - y^2) and z + atanh(y / x) * 2^31.  Measured maxima 21.6 (radius) and 124.0 (angle; an x of 2^28 loses
    `x >> i` bits early); bounds 43.2 and 248."""
    rng = np.random.default_rng(10)
    x = rng.integers(1 << 28, (1 << 30) + 1, N_SANITY)
    y = (rng.uniform(-0.75, 0.75, N_SANITY) * x).astype(np.int64)
    z = rng.integers(-(1 << 20), (1 << 20) + 1, N_SANITY)
    got = S.function_np("sqrt_atanh2", np.stack([x, y], -1), z).astype(np.float64)
    xf, yf = x.astype(np.float64), y.astype(np.float64)
    d = np.abs(got - np.stack([S.hyperbolic_gain() * np.sqrt(xf ** 2 - yf ** 2), z + np.arctanh(yf / xf) * S.Q31], -1))
    assert d[:, 0].max() < 43.2 and d[:, 1].max() < 248


# ---- the library's host side: needs the built library (`make all`), no GPU
def test_gains_and_prototypes():
    from idsp_amd._lib import load

    fn, _ = load()
    assert fn["cordic_circular_gain"]() == S.circular_gain() and fn["cordic_hyperbolic_gain"]() == S.hyperbolic_gain()
    assert set(_abi.CORDIC) <= set(_abi.UTILS) and all(("cordic_" + n + "_i32") in _abi.CORDIC for n in S.FUNCTIONS)


def test_cpp_argument_validation():
    """tests/cpp/test_cordic_host.cpp: every argument error of the six entries returns IDSP_EINVAL with a message before anything
    touches a device (plain g++ against the C ABI and the C++ mirrors of include/idsp_hip.hpp)"""
    exe = os.path.join(ROOT, "build", "test_cordic_host")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Iinclude", "tests/cpp/test_cordic_host.cpp", "-Lidsp_amd/lib", "-lidsp_hip",
                    "-Wl,-rpath,$ORIGIN/../idsp_amd/lib", "-o", exe], cwd=ROOT, check=True)
    r = subprocess.run([exe], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "cordic argument-validation tests passed" in r.stdout
