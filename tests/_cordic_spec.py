"""Specification of the CORDIC family (reference: src/cordic.rs:13-107, tables build.rs:69-119), restated twice:

  cordic_int(vectoring, coord, x, y, z)   plain Python integers, one element, in the shape of the reference's loop
  cordic_np(vectoring, coord, x, y, z)    numpy over arrays from a flat schedule of (shift, angle), wrapping emulated in int64

The reference writes `x -= dx`, `y += dy` and `-x` with plain operators (:31-32, :59-71): a release build wraps them, a debug
build panics.  Both restatements wrap — the stance of SURVEY section 8(a) — so `-i32::MIN` is `i32::MIN`.

The engine has no checker-library twin of these functions; the GPU tests hold the kernels to `cordic_np` bit for bit, and
tests/test_cordic_spec.py holds the two restatements to each other and to the reference's own test data.

The error measures of the reference's tests (`cos_sin_err`, `sqrt_atan2_err`, :129-150) and the case sets of `meanmax_rot` and
`meanmax_vect` (:201-245) are here as well, split into "inputs" and "errors of these outputs" so that the same cases can be run
through the device.  The reference draws its random values from `StdRng::seed_from_u64(42)` (:177-178); that stream cannot be
reproduced without the rand crate, so `test_values` draws from a seeded numpy generator instead."""
import math

import numpy as np

ROTATE, DEROTATE = False, True           # :5-6
CIRCULAR, HYPERBOLIC, LINEAR = 0, 1, 2   # :7-9
DEPTH = 30                               # build.rs:70
Q31 = float(1 << 31)                     # :117
I32_MIN = -(1 << 31)

# name -> (vectoring, coord, pair result) (:80-107)
FUNCTIONS = {
    "cos_sin": (ROTATE, CIRCULAR, True),
    "sqrt_atan2": (DEROTATE, CIRCULAR, True),
    "mul": (ROTATE, LINEAR, False),
    "div": (DEROTATE, LINEAR, False),
    "cosh_sinh": (ROTATE, HYPERBOLIC, True),
    "sqrt_atanh2": (DEROTATE, HYPERBOLIC, True),
}

# `test_values` without its random head (:179-197)
FIXED_VALUES = [0, 1, -1, 0xF, -0xF, 0x55555555, -0x55555555, 0x5AAAAAAA, -0x5AAAAAAA, 0x7FFFFFFF, -0x7FFFFFFF,
                1 << 29, -(1 << 29), 1 << 30, -(1 << 30), I32_MIN, (1 << 31) - 1]


# ------------------------------------------------------------------ tables (build.rs:69-119)
def _round(v: float) -> int:
    """f64::round: half away from zero"""
    return int(math.floor(v + 0.5)) if v >= 0 else -int(math.floor(-v + 0.5))


def circular_table():
    return [_round(math.atan(0.5 ** i) / math.pi * Q31) for i in range(DEPTH)]  # build.rs:87


def hyperbolic_table():
    return [_round(math.atanh(0.5 ** (i + 1)) * Q31) for i in range(DEPTH)]  # build.rs:115


def circular_gain() -> float:
    f = 1.0
    for i in range(DEPTH):
        f = f * math.sqrt(1.0 + 0.25 ** i)  # build.rs:80
    return f


def hyperbolic_gain() -> float:
    f, k = 1.0, 4
    for i in range(1, DEPTH):  # build.rs:92-104
        if i == k:
            k, r = 3 * i + 1, 2
        else:
            r = 1
        for _ in range(r):
            f *= math.sqrt(1.0 - 0.25 ** i)
    return f


CORDIC_CIRCULAR = circular_table()
CORDIC_HYPERBOLIC = hyperbolic_table()


# ------------------------------------------------------------------ restatement 1: Python integers
def wrap(v: int) -> int:
    """two's complement i32 of any integer"""
    return ((v + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


def cordic_int(vectoring: bool, coord: int, x: int, y: int, z: int):
    """`cordic::<VECTORING, COORD>(x, y, z, None)` (:13-77), line by line"""
    table = CORDIC_CIRCULAR if coord == CIRCULAR else CORDIC_HYPERBOLIC  # :20-23
    left = x < 0 if vectoring else wrap(z - (I32_MIN >> 1)) < 0           # :25-29
    if left:                                                              # :30-34
        x = wrap(-x)
        y = wrap(-y)
        z = wrap(z - I32_MIN)
    k = 4                                                                 # :36
    for i, a in enumerate(table):                                         # :37
        if coord == LINEAR:                                               # :39-41
            a = wrap(0x80000000 >> i)
        if coord == HYPERBOLIC:                                           # :43-45
            i += 1
        if coord == HYPERBOLIC and i == k:                                # :47-52
            k = 3 * i + 1
            repeat = 2
        else:
            repeat = 1
        for _ in range(repeat):                                           # :53
            lower = y <= 0 if vectoring else z >= 0                       # :55
            dx, dy = y >> i, x >> i                                       # :56
            if lower:                                                     # :57-64
                if coord == CIRCULAR:
                    x = wrap(x - dx)
                elif coord == HYPERBOLIC:
                    x = wrap(x + dx)
                y = wrap(y + dy)
                z = wrap(z - a)
            else:                                                         # :65-73
                if coord == CIRCULAR:
                    x = wrap(x + dx)
                elif coord == HYPERBOLIC:
                    x = wrap(x - dx)
                y = wrap(y - dy)
                z = wrap(z + a)
    return x, (z if vectoring else y)                                     # :76


def function_int(name: str, x: int, y: int, z: int):
    """the public function `name` (:80-107): a pair, or for mul / div the second of the pair"""
    vectoring, coord, pair = FUNCTIONS[name]
    r = cordic_int(vectoring, coord, x, y, z)
    return r if pair else r[1]


# ------------------------------------------------------------------ restatement 2: numpy
def _w(v):
    """int64 array -> the i32 it wraps to, still int64"""
    return ((v + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


def schedule(coord: int):
    """the micro-rotations of one call as a flat list of (shift, angle): 30 entries, hyperbolic 32 (shifts 4 and 13 twice)"""
    if coord == CIRCULAR:
        return [(j, CORDIC_CIRCULAR[j]) for j in range(DEPTH)]
    if coord == LINEAR:
        return [(j, wrap(0x80000000 >> j)) for j in range(DEPTH)]
    out = []
    for j in range(DEPTH):
        out += [(j + 1, CORDIC_HYPERBOLIC[j])] * (2 if j + 1 in (4, 13) else 1)
    return out


def cordic_np(vectoring: bool, coord: int, x, y, z):
    """arrays of i32 values (any integer dtype) -> (first, second) as int32 arrays"""
    x, y, z = (np.array(v, dtype=np.int64) for v in np.broadcast_arrays(x, y, z))
    flip = x < 0 if vectoring else _w(z + (1 << 30)) < 0
    x = np.where(flip, _w(-x), x)
    y = np.where(flip, _w(-y), y)
    z = np.where(flip, _w(z + (1 << 31)), z)
    xsign = {CIRCULAR: -1, HYPERBOLIC: 1, LINEAR: 0}[coord]
    for shift, angle in schedule(coord):
        d = np.where(y <= 0 if vectoring else z >= 0, 1, -1).astype(np.int64)  # +1 where `lower`
        x, y, z = _w(x + xsign * d * (y >> shift)), _w(y + d * (x >> shift)), _w(z - d * angle)
    return x.astype(np.int32), (z if vectoring else y).astype(np.int32)


def function_np(name: str, xy, z=None):
    """xy int32 [..., 2], z int32 [...] or None (= 0) -> int32 [..., 2] (pair functions) or [...] (mul, div): what
    idsp_cordic_<name>_i32 writes"""
    vectoring, coord, pair = FUNCTIONS[name]
    xy = np.asarray(xy)
    first, second = cordic_np(vectoring, coord, xy[..., 0], xy[..., 1], 0 if z is None else np.asarray(z))
    return np.stack([first, second], axis=-1) if pair else second


# ------------------------------------------------------------------ the reference's error measures (:119-150)
def f2i(v):
    """`(x * Q31).round() as i64 as i32` (:119-121), arrays"""
    v = np.asarray(v, np.float64) * Q31
    r = np.where(v >= 0, np.floor(v + 0.5), -np.floor(-v + 0.5))
    return _w(r.astype(np.int64)).astype(np.int32)


def i2f(v):
    """`x as f64 / Q31` (:122-124)"""
    return np.asarray(v, np.float64) / Q31


def test_values(n: int, seed: int):
    """`test_values(n)` (:176-199): n random i32, then the 17 fixed values"""
    rng = np.random.default_rng(seed)
    head = rng.integers(I32_MIN, 1 << 31, size=n, dtype=np.int64)
    return np.concatenate([head, np.array(FIXED_VALUES, np.int64)])


test_values.__test__ = False  # a helper, not a pytest case


def rot_cases(values):
    """the cases of `meanmax_rot` (:206-216) that pass its skip condition: (total count, x, y, z as f64, kernel inputs xy and z)"""
    x, y, z = (i2f(g).reshape(-1) for g in np.meshgrid(values, values, values, indexing="ij"))
    keep = ~(1.0 - x ** 2 - y ** 2 <= 1e-9)  # :210
    x, y, z = x[keep], y[keep], z[keep]
    f = 1.0 / circular_gain()  # `F` (:126)
    return keep.size, x, y, z, np.stack([f2i(x * f), f2i(y * f)], axis=-1), f2i(z)  # the arguments of `cos_sin` (:130)


def rot_errors(out, x, y, z):
    """`cos_sin_err` (:129-139) of the outputs `out` [n, 2] of cos_sin for the cases x, y, z"""
    ox, oy = i2f(out[:, 0]), i2f(out[:, 1])
    s, c = np.sin(z * math.pi), np.cos(z * math.pi)
    dx, dy = ox - (c * x - s * y), oy - (s * x + c * y)
    return np.sqrt(dx ** 2 + dy ** 2) * Q31


def vect_cases(values):
    """the cases of `meanmax_vect` (:230-240): (total count, x, y as f64, kernel input xy); z = 0"""
    x, y = (i2f(g).reshape(-1) for g in np.meshgrid(values, values, indexing="ij"))
    keep = ~(1.0 - x ** 2 - y ** 2 <= 1e-9)  # :233
    x, y = x[keep], y[keep]
    f = 1.0 / circular_gain()
    return keep.size, x, y, np.stack([f2i(x * f), f2i(y * f)], axis=-1)  # :142


def vect_errors(out, x, y):
    """`sqrt_atan2_err` (:141-150) of the outputs `out` [n, 2] of sqrt_atan2"""
    r, z = i2f(out[:, 0]), i2f(out[:, 1])
    r0 = np.sqrt(x ** 2 + y ** 2)
    z0 = np.arctan2(y, x) / math.pi
    da = i2f(f2i(z - z0))
    return np.sqrt((r - r0) ** 2 + (np.sin(da * math.pi) * r0) ** 2) * Q31
