"""Executable specification of the phase consumers: `PLL` (src/pll.rs), `Unwrapper<i64>`, `ClampWrap<W<i32>>`, `overflowing_sub`
and `saturating_scale` (src/unwrap.rs), and the PLL coefficient builders in f32.

Two independent restatements of the reference, each citing its lines:

  * scalar: Python integers (unbounded) with explicit wrap helpers, one sample and one lane at a time;
  * numpy:  vectorised over lanes, a Python loop over frames, unsigned arithmetic with explicit masks (numpy promotes mixed
    signed / unsigned operands to float64 and warns on scalar overflow, so every array here has ONE dtype per expression and
    wraps by construction).  It is the bulk checker of the GPU tests (65536 lanes x 4096 frames in well under a minute).

The checker library (oracle/) has no twin for these entries; parity of the HIP kernels rests on this file, and this file rests on
the reference's own tests (tests/golden/phase_kat.json, tests/test_phase_spec.py).

State words are those of include/idsp_hip.h, word-plane-major `[words, lanes]` uint32:
  ClampWrap {x0, clamp};  Unwrapper {y lo, y hi};  PLL {clamp.x0, clamp.clamp, z0, y0, f0 lo, f0 hi, f lo, f hi, y}.

Test infrastructure only."""
from __future__ import annotations

import math

import numpy as np

I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
PLL_WORDS = 9


# ----------------------------------------------------------------------------------------------------------- scalar
def w32(v: int) -> int:
    """two's-complement wrap to i32"""
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v >> 31 else v


def w64(v: int) -> int:
    v &= 0xFFFFFFFFFFFFFFFF
    return v - (1 << 64) if v >> 63 else v


def overflowing_sub(y: int, x: int):
    """src/unwrap.rs:73-80 on i32: (wrapped y - x, Wrap as -1 / 0 / 1)"""
    delta = w32(y - x)                               # :77
    a, b = delta >= 0, y >= x                        # :78 (delta >= 0).cmp(&(y >= x)), false < true
    return delta, (a > b) - (a < b)


def saturating_scale(lo: int, hi: int, shift: int) -> int:
    """src/unwrap.rs:90-101"""
    assert 0 < shift <= 32                           # :91-92
    hi_range = -1 << (shift - 1)                     # :93
    if hi <= hi_range:                               # :94
        return w32(I32_MIN - hi_range)               # :95
    if -hi <= hi_range:                              # :96
        return w32(hi_range - I32_MIN)               # :97
    return w32((lo >> shift) + w32(hi << (32 - shift)))  # :99


def wrap_add(a: int, b: int) -> int:
    """`Wrap + Wrap` (src/unwrap.rs:49-55)"""
    s = a + b
    return (s > 0) - (s < 0)


class ClampWrap:
    """`ClampWrap<W<i32>>` (src/unwrap.rs:166-194)"""

    def __init__(self, x0=0, clamp=0):
        self.x0, self.clamp = x0, clamp

    def process(self, x: int) -> int:
        _, wrap = overflowing_sub(x, self.x0)        # :185
        self.x0 = x                                  # :186
        self.clamp = wrap_add(self.clamp, wrap)      # :187
        return {-1: I32_MIN, 0: x, 1: I32_MAX}[self.clamp]  # :188-192

    def words(self):
        return [self.x0 & 0xFFFFFFFF, self.clamp & 0xFFFFFFFF]

    @classmethod
    def from_words(cls, w):
        return cls(w32(int(w[0])), w32(int(w[1])))


class Unwrapper:
    """`Unwrapper<i64>` fed i32 (src/unwrap.rs:109-156)"""

    def __init__(self, y=0):
        self.y = y

    def process(self, x: int) -> int:
        dx = w32(x - w32(self.y))                    # :152 x.wrapping_sub(&self.y.as_())
        self.y = w64(self.y + dx)                    # :153
        return dx

    def wraps(self, shift: int) -> int:
        """`wraps::<i32, S>()` (:119-127)"""
        return w32(w32(self.y >> shift) + (w32(self.y >> (shift - 1)) & 1))

    def phase(self) -> int:                          # :130-136, P = i64
        return self.y

    def words(self):
        return [self.y & 0xFFFFFFFF, (self.y >> 32) & 0xFFFFFFFF]

    @classmethod
    def from_words(cls, w):
        return cls(w64(int(w[0]) | (int(w[1]) << 32)))


class PLLState:
    """`PLLState` (src/pll.rs:62-75)"""

    def __init__(self):
        self.clamp, self.z0, self.y0, self.f0, self.f, self.y = ClampWrap(), 0, 0, 0, 0, 0

    def phase(self) -> int:                          # :79-81
        return self.y

    def frequency(self) -> int:                      # :84-86
        return w32(self.f >> 32)

    def words(self):
        return self.clamp.words() + [self.z0 & 0xFFFFFFFF, self.y0 & 0xFFFFFFFF, self.f0 & 0xFFFFFFFF, (self.f0 >> 32) & 0xFFFFFFFF,
                                     self.f & 0xFFFFFFFF, (self.f >> 32) & 0xFFFFFFFF, self.y & 0xFFFFFFFF]

    @classmethod
    def from_words(cls, w):
        w = [int(v) for v in w]
        s = cls()
        s.clamp = ClampWrap.from_words(w[:2])
        s.z0, s.y0, s.y = w32(w[2]), w32(w[3]), w32(w[8])
        s.f0, s.f = w64(w[4] | (w[5] << 32)), w64(w[6] | (w[7] << 32))
        return s


def pll_process(ba, s: PLLState, x: int) -> int:
    """`PLL::process` (src/pll.rs:90-107); ba = `Q32<32>` bits.  `Q32<32> * i32` is the widened i64 product
    (dsp-fixedpoint/src/ops.rs:91-97, src/lib.rs:310-312); sums wrap as in a release build."""
    s.y = w32(s.y + s.frequency())                   # :92
    z0 = s.clamp.process(w32(x + s.y)) >> 1          # :94 (arithmetic shift)
    y0 = w32(z0 + s.z0)                              # :96
    s.z0 = z0                                        # :97
    wide = w64(ba[0] * y0 + ba[1] * s.y0 + ba[2] * w32(s.f0 >> 32))  # :100
    low = (ba[2] * (s.f0 & 0xFFFFFFFF)) >> 32        # :102
    s.f0 = w64(s.f0 + w64(wide + low))               # :99
    s.y0 = y0                                        # :103
    s.f = w64(s.f + s.f0)                            # :105
    return s.y                                       # :106


# ---- coefficient builders in f32 (src/pll.rs:42-57, dsp-fixedpoint/src/num_traits_impl.rs:39-45)
def q32_from_f32(v) -> int:
    """`Q32::<32>::from_f32`: (v * 2^32).round() as i32 — f32 product, round half away from zero, saturating cast, NaN -> 0"""
    with np.errstate(all="ignore"):
        r = np.float32(v) * np.float32(4294967296.0)
    if np.isnan(r):
        return 0
    if np.isinf(r):
        return I32_MAX if r > 0 else I32_MIN
    r = float(r)                                     # exact
    t = math.trunc(r)
    if abs(r - t) >= 0.5:
        t += 1 if r > 0 else -1
    return max(I32_MIN, min(I32_MAX, t))


def pll_from_zpk(zero, pole, gain):
    """src/pll.rs:42-46"""
    f = np.float32
    with np.errstate(all="ignore"):
        zero, pole, gain = f(zero), f(pole), f(gain)
        return [q32_from_f32(gain), q32_from_f32(-gain * zero), q32_from_f32(-(f(1.0) - pole))]


def pll_from_bandwidth(bw, split):
    """src/pll.rs:51-57"""
    f = np.float32
    with np.errstate(all="ignore"):
        bw, split = f(bw), f(split)
        a = bw * f(2.0) * f(math.pi)                 # :52 core::f32::consts::PI
        z = f(1.0) - a / split                       # :53
        p = f(1.0) - a * split                       # :54
        k = -a * a * split                           # :55
    return pll_from_zpk(z, p, k)


# ------------------------------------------------------------------------------------------------------------ numpy
_U32 = np.uint32
_U64 = np.uint64


def _s32(u):
    """uint32 array -> the same bits as int32"""
    return u.view(np.int32)


def _sext(u32):
    """uint32 array (i32 bits) -> sign-extended uint64 bits"""
    return _s32(u32).astype(np.int64).view(_U64)


def _hi(u64):
    return (u64 >> _U64(32)).astype(_U32)


def _lo(u64):
    return (u64 & _U64(0xFFFFFFFF)).astype(_U32)


def _join(lo, hi):
    return lo.astype(_U64) | (hi.astype(_U64) << _U64(32))


def _clamp_wrap_np(x0, clamp, x):
    """one frame of `ClampWrap<W<i32>>` (src/unwrap.rs:184-193); x0, x: uint32 bits, clamp: int8; returns (x0, clamp, out uint32)"""
    delta = x - x0                                                       # :77, uint32 wraps
    a = _s32(delta) >= 0
    b = _s32(x) >= _s32(x0)                                              # :78
    wrap = a.astype(np.int8) - b.astype(np.int8)
    clamp = np.sign(clamp + wrap).astype(np.int8)                        # :49-55, :187
    out = np.where(clamp == 0, x, np.where(clamp < 0, _U32(0x80000000), _U32(0x7FFFFFFF)))  # :188-192
    return x, clamp, out.astype(_U32)


def _frames_of(x, lanes):
    x = np.ascontiguousarray(x, dtype=np.int32).reshape(-1, lanes)
    return x.view(_U32)


def clamp_wrap_np(state, x):
    """state [2, lanes] uint32 (updated), x [frames, lanes] int32 -> y [frames, lanes] int32"""
    lanes = state.shape[1]
    xs = _frames_of(x, lanes)
    x0, clamp = state[0].copy(), _s32(state[1]).astype(np.int8)
    y = np.empty_like(xs)
    for f in range(xs.shape[0]):
        x0, clamp, y[f] = _clamp_wrap_np(x0, clamp, xs[f])
    state[0], state[1] = x0, clamp.astype(np.int32).view(_U32)
    return y.view(np.int32)


def unwrap_np(state, x, mode=0):
    """`Unwrapper<i64>` (src/unwrap.rs:151-155): mode 0 -> dx [frames, lanes] int32, mode 1 -> running y int64"""
    lanes = state.shape[1]
    xs = _frames_of(x, lanes)
    y = _join(state[0], state[1])
    out = np.empty(xs.shape, dtype=_U32 if mode == 0 else _U64)
    for f in range(xs.shape[0]):
        dx = xs[f] - _lo(y)                                              # :152
        y = y + _sext(dx)                                                # :153, uint64 wraps
        out[f] = dx if mode == 0 else y
    state[0], state[1] = _lo(y), _hi(y)
    return out.view(np.int32 if mode == 0 else np.int64)


def unwrap_wraps_np(state, shift):
    """`wraps::<i32, S>()` (src/unwrap.rs:119-127) of every lane, int32"""
    y = _join(state[0], state[1]).view(np.int64)
    a = (y >> np.int64(shift)).astype(np.int32).view(_U32)
    b = (y >> np.int64(shift - 1)).astype(np.int32).view(_U32) & _U32(1)
    return (a + b).view(np.int32)


def pll_np(ba, state, x, output=0):
    """`PLL::process` (src/pll.rs:90-107) over [frames, lanes]; state [9, lanes] uint32 (updated).
    output 0: phase [frames, lanes]; 1: frequency after the sample; 2: [frames, lanes, 2] = {phase, frequency}"""
    lanes = state.shape[1]
    xs = _frames_of(x, lanes)
    b0, b1, a1 = (np.int64(int(v)) for v in ba)
    x0, clamp = state[0].copy(), _s32(state[1]).astype(np.int8)
    z0, y0, y = state[2].copy(), state[3].copy(), state[8].copy()
    f0, fq = _join(state[4], state[5]), _join(state[6], state[7])
    out = np.empty(xs.shape + ((2,) if output == 2 else ()), dtype=_U32)
    for f in range(xs.shape[0]):
        y = y + _hi(fq)                                                  # :92
        x0, clamp, c = _clamp_wrap_np(x0, clamp, xs[f] + y)              # :94
        z = (_s32(c) >> np.int32(1)).view(_U32)                          # :94 arithmetic >> 1
        yn = z + z0                                                      # :96
        z0 = z                                                           # :97
        # :100 three i32 x i32 -> i64 products (each fits i64), summed with wrap in uint64
        wide = ((b0 * _s32(yn).astype(np.int64)).view(_U64) + (b1 * _s32(y0).astype(np.int64)).view(_U64)
                + (a1 * _s32(_hi(f0)).astype(np.int64)).view(_U64))
        low = ((a1 * _lo(f0).astype(np.int64)) >> np.int64(32)).view(_U64)  # :102, |a1| <= 2^31, lo < 2^32: fits i64
        f0 = f0 + (wide + low)                                           # :99
        y0 = yn                                                          # :103
        fq = fq + f0                                                     # :105
        if output == 0:
            out[f] = y
        elif output == 1:
            out[f] = _hi(fq)
        else:
            out[f, :, 0], out[f, :, 1] = y, _hi(fq)
    state[0], state[1] = x0, clamp.astype(np.int32).view(_U32)
    state[2], state[3], state[8] = z0, y0, y
    state[4], state[5], state[6], state[7] = _lo(f0), _hi(f0), _lo(fq), _hi(fq)
    return out.view(np.int32)


# ------------------------------------------------------------------------------------------------- shared test data
def random_state(rng, words, lanes):
    """random non-zero state with the `Wrap` word (word 1 of ClampWrap and PLL states) in {-1, 0, 1}"""
    st = rng.integers(0, 1 << 32, size=(words, lanes), dtype=np.uint64).astype(np.uint32)
    if words in (2, PLL_WORDS):
        st[1] = rng.integers(-1, 2, size=lanes).astype(np.int32).view(np.uint32)
    return st


def adversarial_phases(rng, frames, lanes):
    """[frames, lanes] int32: per lane one of — a ramp that wraps every few samples, i32::MIN / i32::MAX alternations, steps near
    +-2^31, uniform random phases, a slow ramp with noise"""
    kind = rng.integers(0, 5, size=lanes)
    n = np.arange(1, frames + 1, dtype=np.uint64)[:, None]
    step = rng.integers(0, 1 << 32, size=lanes, dtype=np.uint64)
    fast = (rng.integers(1 << 29, 1 << 31, size=lanes, dtype=np.uint64) * rng.choice(np.array([1, 3], dtype=np.uint64), size=lanes))
    near = (np.uint64(1 << 31) + rng.integers(-3, 4, size=lanes).astype(np.int64).view(np.uint64)) & np.uint64(0xFFFFFFFF)
    x = np.empty((frames, lanes), dtype=np.uint32)
    ramp = lambda s: ((n * s[None, :]) & np.uint64(0xFFFFFFFF)).astype(np.uint32)  # noqa: E731
    x[:] = rng.integers(0, 1 << 32, size=(frames, lanes), dtype=np.uint64).astype(np.uint32)
    x[:, kind == 0] = ramp(fast)[:, kind == 0]
    ext = np.where(rng.integers(0, 2, size=(frames, lanes)) == 0, np.uint32(0x80000000), np.uint32(0x7FFFFFFF))
    x[:, kind == 1] = ext[:, kind == 1]
    x[:, kind == 2] = ramp(near)[:, kind == 2]
    slow = ramp(step >> np.uint64(8)) + rng.integers(0, 1 << 16, size=(frames, lanes), dtype=np.uint64).astype(np.uint32)
    x[:, kind == 4] = slow[:, kind == 4]
    return x.view(np.int32)


def random_ba(rng):
    """`PLL::ba` bits: random, with a saturated a1 (as `from_bandwidth(5e-2, 4)` gives) in a third of the draws"""
    ba = [int(v) for v in rng.integers(I32_MIN, I32_MAX + 1, size=3)]
    r = rng.integers(0, 3)
    if r == 0:
        ba[2] = I32_MIN
    elif r == 1:
        ba = pll_from_bandwidth(float(rng.uniform(7e-5, 5e-2)), 4.0)
    return ba
