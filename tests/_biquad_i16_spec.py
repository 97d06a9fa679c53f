"""`Biquad<Q16<F>>` / `BiquadClamp<Q16<F>, i16>` x `DirectForm1<i16>` (src/iir/biquad.rs:366-404 with C = Q<i16, i32, F>, T = i16,
A = Q<i32, i16, F>) as a RELEASE build of the reference computes it, stated twice and independently:

  * `df1` / `df1_clamp` / `chain`: scalar Python integers, one reference line per statement; every i32 and i16 operation goes through
    a `Wraps` counter, so a caller can tell whether a debug build of the reference would have panicked;
  * `chain_np`: numpy over lanes in int32 arrays (whose `*`, `+` wrap, whose `>>` is arithmetic and whose `astype(int16)` truncates),
    on the state layout of include/idsp_hip.h.

`from_sos` / `from_sos_np` restate `From<[[f64;3];2]>` (biquad.rs:545-566) and the float -> Q16 conversion
(dsp-fixedpoint/src/num_traits_impl.rs:32-46) the same way.  There is no twin in the checker library: tests/test_biquad_i16_spec.py holds
the two to each other, to oracle/spec.py: biquad_i32_df1 where nothing wraps, and to known answers."""
from fractions import Fraction
import math

import numpy as np

I16_MIN, I16_MAX = -32768, 32767
ADVERSARIAL = (32767, -32767, -32768, 0)
FRACS = (0, 13, 15, 16, 31)


class Wraps:
    """how many i32 / i16 results left their type (a debug build of the reference panics at the first)"""

    def __init__(self):
        self.i32 = self.i16 = 0


def _i32(v, w=None):
    r = ((v + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)
    if w is not None and r != v:
        w.i32 += 1
    return r


def _i16(v, w=None):
    r = ((v + (1 << 15)) & 0xFFFF) - (1 << 15)
    if w is not None and r != v:
        w.i16 += 1
    return r


class DirectForm1:
    """`DirectForm1<i16>` (biquad.rs:260-269,319): x = [x0, x1], y = [[y0, y1]]; `Default::default()` is all zero"""

    def __init__(self, x=(0, 0), y=(0, 0)):
        self.x, self.y = list(x), list(y)

    def words(self):
        return [self.x[0], self.x[1], self.y[0], self.y[1]]


def df1(ba, frac, st, x0, w=None):
    """biquad.rs:372-382"""
    acc = _i32(ba[0] * x0, w)                   # :373  `Q<i16,i32,F> * i16 -> i32(c) * i32(v)` (dsp-fixedpoint/src/lib.rs:310-312, ops.rs:91-97)
    acc = _i32(acc + _i32(ba[1] * st.x[0], w), w)  # :374  `Add for Q` wraps in release (ops.rs:63-76)
    acc = _i32(acc + _i32(ba[2] * st.x[1], w), w)  # :375
    acc = _i32(acc + _i32(ba[3] * st.y[0], w), w)  # :376
    acc = _i32(acc + _i32(ba[4] * st.y[1], w), w)  # :377
    y0 = _i16(acc >> frac, w)                   # :378  `.as_()`: (acc >> F) as i16 (num_traits_impl.rs:74-90, lib.rs:270-299)
    st.x = [x0, st.x[0]]                        # :379
    st.y = [y0, st.y[0]]                        # :380
    return y0


def clamp(v, lo, hi):
    """num_traits::clamp (the debug_assert!(min <= max) is gone in a release build)"""
    if v < lo:
        return lo
    if v > hi:
        return hi
    return v


def df1_clamp(ba, frac, u, lo, hi, st, x0, w=None):
    """biquad.rs:399-403"""
    y0 = clamp(_i16(df1(ba, frac, st, x0, w) + u, w), lo, hi)  # :400
    st.y[0] = y0                                               # :401
    return y0


def chain(secs, states, xs, w=None):
    """`[C] x [S]` (dsp-process/src/compose.rs:43-77), stage-major as the reference runs it: section k filters the whole block, then
    section k + 1 filters its output.  secs: (ba, frac) or (ba, frac, u, min, max) each; n = 0 copies (:63-65)"""
    ys = list(xs)
    for sec, st in zip(secs, states):
        ys = [df1(sec[0], sec[1], st, v, w) if len(sec) == 2 else df1_clamp(*sec, st, v, w) for v in ys]
    return ys


def from_sos(sos, frac):
    """biquad.rs:551-559, then `(v * 2^F).round() as i16` exactly: half away from zero on the rational value, saturating, NaN -> 0"""
    a0 = 1.0 / sos[3]
    out = []
    for v in (sos[0] * a0, sos[1] * a0, sos[2] * a0, -sos[4] * a0, -sos[5] * a0):
        s = v * 2.0 ** frac
        if math.isnan(s):
            out.append(0)
        elif math.isinf(s):
            out.append(I16_MAX if s > 0 else I16_MIN)
        else:
            r = math.floor(abs(Fraction(s)) + Fraction(1, 2))
            out.append(max(I16_MIN, min(I16_MAX, r if s >= 0 else -r)))
    return out


def from_sos_np(sos, frac):
    """the same over rows: sos [rows, 6] float64 -> [rows, 5] int16"""
    sos = np.asarray(sos, np.float64).reshape(-1, 6)
    with np.errstate(all="ignore"):
        a0 = 1.0 / sos[:, 3]
        v = np.stack([sos[:, 0] * a0, sos[:, 1] * a0, sos[:, 2] * a0, -sos[:, 4] * a0, -sos[:, 5] * a0], axis=1)
        s = np.ldexp(v, frac)
        mag = np.abs(s)
        whole = np.floor(mag)
        r = np.copysign(whole + (mag - whole >= 0.5), s)  # mag - whole is exact
        r = np.where(np.isnan(s), 0.0, np.clip(r, I16_MIN, I16_MAX))
    return r.astype(np.int64).astype(np.int16)


def chain_np(secs, state, x):
    """state: [4 n, lanes] uint32 (word-plane-major {x0, x1, y0, y1} per section, read as low halves, written back sign-extended,
    in place), x: [frames, lanes] int16 -> y [frames, lanes] int16.  Sample-major: all sections per frame"""
    frames, lanes = x.shape
    n = len(secs)
    s = state.view(np.int32).reshape(4 * n, lanes).astype(np.int16).astype(np.int32)  # low halves, sign-extended
    y = np.empty((frames, lanes), np.int16)
    cf = [[np.int32(c) for c in sec[0]] for sec in secs]
    for f in range(frames):
        v = x[f].astype(np.int32)
        for k, sec in enumerate(secs):
            q = s[4 * k:4 * k + 4]
            acc = cf[k][0] * v + cf[k][1] * q[0] + cf[k][2] * q[1] + cf[k][3] * q[2] + cf[k][4] * q[3]  # int32 arrays wrap
            y0 = (acc >> np.int32(sec[1])).astype(np.int16)
            if len(sec) == 5:
                y0 = (y0.astype(np.int32) + np.int32(sec[2])).astype(np.int16)
                y0 = np.where(y0 < sec[3], np.int16(sec[3]), np.where(y0 > sec[4], np.int16(sec[4]), y0)).astype(np.int16)
            q[1], q[0] = q[0].copy(), v
            q[3], q[2] = q[2].copy(), y0.astype(np.int32)
            v = y0.astype(np.int32)
        y[f] = v.astype(np.int16)
    if n:
        state.reshape(4 * n, lanes)[:] = s.view(np.uint32)
    return y


# ------------------------------------------------------------------ test inputs
def inputs(rng, frames, lanes):
    """random i16 with the values at the edges of the type mixed in"""
    x = rng.integers(I16_MIN, I16_MAX + 1, (frames, lanes)).astype(np.int16)
    pick = rng.integers(0, 8, x.shape)
    for i, v in enumerate(ADVERSARIAL):
        x[pick == i] = v
    return x


def random_state(rng, n, lanes):
    """words whose upper halves hold anything: only the low half is the value"""
    return rng.integers(0, 1 << 32, (4 * n, lanes), dtype=np.uint64).astype(np.uint32)


def random_sections(rng, n, clamped):
    """wild coefficients (the wrapping sums are the point), some sections at the edges of i16; every FRACS value comes up"""
    secs = []
    for k in range(n):
        kind = int(rng.integers(0, 4))
        if kind == 0:
            ba = [I16_MAX] * 5
        elif kind == 1:
            ba = [I16_MIN] * 5
        else:
            ba = [int(v) for v in rng.integers(I16_MIN, I16_MAX + 1, 5)]
        frac = int(FRACS[int(rng.integers(0, len(FRACS)))]) if rng.integers(0, 2) else int(rng.integers(0, 32))
        if clamped:
            u = int(rng.integers(I16_MIN, I16_MAX + 1))  # wraps the i16 sum about every other sample
            lo, hi = (int(v) for v in rng.integers(I16_MIN, I16_MAX + 1, 2))  # min > max half the time
            secs.append((ba, frac, u, lo, hi))
        else:
            secs.append((ba, frac))
    return secs


def sos_rows(rng, rows):
    """random sos rows, among them ones that saturate, tie at .5, divide by zero and hold NaN / inf"""
    sos = rng.normal(0, 1.5, (rows, 6))
    sos[:, 3] = rng.choice([1.0, 0.5, -2.0, 1e-6, 3.0], rows)
    sos[rng.integers(0, rows, rows // 20), rng.integers(0, 6, rows // 20)] = np.nan
    sos[rng.integers(0, rows, rows // 20), rng.integers(0, 6, rows // 20)] = np.inf
    sos[rng.integers(0, rows, rows // 40), 3] = 0.0
    tie = rng.integers(0, rows, rows // 10)
    sos[tie, 0] = (rng.integers(-70000, 70000, tie.size) + 0.5) / 8192.0  # ties at F = 13 when a0 = 1
    sos[tie, 3] = 1.0
    return sos
