"""Specification of the exponential swept sine (src/sweptsine.rs of the reference) for the suite: `Sweep` (:22-32), `AccuOsc` with
`Osc` for `W<i32>` (:180-188) and `Sweep`'s host functions (:34-118).

One frame of one lane, with state: i64, rate: i32, accu: i64, emitted: u64 (include/idsp_hip.h):

    s  = state
    t  = wrapping_i64(s + 2^31) >> 32
    ns = s + rate * t
    if ns is outside i64:  out = (0, 0), nothing changes        (`checked_add` -> None: the lane has ended)
    else:                  state = ns; accu = wrapping_i64(accu + s); emitted += 1; out = cossin((accu >> 32) as i32)

Two independent restatements:

  * `*_int`: Python big integers, literal range checks, lane by lane; cossin is oracle.spec's, called per sample.
  * `*_np`: numpy, vectorised over lanes.  The state is held as 32-bit halves in int64 arrays so that no sum can wrap unseen; the
    end test is a range check on the exact high half.  cossin is restated on arrays from oracle.spec's table (`cossin_np`): the
    per-sample Python function of oracle.spec costs microseconds per call, the GPU tests compare up to 40961 x 33 samples per case; tests/test_sweep_spec.py holds `cossin_np` to `oracle.spec.cossin` and the two
    restatements to each other word for word.

State words [7, lanes] uint32: { state lo, hi, accu lo, hi, rate, emitted lo, hi }.

Test infrastructure only."""
from __future__ import annotations

import functools
import math

import numpy as np

from oracle import spec as O

WORDS = 7
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
M32 = 0xFFFFFFFF
BIAS = 1 << 31


# ------------------------------------------------------------------ state words
def pack(state, rate, accu=0, emitted=0) -> np.ndarray:
    """per-lane sequences (or scalars) of Python ints -> [7, lanes] uint32"""
    cols = [np.atleast_1d(np.asarray(v, dtype=object)) for v in (state, rate, accu, emitted)]
    n = max(c.size for c in cols)
    st = np.zeros((WORDS, n), np.uint32)
    for l in range(n):
        s, r, a, e = (int(c[l % c.size]) for c in cols)
        st[:, l] = [s & M32, (s >> 32) & M32, a & M32, (a >> 32) & M32, r & M32, e & M32, (e >> 32) & M32]
    return st


def unpack_lane(st: np.ndarray, lane: int):
    """-> (state, rate, accu, emitted) as Python ints"""
    w = [int(v) for v in st[:WORDS, lane]]
    return O.i64(w[0] | (w[1] << 32)), O.i32(w[4]), O.i64(w[2] | (w[3] << 32)), w[5] | (w[6] << 32)


def emitted_of(st: np.ndarray) -> np.ndarray:
    return st[5].astype(np.uint64) | (st[6].astype(np.uint64) << np.uint64(32))


# ------------------------------------------------------------------ restatement 1: big integers
def sweep_next_int(state: int, rate: int):
    """`Sweep::next` (:26-31): the new state, or None where `checked_add` fails"""
    t = O.i64(state + BIAS) >> 32
    assert -(1 << 31) <= t < (1 << 31)
    ns = state + rate * t
    return ns if I64_MIN <= ns <= I64_MAX else None


def remaining_int(state: int, rate: int, limit: int):
    """samples the sweep still emits, or None if more than `limit`"""
    for n in range(limit + 1):
        state = sweep_next_int(state, rate)
        if state is None:
            return n
    return None


def osc_int(st: np.ndarray, frames: int) -> np.ndarray:
    """`AccuOsc<Sweep>` for `frames` frames on every lane; st updated; -> [frames, lanes, 2] int32"""
    lanes = st.shape[1]
    out = np.zeros((frames, lanes, 2), np.int32)
    for l in range(lanes):
        state, rate, accu, emitted = unpack_lane(st, l)
        for f in range(frames):
            ns = sweep_next_int(state, rate)
            if ns is None:
                break  # the lane has ended: (0, 0) from here on, nothing moves
            accu = O.i64(accu + state)  # Integrator: add first, then read (dsp-process/src/basic.rs:461-466)
            state = ns
            emitted = (emitted + 1) & ((1 << 64) - 1)
            out[f, l] = O.cossin(O.i32(accu >> 32))
        st[:WORDS, l] = pack(state, rate, accu, emitted)[:, 0]
    return out


# ------------------------------------------------------------------ restatement 2: numpy halves
def _i32w(v):
    """int64 array -> wrapped into i32 range (still int64)"""
    return ((v + (1 << 31)) & M32) - (1 << 31)


_TAB = np.array(O.cossin_table(), dtype=np.int64)


def cossin_np(phase) -> tuple:
    """src/cossin.rs:14-67 on an int32 array -> (cos, sin) int64 arrays holding i32 values"""
    u = np.asarray(phase).astype(np.int64) & M32
    p = np.where(u & (1 << 29), ~u & M32, u)
    p = ((p << 3) & M32) >> 10
    lookup = _TAB[p >> 15]
    q = (p & 0x7FFF) - (1 << 14)
    dphi = _i32w(q * int(math.pi / 4 * (1 << 16))) >> 16
    c, s = (lookup & 0xFFFF) + (1 << 16), lookup >> 16
    dcos, dsin = _i32w(s * dphi) >> 7, _i32w(c * dphi) >> 8
    c, s = _i32w((c << 14) - dcos), _i32w((s << 15) + dsin)
    octant = u ^ (u >> 1)
    swap = (octant & (1 << 29)) != 0
    c, s = np.where(swap, s, c), np.where(swap, c, s)
    c = np.where(octant & (1 << 30), _i32w(-c), c)
    s = np.where(octant & (1 << 31), _i32w(-s), s)
    return c, s


class _Halves:
    """the sweep words of [7, lanes] as arrays: state as (signed hi, unsigned lo) in int64, accu and emitted as uint64"""

    def __init__(self, st):
        self.lo = st[0].astype(np.int64)
        self.hi = st[1].view(np.int32).astype(np.int64)
        self.accu = st[2].astype(np.uint64) | (st[3].astype(np.uint64) << np.uint64(32))
        self.rate = st[4].view(np.int32).astype(np.int64)
        self.em = emitted_of(st)

    def peek(self):
        """-> (live, new lo, new hi): the exact sum in halves and a literal range check on the high one"""
        t = _i32w(self.hi + ((self.lo + BIAS) >> 32))
        p = self.rate * t  # |p| <= 2^62: exact in int64
        lo = self.lo + (p & M32)
        hi = self.hi + (p >> 32) + (lo >> 32)  # exact: a few times 2^31 at the most
        return (hi >= -(1 << 31)) & (hi < (1 << 31)), lo & M32, hi

    def next(self):
        """one frame -> (live, phase as int64 holding i32)"""
        live, lo, hi = self.peek()
        s64 = ((self.hi & M32).astype(np.uint64) << np.uint64(32)) | self.lo.astype(np.uint64)
        self.accu = np.where(live, self.accu + s64, self.accu)  # uint64 sums wrap
        self.lo, self.hi = np.where(live, lo, self.lo), np.where(live, hi, self.hi)
        self.em = self.em + live.astype(np.uint64)
        return live, _i32w((self.accu >> np.uint64(32)).astype(np.int64))

    def store(self, st):
        st[0], st[1] = self.lo.astype(np.uint32), (self.hi & M32).astype(np.uint32)
        st[2], st[3] = (self.accu & np.uint64(M32)).astype(np.uint32), (self.accu >> np.uint64(32)).astype(np.uint32)
        st[5], st[6] = (self.em & np.uint64(M32)).astype(np.uint32), (self.em >> np.uint64(32)).astype(np.uint32)


def ended_np(st: np.ndarray) -> np.ndarray:
    """per lane: the next frame would not emit"""
    return ~_Halves(st).peek()[0]


def osc_np(st: np.ndarray, frames: int) -> np.ndarray:
    h = _Halves(st)
    out = np.zeros((frames, st.shape[1], 2), np.int32)
    for f in range(frames):
        live, ph = h.next()
        c, s = cossin_np(ph)
        out[f, :, 0], out[f, :, 1] = np.where(live, c, 0), np.where(live, s, 0)
    h.store(st)
    return out


# ------------------------------------------------------------------ host functions (:34-118)
Q = float(np.float32(1 << 32))


def _as_int(v, bits):
    """Rust's float `as` integer: truncating, saturating, NaN -> 0"""
    v = float(v)
    if v != v:
        return 0
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    if v >= hi:
        return hi
    if v <= lo:
        return lo
    return int(v)


@functools.lru_cache(maxsize=None)
def _expm1f():
    """`f32::exp_m1` is the platform's `expm1f` in the reference (Rust's std calls libm) and in the library.  It is not correctly
    rounded — glibc's and numpy's f32 `expm1` each differ from the rounded f64 result on about 5 % of random arguments, and from each
    other — so the one call is taken from the same libm here; everything around it is restated.  The reference's own figure
    (rate 0x22f40, tests/golden/sweep_kat.json) pins the call itself."""
    import ctypes
    import ctypes.util

    f = ctypes.CDLL(ctypes.util.find_library("m")).expm1f
    f.restype, f.argtypes = ctypes.c_float, [ctypes.c_float]
    return f


def fit(stop, harmonics, cycles):
    """`Sweep::fit` in f32 -> (rate, state); ValueError with the reference's text"""
    f = np.float32
    stop, harmonics, cycles = f(stop), f(harmonics), f(cycles)
    if not (f(0.0) <= stop <= f(0.5)):
        raise ValueError("Stop out of bounds")
    with np.errstate(all="ignore"):
        r = f(Q) * f(_expm1f()(float(stop / (cycles * harmonics))))
        r = float(r)
        rounded = r if (r != r or math.isinf(r)) else math.copysign(math.floor(abs(r) + 0.5), r)  # f32::round: half away from zero
    rate = _as_int(rounded, 32)
    state = O.i64(((rate * _as_int(cycles, 64)) & ((1 << 64) - 1)) << 32)
    if state <= 0:
        raise ValueError("Start out of bounds")
    return rate, state


def rate_f(rate):
    return math.log1p(rate / Q)


def delay(rate, harmonic):
    return math.log(harmonic) / rate_f(rate)


def octave(rate):
    return math.log(2.0) / rate_f(rate)


def decade(rate):
    return math.log(10.0) / rate_f(rate)


def cycles_f(rate, state):
    return state / (Q * rate)


def state_f(rate, state):
    return cycles_f(rate, state) * rate_f(rate)


def continuous(rate, state, t):
    return cycles_f(rate, state) * math.exp(rate_f(rate) * t)


def inverse_filter(rate, state, f):
    """:93-101 with f32 roundings after every operation (libm calls in f32)"""
    g = np.float32
    with np.errstate(all="ignore"):
        r = np.log1p(g(rate) / g(Q), dtype=np.float32)
        f = g(f) / r
        amp = g(2.0) * r * np.sqrt(f, dtype=np.float32)
        inv_cycles = g(Q) * g(rate) / g(state)
        turns = g(0.125) - f * (g(1.0) - np.log(f * inv_cycles, dtype=np.float32))
        a = g(2 * math.pi) * turns
        return complex(amp * np.cos(a, dtype=np.float32), amp * np.sin(a, dtype=np.float32))


# ------------------------------------------------------------------ lane populations
KAT_FIT = (0.3, 3000.0, 3.0)  # the reference test's sweep (:199-202)
KAT_TOTAL = 255515            # samples it emits before `checked_add` fails (tests/golden/sweep_kat.json)
TAIL = 2048

# (state, rate): the corner rows of the issue and their neighbours; what each does is in tests/golden/sweep_kat.json
CORNERS = [
    (1 << 62, 1 << 30), ((1 << 62) + 12345, (1 << 31) - 1), (I64_MAX, 1), (I64_MAX - (1 << 31) + 1, 0), (0, 12345), (0, -(1 << 31)),
    (-(1 << 40), -7), (-(1 << 62), -(1 << 30)), (1 << 62, -(1 << 31)), (I64_MAX, -1), (I64_MIN, -1), (I64_MIN, -(1 << 31)),
    (I64_MIN, 1), (-(1 << 62), 1 << 30), (-(1 << 62) - 12345, (1 << 31) - 1), (I64_MAX, (1 << 31) - 1), (I64_MAX - (1 << 31), 1),
    (-1, (1 << 31) - 1), ((1 << 31) - 1, (1 << 31) - 1), (1 << 31, 1),
]


@functools.lru_cache(maxsize=None)
def kat_tail():
    """the last TAIL + 1 states of the reference test's sweep: entry m has exactly m samples left (entry 0 has ended)"""
    rate, state = fit(*KAT_FIT)
    states = [state]
    for _ in range(KAT_TOTAL):
        states.append(sweep_next_int(states[-1], rate))
    assert sweep_next_int(states[-1], rate) is None
    return rate, states[:-TAIL - 2:-1]


KINDS = ("inside", "before", "never", "random", "corner", "last", "boundary", "underway")


def population(rng, lanes: int, frames: int, boundary: int = 0, variant: int = 0) -> np.ndarray:
    """[7, lanes] uint32 — lane l is of kind KINDS[(l + variant) % 8]:
    inside: ends after 1 .. frames - 1 samples; before: has ended; never: a fresh fit-derived sweep; random: any (state, rate);
    corner: CORNERS in turn; last: its last sample is the call's last frame; boundary: its last sample is frame `boundary` - 1;
    underway: the reference test's sweep somewhere on its way.  accu is random, emitted random with the carries in reach."""
    rate_k, tail = kat_tail()
    assert frames <= TAIL
    fits = [fit(*KAT_FIT), fit(0.5, 1e6, 1.0), fit(0.01, 7.0, 123.0), fit(0.25, 100000.0, 2.9)]
    state, rate = [], []
    for l in range(lanes):
        kind = KINDS[(l + variant) % len(KINDS)]
        turn = l // len(KINDS)
        if kind == "inside":
            s, r = tail[1 + turn % max(frames - 1, 1)], rate_k
        elif kind == "before":
            s, r = (tail[0], rate_k) if turn % 2 == 0 else (I64_MAX - (1 << 32) - turn, (1 << 31) - 1 - turn)
        elif kind == "never":
            r, s = fits[turn % len(fits)]
        elif kind == "random":
            s, r = int(rng.integers(I64_MIN, I64_MAX, endpoint=True)), int(rng.integers(-(1 << 31), (1 << 31) - 1, endpoint=True))
        elif kind == "corner":
            s, r = CORNERS[turn % len(CORNERS)]
        elif kind == "last":
            s, r = tail[frames], rate_k
        elif kind == "boundary":
            s, r = tail[boundary if boundary else 1 + turn % TAIL], rate_k
        else:
            s, r = tail[int(rng.integers(frames + 1, TAIL, endpoint=True))], rate_k
        state.append(s), rate.append(r)
    accu = [int(v) for v in rng.integers(I64_MIN, I64_MAX, size=lanes, endpoint=True)]
    em = [(0, 5, M32, M32 - 2, (1 << 64) - 1, (1 << 64) - 3, 1 << 40)[int(v)] for v in rng.integers(0, 7, size=lanes)]
    return pack(state, rate, accu, em)


def classify(before: np.ndarray, after: np.ndarray, frames: int):
    """-> (inside, ended before, never) lane masks of a call of `frames` frames from state `before` to state `after`"""
    e = (emitted_of(after) - emitted_of(before)).astype(np.int64)
    gone = ended_np(after)
    return (e > 0) & (e < frames) & gone, (e == 0) & ended_np(before), (e == frames) & ~gone
