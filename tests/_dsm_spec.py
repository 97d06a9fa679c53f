"""Two independent restatements of `Dsm<K>::process` (src/dsm.rs:44-57) as a RELEASE build of the reference computes it: every u32
and i8 operation wraps.

  * `Dsm`: a scalar transliteration, line by line, on Python ints with explicit u32 / i8 wrapping; it keeps the bit-shifting of `d`
    as the reference writes it and counts the i8 operations whose exact result left -128..=127 (`wraps`): where a debug build of
    the reference would panic.
  * `dsm_np(order, state_words, x)`: vectorised over lanes, explicit carry arrays instead of the bits of `d`, on the state record of
    include/idsp_hip.h — `state_words[2 * order, lanes]` uint32, rows 0..K-1 = a, rows K..2K-1 = c (read as the low byte, written
    back sign-extended, row 2K-1 never written) — updated in place.

Test infrastructure only."""
from __future__ import annotations

import numpy as np

MAX_ORDER = 8
M32 = 0xFFFFFFFF


def _i8(v: int) -> int:
    """wrapping `as i8` of an exact integer"""
    return ((v + 128) & 0xFF) - 128


class Dsm:
    """`Dsm<K>`: a: [u32; K], c: [i8; K] (:22-26)"""

    def __init__(self, order: int, a=None, c=None):
        assert 0 <= order <= MAX_ORDER
        self.K = order
        self.a = [int(v) & M32 for v in (a if a is not None else [0] * order)]
        self.c = [_i8(int(v)) for v in (c if c is not None else [0] * order)]
        assert len(self.a) == order and len(self.c) == order
        self.wraps = 0

    def _w(self, v: int) -> int:
        """an i8 operation: the wrapped result, counted when the exact one does not fit"""
        if not -128 <= v <= 127:
            self.wraps += 1
        return _i8(v)

    def process(self, x: int) -> int:
        K = self.K
        d = 0                                     # let mut d = 0i8;                       (:45)
        v = x & M32
        for i in range(K):                        # self.a.iter_mut().fold(x, |x, a| {      (:47)
            s = self.a[i] + v
            self.a[i], c = s & M32, s > M32       #     (*a, c) = a.overflowing_add(x);     (:48)
            d = _i8((d << 1) | int(c))            #     d = (d << 1) | c as i8;             (:49)  a shift never panics
            v = self.a[i]                         #     *a                                  (:50)
        y = d & 1                                 # .fold(d & 1, |mut y, c| {               (:52)
        # `take(K - 1)`: K = 0 wraps to usize::MAX in a release build and takes all of an empty array
        for j in range(max(K - 1, 0)):
            d >>= 1                               #     d >>= 1;  (arithmetic on i8)        (:53)
            t = self._w((d & 1) + y)              #     (d & 1) + y
            t = self._w(t - self.c[j])            #               - *c                      (:54)
            y, self.c[j] = t, y                   #     (y, *c) = (..., y);
        return y                                  #     y })                                (:55-56)


def dsm_np(order: int, state_words: np.ndarray, x: np.ndarray) -> np.ndarray:
    """x: [frames, lanes] uint32 -> y: [frames, lanes] int8; `state_words` ([2 * order, lanes] uint32) updated in place"""
    K = order
    x = np.asarray(x, dtype=np.uint32)
    frames, lanes = x.shape
    assert state_words.dtype == np.uint32 and state_words.shape == (2 * K, lanes)
    y = np.zeros((frames, lanes), np.int8)
    if K == 0:
        return y
    a = state_words[:K].astype(np.uint64)
    c = (state_words[K:2 * K - 1] & 0xFF).astype(np.int64)   # the low byte ...
    c = np.where(c >= 128, c - 256, c)                        # ... as i8
    carry = np.zeros((K, lanes), np.int64)
    for f in range(frames):
        v = x[f].astype(np.uint64)
        for i in range(K):
            s = a[i] + v
            carry[i] = (s >> np.uint64(32)).astype(np.int64)
            a[i] = s & np.uint64(M32)
            v = a[i]
        out = carry[K - 1].copy()
        for j in range(K - 1):
            nxt = carry[K - 2 - j] + out - c[j]
            nxt = ((nxt + 128) & 0xFF) - 128  # wrapping i8
            c[j] = out
            out = nxt
        y[f] = out.astype(np.int8)
    state_words[:K] = a.astype(np.uint32)
    state_words[K:2 * K - 1] = c.astype(np.int32).view(np.uint32)  # sign-extended
    return y


def random_state(rng, order: int, lanes: int) -> np.ndarray:
    """a: random u32; c: i8 uniform in -128..=127, stored with RANDOM upper bytes (only the low byte counts); row 2K-1 random too"""
    st = rng.integers(0, 1 << 32, (2 * order, lanes), dtype=np.uint64).astype(np.uint32)
    return st


def inputs(rng, frames: int, lanes: int) -> np.ndarray:
    """random words, with lanes of constants, 0, 0xFFFFFFFF, 0x80000000, 1 and alternating extremes mixed in"""
    x = rng.integers(0, 1 << 32, (frames, lanes), dtype=np.uint64).astype(np.uint32)
    special = [0x87654321, 0, 0xFFFFFFFF, 0x80000000, 1]
    for k, v in enumerate(special):
        if lanes > 1 + k:
            x[:, 1 + k::11] = v
    if lanes > 7:
        x[0::2, 7::11] = 0xFFFFFFFF
        x[1::2, 7::11] = 0
    return x
