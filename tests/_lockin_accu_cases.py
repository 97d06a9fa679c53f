"""Cases and specifications of idsp_lockin_i32_accu_process, shared by the CPU and the GPU tests.

The specification is a composition of two that the tree already holds: `accu_lo_np` (tests/_rpll_spec.py) fed to the checker
library's lockin_i32_lo_process, as tests/_rpll_chain.py does.  `per_sample_int` restates the same thing one sample at a time in
Python integers on oracle/spec.py; tests/test_lockin_accu_spec.py holds the two to each other bit for bit.

Conventions: ks = [[k0(, k1)]] * cascade; lo_cfg = (batch_log2, harmonic, offset); st [4 * order * cascade, lanes] uint32 = the I
arm's `[LowpassState<N>; K]` words, then the Q arm's (updated in place); x [frames, lanes] int32; accu [updates, lanes, 2] int32;
y [frames, lanes, 2] int32.

Test infrastructure only."""
import ctypes as C

import numpy as np

from oracle import spec as O
from tests import _harness as H
from tests import _rpll_spec as S

SHAPES = [(n, k) for n in (1, 2) for k in (1, 2, 3, 4)]  # (order, cascade): the eight the lock-in entries take
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1


def lowpass_ks(rng, order, cascade):
    """[k^2 / 2^32, -k sqrt 2] (src/lowpass.rs:37-38) or one gain, per cascade element"""
    ks = []
    for _ in range(cascade):
        k = int(rng.integers(1 << 16, 1 << 29))
        ks.append([int(rng.integers(1, I32_MAX))] if order == 1 else [int(k * k >> 32) or 1, -int(k * 1.4142135623730951)])
    return ks


def arm_words(order, cascade):
    return 4 * order * cascade


def random_state(rng, order, cascade, lanes):
    return rng.integers(0, 1 << 32, size=(arm_words(order, cascade), lanes), dtype=np.uint64).astype(np.uint32)


def adversarial_x(rng, frames, lanes):
    """full-range samples with i32::MIN, i32::MAX and 0 among them (the mixer's product and the lowpass's saturating subtraction)"""
    x = rng.integers(I32_MIN, 1 << 31, size=(frames, lanes), dtype=np.int64)
    pick = rng.random((frames, lanes))
    x[pick < 0.05] = I32_MIN
    x[(pick >= 0.05) & (pick < 0.10)] = I32_MAX
    x[(pick >= 0.10) & (pick < 0.15)] = 0
    x.reshape(-1)[:3] = (I32_MIN, I32_MAX, 0)[:x.size]
    return x.astype(np.int32)


def spec(ks, lo_cfg, st, x, accu):
    """accu_lo_np -> the checker library's lockin_i32_lo_process (FrameMajor); st is updated in place"""
    frames, lanes = x.shape
    assert accu.shape == (frames >> lo_cfg[0], lanes, 2) and frames == accu.shape[0] << lo_cfg[0]
    lo = np.ascontiguousarray(S.accu_lo_np(lo_cfg, accu))
    y = np.empty((frames, lanes, 2), np.int32)
    cfg = H.lockin_cfg(ks)
    assert H.oracle().fn["lockin_i32_lo_process"](C.byref(cfg), H._ptr(st), H._ptr(np.ascontiguousarray(x)), H._ptr(lo), H._ptr(y), lanes, frames, H.FM) == 0
    return y


def per_sample_int(ks, lo_cfg, st, x, accu):
    """`Accu::new(a.state, (a.step as u32 >> k) as i32) * h + Accu::new(offset, 0)` (src/accu.rs:40-54), `next()` per sample
    (:34-37), `Complex::from_angle` (src/complex.rs:237-240), the mixer and the arms (src/lockin.rs:17-39); st is updated in place"""
    k, h, offset = lo_cfg
    frames, lanes = x.shape
    order, cascade = len(ks[0]), len(ks)
    nk = order * cascade
    y = np.empty((frames, lanes, 2), np.int32)
    for l in range(lanes):
        arms = [[[O.i64(int(st[arm * 2 * nk + (c * order + j) * 2, l]) | (int(st[arm * 2 * nk + (c * order + j) * 2 + 1, l]) << 32)) for j in range(order)]
                 for c in range(cascade)] for arm in range(2)]
        for u in range(frames >> k):
            state = O.i32(O.i32(int(accu[u, l, 0]) * h) + offset)
            step = O.i32(O.i32((int(accu[u, l, 1]) & S.M32) >> k) * h)
            for j in range(1 << k):
                state = O.i32(state + step)
                t = (u << k) + j
                y[t, l] = O.lockin(ks, arms, int(x[t, l]), state)
        for arm in range(2):
            for c in range(cascade):
                for j in range(order):
                    w = arm * 2 * nk + (c * order + j) * 2
                    st[w, l], st[w + 1, l] = arms[arm][c][j] & S.M32, (arms[arm][c][j] >> 32) & S.M32
    return y
