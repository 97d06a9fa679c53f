"""Specification of idsp_rpll_i32 and idsp_accu_lo_i32: two independent restatements of each function, cited line by line against
the reference (src/rpll.rs, src/accu.rs, src/complex.rs:237-240), and the reference's test `Harness` (src/rpll.rs:105-206).

Restatement 1 (`rpll_int`, `accu_lo_int`) uses Python integers, one sample at a time, and `cossin` of oracle/spec.py.
Restatement 2 (`rpll_np`, `accu_lo_np`) uses numpy over lanes: uint64 arithmetic that wraps by itself, and the table form of cossin
(tests/_sweep_spec.py, held to oracle/spec.py there).  tests/test_rpll_spec.py holds the two to each other bit for bit and to the
reference's own limits (tests/golden/rpll_kat.json).

Conventions: cfg = (dt2, shift_frequency, shift_phase); st [4, lanes] uint32 = { x, ff, f, y } (updated in place); ts
[frames, lanes, 2] int32 = { some, x }; accu [frames, lanes, 2] int32 = { state, step }; lo_cfg = (batch_log2, harmonic, offset).

Test infrastructure only."""
import json
import os

import numpy as np

from oracle import spec as O
from tests._sweep_spec import cossin_np

WORDS = 4
M32 = 0xFFFFFFFF
M64 = 0xFFFFFFFFFFFFFFFF

# (dt2, shift_frequency, shift_phase): the smallest and largest of every shift, and the reference test's own
CONFIGS = [(0, 1, 0), (0, 32, 31), (8, 9, 8), (8, 23, 22), (11, 23, 23), (30, 31, 30), (30, 32, 61)]
LO_K = [0, 1, 3, 7, 10]
LO_HARMONICS = [0, 1, -1, 3, (1 << 31) - 1, -(1 << 31)]


def cfg_ok(cfg) -> bool:
    """the ranges in which every shift of :58-74 is defined (include/idsp_hip.h)"""
    dt2, sf, sp = cfg
    return 0 <= dt2 <= 30 and dt2 < sf <= 32 and dt2 <= sp <= dt2 + 31


# ------------------------------------------------------------------ restatement 1: Python integers
def rpll_step_int(cfg, s, some, x):
    """`RPLLConfig::process` (src/rpll.rs:47-77) on s = [x, ff, f, y] (x, y as i32 values; ff, f as u32 values) -> (y, f as i32)"""
    dt2, sf, sp = cfg
    s[3] = O.i32(s[3] + O.i32(s[2]))                                    # :51 state.y += W(state.f.0 as i32)
    if some:                                                           # :52
        dx = O.i32(x - s[0])                                           # :54
        s[0] = x                                                       # :56
        p_sig_64 = (s[1] * (dx & M64)) & M64                           # :58 `dx.0 as u64` of an i32: sign extension
        p_sig = (((p_sig_64 + (1 << (sf - 1))) & M64) >> sf) & M32     # :60-62
        p_ref = (1 << (32 + dt2 - sf)) & M32                           # :64 (a u32; the exponent is 0..31 for a valid cfg)
        s[1] = (s[1] + p_ref - p_sig) & M32                            # :66
        dt = O.i32(-x) & ((1 << dt2) - 1)                              # :68
        y_ref = O.i32(((s[2] >> dt2) * dt) & M32)                      # :70 the old f
        dy = O.i32(y_ref - s[3]) >> (sp - dt2)                         # :72 Python's >> on a negative int is arithmetic
        s[2] = (s[1] + (dy & M32)) & M32                               # :74
    return s[3], O.i32(s[2])                                           # :76


def rpll_int(cfg, st, ts):
    frames, lanes = ts.shape[:2]
    out = np.empty((frames, lanes, 2), np.int32)
    for l in range(lanes):
        s = [O.i32(int(st[0, l])), int(st[1, l]), int(st[2, l]), O.i32(int(st[3, l]))]
        for f in range(frames):
            out[f, l] = rpll_step_int(cfg, s, int(ts[f, l, 0]) != 0, int(ts[f, l, 1]))
        st[:, l] = [v & M32 for v in s]
    return out


def accu_lo_int(lo_cfg, accu):
    """sample = Accu::new(a.state, (a.step as u32 >> k) as i32) * harmonic + Accu::new(offset, 0) (src/accu.rs:40-54), then j + 1
    calls of `next()` (:34-37) and `Complex::from_angle` (src/complex.rs:237-240) for sample j of the update"""
    k, h, offset = lo_cfg
    updates, lanes = accu.shape[:2]
    out = np.empty((updates << k, lanes, 2), np.int32)
    for u in range(updates):
        for l in range(lanes):
            state = O.i32(O.i32(int(accu[u, l, 0]) * h) + offset)       # `Mul` then `Add` of the states
            step = O.i32(O.i32((int(accu[u, l, 1]) & M32) >> k) * h)    # the logical shift, then `Mul`; `+ 0`
            for j in range(1 << k):
                state = O.i32(state + step)                            # next(): pre-increment
                out[(u << k) + j, l] = O.cossin(state)
    return out


# ------------------------------------------------------------------ restatement 2: numpy over lanes
def rpll_np(cfg, st, ts):
    dt2, sf, sp = cfg
    frames, lanes = ts.shape[:2]
    out = np.empty((frames, lanes, 2), np.int32)
    x0, ff, f, y = (st[i].astype(np.uint64) for i in range(4))         # u32 values held in uint64
    m32, one = np.uint64(M32), np.uint64(1)
    half, p_ref = one << np.uint64(sf - 1), (one << np.uint64(32 + dt2 - sf)) & m32
    with np.errstate(over="ignore"):
        for t in range(frames):
            some = ts[t, :, 0] != 0
            x = ts[t, :, 1].astype(np.int64).astype(np.uint64) & m32
            y = (y + f) & m32                                                           # :51
            dx = ((x - x0) & m32).astype(np.uint32).view(np.int32).astype(np.int64)     # :54 as a signed value
            p64 = ff * dx.astype(np.uint64)                                             # :58 wraps modulo 2^64 by itself
            p_sig = ((p64 + half) >> np.uint64(sf)) & m32                               # :60-62
            nff = (ff + p_ref - p_sig) & m32                                            # :66
            dt = (-x.astype(np.int64)).astype(np.uint64) & np.uint64((1 << dt2) - 1)    # :68
            y_ref = ((f >> np.uint64(dt2)) * dt) & m32                                  # :70
            d = ((y_ref - y) & m32).astype(np.uint32).view(np.int32) >> np.int32(sp - dt2)  # :72 arithmetic on int32
            nf = (nff + d.astype(np.int64).astype(np.uint64)) & m32                     # :74
            x0, ff, f = np.where(some, x, x0), np.where(some, nff, ff), np.where(some, nf, f)
            out[t, :, 0] = y.astype(np.uint32).view(np.int32)
            out[t, :, 1] = f.astype(np.uint32).view(np.int32)
    for i, v in enumerate((x0, ff, f, y)):
        st[i] = v.astype(np.uint32)
    return out


def accu_lo_phase_np(lo_cfg, accu):
    """the sample phases [updates << k, lanes] (uint32) behind accu_lo_np"""
    k, h, offset = lo_cfg
    updates, lanes = accu.shape[:2]
    a = accu.astype(np.int64)
    hh = np.int64(h)
    state = ((a[..., 0] * hh + offset) & M32)[:, None, :]
    step = ((((a[..., 1] & M32) >> k) * hh) & M32)[:, None, :]
    j1 = np.arange(1, (1 << k) + 1, dtype=np.int64)[None, :, None]
    return ((state + j1 * step) & M32).reshape(updates << k, lanes).astype(np.uint32)


def accu_lo_np(lo_cfg, accu):
    ph = accu_lo_phase_np(lo_cfg, accu)
    c, s = cossin_np(ph.view(np.int32))
    return np.stack([c, s], axis=-1).astype(np.int32)


# ------------------------------------------------------------------ inputs
def random_state(rng, lanes):
    st = rng.integers(0, 1 << 32, size=(WORDS, lanes), dtype=np.uint64).astype(np.uint32)
    st[1, ::5] = M32  # ff = u32::MAX
    return st


def adversarial_ts(rng, frames, lanes, density=1 / 3):
    """full-range timestamps; `some` words that are 0, 1 or anything else; steps of 0, +-1, i32::MIN and i32::MAX between timestamps"""
    x = rng.integers(-(1 << 31), 1 << 31, size=(frames, lanes), dtype=np.int64)
    if frames > 1:
        d = np.array([0, 1, -1, -(1 << 31), (1 << 31) - 1, 1 << 20, -(1 << 20)], np.int64)
        pick = rng.random((frames, lanes)) < 0.3
        x = np.where(pick, np.roll(x, 1, axis=0) + d[rng.integers(0, d.size, size=(frames, lanes))], x)
    x[rng.random((frames, lanes)) < 0.02] = -(1 << 31)
    some = (rng.random((frames, lanes)) < density).astype(np.int64)
    some *= np.where(rng.random((frames, lanes)) < 0.5, 1, rng.integers(-(1 << 31), 1 << 31, size=(frames, lanes)) | 1)
    ts = np.empty((frames, lanes, 2), np.int32)
    ts[..., 0] = (some & M32).astype(np.uint32).view(np.int32)
    ts[..., 1] = (x & M32).astype(np.uint32).view(np.int32)
    return ts


def adversarial_accu(rng, updates, lanes):
    """full-range states and steps; every third lane's step has the top bit set (a logical shift differs from an arithmetic one)"""
    a = rng.integers(-(1 << 31), 1 << 31, size=(updates, lanes, 2), dtype=np.int64).astype(np.int32)
    a[:, ::3, 1] |= np.int32(-(1 << 31))
    a[:, 1::7, 1] = -1
    return a


# ------------------------------------------------------------------ the reference's test harness (src/rpll.rs:105-206)
def kat():
    """tests/golden/rpll_kat.json: the seven cases of src/rpll.rs:208-289 and what this specification measured for each"""
    return json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rpll_kat.json")))


def _w32(v):
    """int64 array -> wrapped to i32 values (int64)"""
    return ((v + (1 << 31)) & M32) - (1 << 31)


def _seqsum32(a):
    """`iter().sum::<f32>()`: a sequential f32 sum along axis 0"""
    return np.cumsum(a, axis=0, dtype=np.float32)[-1]


def t_settle(cfg):
    dt2, sf, sp = cfg
    return (1 << (sf - dt2 + 4)) + (1 << (sp - dt2 + 4))  # :176-177


class Harness:
    """`Harness` (:105-132) vectorised over lanes: per-lane `period`, `next` and `noise`, one configuration.  The timestamps do not
    depend on the RPLL, so `timestamps(n)` produces the input of n updates (and what `errors` needs), any implementation turns it
    into `Accu`s, and `errors` / `stats` form the reference's figures from them.  The noise comes from a numpy generator: the
    reference's `StdRng::seed_from_u64(42)` cannot be reproduced here."""

    def __init__(self, cfg, period, nxt, noise, seed=42):
        self.cfg = tuple(cfg)
        self.period = np.atleast_1d(np.asarray(period, np.int64))
        self.next = np.atleast_1d(np.asarray(nxt, np.int64)).copy()
        self.noise = np.atleast_1d(np.asarray(noise, np.int64))
        self.next_noisy = self.next.copy()
        self.time = np.zeros_like(self.next)
        self.rng = np.random.default_rng(seed)
        assert (self.period >= 1 << self.cfg[0]).all()  # :135 at most one timestamp per update()

    def lockable(self):
        """:136-137, the periods the reference's harness accepts for this configuration"""
        return (self.period < 1 << self.cfg[1]) & (self.period < 1 << (self.cfg[2] + 1))

    def timestamps(self, n):
        """-> ts [n, lanes, 2] int32, and (time, next) [n, lanes] after each update's timestamp decision (for `errors`)"""
        lanes, dt2 = self.period.size, self.cfg[0]
        ts = np.zeros((n, lanes, 2), np.int32)
        tm, nx = np.empty((n, lanes), np.int64), np.empty((n, lanes), np.int64)
        for i in range(n):
            late = _w32(self.time - self.next_noisy)
            due = late >= 0                                                            # :142
            assert (late[due] < 1 << dt2).all()                                        # :143
            self.next = np.where(due, _w32(self.next + self.period), self.next)        # :144
            ts[i, :, 0] = due
            ts[i, :, 1] = np.where(due, self.next_noisy, 0)                            # :145
            p_noise = self.rng.integers(-self.noise, self.noise + 1)                   # :146 -noise..=noise
            self.next_noisy = np.where(due, _w32(self.next + p_noise), self.next_noisy)  # :147
            tm[i], nx[i] = self.time, self.next
            self.time = _w32(self.time + (1 << dt2))                                   # :170
        return ts, (tm, nx)

    def errors(self, accu, book):
        """(y, f) [n, lanes] float32 of :155-167 from the `Accu`s ({ phase(), frequency() } after each update)"""
        tm, nx = book
        dt2 = self.cfg[0]
        yi, fi = accu[..., 0].astype(np.int64), accu[..., 1].astype(np.int64) & M32
        num = _w32(tm - nx) * (1 << 32)                                                # :156 i64
        q = np.abs(num) // self.period * np.sign(num)                                  # Rust's `/` truncates toward zero
        y_ref = _w32(q)                                                                # `as i32`
        y = _w32(yi - y_ref).astype(np.float32) / np.float32(2.0 ** 32)                # :159
        p_sig = fi.astype(np.uint64) * self.period.astype(np.uint64)                   # :162
        with np.errstate(over="ignore"):
            d = (p_sig - np.uint64(1 << (32 + dt2))).view(np.int64)                    # :165 wrapping_sub, `as i64`
        f = d.astype(np.float32) / np.float32(2.0 ** (32 + dt2))                       # :165-166
        return y, f

    @staticmethod
    def stats(y, f):
        """[fm, fs, ym, ys] per lane as :183-186, in f32 with sequential sums"""
        n = np.float32(f.shape[0])
        fm = _seqsum32(f) / n
        fs = np.sqrt(_seqsum32((f - fm) * (f - fm))) / n
        ym = _seqsum32(y) / n
        ys = np.sqrt(_seqsum32((y - ym) * (y - ym))) / n
        return np.stack([fm, fs, ym, ys])


def harness_case_int(case, n, seed):
    """One case of the reference's tests (:208-289) on restatement 1, harness and RPLL in one scalar loop (the settling times of the
    narrow cases are 8e5 updates): -> [fm, fs, ym, ys] as `measure` forms them (:175-186)."""
    cfg = tuple(case["cfg"])
    dt2 = cfg[0]
    period, nxt, noise = case["period"], case["next"], case["noise"]
    assert (1 << dt2) <= period < (1 << cfg[1]) and period < (1 << (cfg[2] + 1))      # :135-137
    settle = t_settle(cfg)
    draws = np.random.default_rng(seed).integers(-noise, noise + 1, size=(settle + n) * (1 << dt2) // period + 4).tolist()
    s = [0, 0, 0, 0]
    time, next_noisy, edge = 0, nxt, 0
    ys, fs = np.empty(n, np.float32), np.empty(n, np.float32)
    p_ref, scale_f = 1 << (32 + dt2), np.float32(2.0 ** (32 + dt2))
    for i in range(settle + n):
        late = O.i32(time - next_noisy)
        if late >= 0:
            assert late < 1 << dt2
            nxt = O.i32(nxt + period)
            yi, fi = rpll_step_int(cfg, s, True, next_noisy)
            next_noisy = O.i32(nxt + draws[edge])
            edge += 1
        else:
            yi, fi = rpll_step_int(cfg, s, False, 0)
        if i >= settle:
            num = O.i32(time - nxt) * (1 << 32)
            q = abs(num) // period
            y_ref = O.i32(q if num >= 0 else -q)
            ys[i - settle] = np.float32(O.i32(yi - y_ref))
            fs[i - settle] = np.float32(O.i64(((fi & M32) * period - p_ref) & M64))
        time = O.i32(time + (1 << dt2))
    return Harness.stats((ys / np.float32(2.0 ** 32))[:, None], (fs / scale_f)[:, None])[:, 0]


# ------------------------------------------------------------------ the chain: timestamps -> RPLL -> batch LO -> demodulation
def chain_case(cfg, period, k, harmonic, updates, seed, amplitude=1.0):
    """Per lane a reference with edges at edge0 + n * period and a tone cos(2 pi h (t - edge0) / period + phi) sampled 2^k times
    per update: sample j of update u is taken at counter time u 2^dt2 + (j + 1) 2^(dt2 - k), the instant the LO's `next()` number
    j + 1 stands for.  period, harmonic: one value or one per lane.  -> (ts [updates, lanes, 2], tone [updates << k, lanes] f64,
    phi [lanes], harmonic [lanes])"""
    rng = np.random.default_rng(seed)
    period = np.atleast_1d(np.asarray(period, np.int64))
    lanes = period.size
    h = np.broadcast_to(np.asarray(harmonic, np.int64), (lanes,))
    edge0 = rng.integers(0, period)
    phi = rng.uniform(-np.pi, np.pi, size=lanes)
    ts, _ = Harness(cfg, period, edge0, np.zeros(lanes, np.int64)).timestamps(updates)
    dt2 = cfg[0]
    t = (np.arange(updates, dtype=np.float64)[:, None] * (1 << dt2) + np.arange(1, (1 << k) + 1)[None, :] * 2.0 ** (dt2 - k)).reshape(-1, 1)
    tone = amplitude * np.cos(2 * np.pi * h[None, :] * (t - edge0[None, :]) / period[None, :] + phi[None, :])
    return ts, tone, phi, h
