"""The reference-locked lock-in as one case, shared by the CPU and the GPU form of the chain test: per lane a reference of its own
period, a tone at harmonic h of it with its own phase phi, timestamps -> RPLL -> batch LO (harmonic h) -> lock-in with an
external LO.  The specification side (tests/_rpll_spec.py and the checker library's lockin_i32_lo_process) is computed once.

Test infrastructure only."""
import ctypes as C
import functools

import numpy as np

from tests import _harness as H
from tests import _rpll_spec as S

CFG = (8, 9, 8)
LANES, UPDATES, K = 256, 2048, 3
HARMONICS = (1, 2, 3)  # lane l carries a tone at harmonic 1 + l % 3; accu_lo takes one harmonic per call, so the chain runs once per harmonic
LOCKIN_K = [[1 << 23]]  # `[Lowpass<1>; 1]`, time constant 2^8 samples: settled long before the last quarter, ripple at 2 h f far below the bound
AMPLITUDE = 1 << 28


def lockin_cfg():
    return H.lockin_cfg(LOCKIN_K)


@functools.lru_cache(maxsize=None)
def chain():
    """-> dict(ts, x, phi, h, accu, rpll_state, want {harmonic: [frames, lanes, 2]}, arms {harmonic: state after}); never modified"""
    rng = np.random.default_rng(11)
    period = rng.integers(300, 500, size=LANES)
    h = 1 + np.arange(LANES) % 3
    ts, tone, phi, _ = S.chain_case(CFG, period, K, h, UPDATES, seed=12, amplitude=float(AMPLITUDE))
    x = np.ascontiguousarray(np.round(tone).astype(np.int32))
    st = np.zeros((S.WORDS, LANES), np.uint32)
    accu = S.rpll_np(CFG, st, ts)
    frames = UPDATES << K
    want, arms = {}, {}
    cfg = lockin_cfg()
    for hh in HARMONICS:
        lo = np.ascontiguousarray(S.accu_lo_np((K, hh, 0), accu))
        so, y = np.zeros((4, LANES), np.uint32), np.empty((frames, LANES, 2), np.int32)
        assert H.oracle().fn["lockin_i32_lo_process"](C.byref(cfg), H._ptr(so), H._ptr(x), H._ptr(lo), H._ptr(y), LANES, frames, H.FM) == 0
        want[hh], arms[hh] = y, so
    out = dict(ts=ts, x=x, phi=phi, h=h, accu=accu, rpll_state=st, want=want, arms=arms, frames=frames)
    for v in (ts, x, phi, accu, st, *want.values(), *arms.values()):
        v.setflags(write=False)
    return out


def phase_error(case, hh, y):
    """|atan2(mean Q, mean I) + phi| (wrapped to +-pi) over the last quarter of y [frames, lanes, 2], for the lanes whose tone is at harmonic hh"""
    sel = case["h"] == hh
    q = case["frames"] // 4 * 3
    m = y[q:, sel].astype(np.float64).mean(axis=0)
    d = np.arctan2(m[:, 1], m[:, 0]) + case["phi"][sel]
    return np.abs((d + np.pi) % (2 * np.pi) - np.pi)
