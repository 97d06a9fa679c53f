"""`ByLane<[Biquad<Q16<F>>; N]>` / `ByLane<[BiquadClamp<Q16<F>, i16>; N]>` x `DirectForm1<i16>` (dsp-process/src/compose.rs:363-390 over
src/iir/biquad.rs:366-404): lane l runs configuration l on state l.  `chain_np` restates the chain of tests/_biquad_i16_spec.py with the
coefficients as arrays `[n, CV, lanes]` (the plane layout of include/idsp_hip.h: CV = 5 {b0, b1, b2, a1, a2}, CV = 8 {.., u, min, max})
broadcast over the lanes, one `frac` for the bank.  tests/test_biquad_i16_bylane_spec.py holds it, lane by lane, to the shared-coefficient
specification the project already trusts."""
import numpy as np

from tests import _biquad_i16_spec as S


def chain_np(coef, frac, state, x):
    """coef: [n, 5 | 8, lanes] int16, state: [4 n, lanes] uint32 (in place, as S.chain_np), x: [frames, lanes] int16 -> y [frames, lanes]"""
    frames, lanes = x.shape
    n, cv = coef.shape[0], coef.shape[1]
    assert cv in (5, 8) and coef.shape[2] == lanes and coef.dtype == np.int16 and 0 <= frac <= 31
    c = coef.astype(np.int32)
    s = state.view(np.int32).reshape(4 * n, lanes).astype(np.int16).astype(np.int32)  # low halves, sign-extended
    y = np.empty((frames, lanes), np.int16)
    for f in range(frames):
        v = x[f].astype(np.int32)
        for k in range(n):
            q = s[4 * k:4 * k + 4]
            acc = c[k, 0] * v + c[k, 1] * q[0] + c[k, 2] * q[1] + c[k, 3] * q[2] + c[k, 4] * q[3]  # int32 arrays wrap
            y0 = (acc >> np.int32(frac)).astype(np.int16)
            if cv == 8:
                y0 = (y0.astype(np.int32) + c[k, 5]).astype(np.int16)  # wrapping i16 sum
                y0 = np.where(y0 < coef[k, 6], coef[k, 6], np.where(y0 > coef[k, 7], coef[k, 7], y0)).astype(np.int16)  # min first
            q[1], q[0] = q[0].copy(), v
            q[3], q[2] = q[2].copy(), y0.astype(np.int32)
            v = y0.astype(np.int32)
        y[f] = v.astype(np.int16)
    if n:
        state.reshape(4 * n, lanes)[:] = s.view(np.uint32)
    return y


def planes(lane_secs, clamped):
    """lane_secs[l][k] = (ba, frac[, u, min, max]) -> coef [n, 5 | 8, lanes] int16"""
    lanes, n = len(lane_secs), len(lane_secs[0])
    coef = np.zeros((n, 8 if clamped else 5, lanes), np.int16)
    for l, secs in enumerate(lane_secs):
        assert len(secs) == n
        for k, sec in enumerate(secs):
            coef[k, :5, l] = sec[0]
            if clamped:
                coef[k, 5:, l] = sec[2:]
    return coef


def random_planes(rng, n, clamped, lanes, frac=None):
    """the distribution of S.random_sections drawn for every (section, lane) at once, for banks of many lanes: a quarter of the sections
    all 32767, a quarter all -32768, the rest random; u, min, max random (min > max half the time) -> (frac, coef [n, 5 | 8, lanes])"""
    if frac is None:
        frac = int(S.FRACS[int(rng.integers(0, len(S.FRACS)))]) if rng.integers(0, 2) else int(rng.integers(0, 32))
    coef = rng.integers(S.I16_MIN, S.I16_MAX + 1, (n, 8 if clamped else 5, lanes)).astype(np.int16)
    kind = rng.integers(0, 4, (n, 1, lanes))
    coef[:, :5] = np.where(kind == 0, np.int16(S.I16_MAX), np.where(kind == 1, np.int16(S.I16_MIN), coef[:, :5]))
    return frac, coef


def sections_of(coef, frac, lane):
    """lane `lane` of the planes as the section tuples of tests/_biquad_i16_spec.py"""
    return [(coef[k, :5, lane].tolist(), frac, *coef[k, 5:, lane].tolist()) for k in range(coef.shape[0])]


def random_bank(rng, n, clamped, lanes, frac=None):
    """every lane its own S.random_sections, all re-stamped with one frac (a random one of S.FRACS or 0..31 unless given)
    -> (lane_secs, frac, coef)"""
    if frac is None:
        frac = int(S.FRACS[int(rng.integers(0, len(S.FRACS)))]) if rng.integers(0, 2) else int(rng.integers(0, 32))
    lane_secs = [[(sec[0], frac, *sec[2:]) for sec in S.random_sections(rng, n, clamped)] for _ in range(lanes)]
    return lane_secs, frac, planes(lane_secs, clamped)
