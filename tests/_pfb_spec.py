"""numpy specification of the four-channel polyphase channelizer (reference: examples/polyphase_channelizer.rs), in two
independent restatements that tests/test_pfb_spec.py holds against each other:

  `bank_scalar`  one lane, `numpy.float32` scalars, the circular `hist` / `head` of `BankState` exactly as the reference walks them
  `bank_np`      every lane at once, direct (non-circular) indexing into [history | x] in time order; the circular state is
                 rebuilt at the end

Both keep f32 throughout and never fuse: a numpy product is rounded to f32 before the sum sees it.

State words (include/idsp_hip.h): uint32 [8*taps + 1, lanes]; word (slot*4 + m)*2 + c is `hist[slot][m][c]`, word 8*taps is `head`.
Frames travel as float32 [frames, lanes, 4, 2] = [f][lane][m][re, im].

Test infrastructure only."""
from __future__ import annotations

import numpy as np

F32 = np.float32
M = 4  # :19
TAU = F32(6.2831855)  # std::f32::consts::TAU (:17)


# ---------------------------------------------------------------------------------------------------------------- prototype
def sinc(x):
    """:29-31"""
    x = F32(x)
    return F32(1.0) if x == 0 else F32(np.sin(x) / x)


def prototype(taps):
    """:33-44 for M * taps coefficients, numpy f32 (cos / sin are numpy's f32 routines, not the reference's libm)."""
    n_taps = M * taps
    fc = F32(0.5) / F32(M) * F32(0.9)  # :34
    mid = F32(n_taps - 1) * F32(0.5)  # :35
    h = np.empty(n_taps, F32)
    for i in range(n_taps):  # :36-40
        n = F32(i) - mid
        w = F32(0.54) - F32(0.46) * F32(np.cos(TAU * F32(i) / F32(n_taps - 1)))
        h[i] = F32(2.0) * fc * sinc(TAU * fc * n) * w
    s = F32(-0.0)  # f32::sum (:41)
    for v in h:
        s = F32(s + v)
    return (h / s).astype(F32)  # :42


def coeff_of(h):
    """`bytemuck::cast` (:104): coeff[tap][m] = h[tap*4 + m]"""
    return np.ascontiguousarray(np.asarray(h, F32).reshape(-1, M))


# ------------------------------------------------------------------------------------------------------------------- state
def pack_state(hist, head):
    """hist float32 [taps, lanes, 4, 2] (physical slots), head [lanes] -> uint32 [8*taps + 1, lanes]"""
    taps, lanes = hist.shape[:2]
    st = np.empty((8 * taps + 1, lanes), np.uint32)
    st[:8 * taps] = np.ascontiguousarray(hist.transpose(0, 2, 3, 1)).reshape(8 * taps, lanes).view(np.uint32)
    st[8 * taps] = np.asarray(head, np.uint32)
    return st


def unpack_state(st):
    """-> (hist float32 [taps, lanes, 4, 2], head int64 [lanes])"""
    taps, lanes = (st.shape[0] - 1) // 8, st.shape[1]
    hist = np.ascontiguousarray(st[:8 * taps]).view(F32).reshape(taps, M, 2, lanes).transpose(0, 3, 1, 2)
    return np.ascontiguousarray(hist), st[8 * taps].astype(np.int64)


# ------------------------------------------------------------------------------------------------------------- restatement 1
def dft4_scalar(x):
    """`Dft4::process` (:80-100) on one frame [4][2] of numpy.float32 scalars: the eight sums as written, left to right."""
    return [
        [x[0][0] + x[1][0] + x[2][0] + x[3][0], x[0][1] + x[1][1] + x[2][1] + x[3][1]],  # :83-86
        [x[0][0] + x[1][1] - x[2][0] - x[3][1], x[0][1] - x[1][0] - x[2][1] + x[3][0]],  # :87-90
        [x[0][0] - x[1][0] + x[2][0] - x[3][0], x[0][1] - x[1][1] + x[2][1] - x[3][1]],  # :91-94
        [x[0][0] - x[1][1] - x[2][0] + x[3][1], x[0][1] + x[1][0] - x[2][1] - x[3][0]],  # :95-98
    ]


def bank_scalar(coeff, dft, st, lane, x):
    """One lane through `PolyphaseBank::process` (:57-75) (and `Dft4` when dft): st uint32 [8*taps + 1, lanes], column `lane`
    read and written back; x float32 [frames, 4, 2]; returns float32 [frames, 4, 2]."""
    taps = coeff.shape[0]
    hist = [[[F32(st[(s * M + m) * 2 + c, lane:lane + 1].view(F32)[0]) for c in range(2)] for m in range(M)] for s in range(taps)]
    head = int(st[8 * taps, lane])
    c = [[F32(coeff[t][m]) for m in range(M)] for t in range(taps)]
    out = np.empty((x.shape[0], M, 2), F32)
    with np.errstate(all="ignore"):
        for f in range(x.shape[0]):
            head = (head + taps - 1) % taps  # :59
            hist[head] = [[F32(x[f, m, 0]), F32(x[f, m, 1])] for m in range(M)]  # :60
            y = [[F32(0.0), F32(0.0)] for _ in range(M)]  # :62
            for tap in range(taps):  # :63
                h = hist[(head + tap) % taps]  # :67
                for m in range(M):  # :64-68
                    y[m][0] = y[m][0] + h[m][0] * c[tap][m]  # :69
                    y[m][1] = y[m][1] + h[m][1] * c[tap][m]  # :70
            if dft:
                y = dft4_scalar(y)  # :107-109
            out[f] = y
    for s in range(taps):
        for m in range(M):
            for cc in range(2):
                st[(s * M + m) * 2 + cc, lane:lane + 1] = np.array([hist[s][m][cc]], F32).view(np.uint32)
    st[8 * taps, lane] = head
    return out


# ------------------------------------------------------------------------------------------------------------- restatement 2
def dft4_np(v):
    """:80-100 on [..., 4, 2]"""
    r, i = v[..., 0], v[..., 1]
    o = np.empty_like(v)
    o[..., 0, 0] = r[..., 0] + r[..., 1] + r[..., 2] + r[..., 3]
    o[..., 0, 1] = i[..., 0] + i[..., 1] + i[..., 2] + i[..., 3]
    o[..., 1, 0] = r[..., 0] + i[..., 1] - r[..., 2] - i[..., 3]
    o[..., 1, 1] = i[..., 0] - r[..., 1] - i[..., 2] + r[..., 3]
    o[..., 2, 0] = r[..., 0] - r[..., 1] + r[..., 2] - r[..., 3]
    o[..., 2, 1] = i[..., 0] - i[..., 1] + i[..., 2] - i[..., 3]
    o[..., 3, 0] = r[..., 0] - i[..., 1] - r[..., 2] + i[..., 3]
    o[..., 3, 1] = i[..., 0] + r[..., 1] - i[..., 2] - r[..., 3]
    return o


def bank_np(coeff, dft, st, x):
    """Every lane: st uint32 [8*taps + 1, lanes] (updated in place), x float32 [frames, lanes, 4, 2] -> y of that shape.
    y[f] = sum over tap, in order, of x[f - tap] * coeff[tap] (:63-72 with the circular index resolved), starting from +0.0."""
    taps = coeff.shape[0]
    frames, lanes = x.shape[:2]
    hist, head = unpack_state(st)
    head = head % taps
    ln = np.arange(lanes)
    # time order, oldest first: ext[taps - 1 - k] = the frame k + 1 steps back = hist[(head + k) % taps] (:67 at tap = k + 1 of the next step)
    ext = np.empty((taps + frames, lanes, M, 2), F32)
    for k in range(taps):
        ext[taps - 1 - k] = hist[(head + k) % taps, ln]
    ext[taps:] = x
    y = np.zeros((frames, lanes, M, 2), F32)  # :62
    with np.errstate(all="ignore"):
        for tap in range(taps):
            y = y + ext[taps - tap:taps - tap + frames] * coeff[tap][None, None, :, None]  # :69-70
        if dft:
            y = dft4_np(y)
    new_head = (head - frames) % taps  # :59, `frames` times
    new_hist = np.empty_like(hist)
    for k in range(taps):
        new_hist[(new_head + k) % taps, ln] = ext[taps + frames - 1 - k]
    st[...] = pack_state(new_hist, new_head)
    return y


# ----------------------------------------------------------------------------------------------------------------- fixture
def tone(freq, n):
    """:123-127: n I/Q samples `Complex::from_angle(TAU * freq * i)`, f32 -> [n, 2]"""
    ang = (TAU * F32(freq) * np.arange(n, dtype=F32)).astype(F32)
    return np.stack([np.cos(ang), np.sin(ang)], axis=-1).astype(F32)


def frames_of(iq):
    """`as_chunks` (:113): [n, 2] -> [n / 4, 4, 2]"""
    return np.ascontiguousarray(iq.reshape(-1, M, 2))


def channel_powers(y, drop=128):
    """:131-142 on y [frames, ..., 4, 2] -> [..., 4]: mean power per channel over the frames from `drop` on, f32 in frame order"""
    p = np.zeros(y.shape[1:-1], F32)
    for f in range(drop, y.shape[0]):
        p = p + (y[f, ..., 0] * y[f, ..., 0] + y[f, ..., 1] * y[f, ..., 1])
    return p / F32(y.shape[0] - drop)


ROUTING = [(0.0, 0), (0.25, 1), (0.5, 2), (0.75, 3)]  # :168


def assert_routed(p, want):
    """:170-177 on one lane's channel powers"""
    assert int(np.argmax(p)) == want, (p, want)
    other = max(float(p[i]) for i in range(M) if i != want)
    assert float(p[want]) > 10.0 * other, (p, want)


def random_state(rng, taps, lanes, heads=None):
    """random `hist`, and `head` = every possible value in turn over the lanes (or `heads`)"""
    hist = rng.standard_normal((taps, lanes, M, 2)).astype(F32)
    head = np.arange(lanes) % taps if heads is None else np.asarray(heads)
    return pack_state(hist, head)
