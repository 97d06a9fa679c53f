"""idsp_dsm_u32 on the device against tests/_dsm_spec.py: every output byte and every state word, `array_equal`.  Outputs start
poisoned with -77, every buffer sits in the guard bands of tests/_guard.py, x is uploaded read-only, and the gap bytes of a pitched
y row must keep their poison."""
import ctypes as C

import numpy as np
import pytest
import torch

from idsp_amd import _abi
from tests import _dsm_spec as S
from tests._guard import Guards

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FM, LM = _abi.FRAME_MAJOR, _abi.LANE_MAJOR
POISON = -77
XGAP = 0x5A5A5A5A  # what the gaps of a pitched x hold
PREFIX = {FM: "dsm_frame_major", LM: "dsm_lane_major"}

SHAPES = [(1, 1), (1, 1000), (2, 3), (3, 5), (4, 4), (5, 9), (63, 33), (64, 32), (65, 31), (127, 7), (129, 2), (255, 257), (256, 8), (257, 1),
          (1000, 1000), (4099, 33), (16384, 130), (65537, 33)]


def _ptr(t, off_bytes=0):
    return C.c_void_p(t.data_ptr() + off_bytes) if t is not None else None


def _rows(layout, lanes, frames):
    """(rows, row): FrameMajor rows are frames of `lanes` elements, LaneMajor rows are lanes of `frames` elements"""
    return (frames, lanes) if layout == FM else (lanes, frames)


def _pitched(a2d, pitch, gap):
    """[rows, row] -> flat buffer of (rows - 1) * pitch + row elements, `gap` between the rows"""
    rows, row = a2d.shape
    buf = np.full((rows - 1) * pitch + row, gap, a2d.dtype)
    for r in range(rows):
        buf[r * pitch:r * pitch + row] = a2d[r]
    return buf


def run(gpu, order, layout, st, x, xp=0, yp=0, x_off=0, y_off=0, null_state=False):
    """one call; x: [frames, lanes] uint32, st: [2 K, lanes] uint32 -> (y [frames, lanes] int8, state after).  Checks the guard
    bands, the read-only x, the gaps of y and the kernel name."""
    frames, lanes = x.shape
    rows, row = _rows(layout, lanes, frames)
    xl, yl = xp or row, yp or row
    g = Guards(DEV)
    x2 = x if layout == FM else np.ascontiguousarray(x.T)
    xd = g.upload("x", _pitched(x2, xl, np.uint32(XGAP)), off=x_off, readonly=True)
    yd = g.full("y", (rows - 1) * yl + row, torch.int8, POISON, off=y_off)
    sd = None if null_state else g.upload("state", st)
    rc = gpu.fn["dsm_u32"](order, _ptr(sd), _ptr(xd), xp, _ptr(yd), yp, lanes, frames, layout, None)
    torch.cuda.synchronize()
    what = (order, layout, lanes, frames, xp, yp, x_off, y_off, gpu.last_kernel())
    assert rc == 0, (what, gpu.err())
    g.check(what)
    assert gpu.last_kernel().startswith(PREFIX[layout]), what
    yb = yd.cpu().numpy()
    idx = (np.arange(rows)[:, None] * yl + np.arange(row)[None, :]).reshape(-1)
    gap = np.ones(yb.size, bool)
    gap[idx] = False
    assert (yb[gap] == POISON).all(), ("a gap byte of y was written", what)
    y2 = yb[idx].reshape(rows, row)
    y = y2 if layout == FM else np.ascontiguousarray(y2.T)
    return y, (st.copy() if null_state else sd.cpu().numpy().view(np.uint32).reshape(st.shape))


def _case(order, lanes, frames, seed, zero_state=False):
    rng = np.random.default_rng(seed)
    x = S.inputs(rng, frames, lanes)
    st = np.zeros((2 * order, lanes), np.uint32) if zero_state else S.random_state(rng, order, lanes)
    want_st = st.copy()
    want = S.dsm_np(order, want_st, x)
    return x, st, want, want_st


@pytest.mark.parametrize("order", range(S.MAX_ORDER + 1))
def test_parity(gpu, order):
    for n, (lanes, frames) in enumerate(SHAPES):
        x, st, want, want_st = _case(order, lanes, frames, 1000 * order + n)
        for layout in (FM, LM):
            y, got_st = run(gpu, order, layout, st, x)
            assert np.array_equal(y, want), (order, layout, lanes, frames, gpu.last_kernel())
            assert np.array_equal(got_st, want_st), (order, layout, lanes, frames, "state", gpu.last_kernel())
            if order == 0:
                assert not y.any()
    if order == 0:  # no state: NULL is accepted
        x, st, want, _ = _case(0, 65, 31, 7)
        for layout in (FM, LM):
            y, _ = run(gpu, 0, layout, st, x, null_state=True)
            assert not y.any()


def _pitches(row):
    return [0, row + 1, row + 3, -(-row // 4) * 4, -(-row // 64) * 64]


@pytest.mark.parametrize("layout", [FM, LM])
@pytest.mark.parametrize("order", [1, 3, 8])
def test_alignment_and_pitch(gpu, order, layout):
    """y at every byte offset from the 512-byte grid, x at every word offset from the 16-byte grid, five pitches on either side: the y
    side and the x side each walk all their (offset, pitch) pairs against a dense aligned partner, then both walk together"""
    for n, (lanes, frames) in enumerate([(5, 9), (65, 31), (1000, 33)]):
        x, st, want, want_st = _case(order, lanes, frames, 50 * order + n)
        row = _rows(layout, lanes, frames)[1]
        ps = _pitches(row)
        combos = [(0, 0, y_off, yp) for y_off in range(4) for yp in ps]
        combos += [(x_off, xp, 0, 0) for x_off in (0, 4, 8, 12) for xp in ps]
        combos += [(4 * (i % 4), ps[(i + 1) % 5], (i + 1) % 4, ps[(2 * i + 3) % 5]) for i in range(5)]
        for x_off, xp, y_off, yp in combos:
            y, got_st = run(gpu, order, layout, st, x, xp=xp, yp=yp, x_off=x_off, y_off=y_off)
            what = (order, layout, lanes, frames, x_off, xp, y_off, yp, gpu.last_kernel())
            assert np.array_equal(y, want), what
            assert np.array_equal(got_st, want_st), what


@pytest.mark.parametrize("order", [2, 8])
@pytest.mark.parametrize("lanes,frames,chunks", [(1000, 333, [1, 7, 100, 225]), (65, 4096, [4000, 95, 1]), (16384, 130, [33, 1, 64, 32])])
def test_chunks(gpu, order, lanes, frames, chunks):
    """consecutive calls on one state equal one call and the spec; the layout may change between the calls of one state"""
    assert sum(chunks) == frames
    x, st, want, want_st = _case(order, lanes, frames, 77 + order)
    for layouts in ([FM] * len(chunks), [LM] * len(chunks), [(FM, LM)[i % 2] for i in range(len(chunks))]):
        cur, at, parts = st, 0, []
        for n, layout in zip(chunks, layouts):
            y, cur = run(gpu, order, layout, cur, x[at:at + n])
            parts.append(y)
            at += n
        assert np.array_equal(np.concatenate(parts), want), (order, lanes, frames, layouts)
        assert np.array_equal(cur, want_st), (order, lanes, frames, layouts, "state")
    one, one_st = run(gpu, order, LM, st, x)
    assert np.array_equal(one, want) and np.array_equal(one_st, want_st)


def test_zero_state_is_the_default_and_the_reference_doctest(gpu):
    """`Dsm::<3>::default()` fed 0x87654321 (src/dsm.rs:11-20) in 64 lanes, 2^20 frames LaneMajor in ONE call: the reference's own bound
    |mean(y) / (x / 2^32) - 1| < n^-1/2 per lane — the statistical bound, at the full 2^20 frames — all lanes identical, and the exact sum
    invariant of tests/test_dsm_spec.py on top"""
    lanes, n, xv = 64, 1 << 20, 0x87654321
    x = torch.full((lanes * n,), xv - (1 << 32), dtype=torch.int32, device=DEV)
    y = torch.full((lanes * n,), POISON, dtype=torch.int8, device=DEV)
    st = torch.zeros((6, lanes), dtype=torch.int32, device=DEV)
    assert gpu.fn["dsm_u32"](3, _ptr(st), _ptr(x), 0, _ptr(y), 0, lanes, n, LM, None) == 0, gpu.err()
    torch.cuda.synchronize()
    assert gpu.last_kernel().startswith(PREFIX[LM])
    y = y.reshape(lanes, n)
    assert bool((y == y[0]).all()), "lanes fed the same input differ"
    assert int(y.min()) >= -3 and int(y.max()) <= 4  # 1 - 2^(K-1) ..= 2^(K-1)
    sums = y.sum(dim=1, dtype=torch.int64).cpu().numpy()
    assert (np.abs(sums / n / (xv / 2.0 ** 32) - 1.0) < n ** -0.5).all()
    c = st.cpu().numpy()
    assert np.array_equal(sums, ((n * xv) >> 32) + c[4].astype(np.int64))  # + c[K-2]
    # the same from the spec's state after as many frames: a is n * x mod 2^32 per stage only for stage 0; check that one exactly
    assert (c[0].view(np.uint32) == (n * xv) & 0xFFFFFFFF).all() and not c[5].any()


@pytest.mark.parametrize("layout", [FM, LM])
def test_callers_stream(gpu, layout):
    """the launch is ordered behind the caller's stream and the call does not wait for the device (tests/_on_stream.py)"""
    from tests import _on_stream as OS

    order, lanes, frames = 3, 1000, 64
    x, st, want, want_st = _case(order, lanes, frames, 5)
    assert st.any()  # a non-zero state: the call is not blind
    g = Guards(DEV)
    c = OS.Call("dsm_u32", g)
    xd = c.stage("x", x if layout == FM else np.ascontiguousarray(x.T), readonly=True)
    yd, sd = c.read(c.out("y", lanes * frames, torch.int8, POISON)), c.read(c.stage("state", st))
    rc, (yb, sb) = c.run(lambda s: gpu.fn["dsm_u32"](order, _ptr(sd), _ptr(xd), 0, _ptr(yd), 0, lanes, frames, layout, s))
    torch.cuda.synchronize()
    g.check(("dsm_u32 on the caller's stream", layout, gpu.last_kernel()))
    assert rc == 0, gpu.err()
    assert c.armed and not c.blind
    y = yb.view(np.int8).reshape((frames, lanes) if layout == FM else (lanes, frames))
    assert np.array_equal(y if layout == FM else y.T, want)
    assert np.array_equal(sb.view(np.uint32).reshape(st.shape), want_st)


def test_rejections_write_nothing(gpu):
    lanes, frames, order = 16, 8, 3
    rng = np.random.default_rng(3)
    g = Guards(DEV)
    # one buffer that holds a pitched x (rows of 16 words, 32 apart); y is put at places inside and around it
    xbuf = g.upload("x", rng.integers(0, 1 << 32, 8 * 32, dtype=np.uint64).astype(np.uint32))
    g.freeze("x")
    yd = g.full("y", lanes * frames, torch.int8, POISON)
    g.freeze("y")
    sd = g.upload("state", S.random_state(rng, order, lanes), readonly=True)
    dsm = lambda x, xp, y, yp, layout=FM: gpu.fn["dsm_u32"](order, _ptr(sd), x, xp, y, yp, lanes, frames, layout, None)  # noqa: E731
    bad = [
        dsm(_ptr(xbuf), 0, _ptr(xbuf), 0),                 # y == x
        dsm(_ptr(xbuf), 0, _ptr(xbuf, 4 * 127), 0),        # y begins on the last word of x
        dsm(_ptr(xbuf, 127), 0, _ptr(xbuf), 0),            # x unaligned (and overlapping)
        dsm(_ptr(xbuf, 124), 0, _ptr(xbuf), 0),            # x begins on the last bytes of y
        dsm(_ptr(xbuf), 32, _ptr(xbuf, 64), 128),          # y rows inside the gaps of the pitched x
        dsm(_ptr(xbuf), 32, _ptr(xbuf, 64), 128, LM),
        dsm(_ptr(xbuf), 15, _ptr(yd), 0),                  # pitch shorter than a row
        dsm(_ptr(xbuf), 0, _ptr(yd), 15),
        dsm(_ptr(xbuf), 7, _ptr(yd), 0, LM),
        dsm(_ptr(xbuf), 0, _ptr(yd), 7, LM),
    ]
    torch.cuda.synchronize()
    assert all(rc == _abi.IDSP_EINVAL for rc in bad), bad
    assert gpu.err()
    g.check("rejected calls")
