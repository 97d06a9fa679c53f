"""idsp_dsm_u32 on the device against tests/_dsm_spec.py: every output byte and every state word, `array_equal`.  Outputs start
poisoned with -77, every buffer sits in the guard bands of tests/_guard.py, x is uploaded read-only, and the gap bytes of a pitched
y row must keep their poison."""
import numpy as np
import pytest
import torch

from idsp_amd import _abi
from tests import _dsm_spec as S
from tests import _subword_rows as R
from tests._guard import Guards
from tests._subword_rows import DEV, FM, LM, POISON
from tests._subword_rows import ptr as _ptr

pytestmark = pytest.mark.gpu
XGAP = 0x5A5A5A5A  # what the gaps of a pitched x hold
PREFIX = {FM: "dsm_frame_major", LM: "dsm_lane_major"}
K = {**R.constants("subword_rows.h"), **R.constants("dsm_kernels.h")}  # kFmU, kLmTS, kLmOT

SHAPES = [(1, 1), (1, 1000), (2, 3), (3, 5), (4, 4), (5, 9), (63, 33), (64, 32), (65, 31), (127, 7), (129, 2), (255, 257), (256, 8), (257, 1),
          (1000, 1000), (4099, 33), (16384, 130), (65537, 33)]


def run(gpu, order, layout, st, x, xp=0, yp=0, x_off=0, y_off=0, null_state=False, kernel=None):
    """one call; x: [frames, lanes] uint32, st: [2 K, lanes] uint32 -> (y [frames, lanes] int8, state after).  x_off / y_off: bytes.
    Checks the guard bands, the read-only x, the gaps of y and the kernel name (its prefix, or all of it where `kernel` is given)."""
    y, got_st, _ = R.run(gpu, lambda *a: gpu.fn["dsm_u32"](order, *a, None), layout, st, x, x_gap=np.uint32(XGAP), y_dtype=torch.int8,
                         kernel_ok=lambda k, *_: k == kernel if kernel else k.startswith(PREFIX[layout]), xp=xp, yp=yp, x_off=x_off, y_off=y_off,
                         null_state=null_state, what=("dsm_u32", order))
    return y, got_st


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


@pytest.mark.parametrize("layout", [FM, LM])
@pytest.mark.parametrize("order", [1, 3, 8])
def test_alignment_and_pitch(gpu, order, layout):
    """y at every byte offset from the 512-byte grid, x at every word offset from the 16-byte grid, five pitches on either side: the y
    side and the x side each walk all their (offset, pitch) pairs against a dense aligned partner, then both walk together"""
    for n, (lanes, frames) in enumerate([(5, 9), (65, 31), (1000, 33)]):
        x, st, want, want_st = _case(order, lanes, frames, 50 * order + n)
        ps = R.pitches(R.rows_of(layout, lanes, frames)[1], 4, 64)
        combos = R.combos(ps, x_offs=(0, 4, 8, 12), y_offs=range(4), both=5, y_step=1)
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


@pytest.mark.parametrize("layout", [FM, LM])
@pytest.mark.parametrize("order", [1, 8])
def test_window_and_tile_edges(gpu, order, layout):
    """frame counts one below, at and one above the counts the walkers of idsp_amd/csrc/subword_rows.h turn on — FrameMajor the window
    depth U, 2 U and 3 U + 1; LaneMajor the input tile TS, the output tile OT TS and one past the next input tile, each on an aligned y
    with a pitch of whole dwords (dword runs) and on the same rows one byte further (byte runs) — in 3 lanes and in 65 (two waves, the last
    one ragged): one call, and two calls cut at U / TS on one state, equal the spec in every byte and every state word"""
    U, TS, OT = K["kFmU"], K["kLmTS"], K["kLmOT"]
    counts, cut = (R.around(U, 2 * U) + [3 * U + 1], U) if layout == FM else (R.around(TS, OT * TS) + [(OT + 1) * TS + 1], TS)
    forms = [(0, None)] if layout == FM else [(0, "dsm_lane_major[dword runs]"), (1, "dsm_lane_major[byte runs]")]
    for lanes in (3, 65):
        for n, frames in enumerate(counts):
            x, st, want, want_st = _case(order, lanes, frames, 300 * order + 10 * lanes + n)
            yp = 0 if layout == FM else -(-frames // 4) * 4
            for y_off, kernel in forms:
                one = lambda s, xs: run(gpu, order, layout, s, xs, yp=yp, y_off=y_off, kernel=kernel)  # noqa: E731
                for y, got_st in R.whole_and_split(one, st, x, cut):
                    assert np.array_equal(y, want), (order, layout, lanes, frames, y_off)
                    assert np.array_equal(got_st, want_st), (order, layout, lanes, frames, y_off, "state")


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
