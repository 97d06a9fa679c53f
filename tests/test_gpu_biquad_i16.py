"""idsp_biquad_i16_df1 / _df1_clamp on the device against tests/_biquad_i16_spec.py: every output element and every state word,
`array_equal`.  Outputs start poisoned with -77, every buffer sits in the guard bands of tests/_guard.py, x is uploaded read-only where
the call is not in place, and the gap elements of a pitched y row must keep their poison.  Every call is also held to the kernel form
the header promises for its addresses and pitches (include/idsp_hip.h, idsp_amd/csrc/biquad_i16_plan.h), restated here."""
import ctypes as C

import numpy as np
import pytest
import torch

from idsp_amd import _abi
from tests import _biquad_i16_spec as S
from tests import _subword_rows as R
from tests._guard import Guards
from tests._subword_rows import DEV, FM, LM, POISON
from tests._subword_rows import rows_of as _rows

pytestmark = pytest.mark.gpu
XGAP = 0x5A5A  # what the gaps of a pitched x hold
FRAMES = "biquad_i16_frame_major"
DWORDS, HALVES = "biquad_i16_lane_major[dword runs]", "biquad_i16_lane_major[half runs]"
K = {**R.constants("subword_rows.h"), **R.constants("biquad_i16_kernels.h")}  # kFmU, kLmTW, kLmTS

SHAPES = [(1, 1), (1, 1000), (2, 3), (3, 5), (5, 9), (63, 33), (64, 32), (65, 31), (127, 7), (128, 8), (129, 2), (255, 257), (256, 8), (257, 1),
          (511, 3), (512, 4), (513, 5), (1000, 1000), (4099, 33), (16384, 130), (24577, 33), (65537, 33)]
NS = [1, 2, 4, 5, 9]


def _ptr(t, off_elems=0):
    return R.ptr(t, 2 * off_elems)


def cfg_of(secs):
    """-> (entry name, ctypes array of the sections)"""
    clamped = bool(secs) and len(secs[0]) == 5
    arr = ((_abi.BiquadClampI16 if clamped else _abi.BiquadI16) * max(len(secs), 1))()
    for a, s in zip(arr, secs):
        a.ba[:] = s[0]
        a.frac = s[1]
        if clamped:
            a.u, a.min, a.max = s[2:]
    return ("biquad_i16_df1_clamp" if clamped else "biquad_i16_df1"), arr


def kernel_for(layout, lanes, x_addr, y_addr, xl, yl):
    """the header's rule: FrameMajor has one form; LaneMajor rows of x and y on the 4-byte grid take the dword runs"""
    grid4 = x_addr % 4 == 0 and y_addr % 4 == 0 and xl % 2 == 0 and yl % 2 == 0
    if layout == LM:
        return DWORDS if grid4 else HALVES
    return FRAMES


def run(gpu, secs, layout, st, x, xp=0, yp=0, x_off=0, y_off=0, inplace=False, clamped=False):
    """one call; x: [frames, lanes] int16, st: [4 n, lanes] uint32 -> (y [frames, lanes] int16, state after, kernel name).  x_off / y_off:
    ELEMENTS between the 512-byte grid and the first sample.  Checks the guard bands, the read-only x, the gaps of y and the kernel."""
    name, cfg = cfg_of(secs)
    if not secs and clamped:
        name = "biquad_i16_df1_clamp"

    def kernel_ok(kernel, x_addr, y_addr, xl, yl):
        if not secs:
            return True
        if len(secs) > 4:  # the last pass of a chain longer than one launch runs in place on y
            x_addr, xl = y_addr, yl
        return kernel == kernel_for(layout, x.shape[1], x_addr, y_addr, xl, yl)

    return R.run(gpu, lambda *a: gpu.fn[name](cfg, len(secs), *a, None), layout, st, x, x_gap=np.int16(XGAP), y_dtype=torch.int16, kernel_ok=kernel_ok,
                 xp=xp, yp=yp, x_off=2 * x_off, y_off=2 * y_off, inplace=inplace, what=(name, len(secs)))


def _case(n, clamped, lanes, frames, seed, zero_state=False):
    rng = np.random.default_rng(seed)
    secs = S.random_sections(rng, n, clamped)
    x = S.inputs(rng, frames, lanes)
    st = np.zeros((4 * n, lanes), np.uint32) if zero_state else S.random_state(rng, n, lanes)
    want_st = st.copy()
    want = S.chain_np(secs, want_st, x)
    return secs, x, st, want, want_st


@pytest.mark.parametrize("clamped", [False, True])
@pytest.mark.parametrize("n", NS)
def test_parity(gpu, n, clamped):
    seen = set()
    for i, (lanes, frames) in enumerate(SHAPES):
        secs, x, st, want, want_st = _case(n, clamped, lanes, frames, 1000 * n + 100 * clamped + i)
        for layout in (FM, LM):
            y, got_st, kernel = run(gpu, secs, layout, st, x)
            assert np.array_equal(y, want), (n, clamped, layout, lanes, frames, kernel)
            assert np.array_equal(got_st, want_st), (n, clamped, layout, lanes, frames, "state", kernel)
            seen.add(kernel)
    assert seen == {FRAMES, DWORDS, HALVES}  # dense LaneMajor rows: even row lengths are on the 4-byte grid, odd ones are not


@pytest.mark.parametrize("layout,lanes,frames,xp,x_off,kernel", [
    (FM, 128, 8, 0, 0, FRAMES), (FM, 129, 2, 130, 0, FRAMES), (FM, 128, 8, 0, 1, FRAMES), (FM, 65536, 2, 0, 0, FRAMES),  # (four waves per workgroup from 65536 lanes)
    (LM, 64, 32, 0, 0, DWORDS), (LM, 65, 31, 32, 0, DWORDS), (LM, 65, 31, 0, 0, HALVES), (LM, 64, 32, 0, 3, HALVES),
    (LM, 3, 300, 0, 0, DWORDS), (LM, 3, 301, 302, 0, DWORDS), (LM, 3, 301, 0, 0, HALVES),  # whole tiles, then a partial one with an odd tail
])
def test_every_kernel_form(gpu, layout, lanes, frames, xp, x_off, kernel):
    """each form the dispatch can pick, by name, with the alignment that selects it"""
    secs, x, st, want, want_st = _case(2, True, lanes, frames, 31)
    y, got_st, got = run(gpu, secs, layout, st, x, xp=xp, yp=xp, x_off=x_off, y_off=x_off)
    assert got == kernel
    assert np.array_equal(y, want) and np.array_equal(got_st, want_st)


@pytest.mark.parametrize("layout", [FM, LM])
@pytest.mark.parametrize("n,clamped", [(1, False), (2, True), (5, False)])
def test_alignment_and_pitch(gpu, n, clamped, layout):
    """x and y at every element offset 0..7 from the 16-byte grid, five pitches on either side (dense — odd rows among them —, row + 1,
    row + 3, the row rounded up to 2 and to 32 elements): the y side and the x side each walk all their (offset, pitch) pairs against a
    dense aligned partner, then both walk together"""
    for i, (lanes, frames) in enumerate([(5, 9), (65, 31), (130, 129)]):
        secs, x, st, want, want_st = _case(n, clamped, lanes, frames, 50 * n + i)
        ps = R.pitches(_rows(layout, lanes, frames)[1], 2, 32)
        for x_off, xp, y_off, yp in R.combos(ps, x_offs=range(8), y_offs=range(8), both=10, y_step=3):
            y, got_st, kernel = run(gpu, secs, layout, st, x, xp=xp, yp=yp, x_off=x_off, y_off=y_off)
            what = (n, clamped, layout, lanes, frames, x_off, xp, y_off, yp, kernel)
            assert np.array_equal(y, want), what
            assert np.array_equal(got_st, want_st), what


@pytest.mark.parametrize("layout", [FM, LM])
@pytest.mark.parametrize("n,clamped", [(1, True), (5, False)])
def test_inplace(gpu, n, clamped, layout):
    """y == x, dense and pitched, on and off the 4-byte grid; a dense pitch and its explicit value name the same pitch"""
    for i, (lanes, frames) in enumerate([(5, 9), (64, 32), (65, 31), (130, 300), (1000, 129)]):
        secs, x, st, want, want_st = _case(n, clamped, lanes, frames, 70 * n + i)
        row = _rows(layout, lanes, frames)[1]
        for off in (0, 1, 2):
            for xp in R.pitches(row, 2, 32):
                y, got_st, kernel = run(gpu, secs, layout, st, x, xp=xp, x_off=off, inplace=True)
                what = (n, clamped, layout, lanes, frames, off, xp, kernel)
                assert np.array_equal(y, want), what
                assert np.array_equal(got_st, want_st), what
    # x_pitch = 0 with y_pitch = row (and the other way round) is the same pitch
    lanes, frames = 64, 32
    secs, x, st, want, want_st = _case(n, clamped, lanes, frames, 9)
    row = _rows(layout, lanes, frames)[1]
    name, cfg = cfg_of(secs)
    for xp, yp in ((0, row), (row, 0)):
        g = Guards(DEV)
        xd = g.upload("xy", x if layout == FM else np.ascontiguousarray(x.T))
        sd = g.upload("state", st)
        assert gpu.fn[name](cfg, n, _ptr(sd), _ptr(xd), xp, _ptr(xd), yp, lanes, frames, layout, None) == 0, gpu.err()
        torch.cuda.synchronize()
        g.check(("in place", xp, yp))
        y = xd.cpu().numpy().reshape(x.shape if layout == FM else x.T.shape)
        assert np.array_equal(y if layout == FM else y.T, want)


@pytest.mark.parametrize("n,clamped", [(2, False), (5, True)])
@pytest.mark.parametrize("lanes,frames,chunks", [(1000, 333, [1, 7, 100, 225]), (65, 1000, [900, 99, 1]), (16384, 130, [33, 1, 64, 32])])
def test_chunks(gpu, n, clamped, lanes, frames, chunks):
    """consecutive calls on one state equal one call and the spec; the layout may change between the calls of one state"""
    assert sum(chunks) == frames
    secs, x, st, want, want_st = _case(n, clamped, lanes, frames, 77 + n)
    for layouts in ([FM] * len(chunks), [LM] * len(chunks), [(FM, LM)[i % 2] for i in range(len(chunks))]):
        cur, at, parts = st, 0, []
        for m, layout in zip(chunks, layouts):
            y, cur, _ = run(gpu, secs, layout, cur, x[at:at + m])
            parts.append(y)
            at += m
        assert np.array_equal(np.concatenate(parts), want), (n, lanes, frames, layouts)
        assert np.array_equal(cur, want_st), (n, lanes, frames, layouts, "state")
    one, one_st, _ = run(gpu, secs, LM, st, x)
    assert np.array_equal(one, want) and np.array_equal(one_st, want_st)


@pytest.mark.parametrize("layout", [FM, LM])
@pytest.mark.parametrize("n,clamped", [(1, False), (1, True), (4, False), (4, True)])
def test_window_and_tile_edges(gpu, n, clamped, layout):
    """frame counts one below, at and one above the counts the walkers of idsp_amd/csrc/subword_rows.h turn on — FrameMajor the window
    depth U, 2 U and 3 U + 1, out of place and in place; LaneMajor the tile TS and 2 TS, with rows on the dword grid (an even pitch), off
    it (x one element further) and in place — in 3 lanes and in 65 (two waves, the last one ragged): one call, and two calls cut at U / TS
    on one state, equal the spec in every element and every state word"""
    U, TS = K["kFmU"], K["kLmTS"]
    counts, cut = (R.around(U, 2 * U) + [3 * U + 1], U) if layout == FM else (R.around(TS, 2 * TS), TS)
    # (x_off, inplace, kernel)
    forms = [(0, False, FRAMES), (0, True, FRAMES)] if layout == FM else [(0, False, DWORDS), (1, False, HALVES), (0, True, DWORDS)]
    for lanes in (3, 65):
        for i, frames in enumerate(counts):
            secs, x, st, want, want_st = _case(n, clamped, lanes, frames, 300 * n + 100 * clamped + 10 * lanes + i)
            pitch = 0 if layout == FM else -(-frames // 2) * 2
            for x_off, inplace, kernel in forms:
                def one(s, xs):
                    y, got_st, got = run(gpu, secs, layout, s, xs, xp=pitch, yp=pitch, x_off=x_off, inplace=inplace)
                    assert got == kernel, (n, clamped, layout, lanes, frames, x_off, inplace)
                    return y, got_st

                for y, got_st in R.whole_and_split(one, st, x, cut):
                    assert np.array_equal(y, want), (n, clamped, layout, lanes, frames, x_off, inplace)
                    assert np.array_equal(got_st, want_st), (n, clamped, layout, lanes, frames, x_off, inplace, "state")


@pytest.mark.parametrize("layout", [FM, LM])
def test_no_sections_copy(gpu, layout):
    """n == 0: y.copy_from_slice(x) (compose.rs:63-65), the state is left alone; with pitches, and in place"""
    rng = np.random.default_rng(4)
    for lanes, frames in ((5, 9), (64, 32), (1000, 33)):
        x = S.inputs(rng, frames, lanes)
        st = S.random_state(rng, 1, lanes)
        row = _rows(layout, lanes, frames)[1]
        for clamped in (False, True):
            for xp, yp, x_off, y_off, inplace in ((0, 0, 0, 0, False), (row + 1, row + 3, 1, 2, False), (row + 3, 0, 0, 0, True)):
                y, got_st, _ = run(gpu, [], layout, st, x, xp=xp, yp=yp, x_off=x_off, y_off=y_off, inplace=inplace, clamped=clamped)
                assert np.array_equal(y, x) and np.array_equal(got_st, st)


KNOWN = [
    ([553, 1105, 553, 9363, -3382], 13, [1000, -2000, 32767, -32768, 0, 0, 5, 12345], [67, 76, 2068, 4405, 1972, -1777, -2845, -1685], None),
    ([32767] * 5, 0, [32767, 32767, -32768, 1, 2], [1, -32767, 0, -1, 32766], [2, 1, 32766, -1]),
    ([1 << 14, 0, 0, 0, 0], 14, [32767, -32768, 0, 1, -1, 12345], [32767, -32768, 0, 1, -1, 12345], None),  # identity
]


@pytest.mark.parametrize("layout", [FM, LM])
@pytest.mark.parametrize("lanes", [3, 64])
def test_zero_state_is_the_default_and_known_answers(gpu, lanes, layout):
    for ba, frac, xs, ys, state in KNOWN:
        x = np.repeat(np.array(xs, np.int16)[:, None], lanes, axis=1)
        st = np.zeros((4, lanes), np.uint32)
        y, got_st, kernel = run(gpu, [(ba, frac)], layout, st, x)
        assert np.array_equal(y, np.repeat(np.array(ys, np.int16)[:, None], lanes, axis=1)), (ba, frac, layout, kernel)
        words = got_st.view(np.int32)
        if state is None:
            state = [xs[-1], xs[-2], ys[-1], ys[-2]]
        assert (words == np.array(state, np.int32)[:, None]).all(), (ba, frac, layout, "state", kernel)  # sign-extended


@pytest.mark.parametrize("layout", [FM, LM])
@pytest.mark.parametrize("lanes,frames", [(1000, 64), (999, 65)])
def test_callers_stream(gpu, layout, lanes, frames):
    """the launches (two passes: five sections) are ordered behind the caller's stream and the call does not wait for the device
    (tests/_on_stream.py)"""
    from tests import _on_stream as OS

    secs, x, st, want, want_st = _case(5, True, lanes, frames, 5)
    assert st.any()  # a non-zero state: the call is not blind
    name, cfg = cfg_of(secs)
    g = Guards(DEV)
    c = OS.Call(name, g)
    xd = c.stage("x", x if layout == FM else np.ascontiguousarray(x.T), readonly=True)
    yd, sd = c.read(c.out("y", lanes * frames, torch.int16, POISON)), c.read(c.stage("state", st))
    rc, (yb, sb) = c.run(lambda s: gpu.fn[name](cfg, 5, _ptr(sd), _ptr(xd), 0, _ptr(yd), 0, lanes, frames, layout, s))
    torch.cuda.synchronize()
    g.check((name, "on the caller's stream", layout, gpu.last_kernel()))
    assert rc == 0, gpu.err()
    assert c.armed and not c.blind
    y = yb.view(np.int16).reshape((frames, lanes) if layout == FM else (lanes, frames))
    assert np.array_equal(y if layout == FM else y.T, want)
    assert np.array_equal(sb.view(np.uint32).reshape(st.shape), want_st)


def test_rejections_write_nothing(gpu):
    lanes, frames = 16, 8
    rng = np.random.default_rng(3)
    secs = S.random_sections(rng, 2, False)
    name, cfg = cfg_of(secs)
    g = Guards(DEV)
    # one buffer that holds a pitched x (rows of 16 elements, 32 apart); y is put at places inside and around it
    xbuf = g.upload("x", S.inputs(rng, 8, 32).reshape(-1))
    g.freeze("x")
    yd = g.full("y", lanes * frames, torch.int16, POISON)
    g.freeze("y")
    sd = g.upload("state", S.random_state(rng, 2, lanes), readonly=True)
    bq = lambda x, xp, y, yp, layout=FM: gpu.fn[name](cfg, 2, _ptr(sd), x, xp, y, yp, lanes, frames, layout, None)  # noqa: E731
    odd = lambda t, e=0: C.c_void_p(t.data_ptr() + 2 * e + 1)  # noqa: E731
    bad = [
        bq(_ptr(xbuf), 0, _ptr(xbuf, 127), 0),            # y begins on the last element of x: partial overlap
        bq(_ptr(xbuf, 1), 0, _ptr(xbuf), 0),              # x one element into y
        bq(_ptr(xbuf), 0, _ptr(xbuf), 17),                # y == x with another pitch
        bq(_ptr(xbuf), 32, _ptr(xbuf), 0),
        bq(_ptr(xbuf), 32, _ptr(xbuf, 16), 32),           # y rows inside the gaps of the pitched x: the EXTENTS overlap
        bq(_ptr(xbuf), 32, _ptr(xbuf, 16), 32, LM),
        bq(odd(xbuf), 0, _ptr(yd), 0),                    # odd addresses
        bq(_ptr(xbuf), 0, odd(yd), 0),
        bq(odd(xbuf), 0, odd(xbuf), 0, LM),
        bq(_ptr(xbuf), 15, _ptr(yd), 0),                  # pitch shorter than a row
        bq(_ptr(xbuf), 0, _ptr(yd), 15),
        bq(_ptr(xbuf), 7, _ptr(yd), 0, LM),
        bq(_ptr(xbuf), 0, _ptr(yd), 7, LM),
        bq(_ptr(xbuf), 0, _ptr(yd), 0, 2),                # layout
    ]
    cfg[1].frac = 32
    bad.append(bq(_ptr(xbuf), 0, _ptr(yd), 0))            # frac outside 0..31
    torch.cuda.synchronize()
    assert all(rc == _abi.IDSP_EINVAL for rc in bad), bad
    assert gpu.err()
    g.check("rejected calls")


@pytest.mark.parametrize("layout", [FM, LM])
def test_rows_beyond_4_gib(gpu, layout):
    """two rows 2^31 + 2 elements apart: the second starts 2^32 + 4 bytes into x and y (64-bit row offsets in every form's addressing).
    The buffers are not initialised; only the two rows are touched and compared"""
    pitch = (1 << 31) + 2
    row = 1002
    lanes, frames = (row, 2) if layout == FM else (2, row)
    secs, x, st, want, want_st = _case(2, True, lanes, frames, 8)
    name, cfg = cfg_of(secs)
    x2 = x if layout == FM else np.ascontiguousarray(x.T)
    xd = torch.empty(pitch + row, dtype=torch.int16, device=DEV)
    yd = torch.empty(pitch + row, dtype=torch.int16, device=DEV)
    for r in range(2):
        xd[r * pitch:r * pitch + row] = torch.from_numpy(x2[r].copy()).to(DEV)
        yd[r * pitch:r * pitch + row] = POISON
    sd = torch.from_numpy(st.view(np.int32).copy()).to(DEV)
    assert gpu.fn[name](cfg, 2, _ptr(sd), _ptr(xd), pitch, _ptr(yd), pitch, lanes, frames, layout, None) == 0, gpu.err()
    torch.cuda.synchronize()
    assert gpu.last_kernel() == (FRAMES if layout == FM else DWORDS)
    y2 = np.stack([yd[r * pitch:r * pitch + row].cpu().numpy() for r in range(2)])
    assert np.array_equal(y2 if layout == FM else y2.T, want)
    assert np.array_equal(sd.cpu().numpy().view(np.uint32), want_st)
    del xd, yd
    torch.cuda.empty_cache()


def test_python_mirror(gpu):
    """process.BiquadQ16 / BiquadQ16Lanes: block, inplace and LaneMajor views, plain and clamped, against the spec"""
    from idsp_amd import process as P

    lanes, frames = 66, 40
    for clamped in (False, True):
        secs, x, st, want, want_st = _case(3, clamped, lanes, frames, 12, zero_state=True)
        op = P.BiquadQ16Lanes([P.BiquadQ16(s[0], s[1], *s[2:]) for s in secs], lanes, DEV)
        assert op.clamp == clamped and tuple(op.state.shape) == (12, lanes)
        xd = torch.from_numpy(x.copy()).to(DEV)
        y = op.block(xd, torch.full_like(xd, POISON))
        assert np.array_equal(y.cpu().numpy(), want)
        assert np.array_equal(op.state.cpu().numpy().view(np.uint32), want_st)
        op.reset()
        assert np.array_equal(op.inplace(xd.clone()).cpu().numpy(), want)
        op.reset()
        xl, yl = torch.from_numpy(np.ascontiguousarray(x.T)).to(DEV), torch.full((lanes, frames), POISON, dtype=torch.int16, device=DEV)
        op.process_view(P.View(xl, P.LaneMajor, lanes), P.ViewMut(yl, P.LaneMajor, lanes))
        assert np.array_equal(yl.cpu().numpy().T, want)
    q = P.BiquadQ16.from_sos([0.06745527388907189, 0.13491054777814377, 0.06745527388907189, 1.4158, -1.1429805025399011, 0.4128015980961886], 13)
    assert q.frac == 13 and not q.clamp and q.ba == S.from_sos([0.06745527388907189, 0.13491054777814377, 0.06745527388907189, 1.4158,
                                                                  -1.1429805025399011, 0.4128015980961886], 13)
