"""idsp_biquad_i16_df1_bylane / _df1_clamp_bylane on the device against tests/_biquad_i16_bylane_spec.py: every output element and every
state word, `array_equal`.  The calls go through tests/_subword_rows.py: run (outputs poisoned, guard bands, read-only x, the gaps of a
pitched y); the coefficient planes are uploaded read-only into guard bands of the test's own, and every call is held to the by-lane kernel
name its addresses and pitches select (include/idsp_hip.h, idsp_amd/csrc/biquad_i16_plan.h)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from idsp_amd import _abi
from tests import _biquad_i16_bylane_spec as B
from tests import _biquad_i16_spec as S
from tests import _subword_rows as R
from tests._guard import Guards
from tests._subword_rows import DEV, FM, LM, POISON
from tests._subword_rows import rows_of as _rows

pytestmark = pytest.mark.gpu
XGAP = 0x5A5A  # what the gaps of a pitched x hold
FRAMES = "biquad_i16_bylane_frame_major"
DWORDS, HALVES = "biquad_i16_bylane_lane_major[dword runs]", "biquad_i16_bylane_lane_major[half runs]"
K = {**R.constants("subword_rows.h"), **R.constants("biquad_i16_kernels.h")}  # kFmU, kLmTW, kLmTS

SHAPES = [(1, 1), (1, 1000), (3, 5), (63, 33), (64, 32), (65, 31), (129, 2), (257, 1), (1000, 1000), (4099, 33), (65537, 33)]
NS = [1, 4, 5, 9]  # one pass, a full pass, two passes, three passes


def _ptr(t, off_elems=0):
    return R.ptr(t, 2 * off_elems)


def entry(clamped):
    return "biquad_i16_df1_clamp_bylane" if clamped else "biquad_i16_df1_bylane"


def kernel_for(layout, x_addr, y_addr, xl, yl):
    """the header's rule: FrameMajor has one form; LaneMajor rows of x and y on the 4-byte grid take the dword runs"""
    grid4 = x_addr % 4 == 0 and y_addr % 4 == 0 and xl % 2 == 0 and yl % 2 == 0
    if layout == LM:
        return DWORDS if grid4 else HALVES
    return FRAMES


def run(gpu, coef, frac, layout, st, x, xp=0, yp=0, x_off=0, y_off=0, inplace=False, coef_off=0):
    """one call; coef: [n, 5 | 8, lanes] int16, x: [frames, lanes] int16, st: [4 n, lanes] uint32 -> (y, state after, kernel name).
    x_off / y_off / coef_off: ELEMENTS between the 512-byte grid and the first element.  On top of the checks of R.run: the planes are
    read-only and nothing is written around them."""
    n, clamped = coef.shape[0], coef.shape[1] == 8
    name = entry(clamped)
    cg = Guards(DEV)
    cd = cg.upload("coef", coef.reshape(-1), off=2 * coef_off, readonly=True) if coef.size else None

    def kernel_ok(kernel, x_addr, y_addr, xl, yl):
        if n == 0:
            return True
        if n > 4:  # the last pass of a chain longer than one launch runs in place on y
            x_addr, xl = y_addr, yl
        return kernel == kernel_for(layout, x_addr, y_addr, xl, yl)

    out = R.run(gpu, lambda *a: gpu.fn[name](_ptr(cd), frac, n, *a, None), layout, st, x, x_gap=np.int16(XGAP), y_dtype=torch.int16, kernel_ok=kernel_ok,
                xp=xp, yp=yp, x_off=2 * x_off, y_off=2 * y_off, inplace=inplace, what=(name, n, frac, coef_off))
    cg.check((name, n, frac, layout, x.shape, "coef", coef_off))
    return out


@functools.lru_cache(maxsize=None)
def _cached(n, clamped, lanes, frames, seed, zero_state):
    rng = np.random.default_rng(seed)
    frac, coef = B.random_planes(rng, n, clamped, lanes)
    x = S.inputs(rng, frames, lanes)
    st = np.zeros((4 * n, lanes), np.uint32) if zero_state else S.random_state(rng, n, lanes)
    want_st = st.copy()
    want = B.chain_np(coef, frac, want_st, x)
    for a in (coef, x, st, want, want_st):
        a.setflags(write=False)  # computed once, shared, never changed
    return coef, frac, x, st, want, want_st


def _case(n, clamped, lanes, frames, seed, zero_state=False):
    """every lane its own random sections -> (coef, frac, x, state before, y wanted, state wanted)"""
    return _cached(n, clamped, lanes, frames, seed, zero_state)


@pytest.mark.parametrize("clamped", [False, True])
@pytest.mark.parametrize("n", NS)
def test_parity(gpu, n, clamped):
    seen = set()
    for i, (lanes, frames) in enumerate(SHAPES):
        coef, frac, x, st, want, want_st = _case(n, clamped, lanes, frames, 1000 * n + 100 * clamped + i)
        for layout in (FM, LM):
            y, got_st, kernel = run(gpu, coef, frac, layout, st, x)
            assert np.array_equal(y, want), (n, clamped, layout, lanes, frames, kernel)
            assert np.array_equal(got_st, want_st), (n, clamped, layout, lanes, frames, "state", kernel)
            seen.add(kernel)
    assert seen == {FRAMES, DWORDS, HALVES}  # dense LaneMajor rows: even row lengths are on the 4-byte grid, odd ones are not


@pytest.mark.parametrize("layout", [FM, LM])
@pytest.mark.parametrize("lanes,frames", [(65, 31), (130, 129)])
@pytest.mark.parametrize("n,clamped", [(2, True), (5, False)])
def test_coef_off_the_4_byte_grid(gpu, n, clamped, lanes, frames, layout):
    """coef one element off the 4-byte grid: with 65 lanes the odd planes land ON it, the even ones off; with 130 lanes all are off"""
    coef, frac, x, st, want, want_st = _case(n, clamped, lanes, frames, 40 + n)
    for coef_off in (1, 3):
        y, got_st, kernel = run(gpu, coef, frac, layout, st, x, coef_off=coef_off)
        assert np.array_equal(y, want), (n, clamped, layout, lanes, frames, coef_off, kernel)
        assert np.array_equal(got_st, want_st), (n, clamped, layout, lanes, frames, coef_off, "state", kernel)


@pytest.mark.parametrize("layout,lanes,frames,xp,x_off,kernel", [
    (FM, 128, 8, 0, 0, FRAMES), (FM, 129, 2, 130, 0, FRAMES), (FM, 128, 8, 0, 1, FRAMES), (FM, 65536, 2, 0, 0, FRAMES),  # (four waves per workgroup from 65536 lanes)
    (LM, 64, 32, 0, 0, DWORDS), (LM, 65, 31, 32, 0, DWORDS), (LM, 65, 31, 0, 0, HALVES), (LM, 64, 32, 0, 3, HALVES),
    (LM, 3, 300, 0, 0, DWORDS), (LM, 3, 301, 302, 0, DWORDS), (LM, 3, 301, 0, 0, HALVES),  # whole tiles, then a partial one with an odd tail
])
def test_every_kernel_form(gpu, layout, lanes, frames, xp, x_off, kernel):
    """each form the dispatch can pick, by name, with the alignment that selects it (the rows of tests/test_gpu_biquad_i16.py)"""
    coef, frac, x, st, want, want_st = _case(2, True, lanes, frames, 31)
    y, got_st, got = run(gpu, coef, frac, layout, st, x, xp=xp, yp=xp, x_off=x_off, y_off=x_off)
    assert got == kernel
    assert np.array_equal(y, want) and np.array_equal(got_st, want_st)


@pytest.mark.parametrize("layout", [FM, LM])
def test_alignment_and_pitch(gpu, layout):
    """x and y at every element offset 0..7 from the 16-byte grid, five pitches on either side: the walk of tests/test_gpu_biquad_i16.py
    on one (n, clamped) pair and two shapes — the row addressing is shared and walked in full there; new here is only that the
    coefficient loads sit next to it"""
    n, clamped = 2, True
    for i, (lanes, frames) in enumerate([(5, 9), (65, 31)]):
        coef, frac, x, st, want, want_st = _case(n, clamped, lanes, frames, 50 * n + i)
        ps = R.pitches(_rows(layout, lanes, frames)[1], 2, 32)
        for x_off, xp, y_off, yp in R.combos(ps, x_offs=range(8), y_offs=range(8), both=10, y_step=3):
            y, got_st, kernel = run(gpu, coef, frac, layout, st, x, xp=xp, yp=yp, x_off=x_off, y_off=y_off)
            what = (layout, lanes, frames, x_off, xp, y_off, yp, kernel)
            assert np.array_equal(y, want), what
            assert np.array_equal(got_st, want_st), what


@pytest.mark.parametrize("layout", [FM, LM])
def test_inplace(gpu, layout):
    """y == x, dense and pitched, on and off the 4-byte grid; five sections: the second pass is in place either way"""
    n, clamped = 5, False
    for i, (lanes, frames) in enumerate([(5, 9), (65, 31)]):
        coef, frac, x, st, want, want_st = _case(n, clamped, lanes, frames, 70 * n + i)
        row = _rows(layout, lanes, frames)[1]
        for off in (0, 1, 2):
            for xp in R.pitches(row, 2, 32):
                y, got_st, kernel = run(gpu, coef, frac, layout, st, x, xp=xp, x_off=off, inplace=True)
                what = (layout, lanes, frames, off, xp, kernel)
                assert np.array_equal(y, want), what
                assert np.array_equal(got_st, want_st), what


@pytest.mark.parametrize("layout", [FM, LM])
def test_window_and_tile_edges(gpu, layout):
    """frame counts one below, at and one above the counts the walkers of idsp_amd/csrc/subword_rows.h turn on — FrameMajor the window depth
    U and 2 U, out of place and in place; LaneMajor the tile TS and 2 TS, rows on the dword grid, off it and in place — in 3 lanes and in
    65 (two waves, the last one ragged): one call, and two calls cut at U / TS on one state, equal the spec"""
    n, clamped = 4, True
    U, TS = K["kFmU"], K["kLmTS"]
    counts, cut = (R.around(U, 2 * U), U) if layout == FM else (R.around(TS, 2 * TS), TS)
    forms = [(0, False, FRAMES), (0, True, FRAMES)] if layout == FM else [(0, False, DWORDS), (1, False, HALVES), (0, True, DWORDS)]
    for lanes in (3, 65):
        for i, frames in enumerate(counts):
            coef, frac, x, st, want, want_st = _case(n, clamped, lanes, frames, 300 * n + 10 * lanes + i)
            pitch = 0 if layout == FM else -(-frames // 2) * 2
            for x_off, inplace, kernel in forms:
                def one(s, xs):
                    y, got_st, got = run(gpu, coef, frac, layout, s, xs, xp=pitch, yp=pitch, x_off=x_off, inplace=inplace)
                    assert got == kernel, (layout, lanes, frames, x_off, inplace)
                    return y, got_st

                for y, got_st in R.whole_and_split(one, st, x, cut):
                    assert np.array_equal(y, want), (layout, lanes, frames, x_off, inplace)
                    assert np.array_equal(got_st, want_st), (layout, lanes, frames, x_off, inplace, "state")


@pytest.mark.parametrize("n,clamped", [(2, False), (5, True)])
@pytest.mark.parametrize("lanes,frames,chunks", [(1000, 333, [1, 7, 100, 225]), (65, 1000, [900, 99, 1])])
def test_chunks(gpu, n, clamped, lanes, frames, chunks):
    """consecutive calls on one state equal one call and the spec; the layout may change between the calls of one state"""
    assert sum(chunks) == frames
    coef, frac, x, st, want, want_st = _case(n, clamped, lanes, frames, 77 + n)
    for layouts in ([FM] * len(chunks), [LM] * len(chunks), [(FM, LM)[i % 2] for i in range(len(chunks))]):
        cur, at, parts = st, 0, []
        for m, layout in zip(chunks, layouts):
            y, cur, _ = run(gpu, coef, frac, layout, cur, x[at:at + m])
            parts.append(y)
            at += m
        assert np.array_equal(np.concatenate(parts), want), (n, lanes, frames, layouts)
        assert np.array_equal(cur, want_st), (n, lanes, frames, layouts, "state")


@pytest.mark.parametrize("n,clamped", [(1, True), (5, False)])
def test_new_coefficients_between_chunks(gpu, n, clamped):
    """`set_lane` mid-stream: the planes are replaced between two chunks and the state is carried — equal to the spec run the same way"""
    lanes, cut = 130, 40
    coef, frac, x, st, _, _ = _case(n, clamped, lanes, 100, 90 + n)
    rng = np.random.default_rng(91)
    _, other = B.random_planes(rng, n, clamped, lanes, frac)
    other[:, :, ::3] = coef[:, :, ::3]  # every third lane keeps its configuration
    want_st = st.copy()
    want = np.concatenate([B.chain_np(coef, frac, want_st, x[:cut]), B.chain_np(other, frac, want_st, x[cut:])])
    for first, second in ((FM, LM), (LM, FM)):
        y0, mid, _ = run(gpu, coef, frac, first, st, x[:cut])
        y1, end, _ = run(gpu, other, frac, second, mid, x[cut:])
        assert np.array_equal(np.concatenate([y0, y1]), want), (n, clamped, first, second)
        assert np.array_equal(end, want_st), (n, clamped, first, second, "state")


@pytest.mark.parametrize("layout", [FM, LM])
@pytest.mark.parametrize("clamped", [False, True])
def test_equal_lanes_equal_the_shared_entry(gpu, clamped, layout):
    """every lane holds the same five sections: y and state equal what idsp_biquad_i16_df1 / _df1_clamp write for the same input (device
    against device) and the spec"""
    from tests.test_gpu_biquad_i16 import run as run_shared

    lanes, frames, n = 1000, 129, 5
    rng = np.random.default_rng(60 + clamped)
    frac = 13
    secs = [(s[0], frac, *s[2:]) for s in S.random_sections(rng, n, clamped)]
    coef = np.ascontiguousarray(np.repeat(B.planes([secs], clamped), lanes, axis=2))
    x, st = S.inputs(rng, frames, lanes), S.random_state(rng, n, lanes)
    want_st = st.copy()
    want = S.chain_np(secs, want_st, x)
    ys, st_s, ks = run_shared(gpu, secs, layout, st, x)
    yb, st_b, kb = run(gpu, coef, frac, layout, st, x)
    assert kb == ks.replace("biquad_i16_", "biquad_i16_bylane_")
    assert np.array_equal(yb, ys) and np.array_equal(st_b, st_s)
    assert np.array_equal(yb, want) and np.array_equal(st_b, want_st)


@pytest.mark.parametrize("layout", [FM, LM])
@pytest.mark.parametrize("lanes", [3, 67])
def test_known_answers_in_their_own_lanes(gpu, lanes, layout):
    """the three KNOWN rows of tests/test_gpu_biquad_i16.py, zero state.  Their F differ (13, 0, 14) and a bank has ONE F, so the rows
    cannot share a call as they stand: each row runs in its own lane (row i in lane i) of a call at its own F whose other lanes hold
    random sections — the lane yields the known output and its sign-extended state words, untouched by its neighbours, and the neighbours
    equal the spec.  One call more holds rows 0 and 2 together at F = 13 (the identity is 1 << 13 there)"""
    from tests.test_gpu_biquad_i16 import KNOWN

    rng = np.random.default_rng(7)
    for i, (ba, frac, xs, ys, state) in enumerate(KNOWN):
        _, coef = B.random_planes(rng, 1, False, lanes, frac)
        coef[0, :, i] = ba
        x = S.inputs(rng, len(xs), lanes)
        x[:, i] = xs
        want_st = np.zeros((4, lanes), np.uint32)
        want = B.chain_np(coef, frac, want_st, x)
        y, got_st, kernel = run(gpu, coef, frac, layout, np.zeros((4, lanes), np.uint32), x)
        assert y[:, i].tolist() == ys, (ba, frac, layout, kernel)
        if state is None:
            state = [xs[-1], xs[-2], ys[-1], ys[-2]]
        assert got_st.view(np.int32)[:, i].tolist() == state, (ba, frac, layout, "state", kernel)  # sign-extended
        assert np.array_equal(y, want) and np.array_equal(got_st, want_st)
    (ba0, _, xs0, ys0, _), (_, _, xs2, ys2, _) = KNOWN[0], KNOWN[2]
    m = min(len(xs0), len(xs2))
    _, coef = B.random_planes(rng, 1, False, lanes, 13)
    coef[0, :, 0], coef[0, :, 2] = ba0, [1 << 13, 0, 0, 0, 0]
    x = S.inputs(rng, m, lanes)
    x[:, 0], x[:, 2] = xs0[:m], xs2[:m]
    y, _, _ = run(gpu, coef, 13, layout, np.zeros((4, lanes), np.uint32), x)
    assert y[:, 0].tolist() == ys0[:m] and y[:, 2].tolist() == ys2[:m]


@pytest.mark.parametrize("layout", [FM, LM])
def test_no_sections_copy(gpu, layout):
    """n == 0: y.copy_from_slice(x) (compose.rs:63-65), the state is left alone; with pitches, and in place"""
    rng = np.random.default_rng(4)
    for lanes, frames in ((5, 9), (64, 32), (1000, 33)):
        x = S.inputs(rng, frames, lanes)
        st = S.random_state(rng, 1, lanes)
        row = _rows(layout, lanes, frames)[1]
        for cv in (5, 8):
            for xp, yp, x_off, y_off, inplace in ((0, 0, 0, 0, False), (row + 1, row + 3, 1, 2, False), (row + 3, 0, 0, 0, True)):
                y, got_st, _ = run(gpu, np.zeros((0, cv, lanes), np.int16), 13, layout, st, x, xp=xp, yp=yp, x_off=x_off, y_off=y_off, inplace=inplace)
                assert np.array_equal(y, x) and np.array_equal(got_st, st)


@pytest.mark.parametrize("layout", [FM, LM])
@pytest.mark.parametrize("lanes,frames", [(1000, 64), (999, 65)])
def test_callers_stream(gpu, layout, lanes, frames):
    """the launches (two passes: five sections) are ordered behind the caller's stream and the call does not wait for the device
    (tests/_on_stream.py); the planes arrive on that stream too"""
    from tests import _on_stream as OS

    coef, frac, x, st, want, want_st = _case(5, True, lanes, frames, 5)
    assert st.any() and coef.any()  # a non-zero state and bank: the call is not blind
    name = entry(True)
    g = Guards(DEV)
    c = OS.Call(name, g)
    xd = c.stage("x", np.array(x if layout == FM else x.T), readonly=True)  # (copies: the cached case is read-only)
    cd = c.stage("coef", coef.reshape(-1).copy(), readonly=True)
    yd, sd = c.read(c.out("y", lanes * frames, torch.int16, POISON)), c.read(c.stage("state", st.copy()))
    rc, (yb, sb) = c.run(lambda s: gpu.fn[name](_ptr(cd), frac, 5, _ptr(sd), _ptr(xd), 0, _ptr(yd), 0, lanes, frames, layout, s))
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
    _, coef = B.random_planes(rng, 2, False, lanes, 13)
    name = entry(False)
    g = Guards(DEV)
    # one buffer that holds a pitched x (rows of 16 elements, 32 apart); y is put at places inside and around it
    xbuf = g.upload("x", S.inputs(rng, 8, 32).reshape(-1))
    g.freeze("x")
    yd = g.full("y", lanes * frames, torch.int16, POISON)
    g.freeze("y")
    sd = g.upload("state", S.random_state(rng, 2, lanes), readonly=True)
    cd = g.upload("coef", coef.reshape(-1), readonly=True)
    bq = lambda x, xp, y, yp, layout=FM, cf=_ptr(cd), frac=13, entry=name: gpu.fn[entry](cf, frac, 2, _ptr(sd), x, xp, y, yp, lanes, frames, layout, None)  # noqa: E731
    odd = lambda t, e=0: C.c_void_p(t.data_ptr() + 2 * e + 1)  # noqa: E731
    bad = [
        bq(_ptr(xbuf), 0, _ptr(yd), 0, cf=None),          # NULL coef
        bq(_ptr(xbuf), 0, _ptr(yd), 0, LM, cf=None, entry=entry(True)),
        bq(_ptr(xbuf), 0, _ptr(yd), 0, cf=odd(cd)),       # an odd coef address
        bq(_ptr(xbuf), 0, _ptr(yd), 0, LM, cf=odd(cd, 3)),
        bq(_ptr(xbuf), 0, _ptr(yd), 0, frac=32),          # frac outside 0..31
        bq(_ptr(xbuf), 0, _ptr(yd), 0, LM, frac=-1),
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
    coef, frac, x, st, want, want_st = _case(2, True, lanes, frames, 8)
    x2 = x if layout == FM else np.ascontiguousarray(x.T)
    xd = torch.empty(pitch + row, dtype=torch.int16, device=DEV)
    yd = torch.empty(pitch + row, dtype=torch.int16, device=DEV)
    for r in range(2):
        xd[r * pitch:r * pitch + row] = torch.from_numpy(x2[r].copy()).to(DEV)
        yd[r * pitch:r * pitch + row] = POISON
    sd = torch.from_numpy(st.view(np.int32).copy()).to(DEV)
    cd = torch.from_numpy(coef.copy()).to(DEV)
    assert gpu.fn[entry(True)](_ptr(cd), frac, 2, _ptr(sd), _ptr(xd), pitch, _ptr(yd), pitch, lanes, frames, layout, None) == 0, gpu.err()
    torch.cuda.synchronize()
    assert gpu.last_kernel() == (FRAMES if layout == FM else DWORDS)
    y2 = np.stack([yd[r * pitch:r * pitch + row].cpu().numpy() for r in range(2)])
    assert np.array_equal(y2 if layout == FM else y2.T, want)
    assert np.array_equal(sd.cpu().numpy().view(np.uint32), want_st)
    del xd, yd
    torch.cuda.empty_cache()


def test_python_mirror(gpu):
    """process.BiquadQ16ByLane: block, inplace and LaneMajor views, plain and clamped, set_lane and from_sos, against the spec"""
    from idsp_amd import process as P

    lanes, frames, n = 66, 40, 3
    for clamped in (False, True):
        rng = np.random.default_rng(12 + clamped)
        lane_secs, frac, coef = B.random_bank(rng, n, clamped, lanes)
        x = S.inputs(rng, frames, lanes)
        want_st = np.zeros((4 * n, lanes), np.uint32)
        want = B.chain_np(coef, frac, want_st, x)
        op = P.BiquadQ16ByLane([[P.BiquadQ16(s[0], s[1], *s[2:]) for s in secs] for secs in lane_secs], DEV)
        assert op.clamp == clamped and op.frac == frac and tuple(op.state.shape) == (4 * n, lanes)
        assert op.coef.dtype == torch.int16 and np.array_equal(op.coef.cpu().numpy(), coef)
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
        # set_lane between two blocks: the lane's state is kept
        op.reset()
        other = [(s[0], frac, *s[2:]) for s in S.random_sections(rng, n, clamped)]
        coef2 = coef.copy()
        coef2[:, :, 5] = B.planes([other], clamped)[:, :, 0]
        st2 = np.zeros((4 * n, lanes), np.uint32)
        want2 = np.concatenate([B.chain_np(coef, frac, st2, x[:17]), B.chain_np(coef2, frac, st2, x[17:])])
        y0 = op.block(xd[:17].contiguous(), torch.full((17, lanes), POISON, dtype=torch.int16, device=DEV))
        op.set_lane(5, [P.BiquadQ16(s[0], s[1], *s[2:]) for s in other])
        y1 = op.block(xd[17:].contiguous(), torch.full((frames - 17, lanes), POISON, dtype=torch.int16, device=DEV))
        assert np.array_equal(np.concatenate([y0.cpu().numpy(), y1.cpu().numpy()]), want2)
        assert np.array_equal(op.state.cpu().numpy().view(np.uint32), st2)
        with pytest.raises(ValueError):
            op.set_lane(lanes, [P.BiquadQ16(s[0], s[1], *s[2:]) for s in other])
        with pytest.raises(ValueError):
            op.set_lane(0, [P.BiquadQ16(s[0], (frac + 1) % 32, *s[2:]) for s in other])
    sos = S.sos_rows(np.random.default_rng(2), 3 * 2 * 40)[:3 * 2].reshape(3, 2, 6)
    sos[:, :, 3] = np.where(sos[:, :, 3] == 0.0, 1.0, sos[:, :, 3])
    for clamp in (False, True):
        bank = P.BiquadQ16ByLane.from_sos(sos, 13, clamp=clamp, device=DEV)
        got = bank.coef.cpu().numpy()
        assert got.shape == (2, 8 if clamp else 5, 3) and bank.clamp == clamp and bank.frac == 13
        for l in range(3):
            for k in range(2):
                assert got[k, :5, l].tolist() == S.from_sos(sos[l, k].tolist(), 13)
        if clamp:
            assert (got[:, 5] == 0).all() and (got[:, 6] == -32768).all() and (got[:, 7] == 32767).all()
