"""What the GPU tests of the entries with pitched sub-word rows share (tests/test_gpu_dsm.py: u32 in, i8 out; tests/test_gpu_biquad_i16.py:
i16 in and out): pointers at byte offsets, rows and pitches, ONE guarded call with all its checks, the (offset, pitch) walk, and the
kernels' tile constants read from their headers (idsp_amd/csrc/subword_rows.h and the two kernel headers that stand on it).

Test infrastructure only; not a conftest."""
import ctypes as C
import os
import re

import numpy as np
import torch

from idsp_amd import _abi
from tests._guard import Guards

DEV = "cuda:0"
FM, LM = _abi.FRAME_MAJOR, _abi.LANE_MAJOR
POISON = -77
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "idsp_amd", "csrc")


def constants(header):
    """`constexpr int kName = <number or product of earlier names>;` of a kernel header -> {name: value}"""
    out = {}
    for name, expr in re.findall(r"constexpr\s+int\s+(k\w+)\s*=\s*([^;]+);", open(os.path.join(CSRC, header)).read()):
        value = 1
        for factor in expr.split("*"):
            factor = factor.strip()
            value *= int(factor) if factor.isdigit() else out[factor]
        out[name] = value
    return out


def ptr(t, off_bytes=0):
    return C.c_void_p(t.data_ptr() + off_bytes) if t is not None else None


def rows_of(layout, lanes, frames):
    """(rows, row): FrameMajor rows are frames of `lanes` elements, LaneMajor rows are lanes of `frames` elements"""
    return (frames, lanes) if layout == FM else (lanes, frames)


def pitched(a2d, pitch, gap):
    """[rows, row] -> flat buffer of (rows - 1) * pitch + row elements, `gap` between the rows"""
    rows, row = a2d.shape
    buf = np.full((rows - 1) * pitch + row, gap, a2d.dtype)
    for r in range(rows):
        buf[r * pitch:r * pitch + row] = a2d[r]
    return buf


def pitches(row, small, big):
    """dense, two odd gaps, the row rounded up to `small` and to `big` elements"""
    return [0, row + 1, row + 3, -(-row // small) * small, -(-row // big) * big]


def combos(ps, x_offs, y_offs, both, y_step):
    """(x_off, xp, y_off, yp): the y side and the x side each walk all their (offset, pitch) pairs against a dense aligned partner, then
    `both` calls walk the two sides together (y moves through its offsets `y_step` at a time)"""
    out = [(0, 0, y_off, yp) for y_off in y_offs for yp in ps]
    out += [(x_off, xp, 0, 0) for x_off in x_offs for xp in ps]
    out += [(x_offs[i % len(x_offs)], ps[(i + 1) % 5], y_offs[(y_step * i + 1) % len(y_offs)], ps[(2 * i + 3) % 5]) for i in range(both)]
    return out


def run(gpu, call, layout, st, x, *, x_gap, y_dtype, kernel_ok, xp=0, yp=0, x_off=0, y_off=0, inplace=False, null_state=False, what=()):
    """One call.  x: [frames, lanes], st: [words, lanes] uint32 -> (y [frames, lanes], state after, kernel name).
    `call(state, x, xp, y, yp, lanes, frames, layout)` makes the entry call on ctypes pointers and returns its status; xp / yp: pitches in
    elements (0: dense); x_off / y_off: BYTES between the 512-byte grid and the first sample; inplace: y is x (its pitch and offset too);
    `kernel_ok(kernel, x_addr, y_addr, xl, yl)`: whether idsp_last_kernel() is what these addresses and pitches select.
    Checks the status, the guard bands of tests/_guard.py, the read-only x (unless in place), the kernel, and that the gap elements of
    a pitched y kept their poison (in place: what the gaps of x held)."""
    frames, lanes = x.shape
    rows, row = rows_of(layout, lanes, frames)
    if inplace:
        yp, y_off = xp, x_off
    xl, yl = xp or row, yp or row
    g = Guards(DEV)
    x2 = x if layout == FM else np.ascontiguousarray(x.T)
    xd = g.upload("x", pitched(x2, xl, x_gap), off=x_off, readonly=not inplace)
    yd = xd if inplace else g.full("y", (rows - 1) * yl + row, y_dtype, POISON, off=y_off)
    sd = None if null_state else g.upload("state", st)
    rc = call(ptr(sd), ptr(xd), xp, ptr(yd), yp, lanes, frames, layout)
    torch.cuda.synchronize()
    kernel = gpu.last_kernel()
    what = (*what, layout, lanes, frames, xp, yp, x_off, y_off, inplace, kernel)
    assert rc == 0, (what, gpu.err())
    g.check(what)
    assert kernel_ok(kernel, xd.data_ptr(), yd.data_ptr(), xl, yl), what
    yb = yd.cpu().numpy()
    idx = (np.arange(rows)[:, None] * yl + np.arange(row)[None, :]).reshape(-1)
    gap = np.ones(yb.size, bool)
    gap[idx] = False
    assert (yb[gap] == (x_gap if inplace else POISON)).all(), ("a gap element of y was written", what)
    y2 = yb[idx].reshape(rows, row)
    y = y2 if layout == FM else np.ascontiguousarray(y2.T)
    return y, (st.copy() if null_state else sd.cpu().numpy().view(np.uint32).reshape(st.shape)), kernel


def around(*marks):
    """the frame counts one below, at and one above each mark (a window depth, a tile width or a multiple of one)"""
    return [m + d for m in marks for d in (-1, 0, 1)]


def whole_and_split(one, st, x, cut):
    """`one(st, x) -> (y, state after)` on all frames of x, and again as two calls cut at frame `cut` with the state carried (the whole
    call again where no frame lies behind the cut) -> ((y, state) whole, (y, state) split)"""
    whole = one(st, x)
    if cut >= x.shape[0]:
        return whole, whole
    y0, mid = one(st, x[:cut])
    y1, end = one(mid, x[cut:])
    return whole, (np.concatenate([y0, y1]), end)
