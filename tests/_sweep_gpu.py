"""Calling idsp_sweep_i32 through the C ABI for the sweep suites: buffers between guard bands
(tests/_guard.py), outputs poisoned, one state across the chunks of a call, the specification's result cached per case.

Test infrastructure only."""
import ctypes as C
import functools

import numpy as np
import torch

from tests import _harness as H
from tests import _sweep_spec as S
from tests._guard import Guards

DEV = "cuda:0"
POISON = -77
KERNELS = {}  # (entry, layout, lanes, frames) -> idsp_last_kernel()


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def to_layout(a, layout):
    """[frames, lanes(, w)] -> the flat array of `layout`"""
    return np.ascontiguousarray(a if layout == H.FM else np.swapaxes(a, 0, 1))


def from_layout(flat, layout, frames, lanes, width):
    a = flat.reshape((frames, lanes, width) if layout == H.FM else (lanes, frames, width))
    return np.ascontiguousarray(a if layout == H.FM else np.swapaxes(a, 0, 1))


def run(gpu, st, frames, layout, chunks=None):
    """The generator on state st [7, lanes] uint32 (updated).  chunks: frame counts of consecutive calls on one state.
    Returns [frames, lanes, 2] int32."""
    lanes = st.shape[1]
    entry = "sweep_i32"
    gs = Guards(DEV)
    sd = gs.upload("state", st)
    outs, f0 = [], 0
    for n in chunks or [frames]:
        g = Guards(DEV)
        yd = g.full("y", lanes * n * 2, torch.int32, POISON)
        rc = gpu.fn[entry](_ptr(sd), _ptr(yd), lanes, n, layout, None)
        assert rc == 0, gpu.err()
        torch.cuda.synchronize()
        k = KERNELS[(entry, layout, lanes, n)] = gpu.last_kernel()
        g.check((entry, layout, lanes, n, k))
        gs.check((entry, layout, lanes, n, k))
        outs.append(from_layout(yd.cpu().numpy(), layout, n, lanes, 2))
        f0 += n
    assert f0 == frames
    st[...] = sd.cpu().numpy().view(np.uint32)
    return np.concatenate(outs)


@functools.lru_cache(maxsize=None)
def osc_case(lanes, frames, boundary=0, variant=0):
    """-> (state before, state after, output) of the specification; shared, never modified"""
    rng = np.random.default_rng(1000 * variant + 7 * frames + lanes % 997 + boundary)
    st = S.population(rng, lanes, frames, boundary=boundary, variant=variant)
    after = st.copy()
    out = S.osc_np(after, frames)
    for a in (st, after, out):
        a.setflags(write=False)
    return st, after, out


def assert_mixed(cases, frames):
    """The lanes of `cases` [(state before, state after), ..] together hold one that ends strictly inside the call, one that had
    ended before it and one that never ends.  A one-frame call has no inside: there a lane must emit its last sample in it."""
    inside = before = never = False
    for st, after in cases:
        if frames == 1:
            i = ((S.emitted_of(after) - S.emitted_of(st)) == 1) & S.ended_np(after)
            _, b, n = S.classify(st, after, frames)
        else:
            i, b, n = S.classify(st, after, frames)
        inside, before, never = inside or i.any(), before or b.any(), never or n.any()
    assert inside and before and never, (inside, before, never)


def variants_for(lanes):
    """populations per case: three (each lane kind in turn at lane 0) where one population cannot hold all three kinds"""
    return range(3) if lanes < 3 else range(1)
