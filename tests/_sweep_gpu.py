"""Calling idsp_sweep_i32 through the C ABI for the sweep suites: buffers between guard bands
(tests/_guard.py), outputs poisoned, one state across the chunks of a call, the specification's result cached per case.

Test infrastructure only."""
import functools

import numpy as np

from tests import _sweep_spec as S
from tests._stream_proc_cases import DEV, POISON, _ptr, from_layout, run_form, to_layout  # noqa: F401  (the sweep suites use them through this module)

KERNELS = {}  # (entry, layout, lanes, frames) -> idsp_last_kernel()


def run(gpu, st, frames, layout, chunks=None):
    """The generator on state st [7, lanes] uint32 (updated).  chunks: frame counts of consecutive calls on one state.
    Returns [frames, lanes, 2] int32.  (The runner: tests/_stream_proc_cases.py.)"""
    lanes = st.shape[1]
    return run_form(gpu, "sweep", None, st, None, frames, layout, chunks=chunks, record=lambda n, k: KERNELS.__setitem__(("sweep_i32", layout, lanes, n), k))


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
