"""Two interchangeable back ends with numpy in / numpy out so every known-answer
and parity case is written once: `OracleBackend` (CPU restatement, checker) and
`GpuBackend` (the HIP engine through its C ABI, device buffers via torch).

Test infrastructure only."""
from __future__ import annotations

import ctypes as C

import numpy as np

from tests import _harness as H


class OracleBackend:
    name = "oracle"

    def __init__(self):
        self.o = H.oracle()

    def stream(self, op, cfg, n, state, x, lanes, frames, layout, inplace=False):
        x = np.ascontiguousarray(x)
        y = x if inplace else np.empty_like(x)
        rc = self.o.stream(op, cfg, n, state, x, y, lanes, frames, layout)
        return rc, y

    def bylane(self, op, coef, frac, n, state, x, lanes, frames, layout, inplace=False):
        """`op` without the `_bylane` suffix; coef = [n, CV, lanes] planes; frac None for floats."""
        x = np.ascontiguousarray(x)
        coef = np.ascontiguousarray(coef)
        y = x if inplace else np.empty_like(x)
        args = (H._ptr(coef),) + (() if frac is None else (frac,)) + (n, H._ptr(state), H._ptr(x), H._ptr(y), lanes, frames, layout)
        return self.o.fn[op + "_bylane"](*args), y

    def cfgcall(self, op, cfg, state, x, y_shape, y_dtype, lanes, frames, layout):
        x = np.ascontiguousarray(x) if x is not None else None
        y = np.empty(y_shape, dtype=y_dtype)
        rc = self.o.cfgcall(op, cfg, state, x, y, lanes, frames, layout)
        return rc, y

    def cossin(self, phases):
        phases = np.ascontiguousarray(phases, dtype=np.int32)
        out = np.empty((phases.size, 2), dtype=np.int32)
        rc = self.o.fn["cossin_i32"](H._ptr(phases), H._ptr(out), phases.size)
        return rc, out

    def atan2(self, xy):
        xy = np.ascontiguousarray(xy, dtype=np.int32)
        out = np.empty(xy.size // 2, dtype=np.int32)
        rc = self.o.fn["atan2_i32"](H._ptr(xy), H._ptr(out), out.size)
        return rc, out

    def dds(self, state, lanes, frames, layout):
        out = np.empty(lanes * frames * 2, dtype=np.int32)
        rc = self.o.fn["dds_i32"](H._ptr(state), H._ptr(out), lanes, frames, layout)
        return rc, out

    def helper(self, name, *args):
        return self.o.fn[name](*args)


class GpuBackend:
    """Every device buffer of a call sits between guard bands (tests/_guard.py).  After the call and the synchronisation the bands
    of all its buffers are compared with the sentinel, and an input the call must not write (everything except an in-place `x`,
    the state and `y`) with what was uploaded."""
    name = "hip"

    def __init__(self, on_stream=None):
        """on_stream: True / False, or None for what IDSP_TEST_STREAM says"""
        import torch

        self.torch = torch
        self.on_stream = on_stream
        self.last_call = None  # the tests/_on_stream.py Call of the most recent call, when it ran under the arrangement
        self.e = H.engine()
        self.dev = torch.device("cuda:0")
        self.g = None  # the guarded buffers of the call in flight

    # IDSP_TEST_MISALIGN=1: every device buffer starts one element (4 or 8 bytes) into its allocation, so the whole parity
    # suite can be replayed on buffers without 16-byte alignment (tests/test_gpu_misaligned.py does that in a subprocess)
    def _off(self, itemsize):
        import os

        return int(itemsize) if os.environ.get("IDSP_TEST_MISALIGN") else 0

    def _begin(self):
        from tests._guard import Guards

        self.g = Guards(self.dev)

    def _alloc(self, n, dtype, role="y"):
        return self.g.empty(role, int(n), dtype, self._off(self.torch.empty(0, dtype=dtype).element_size()))

    def _up(self, a, role, readonly=False):
        if a is None:
            return None
        a = np.ascontiguousarray(a)
        return self.g.upload(role, a, self._off(a.dtype.itemsize), readonly)

    def _down(self, t, like_dtype):
        a = t.cpu().numpy()
        return a.view(like_dtype) if a.dtype != like_dtype else a

    def _end(self, op):
        self.torch.cuda.synchronize()
        self.g.check(op)

    # IDSP_TEST_STREAM=1: every call below runs under the arrangement of tests/_on_stream.py -- decoys in the buffers, the true inputs
    # copied in on a stream S behind a device-side delay, the call with stream = S, the results read back on S
    # (tests/test_gpu_callers_stream.py replays the parity suites that way in a subprocess)
    def _call(self, entry):
        from tests import _on_stream as OS

        if not (OS.enabled() if self.on_stream is None else self.on_stream):
            return None
        self._begin()
        self.last_call = OS.Call(entry, self.g)
        return self.last_call

    def _stage(self, c, a, role, readonly=False):
        if a is None:
            return None
        a = np.ascontiguousarray(a)
        return c.stage(role, a, self._off(a.dtype.itemsize), readonly)

    def _out(self, c, n, dtype, fill):
        return c.out("y", n, dtype, fill, self._off(self.torch.empty(0, dtype=dtype).element_size()))

    def stream(self, op, cfg, n, state, x, lanes, frames, layout, inplace=False):
        import os

        torch = self.torch
        inplace = inplace or bool(os.environ.get("IDSP_TEST_INPLACE"))  # `Inplace::inplace` for every stream call
        c = self._call(op)
        if c is not None:
            xs = self._stage(c, x, "x", readonly=not inplace)
            ys = xs if inplace else self._out(c, xs.numel(), xs.dtype, -77 if xs.dtype == torch.int32 else float("nan")).reshape(xs.shape)
            ss = self._stage(c, state, "state")
            c.read(ys)
            if ss is not None:
                c.read(ss)
            rc, got = c.run(lambda s: self.e.stream(op, cfg, n, ss, xs, ys, lanes, frames, layout, s))
            self._end(op)
            if ss is not None:
                state[...] = got[1].view(np.uint32).reshape(state.shape)
            return rc, got[0].view(x.dtype).reshape(np.shape(x))
        self._begin()
        xs = self._up(x, "x", readonly=not inplace)
        ys = xs if inplace else self._alloc(xs.numel(), xs.dtype).reshape(xs.shape)
        if not inplace:
            ys.fill_(-77 if xs.dtype == torch.int32 else float("nan"))  # poison: every element must be written
        ss = self._up(state, "state")
        rc = self.e.stream(op, cfg, n, ss, xs, ys, lanes, frames, layout)
        self._end(op)
        if ss is not None:
            state[...] = self._down(ss, np.uint32).reshape(state.shape)
        return rc, self._down(ys, x.dtype).reshape(np.shape(x))

    def bylane(self, op, coef, frac, n, state, x, lanes, frames, layout, inplace=False):
        import os

        torch = self.torch
        inplace = inplace or bool(os.environ.get("IDSP_TEST_INPLACE"))
        c = self._call(op + "_bylane")
        if c is not None:
            xs, cs, ss = self._stage(c, x, "x", readonly=not inplace), self._stage(c, coef, "coef", readonly=True), self._stage(c, state, "state")
            ys = xs if inplace else self._out(c, xs.numel(), xs.dtype, -77 if xs.dtype == torch.int32 else float("nan")).reshape(xs.shape)
            c.read(ys)
            if ss is not None:
                c.read(ss)
            head = (H._ptr(cs),) + (() if frac is None else (frac,)) + (n, H._ptr(ss), H._ptr(xs), H._ptr(ys), lanes, frames, layout)
            rc, got = c.run(lambda s: self.e.fn[op + "_bylane"](*head, s))
            self._end(op + "_bylane")  # the coefficient planes are read-only there
            if ss is not None:
                state[...] = got[1].view(np.uint32).reshape(state.shape)
            return rc, got[0].view(x.dtype).reshape(np.shape(x))
        self._begin()
        xs, cs, ss = self._up(x, "x", readonly=not inplace), self._up(coef, "coef", readonly=True), self._up(state, "state")
        ys = xs if inplace else self._alloc(xs.numel(), xs.dtype).reshape(xs.shape)
        if not inplace:
            ys.fill_(-77 if xs.dtype == torch.int32 else float("nan"))
        args = (H._ptr(cs),) + (() if frac is None else (frac,)) + (n, H._ptr(ss), H._ptr(xs), H._ptr(ys), lanes, frames, layout, None)
        rc = self.e.fn[op + "_bylane"](*args)
        self._end(op + "_bylane")
        if ss is not None:
            state[...] = self._down(ss, np.uint32).reshape(state.shape)
        assert np.array_equal(self._down(cs, coef.dtype).reshape(coef.shape), coef)  # coefficients are read-only
        return rc, self._down(ys, x.dtype).reshape(np.shape(x))

    def cfgcall(self, op, cfg, state, x, y_shape, y_dtype, lanes, frames, layout):
        torch = self.torch
        tdt = {np.dtype(np.float32): torch.float32, np.dtype(np.int64): torch.int64}.get(np.dtype(y_dtype), torch.int32)
        c = self._call(op)
        if c is not None:
            xs = self._stage(c, x, "x", readonly=True)
            ys = self._out(c, int(np.prod(y_shape)), tdt, float("nan") if tdt == torch.float32 else -77)
            ss = self._stage(c, state, "state")
            c.read(ys), c.read(ss)
            rc, got = c.run(lambda s: self.e.cfgcall(op, cfg, ss, xs, ys, lanes, frames, layout, s))
            self._end(op)
            state[...] = got[1].view(np.uint32).reshape(state.shape)
            return rc, got[0].view(y_dtype).reshape(y_shape)
        self._begin()
        xs = self._up(x, "x", readonly=True)
        ys = self._alloc(int(np.prod(y_shape)), tdt)
        ys.fill_(float("nan") if tdt == torch.float32 else -77)  # poison: every element must be written
        ss = self._up(state, "state")
        rc = self.e.cfgcall(op, cfg, ss, xs, ys, lanes, frames, layout)
        self._end(op)
        state[...] = self._down(ss, np.uint32).reshape(state.shape)
        return rc, self._down(ys, y_dtype).reshape(y_shape)

    def cossin(self, phases):
        torch = self.torch
        c = self._call("cossin_i32")
        if c is not None:
            ps = self._stage(c, np.ascontiguousarray(phases, dtype=np.int32), "x", readonly=True)
            out = c.read(self._out(c, ps.numel() * 2, torch.int32, -77))
            rc, got = c.run(lambda s: self.e.fn["cossin_i32"](H._ptr(ps), H._ptr(out), ps.numel(), s))
            self._end("cossin_i32")
            return rc, got[0].view(np.int32).reshape(-1, 2)
        self._begin()
        ps = self._up(np.ascontiguousarray(phases, dtype=np.int32), "x", readonly=True)
        out = self._alloc(ps.numel() * 2, torch.int32)
        rc = self.e.fn["cossin_i32"](H._ptr(ps), H._ptr(out), ps.numel(), None)
        self._end("cossin_i32")
        return rc, out.cpu().numpy().reshape(-1, 2)

    def atan2(self, xy):
        torch = self.torch
        c = self._call("atan2_i32")
        if c is not None:
            xs = self._stage(c, np.ascontiguousarray(xy, dtype=np.int32), "x", readonly=True)
            out = c.read(self._out(c, xs.numel() // 2, torch.int32, -77))
            rc, got = c.run(lambda s: self.e.fn["atan2_i32"](H._ptr(xs), H._ptr(out), out.numel(), s))
            self._end("atan2_i32")
            return rc, got[0].view(np.int32)
        self._begin()
        xs = self._up(np.ascontiguousarray(xy, dtype=np.int32), "x", readonly=True)
        out = self._alloc(xs.numel() // 2, torch.int32)
        rc = self.e.fn["atan2_i32"](H._ptr(xs), H._ptr(out), out.numel(), None)
        self._end("atan2_i32")
        return rc, out.cpu().numpy()

    def dds(self, state, lanes, frames, layout):
        torch = self.torch
        c = self._call("dds_i32")
        if c is not None:
            ss = self._stage(c, state, "state")
            out = c.read(self._out(c, lanes * frames * 2, torch.int32, -77))
            c.read(ss)
            rc, got = c.run(lambda s: self.e.fn["dds_i32"](H._ptr(ss), H._ptr(out), lanes, frames, layout, s))
            self._end("dds_i32")
            state[...] = got[1].view(np.uint32).reshape(state.shape)
            return rc, got[0].view(np.int32)
        self._begin()
        ss = self._up(state, "state")
        out = self._alloc(lanes * frames * 2, torch.int32)
        rc = self.e.fn["dds_i32"](H._ptr(ss), H._ptr(out), lanes, frames, layout, None)
        self._end("dds_i32")
        state[...] = self._down(ss, np.uint32).reshape(state.shape)
        return rc, out.cpu().numpy()

    def helper(self, name, *args):
        return self.e.fn[name](*args)
