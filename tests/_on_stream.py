"""One engine call on a stream of the caller's, arranged so that a launch that went anywhere else LOSES.

include/idsp_hip.h: "`stream` is a `hipStream_t` ... Calls are asynchronous on that stream."  A test that uploads, launches and reads
back on an idle stream cannot hold an entry to that: a launch sent to the null stream usually still finds its inputs in place.  Here,
for one call:

  * every device buffer exists beforehand (guard bands of tests/_guard.py kept).  The inputs -- x, lo, accu, coefficient planes, the
    state -- hold a DECOY (zeros, which is also the reference's default state; a padded buffer gives its own decoy), the outputs a
    poison; the TRUE inputs wait in pinned host memory.  One device-wide synchronisation settles all that.
  * on the stream S (non-blocking, one per `Arrangement`; `shared()` is the process's one) in this order: a device-side DELAY, an
    event, the copies of the true inputs into the buffers, the engine call with `stream = S`, asynchronous copies of the outputs into
    pinned host buffers.  Then `S.synchronize()`, and the results are taken from the pinned buffers before anything device-wide runs.
  * ARMED: the event directly behind the delay has not completed when the engine call has returned.  Whatever the call issued to
    another stream, or did not order behind S, was therefore issued while the true inputs had not arrived: it computes from the decoy.
    An entry that blocks the host (a hidden synchronisation, a blocking copy) can never be armed.
    (The interpreter's garbage collector is kept off from the delay to the call's return: a collection pause is not the entry's.)
  * an unarmed call is not a pass: the whole arrangement is repeated with the delay doubled (decoy, poison, true state again), three
    attempts; the usual reason is the first launch of a kernel loading its code object.  After the third, `NotArmed` names the entry.
  * a call whose true inputs equal the decoy (no input and a zero state, zero lanes or frames) cannot tell the streams apart: BLIND,
    counted in the tally.

What this proves when armed: every launch of the call is ordered behind the caller's stream, and the call does not wait for the
device.  What it cannot: work a call forks to a second stream BEHIND the caller's (lane_stream.h, "second stream") starts after the
inputs either way; a missing join back still has to lose a real race against the read-back.

DELAY_US: the host time from the start of the input copies to the return of the engine call was measured on an MI355X over the 5883
calls of tests/test_gpu_parity.py (profiles/NOTES.md, "The caller's stream"): median 20.1 us; the delay starts at four times that.

The tally (calls, armed at first try, retried, blind, per entry the calls / armed / blind counts, the median, 99th percentile and
maximum of that host time over the armed attempts) is written as JSON to the file IDSP_TEST_STREAM_TALLY names when the process exits.

Test infrastructure only."""
from __future__ import annotations

import atexit
import gc
import json
import os
import time

import numpy as np

DELAY_US = 80  # microseconds: the measured median of 20.1 us (see above) x 4
ATTEMPTS = 3
TALLY_ENV = "IDSP_TEST_STREAM_TALLY"


class NotArmed(AssertionError):
    pass


def enabled():
    """IDSP_TEST_STREAM=1: tests/_backends.py and the `_pitch` runners send their calls through the arrangement"""
    return bool(os.environ.get("IDSP_TEST_STREAM"))


# ------------------------------------------------------------------------------------------------------------------ tally
TALLY = {"calls": 0, "armed_first": 0, "retried": 0, "blind": 0, "entries": {}, "host_us": []}


def tally():
    t = {k: v for k, v in TALLY.items() if k != "host_us"}
    h = TALLY["host_us"]
    t["median_host_us"], t["p99_host_us"], t["max_host_us"] = (float(np.median(h)), float(np.percentile(h, 99)), float(max(h))) if h else (None,) * 3
    return t


def _count(entry, first, blind, host_us):
    e = TALLY["entries"].setdefault(entry, {"calls": 0, "armed": 0, "blind": 0})
    TALLY["calls"] += 1
    e["calls"] += 1
    e["armed"] += 1  # an unarmed call raises instead
    TALLY["armed_first" if first else "retried"] += 1
    if blind:
        TALLY["blind"] += 1
        e["blind"] += 1
    TALLY["host_us"].append(host_us)


@atexit.register
def _write_tally():
    path = os.environ.get(TALLY_ENV)
    if path and TALLY["calls"]:
        with open(path, "w") as f:
            json.dump(tally(), f)


# ------------------------------------------------------------------------------------------------------------------ delay
_DELAY = {}


def _calibrate(torch):
    """device cycles of `torch.cuda._sleep` per microsecond, or the microseconds of one fill of a 64 MiB tensor where torch has no _sleep"""
    if _DELAY:
        return
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    if hasattr(torch.cuda, "_sleep"):
        work, n = (lambda: torch.cuda._sleep(1_000_000)), 1_000_000
    else:
        _DELAY["buf"] = torch.zeros(1 << 24, dtype=torch.int32, device="cuda:0")
        work, n = (lambda: _DELAY["buf"].add_(1)), 1
    work()  # the code object
    torch.cuda.synchronize()
    e0.record()
    work()
    e1.record()
    e1.synchronize()
    us = max(e0.elapsed_time(e1) * 1e3, 1e-3)
    _DELAY["sleep"] = hasattr(torch.cuda, "_sleep")
    _DELAY["per_us"] = n / us if _DELAY["sleep"] else us


def _delay(torch, us):
    """on the current stream"""
    if _DELAY["sleep"]:
        torch.cuda._sleep(max(1, int(us * _DELAY["per_us"])))
    else:
        for _ in range(max(1, int(np.ceil(us / _DELAY["per_us"])))):
            _DELAY["buf"].add_(1)


# ----------------------------------------------------------------------------------------------------------- pinned memory
class _Arena:
    """Pinned host bytes handed out in 64-byte aligned pieces and taken back all at once (pinning per call costs milliseconds)."""

    def __init__(self, torch):
        self.torch, self.chunks, self.used = torch, [], 0

    def reset(self):
        if len(self.chunks) > 1:  # one chunk of the whole size next time
            n = sum(c.numel() for c in self.chunks)
            self.chunks = [self.torch.empty(n, dtype=self.torch.uint8, pin_memory=True)]
        self.used = 0

    def take(self, nbytes):
        at = (self.used + 63) & ~63
        if not self.chunks or at + nbytes > self.chunks[-1].numel():
            self.chunks.append(self.torch.empty(max(2 * (nbytes + 64), 1 << 20), dtype=self.torch.uint8, pin_memory=True))
            at = 0
        self.used = at + nbytes
        return self.chunks[-1][at:at + nbytes]


def _bytes(t):
    """the bytes of a contiguous device tensor"""
    import torch

    assert t.is_contiguous()
    return t.reshape(-1).view(torch.uint8)


def _np_bytes(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


class Arrangement:
    """The stream S with its pinned arenas.  `priority`: of S (torch: lower is higher)."""

    def __init__(self, priority=0):
        import torch

        self.torch = torch
        _calibrate(torch)
        self.S = torch.cuda.Stream(priority=priority)
        self.up, self.down = _Arena(torch), _Arena(torch)

    @property
    def ptr(self):
        import ctypes as C

        return C.c_void_p(self.S.cuda_stream)


_SHARED = []


def shared():
    """the one stream S of this process, created at first use"""
    if not _SHARED:
        _SHARED.append(Arrangement())
    return _SHARED[0]


# ------------------------------------------------------------------------------------------------------------------- a call
class Call:
    """One engine call under the arrangement.  Build: `stage` / `load` the inputs, `out` / `poison` the outputs, `read` what comes back;
    then `run(launch)` with `launch(stream pointer) -> rc`.  The phases (`prepare`, `open`, `launch`, `close`, `collect`) are public for a
    test that interleaves two callers."""

    def __init__(self, entry, guards=None, arr=None, delay_us=None):
        import torch

        self.torch, self.entry, self.g = torch, entry, guards
        self.arr = arr or shared()
        self.delay_us = DELAY_US if delay_us is None else delay_us
        self.loads, self.poisons, self.reads = [], [], []
        self.armed = self.first = None
        self.host_us = 0.0

    # -- building
    def load(self, t, true, decoy=None):
        """device tensor `t` (contiguous) gets `true` (numpy, same bytes) on S; until then it holds `decoy` (numpy) or zeros"""
        tb, db = _np_bytes(true), None if decoy is None else _np_bytes(decoy)
        assert tb.size == _bytes(t).numel() and (db is None or db.size == tb.size), (self.entry, "size of a staged input")
        self.loads.append((t, tb, db))

    def stage(self, role, a, off=0, readonly=False, decoy=None):
        """a guarded buffer shaped like `a` (uint32 travels as int32) that gets `a` on S; readonly: Guards.check holds it to `a`"""
        torch = self.torch
        a = np.ascontiguousarray(a)
        a = a.view(np.int32) if a.dtype == np.uint32 else a
        t = self.g.empty(role, a.size, torch.from_numpy(a[:0].reshape(-1)).dtype, off)
        self.load(t, a, decoy)
        if readonly:  # what the buffer holds once the true input has arrived, bands included
            b = self.g.bufs[-1]
            b.frozen = b.raw.clone()
            b.frozen[b.lo:b.hi] = torch.from_numpy(_np_bytes(a).copy()).to(b.raw.device)
        return t.reshape(a.shape)

    def out(self, role, nelem, dtype, fill, off=0):
        t = self.g.empty(role, int(nelem), dtype, off)
        self.poison(t, fill)
        return t

    def poison(self, t, fill):
        self.poisons.append((t, fill))

    def read(self, t):
        self.reads.append(t)
        return t

    @property
    def blind(self):
        return all(tb.size == 0 or (not tb.any() if db is None else np.array_equal(tb, db)) for _, tb, db in self.loads)

    # -- phases
    def prepare(self):
        """decoys and poison, on the current stream; the caller synchronises the device afterwards"""
        torch = self.torch
        self.arr.up.reset(), self.arr.down.reset()
        self._pinned = []
        for t, tb, db in self.loads:
            if db is None:
                _bytes(t).zero_()
            else:
                _bytes(t).copy_(torch.from_numpy(db.copy()))
            h = self.arr.up.take(tb.size)
            h.numpy()[...] = tb
            self._pinned.append(h)
        for t, fill in self.poisons:
            t.fill_(fill)
        self._hosts = [self.arr.down.take(_bytes(t).numel()) for t in self.reads]

    def open(self, delay_us):
        """the delay, the event behind it and the copies of the true inputs, on S"""
        torch = self.torch
        self.event = torch.cuda.Event()
        with torch.cuda.stream(self.arr.S):
            _delay(torch, delay_us)
            self.event.record()
            self._t0 = time.perf_counter()
            for (t, tb, _), h in zip(self.loads, self._pinned):
                if tb.size:
                    _bytes(t).copy_(h, non_blocking=True)

    def launch(self, fn, null_stream=False):
        """`null_stream`: the control -- the engine is handed NULL although everything else sits on S"""
        rc = fn(None if null_stream else self.arr.ptr)
        self.host_us = (time.perf_counter() - self._t0) * 1e6
        self.armed = not self.event.query()
        return rc

    def close(self):
        """asynchronous copies of the results on S, directly behind the call"""
        with self.torch.cuda.stream(self.arr.S):
            for t, h in zip(self.reads, self._hosts):
                if h.numel():
                    h.copy_(_bytes(t), non_blocking=True)

    def collect(self):
        """waits for S alone; the results as numpy arrays (uint8, the caller views them)"""
        self.arr.S.synchronize()
        return [h.numpy().copy() for h in self._hosts]

    # -- the whole arrangement
    def run(self, launch, null_stream=False):
        """-> (rc, [bytes of each `read` tensor]); raises NotArmed when three attempts did not arm"""
        torch = self.torch
        for attempt in range(ATTEMPTS):
            self.prepare()
            torch.cuda.synchronize()
            collecting = gc.isenabled()
            gc.disable()  # no collection pause of the interpreter between the delay and the call's return
            try:
                self.open(self.delay_us * (1 << attempt))
                rc = self.launch(launch, null_stream)
            finally:
                if collecting:
                    gc.enable()
            self.close()
            got = self.collect()
            if self.armed:
                self.first = attempt == 0
                _count(self.entry, self.first, self.blind, self.host_us)
                return rc, got
        raise NotArmed(f"{self.entry}: the call blocked the host: after {ATTEMPTS} attempts, the last with a device-side delay of "
                       f"{self.delay_us * (1 << (ATTEMPTS - 1))} us in front of it on the caller's stream, the delay had always ended when the "
                       f"call returned ({self.host_us:.0f} us after the copies began); nothing was compared")


def pitch_call(eng, entry, cfg, n, st0, xfull, xdecoy, x_off, xpitch, ypitch, ysize, lanes, frames, layout, inplace, fill, guards=None, arr=None):
    """`<entry>` (a `_pitch` twin) on padded buffers: `xfull` is the whole x buffer (padding = the caller's sentinel, numpy), `xdecoy` the
    same with zeros where the samples are; `x_off` elements into both buffers the call starts.  -> (rc, y buffer, state, Call)"""
    import ctypes as C

    import torch

    from tests._guard import Guards

    g = guards or Guards("cuda:0")
    c = Call(entry, g, arr)
    xb = c.stage("x", xfull, readonly=not inplace, decoy=xdecoy)
    yb = xb if inplace else c.out("y", ysize, xb.dtype, fill)
    sg = c.stage("state", st0)
    esz = xb.element_size()
    c.read(yb), c.read(sg)
    rc, (yh, sh) = c.run(lambda s: eng.fn[entry](C.cast(cfg, C.c_void_p), n, C.c_void_p(sg.data_ptr()), C.c_void_p(xb.data_ptr() + x_off * esz), xpitch,
                                                 C.c_void_p(yb.data_ptr() + x_off * esz), ypitch, lanes, frames, layout, s))
    torch.cuda.synchronize()
    g.check((entry, lanes, frames, xpitch, inplace))
    return rc, yh.view(np.asarray(xfull).dtype), sh.view(np.uint32).reshape(np.shape(st0)), c
