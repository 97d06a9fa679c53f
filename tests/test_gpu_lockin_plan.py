"""The eight lock-in entries held to the table of tests/_lockin_plan_cases.py on the GPU: every row that fits on the device (at most 65600
lanes x 48 frames) is one real call on zeroed x and state, and `idsp_last_kernel()` must name the row's kernel and y must have been written
(all zero).  tests/test_lockin_plan.py holds `plan_lockin` to the same rows without a GPU, launch parameters included; the start-up stagger
is a kernel argument of calls of 2048 frames or more and is pinned there only.

Rows with switches run in a fresh child process per switch set (the library reads them once per process), as
tests/test_gpu_lockin_forms_forced.py does.  Reference: src/lockin.rs:11-39."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest

from tests import _lockin_plan_cases as L

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = sorted({c.entry for c in L.CASES})
SWITCH_SETS = sorted({json.dumps(c.sw, sort_keys=True) for c in L.CASES if c.gpu and c.sw})


def run_rows(eng, rows):
    """-> the rows that failed, with what the library said"""
    import torch

    from idsp_amd import _abi
    from tests import _harness as H

    def buf(n, dtype, off=0, fill=0):
        t = torch.full((n + 16,), fill, dtype=dtype, device="cuda")
        assert off % t.element_size() == 0 and t.data_ptr() % 64 == 0
        return t[off // t.element_size():][:n]

    def ptr(t):
        return C.c_void_p(t.data_ptr())

    bad = []
    for c in rows:
        n, layout = c.lanes * c.frames, H.FM if c.layout == "FM" else H.LM
        f32 = c.entry == "f32_biquad_lo_process"
        dt = torch.float32 if f32 else torch.int32
        x, st = buf(n, dt, c.off[0]), buf(64 * c.lanes, torch.int32)
        y = buf(n, torch.int64, c.off[1], 7) if c.entry == "norm_sqr" else buf(n * (1 if c.entry == "arg" else 2), dt, c.off[1], 7)
        lo = buf(2 * n, dt)
        cfg = _abi.LockinI32()
        cfg.order, cfg.cascade = c.a, c.b
        for i in range(c.b):
            cfg.k[i][0], cfg.k[i][1] = 1 << 20, -(1 << 26)
        sec = (_abi.BiquadF32 * 4)() if f32 else (_abi.BiquadI32 * 4)()
        for s in sec:
            s.ba[:] = [1, 0, 0, 0, 0]
            if not f32:
                s.frac = 30
        fn, tail = eng.fn["lockin_f32_biquad_lo_process" if f32 else "lockin_i32_" + c.entry], (c.lanes, c.frames, layout, None)
        if c.entry in L.READOUTS:
            rc = fn(C.byref(cfg), ptr(st), ptr(x), ptr(y), *tail)
        elif c.entry == "biquad_process":
            rc = fn(C.cast(sec, C.c_void_p), c.a, ptr(st), ptr(x), ptr(y), *tail)
        elif c.entry == "lo_process":
            rc = fn(C.byref(cfg), ptr(st), ptr(x), ptr(lo), ptr(y), *tail)
        elif c.entry == "accu_process":
            rc = fn(C.byref(cfg), C.byref(_abi.AccuLo(0, 1, 0)), ptr(st), ptr(x), ptr(lo), ptr(y), *tail)  # batch_log2 = 0: an `Accu` row per frame
        else:
            rc = fn(C.cast(sec, C.c_void_p), c.a, ptr(st), ptr(x), ptr(lo), ptr(y), *tail)
        torch.cuda.synchronize()
        k = eng.last_kernel()
        if c.name.startswith("stream_<"):
            named = k.startswith("stream_") and "::" + c.name[len("stream_<"):-1] + ">" in k
        else:
            named = k == c.name
        if rc != 0 or not named or int(y.abs().max()) != 0:
            bad.append((L.cli_line(c), c.name, k, rc, eng.err() if rc else "", int(y.abs().max())))
    return bad


@pytest.mark.parametrize("entry", ENTRIES)
def test_default_dispatch(gpu, entry):
    from tests import _harness as H

    rows = [c for c in L.CASES if c.gpu and not c.sw and c.entry == entry]
    assert rows
    bad = run_rows(H.engine(), rows)
    assert not bad, (len(bad), bad[:5])


@pytest.mark.parametrize("switches", SWITCH_SETS, ids=lambda s: ",".join("%s=%s" % (k[5:], v) for k, v in json.loads(s).items()))
def test_switches(gpu, switches):
    env = dict(os.environ, IDSP_DIAG="1", **json.loads(switches))
    r = subprocess.run([sys.executable, "-m", "tests.test_gpu_lockin_plan", switches], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("rows ok"), r.stdout[-3000:] + r.stderr[-2000:]


if __name__ == "__main__":  # the child of test_switches: the rows of one switch set, which the parent has put into the environment
    from tests import _harness as H

    rows = [c for c in L.CASES if c.gpu and c.sw and json.dumps(c.sw, sort_keys=True) == sys.argv[1]]
    bad = run_rows(H.engine(), rows)
    for b in bad:
        print(b)
    print(len(rows), "rows ok" if rows and not bad else "rows, %d failed" % len(bad))
    sys.exit(1 if bad or not rows else 0)
