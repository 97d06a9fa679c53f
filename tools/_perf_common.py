"""What tools/perf_dsm.py and tools/perf_biquad_i16.py share: the HIP-event timing of one entry call and the JSON-line writer."""
import ctypes
import json


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def timed(call, warmup, calls, last_error):
    """ms per call: `warmup` calls held to status 0, then the HIP-event time of `calls` back-to-back calls"""
    import torch

    for _ in range(warmup):
        assert call() == 0, last_error()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        call()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def line_writer(path, mode, label=None):
    """-> emit(record): one JSON object per line to stdout and, if given, to the file `path`; `label`, if not None, leads every line"""
    out = open(path, mode) if path else None

    def emit(rec):
        line = json.dumps(rec if label is None else dict(label=label, **rec))
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    return emit
