#!/usr/bin/env python3
"""Time idsp_dsm_u32 on an MI355X (a plain tool, not a test; profiles/NOTES.md, "Dsm").

  python tools/perf_dsm.py [--out FILE.jsonl] [--lanes 65536 16384] [--frames 4096] [--orders 1 3 8] [--label TEXT]

Per shape (65536 and 16384 lanes x 4096 frames), order K in {1, 3, 8} and layout: HIP-event time of 20 calls after 5 warm-ups, three
rounds, the median reported with the minimum and maximum.  LaneMajor is timed twice, ALTERNATED round by round: on an aligned y (dword
runs) and on the same buffer one byte further (byte runs) — the two store forms of the LaneMajor kernel; FrameMajor has one form (the
packed quad store that was built beside it is in NOTES with its figures).  The comparator is idsp_unwrap_i32 at the same shape in the
same run: 4 bytes in and 4 out per sample, trivial arithmetic, the existing launch path; Dsm moves 5 bytes per sample, 5/8 of it.
One JSON line per measurement; with --label every line carries the label and --out is appended to, so that the runs of an A/B comparison
share one file.  Needs a GPU (no fallback)."""
from __future__ import annotations

import argparse
import ctypes as C
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools import _perf_common as PC  # noqa: E402

WARMUP, CALLS, ROUNDS = 5, 20, 3


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--lanes", type=int, nargs="+", default=[65536, 16384])
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--orders", type=int, nargs="+", default=[1, 3, 8])
    ap.add_argument("--label")
    args = ap.parse_args()

    import torch

    from idsp_amd import _abi
    from idsp_amd._lib import load

    if not torch.cuda.is_available():
        print("perf_dsm: no GPU", file=sys.stderr)
        return 2
    fn, _ = load()
    dev = "cuda:0"
    emit = PC.line_writer(args.out, "a" if args.label is not None else "w", args.label)

    ptr = PC.ptr

    def timed(call):
        return PC.timed(call, WARMUP, CALLS, fn["last_error"])

    emit({"device": torch.cuda.get_device_name(0), "warmup": WARMUP, "calls": CALLS, "rounds": ROUNDS, "frames": args.frames})
    for lanes in args.lanes:
        frames = args.frames
        n = lanes * frames
        g = torch.Generator(device=dev).manual_seed(lanes)
        x = torch.randint(-(1 << 31), (1 << 31) - 1, (n,), dtype=torch.int32, device=dev, generator=g)
        y8 = torch.empty(n + 4, dtype=torch.int8, device=dev)
        y32 = torch.empty(n, dtype=torch.int32, device=dev)
        for layout, lname in ((_abi.FRAME_MAJOR, "FrameMajor"), (_abi.LANE_MAJOR, "LaneMajor")):
            st2 = torch.zeros((2, lanes), dtype=torch.int32, device=dev)
            ref = [timed(lambda: fn["unwrap_i32"](ptr(st2), ptr(x), ptr(y32), lanes, frames, layout, None)) for _ in range(ROUNDS)]
            ref_ms = statistics.median(ref)
            emit({"entry": "unwrap_i32", "lanes": lanes, "frames": frames, "layout": lname, "kernel": fn["last_kernel"]().decode(),
                  "ms": ref_ms, "ms_min": min(ref), "ms_max": max(ref), "bytes_per_sample": 8, "gbs": n * 8 / ref_ms / 1e6})
            offsets = (0, 1) if layout == _abi.LANE_MAJOR else (0,)  # y one byte off the 4-byte grid: the byte runs of the LaneMajor kernel
            for order in args.orders:
                st = torch.zeros((2 * order, lanes), dtype=torch.int32, device=dev)
                ms, kernels = {o: [] for o in offsets}, {}
                for _ in range(ROUNDS):  # alternate the forms: whatever else the box does hits both
                    for off in offsets:
                        ms[off].append(timed(lambda: fn["dsm_u32"](order, ptr(st), ptr(x), 0, C.c_void_p(y8.data_ptr() + off), 0, lanes, frames, layout, None)))
                        kernels[off] = fn["last_kernel"]().decode()
                for off in offsets:
                    med = statistics.median(ms[off])
                    emit({"entry": "dsm_u32", "order": order, "lanes": lanes, "frames": frames, "layout": lname, "y_offset": off, "kernel": kernels[off],
                          "ms": med, "ms_min": min(ms[off]), "ms_max": max(ms[off]), "bytes_per_sample": 5, "gbs": n * 5 / med / 1e6,
                          "time_over_unwrap": med / ref_ms})
    return 0


if __name__ == "__main__":
    sys.exit(main())
