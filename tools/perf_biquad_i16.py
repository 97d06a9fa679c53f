#!/usr/bin/env python3
"""Time idsp_biquad_i16_df1 on an MI355X against idsp_biquad_i32_df1 (a plain tool, not a test; profiles/NOTES.md, "Biquad i16").

  python tools/perf_biquad_i16.py [--out FILE.jsonl] [--lanes 65536 16384] [--frames 4096] [--sections 1] [--label TEXT]
  python tools/perf_biquad_i16.py --bylane [--out FILE.jsonl] [--lanes 65536 16384] [--frames 4096] [--sections 1 4] [--label TEXT]

Per shape (65536 and 16384 lanes x 4096 frames) and layout, one low-pass section: the i32 call, the i16 call and the i16 call in place,
INTERLEAVED round by round in one process (whatever else the box does hits all three): HIP-event time of 100 calls after 5 warm-ups,
seven rounds, the median reported with the minimum and maximum — for the i32 comparator too, so that its spread stands beside every
ratio.  The i16 call moves 4 bytes per sample (2 in, 2 out), the i32 call 8: `peak` is the i16 call's own bytes over its time as a
fraction of the 8 TB/s HBM peak, `time_over_i32` the ratio t_i16 / t_i32 (0.5 where both are memory-bound).
The kernel form is the library's choice (idsp_last_kernel() is recorded); to time another FrameMajor workgroup size run the tool again
under IDSP_DIAG=1 with IDSP_BQ16_FM_BLOCK=64 / 128 / 256 (read once per process) and give the run a --label.
--bylane times idsp_biquad_i16_df1_bylane / _df1_clamp_bylane against the shared-coefficient entry of the same build by the same method
(profiles/NOTES.md, "Biquad i16 by lane"): per shape, layout, section count (1 and 4) and plain / clamped, the shared call, the by-lane
call with EVERY lane holding that same section (the arithmetic is identical; the clamp is the whole i16 range) and both again in place,
interleaved round by round; `time_over_shared` is t_bylane / t_shared of the same placement, and the shared call's own spread stands
beside it.
One JSON line per measurement; needs a GPU (no fallback)."""
from __future__ import annotations

import argparse
import ctypes as C
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools import _perf_common as PC  # noqa: E402

WARMUP, CALLS, ROUNDS = 5, 100, 7
HBM_PEAK = 8.0e12  # bytes / s


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--lanes", type=int, nargs="+", default=[65536, 16384])
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--sections", type=int, nargs="+", default=None, help="default 1; with --bylane 1 and 4")
    ap.add_argument("--bylane", action="store_true", help="the by-lane entries against the shared-coefficient entries")
    ap.add_argument("--label", default="default")
    args = ap.parse_args()

    import torch

    from idsp_amd import _abi
    from idsp_amd._lib import load

    if not torch.cuda.is_available():
        print("perf_biquad_i16: no GPU", file=sys.stderr)
        return 2
    fn, _ = load()
    dev = "cuda:0"
    emit = PC.line_writer(args.out, "a", args.label)

    ptr = PC.ptr

    def timed(call):
        return PC.timed(call, WARMUP, CALLS, fn["last_error"])

    lp = (C.c_double * 6)(0.06745527388907189, 0.13491054777814377, 0.06745527388907189, 1.0, -1.1429805025399011, 0.4128015980961886)  # low-pass, f0 = 0.1
    if args.bylane:
        return bylane(args, fn, emit, timed, lp)
    if len(args.sections or [1]) != 1:
        ap.error("--sections takes one count without --bylane")
    ns = (args.sections or [1])[0]
    c16, c32 = (_abi.BiquadI16 * ns)(), (_abi.BiquadI32 * ns)()
    for k in range(ns):
        assert fn["biquad_i16_from_sos"](lp, 13, C.byref(c16[k])) == 0 and fn["biquad_i32_from_sos"](lp, 29, C.byref(c32[k])) == 0

    emit({"device": torch.cuda.get_device_name(0), "warmup": WARMUP, "calls": CALLS, "rounds": ROUNDS, "frames": args.frames, "sections": ns,
          "switches": {k: v for k, v in os.environ.items() if k.startswith("IDSP_")}})
    for lanes in args.lanes:
        frames = args.frames
        n = lanes * frames
        g = torch.Generator(device=dev).manual_seed(lanes)
        x16 = torch.randint(-12000, 12001, (n,), dtype=torch.int16, device=dev, generator=g)
        x32 = torch.randint(-(1 << 24), 1 << 24, (n,), dtype=torch.int32, device=dev, generator=g)
        y16, xy16, y32 = torch.empty_like(x16), x16.clone(), torch.empty_like(x32)
        for layout, lname in ((_abi.FRAME_MAJOR, "FrameMajor"), (_abi.LANE_MAJOR, "LaneMajor")):
            s16, s16i, s32 = (torch.zeros((4 * ns, lanes), dtype=torch.int32, device=dev) for _ in range(3))
            calls = {
                "biquad_i32_df1": lambda: fn["biquad_i32_df1"](c32, ns, ptr(s32), ptr(x32), ptr(y32), lanes, frames, layout, None),
                "biquad_i16_df1": lambda: fn["biquad_i16_df1"](c16, ns, ptr(s16), ptr(x16), 0, ptr(y16), 0, lanes, frames, layout, None),
                "biquad_i16_df1 in place": lambda: fn["biquad_i16_df1"](c16, ns, ptr(s16i), ptr(xy16), 0, ptr(xy16), 0, lanes, frames, layout, None),
            }
            ms, kernels = {k: [] for k in calls}, {}
            for _ in range(ROUNDS):
                for k, call in calls.items():
                    ms[k].append(timed(call))
                    kernels[k] = fn["last_kernel"]().decode()
            ref = statistics.median(ms["biquad_i32_df1"])
            for k in calls:
                med, bps = statistics.median(ms[k]), (8 if k == "biquad_i32_df1" else 4)
                emit({"entry": k, "lanes": lanes, "frames": frames, "layout": lname, "kernel": kernels[k], "ms": round(med, 5), "ms_min": round(min(ms[k]), 5),
                      "ms_max": round(max(ms[k]), 5), "spread": round((max(ms[k]) - min(ms[k])) / med, 4), "bytes_per_sample": bps,
                      "peak": round(n * bps / (med * 1e-3) / HBM_PEAK, 4), "time_over_i32": round(med / ref, 4)})
    return 0


def bylane(args, fn, emit, timed, lp) -> int:
    import torch

    from idsp_amd import _abi

    dev, ptr = "cuda:0", PC.ptr
    q = _abi.BiquadI16()
    assert fn["biquad_i16_from_sos"](lp, 13, C.byref(q)) == 0
    emit({"device": torch.cuda.get_device_name(0), "warmup": WARMUP, "calls": CALLS, "rounds": ROUNDS, "frames": args.frames, "mode": "bylane",
          "switches": {k: v for k, v in os.environ.items() if k.startswith("IDSP_")}})
    for lanes in args.lanes:
        frames = args.frames
        n = lanes * frames
        g = torch.Generator(device=dev).manual_seed(lanes)
        x = torch.randint(-12000, 12001, (n,), dtype=torch.int16, device=dev, generator=g)
        y, xy_s, xy_b = torch.empty_like(x), x.clone(), x.clone()
        for ns in (args.sections or [1, 4]):
            for clamped in (False, True):
                cfg = ((_abi.BiquadClampI16 if clamped else _abi.BiquadI16) * ns)()
                for c in cfg:
                    c.ba[:], c.frac = list(q.ba), 13
                    if clamped:
                        c.u, c.min, c.max = 0, -32768, 32767
                cv = 8 if clamped else 5
                sec = torch.tensor(list(q.ba) + ([0, -32768, 32767] if clamped else []), dtype=torch.int16)
                coef = sec.reshape(1, cv, 1).expand(ns, cv, lanes).contiguous().to(dev)  # every lane holds the shared call's section
                shared = "biquad_i16_df1_clamp" if clamped else "biquad_i16_df1"
                for layout, lname in ((_abi.FRAME_MAJOR, "FrameMajor"), (_abi.LANE_MAJOR, "LaneMajor")):
                    st = [torch.zeros((4 * ns, lanes), dtype=torch.int32, device=dev) for _ in range(4)]
                    calls = {
                        (shared, False): lambda: fn[shared](cfg, ns, ptr(st[0]), ptr(x), 0, ptr(y), 0, lanes, frames, layout, None),
                        (shared + "_bylane", False): lambda: fn[shared + "_bylane"](ptr(coef), 13, ns, ptr(st[1]), ptr(x), 0, ptr(y), 0, lanes, frames, layout, None),
                        (shared, True): lambda: fn[shared](cfg, ns, ptr(st[2]), ptr(xy_s), 0, ptr(xy_s), 0, lanes, frames, layout, None),
                        (shared + "_bylane", True): lambda: fn[shared + "_bylane"](ptr(coef), 13, ns, ptr(st[3]), ptr(xy_b), 0, ptr(xy_b), 0, lanes, frames, layout, None),
                    }
                    ms, kernels = {k: [] for k in calls}, {}
                    for _ in range(ROUNDS):
                        for k, call in calls.items():
                            ms[k].append(timed(call))
                            kernels[k] = fn["last_kernel"]().decode()
                    for (name, inplace) in calls:
                        k = (name, inplace)
                        med, ref = statistics.median(ms[k]), statistics.median(ms[(shared, inplace)])
                        emit({"entry": name + (" in place" if inplace else ""), "lanes": lanes, "frames": frames, "layout": lname, "sections": ns,
                              "clamped": clamped, "kernel": kernels[k], "ms": round(med, 5), "ms_min": round(min(ms[k]), 5), "ms_max": round(max(ms[k]), 5),
                              "spread": round((max(ms[k]) - min(ms[k])) / med, 4), "peak": round(n * 4 / (med * 1e-3) / HBM_PEAK, 4),
                              "time_over_shared": round(med / ref, 4)})
    return 0


if __name__ == "__main__":
    sys.exit(main())
