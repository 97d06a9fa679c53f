"""The phase consumers, the RPLL and the swept sine as processors of the shared launcher `launch_stream` (idsp_amd/csrc/lane_stream.h):
what the launcher branches on for each of them, which kernel it must therefore take at a given shape, and the smallest shapes on both
sides of every condition that selects a kernel.

Three things live here and are shared by tests/test_stream_proc_cases.py (no GPU), tests/test_gpu_stream_proc_dispatch.py and
tests/test_gpu_stream_argument.py:

  * TRAITS: one row per form, copied by hand from phase_procs.h, rpll_procs.h and sweep_procs.h;
  * expected_kernel(): the conditions of `plan_stream` (stream_plan.h: the choice `launch_stream` makes, `sweep_takes` included) restated in Python for dense
    tensors without IDSP_DIAG, written from the launcher's source.  Every threshold is read from dispatch_thresholds.h by name when the
    module is imported; the few literals of the launcher itself are the named constants below, each with its source line;
  * CASES / UNREACHABLE: the case table and the branches no default dispatch of a form can reach;
  * the inputs, the specification and the runner through the C ABI (moved here from test_gpu_phase.py, test_gpu_rpll.py and
    tests/_sweep_gpu.py, which import them back).

Imports neither torch nor the library at module level.  Test infrastructure only."""
from __future__ import annotations

import collections
import ctypes as C
import functools
import os
import re

import numpy as np

from idsp_amd import _abi
from tests import _phase_spec as PS
from tests import _rpll_spec as RS
from tests import _sweep_spec as WS

FM, LM = _abi.FRAME_MAJOR, _abi.LANE_MAJOR
DEV = "cuda:0"
POISON = -77
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "idsp_amd", "csrc")


# ------------------------------------------------------------------------------------------------ thresholds, parsed by name
def _constants(path):
    """every `constexpr <integer type> a = 1, b = 2;` of a header -> {name: value} (values that are plain integer literals)"""
    out = {}
    for m in re.finditer(r"constexpr\s+(?:size_t|int|unsigned)\s+([^;]+);", open(path).read()):
        for item in m.group(1).split(","):
            nv = re.fullmatch(r"\s*(k\w+)\s*=\s*(\d+)\s*", item)
            if nv:
                out[nv.group(1)] = int(nv.group(2))
    return out


THR = _constants(os.path.join(CSRC, "dispatch_thresholds.h"))
_LS = _constants(os.path.join(CSRC, "lane_stream.h"))
K_WAVE, K_FM_BLOCK, K_LM_RUN = _LS["kWave"], _LS["kFmBlock"], _LS["kLmRun"]
# the small constants of the dispatch (stream_plan.h reads them from the header by these names; compared here as plain values):
FEW_MAX_LANES, FEW_MIN_FRAMES = THR["kFewMaxLanes"], THR["kFewMinFrames"]        # `lanes <= 3 && frames >= 64`: the whole call on stream_frame_major_few
ODD_MIN_BODY, ODD_MIN_FRAMES = THR["kOddSplitMinBody"], THR["kOddSplitMinFrames"]  # `odd && body >= 8192 && frames >= 16`: the lanes % 4 split
ROUND_LANES = 256 * K_FM_BLOCK             # a whole round of the LDS-DMA kernel: 256 blocks of 256 lanes
ROUND_MIN_FRAMES, ROUND_MAX_ROUNDS = THR["kRoundsSplitMinFrames"], THR["kRoundsSplitMaxRounds"]
STAGED_MIN_FRAMES = THR["kStagedMinFrames"]  # FrameMajor staged kernel: `frames >= 16`
HEAVY_COST, LDS_COST = THR["kHeavyCost"], 120  # `COST > 120` is heavy; LDS_ELIGIBLE defaults to `COST <= 120` (lane_stream.h LdsEligibleOf)
SWEEP_MAX_GRID = 256                       # stream_plan.h: one workgroup per CU

# thresholds of the header that no condition of these forms' dispatch reads, with the reason
NOT_CONSULTED = {
    "kSweepMinLanes": "8-byte outputs on the sweep kernel: unwrap1 is LDS_ELIGIBLE = false, pll2 has COST 160",
    "kSweepMinLptSeveralSweeps": "several sweeps per launch (more than 256 x 4 x 256 lanes); read directly by sweep_takes",
    "kPairMaxCost": "a compile-time condition on COST, read directly (no side of it depends on the shape)",
    "kDuoMinLanes": "two-wave chain kernel: biquad chains only", "kDuo4MaxLanes": "two-wave chain kernel: biquad chains only",
    "kStaggerMinWorkgroups": "lockin_plan.h / readout_plan.h", "kStaggerMinFrames": "lockin_plan.h / readout_plan.h",
    "kStaggerMaxFrames": "lockin_plan.h / readout_plan.h", "kLockinStaggerTicks": "lockin_plan.h", "kFmDiscStaggerTicks": "readout_plan.h (fm_disc.hip)",
    # the lock-in entries' own dispatch: tests/_lockin_plan_cases.py holds a row on each side of every one of them
    "kSplitMaxLanes": "lockin_plan.h", "kLockinSixWavesMaxLanes": "lockin_plan.h", "kLockinStagesOneGroupMaxLanes": "lockin_plan.h",
    "kLockinSixWavesArmWeight": "lockin_plan.h", "kLockinB16MinLanes": "lockin_plan.h", "kLockinB16MaxLanes": "lockin_plan.h",
    "kLockinWavesMaxLanes": "lockin_plan.h", "kLockinTailMinFrames": "lockin_plan.h",
    # compared as the plain constants above, not through _cmp: tests/test_stream_proc_cases.py `minimum()` holds a case on each side of them
    "kHeavyCost": "HEAVY_COST: a compile-time condition on COST", "kFewMaxLanes": "FEW_MAX_LANES", "kFewMinFrames": "FEW_MIN_FRAMES",
    "kOddSplitMinBody": "ODD_MIN_BODY", "kOddSplitMinFrames": "ODD_MIN_FRAMES", "kRoundsSplitMinFrames": "ROUND_MIN_FRAMES",
    "kRoundsSplitMaxRounds": "ROUND_MAX_ROUNDS", "kStagedMinFrames": "STAGED_MIN_FRAMES", "kLmStagedMinRowBytes": "K_LM_RUN // 4 (lane_stream.h asserts the two equal)",
    # launch parameters that do not change the kernel's name (grid order, block size, prefetch depth), or that no shipped processor reaches
    "kStagedXcdcMinGrid": "the staged kernel's block order: not in the name", "kSweepXcdcMinGrid": "fewer than 8 workgroups of a sweep: below kSweepMinLanesFps",
    "kSweepFpsMaxBlockLanes": "read directly by _launch_sweep (`g.bw <= 128`)",
    "kWindowBlockMinWaves": "the register-window kernel's block size: not in the name",
    "kWindowDeepMaxWaves": "the register-window kernel's prefetch depth: not in the name", "kWindowXcdcMinGrid": "IDSP_FM_XCDC only",
}

_TRACE = None  # while set: (threshold, outcome, |value - threshold|) of every comparison expected_kernel evaluates


def _cmp(name, value, op):
    t = THR[name]
    r = {">=": value >= t, "<": value < t, "<=": value <= t, ">": value > t}[op]
    if _TRACE is not None:
        # the side is told by the outcome of `value >= t` (or `value > t` for <= / >), whatever the operator's direction
        above = value >= t if op in (">=", "<") else value > t
        _TRACE.add((name, above, abs(value - t)))
    return r


# ------------------------------------------------------------------------------------------------ the processors
Traits = collections.namedtuple("Traits", "proc entry in_bytes out_bytes has_in cost lds_eligible batch lm_staged lm_one_form words")


def _traits(proc, entry, in_bytes, out_bytes, has_in, cost, words, lds_eligible=None, batch=1, lm_staged=True, lm_one_form=False):
    return Traits(proc, entry, in_bytes, out_bytes, has_in, cost, cost <= LDS_COST if lds_eligible is None else lds_eligible, batch, lm_staged,
                  lm_one_form, words)


# (IN_DIV is 1 for all of them; none declares LM_STAGED, LM_ONE_FORM, MAX_U, SWEEP_MAX_LPT or SWEEP_UNPACED; UnwrapProc declares LDS_ELIGIBLE = MODE == 0)
TRAITS = {
    "clamp": _traits("ClampWrapProc", "clamp_wrap_i32", 4, 4, True, 40, 2),
    "unwrap0": _traits("UnwrapProc<0>", "unwrap_i32", 4, 4, True, 16, 2, lds_eligible=True),
    "unwrap1": _traits("UnwrapProc<1>", "unwrap_i32_phase", 4, 8, True, 16, 2, lds_eligible=False),
    "pll0": _traits("PllProc<0>", "pll_i32", 4, 4, True, 160, 9),
    "pll1": _traits("PllProc<1>", "pll_i32", 4, 4, True, 160, 9),
    "pll2": _traits("PllProc<2>", "pll_i32", 4, 8, True, 160, 9),
    "rpll": _traits("RpllProc", "rpll_i32", 8, 8, True, 150, 4),
    "sweep": _traits("SweepProc", "sweep_i32", 4, 8, False, 120, 7, batch=4),  # `In` is an unused int32_t
}
FORMS = list(TRAITS)
FOUR_BYTE = [f for f in FORMS if TRAITS[f].out_bytes == 4]  # y == x allowed


def _fm_staged(t):   # FmStagedOf (lane_stream.h)
    return t.has_in and t.in_bytes == t.out_bytes and t.in_bytes in (4, 8) and t.batch == 1


def _lm_staged(t):   # LmStagedOf
    return (not t.has_in or t.in_bytes == t.out_bytes) and t.out_bytes in (4, 8) and t.batch in (1, 4) and t.lm_staged


def _four_four(t):
    return t.has_in and t.in_bytes == 4 and t.out_bytes == 4


# ------------------------------------------------------------------------------------------------ fm_sweep.h
Geom = collections.namedtuple("Geom", "lpt grid bw rounds")


def sweep_geometry(lanes, max_lpt, max_grid=SWEEP_MAX_GRID):
    """stream_plan.h `sweep_geometry`; None: not coverable"""
    if lanes < 16 or max_lpt < 1:
        return None
    cap = max_grid * max_lpt * 256
    rounds = (lanes + cap - 1) // cap
    lr = (lanes + rounds - 1) // rounds
    lr = (lr + 15) // 16 * 16
    lpt = 1
    while lpt < max_lpt and max_grid * lpt * 256 < lr:
        lpt *= 2
    best, pick = 1e30, None
    for bw in range(256, 15, -16):
        per = lpt * bw
        g = (lr + per - 1) // per
        if g > max_grid:
            continue
        score = float(g * per - lr) / float(lr) + 0.25 * (float(max_grid - g) / float(max_grid)) + (256 - bw) * 1e-5
        if score < best:
            best, pick = score, (bw, g)
    if pick is None:
        return None
    return Geom(lpt, pick[1], pick[0], rounds)


def _sweep_max_lpt(t):  # SweepMaxLptOf
    return 4 if t.cost <= 120 else 2


def sweep_takes(t, lanes):
    g = sweep_geometry(lanes, _sweep_max_lpt(t))
    return g is not None and (g.rounds == 1 or g.lpt >= THR["kSweepMinLptSeveralSweeps"])


class Expected(str):
    """the prefix of idsp_last_kernel() up to and including `<`; `.suffix`: what the name must end with ("" for none)"""
    suffix = ""


def _name(prefix, suffix=""):
    e = Expected(prefix + "<")
    e.suffix = suffix
    return e


def _launch_sweep(t, lanes, on_grid64):
    g = sweep_geometry(lanes, _sweep_max_lpt(t))
    blocks = {1: "1 block", 2: "2 blocks", 4: "4 blocks", 8: "8 blocks", 16: "16 blocks"}[g.lpt]
    xcdc = not on_grid64 and g.grid >= 8
    suffix = ""
    if g.lpt == 1 and t.out_bytes == 4 and g.bw <= 128:  # several frames per segment (the 32-bit guard needs rows of gigabytes)
        f = 256 // g.bw
        suffix = " [%d frame%s/segment]" % (f, "" if f == 1 else "s")
    return _name("stream_frame_major_sweep[%s/workgroup%s]" % (blocks, ", XCD-contiguous" if xcdc else ""), suffix)


# ------------------------------------------------------------------------------------------------ launch_stream
def _frame_major(t, lanes, frames, xl, yl, xa, ya, split_remainder=False):
    """xl / yl: row pitch in elements; xa / ya: the addresses of x and y modulo 64"""
    isz, osz = t.in_bytes, t.out_bytes
    if _four_four(t):
        if lanes <= FEW_MAX_LANES and frames >= FEW_MIN_FRAMES:
            return _name("stream_frame_major_few")
        odd = lanes % 4
        body = lanes - odd
        if odd and body >= ODD_MIN_BODY and frames >= ODD_MIN_FRAMES and (_fm_staged(t) or t.lds_eligible):
            inner = _frame_major(t, body, frames, xl, yl, xa, ya)
            return _name(inner[:-1], inner.suffix + " + stream_frame_major_few (lanes % 4, second stream)")
    if _fm_staged(t) and _four_four(t) and t.cost <= LDS_COST:
        head = lanes // ROUND_LANES * ROUND_LANES
        tail = lanes - head
        rounds = head // ROUND_LANES
        head_on_sweep = t.lds_eligible and head != 0 and sweep_takes(t, head)
        rounds_ok = not head_on_sweep or (rounds & (rounds - 1) == 0 and rounds <= ROUND_MAX_ROUNDS)
        if (head and tail and _cmp("kSplitTailMax", tail, "<=") and rounds_ok and lanes % 4 == 0 and frames >= ROUND_MIN_FRAMES and
                t.lds_eligible and xl * 4 < 1 << 28 and yl * 4 < 1 << 28):
            inner = _frame_major(t, head, frames, xl, yl, xa, ya)
            which = "stream_frame_major_sweep" if inner.startswith("stream_frame_major_sweep") else "stream_frame_major_lds"
            return _name(which + " + stream_frame_major_staged (remainder, second stream)")
    if _fm_staged(t) and _four_four(t) and t.cost <= THR["kPairMaxCost"]:
        grid64 = xa % 64 == 0 and ya % 64 == 0 and (xl * 4) % 64 == 0 and (yl * 4) % 64 == 0
        if (not split_remainder and _cmp("kPairMaxLanes", lanes, "<=") and _cmp("kPairMinFrames", frames, ">=") and lanes % 4 == 0 and grid64 and
                xl * 4 < 1 << 28 and yl * 4 < 1 << 28):
            return _name("stream_frame_major_pair[compute + mover wave per 32 lanes]")
    if t.has_in and isz == 4 and t.lds_eligible:
        on_grid64 = xa % 64 == 0 and ya % 64 == 0 and (xl * isz) % 64 == 0 and (yl * osz) % 64 == 0
        off_grid_ok = on_grid64 or lanes > THR["kLdsGridCap"] * K_FM_BLOCK or (osz == 4 and _cmp("kSweepOffGridSmallMax", lanes, "<="))
        if not on_grid64 and _TRACE is not None:
            _TRACE.add(("kLdsGridCap", lanes > THR["kLdsGridCap"] * K_FM_BLOCK, abs(lanes - THR["kLdsGridCap"] * K_FM_BLOCK)))
        sweep_min = "kSweepMinLanesFps" if osz == 4 else "kSweepMinLanes"
        if off_grid_ok and lanes % 4 == 0 and _cmp(sweep_min, lanes, ">=") and _cmp("kSweepMinFrames", frames, ">=") and sweep_takes(t, lanes):
            return _launch_sweep(t, lanes, on_grid64)
    if _fm_staged(t):
        heavy = t.cost > HEAVY_COST
        # (the frame and row conditions first: the lane window is then traced only where it decides)
        rows = frames >= STAGED_MIN_FRAMES and (lanes * isz) % 16 == 0 and xl * isz < 1 << 28 and yl * isz < 1 << 28
        if not rows:
            in_range = False
        elif heavy:
            in_range = _cmp("kStagedHeavyMinLanes", lanes, ">=") and _cmp("kStagedHeavyMaxLanes", lanes, "<")
        else:
            in_range = _cmp("kStagedMaxLanes", lanes, "<")
        if in_range:
            off64 = (xl * isz) % 64 != 0 or (yl * isz) % 64 != 0 or xa % 64 != 0 or ya % 64 != 0
            if heavy:
                lw = 32
            else:
                lw = 64 if _cmp("kStaged64LanesOffGrid" if off64 else "kStaged64Lanes", lanes, ">=") else 32 if _cmp("kStaged32Lanes", lanes, ">=") else 16
            return _name("stream_frame_major_staged[%d lanes/wave]" % lw)
    if t.has_in and isz == 4:
        waves = (lanes + K_WAVE - 1) // K_WAVE
        ow = osz // 4
        if t.lds_eligible and _cmp("kLdsMinWaves", waves, ">=") and (lanes % K_FM_BLOCK == 0 or (ow == 1 and lanes % 4 == 0)):
            misaligned = (xl * 4) % 64 != 0 or (yl * ow * 4) % 64 != 0 or xa % 64 != 0 or ya % 64 != 0
            return _name("stream_frame_major_lds[XCD-contiguous blocks]" if misaligned else "stream_frame_major_lds")
    return _name("stream_frame_major")


def _lane_major(t, lanes, frames, xa, ya):
    if _lm_staged(t):
        isz = t.in_bytes if t.has_in else 0
        osz = t.out_bytes
        wide = max(isz, osz)
        x_ok = not t.has_in or (xa % 16 == 0 and (frames * isz) % 16 == 0 and frames * isz < 1 << 26)
        if frames * wide >= K_LM_RUN // 4 and x_ok and ya % 16 == 0 and (frames * osz) % 16 == 0 and frames * osz < 1 << 26:
            heavy = t.cost > HEAVY_COST
            lw = 64 if _cmp("kLmStaged64Lanes", lanes, ">=") else 32 if (_cmp("kLmStaged32Lanes", lanes, ">=") or heavy) else 16
            if t.lm_one_form or lw == 64:
                return _name("stream_lane_major_staged")
            if lw == 16 and not heavy:
                return _name("stream_lane_major_staged[16 lanes/wave]")
            return _name("stream_lane_major_staged[32 lanes/wave]")
    return _name("stream_lane_major")


def expected_kernel(form, layout, lanes, frames, x_off=0, y_off=0):
    """The kernel `launch_stream` takes for a dense call of `form`: the prefix of idsp_last_kernel() up to and including `<`, with the
    suffix the name must end with in `.suffix`.  x_off / y_off: bytes between the 512-byte grid and x / y."""
    t = TRAITS[form]
    if layout == LM:
        return _lane_major(t, lanes, frames, x_off % 64, y_off % 64)
    return _frame_major(t, lanes, frames, lanes, lanes, x_off % 64, y_off % 64)


def traced(form, layout, lanes, frames, x_off=0, y_off=0):
    """-> (expected kernel, the set of (threshold, on or above it, distance) the decision evaluated)"""
    global _TRACE
    _TRACE = set()
    try:
        return expected_kernel(form, layout, lanes, frames, x_off, y_off), _TRACE
    finally:
        _TRACE = None


def kernel_key(e):
    """prefix and suffix with the frames-per-segment count taken out of the suffix (a detail of the same kernel form)"""
    return (str(e), re.sub(r"\[\d+ frames?/segment\]", "[n frames/segment]", e.suffix))


# ------------------------------------------------------------------------------------------------ the case table
Case = collections.namedtuple("Case", "form layout lanes frames x_off y_off branch")


def _case(form, layout, lanes, frames, branch, x_off=0, y_off=0):
    return Case(form, layout, lanes, frames, x_off, y_off, branch)


def _cheap_fm(form):
    T = THR
    rows = [
        ("few", (3, 64)), ("off few: frames", (3, 63)), ("off few: lanes", (4, 64)),
        ("lanes % 4 split", (ODD_MIN_BODY + 1, 16)), ("off lanes % 4 split: body", (ODD_MIN_BODY - 3, 16)), ("off lanes % 4 split: frames", (ODD_MIN_BODY + 1, 15)),
        ("lanes % 4 split of a sweep", (T["kSweepMinLanesFps"] + 1, 16)),
        ("round split, rows off the 64-byte grid", (ROUND_LANES + 4, 16)), ("round split, largest remainder", (ROUND_LANES + T["kSplitTailMax"], 16)),
        ("off round split: remainder", (ROUND_LANES + T["kSplitTailMax"] + 4, 16)), ("off round split: frames", (ROUND_LANES + 4, 15)),
        ("round split + lanes % 4 split", (ROUND_LANES + 5, 16)),
        ("power-of-two rule of the round split", (3 * ROUND_LANES + 4096, 16)),
        ("pair, fewest lanes", (16, T["kPairMinFrames"])), ("pair, most lanes", (T["kPairMaxLanes"], T["kPairMinFrames"])),
        ("off pair: rows of 16 bytes are off the 64-byte grid", (4, T["kPairMinFrames"])),
        ("off pair: frames", (T["kPairMaxLanes"], T["kPairMinFrames"] - 1)), ("off pair: lanes (and rows off the grid)", (T["kPairMaxLanes"] + 4, T["kPairMinFrames"])),
        ("off pair: lanes, rows on the grid", (T["kPairMaxLanes"] + 16, T["kPairMinFrames"])),
        ("sweep, several frames per segment", (T["kSweepMinLanesFps"], T["kSweepMinFrames"])), ("off sweep: lanes", (T["kSweepMinLanesFps"] - 4, T["kSweepMinFrames"])),
        ("off sweep: lanes, rows on the 64-byte grid (staged, 32 lanes per wave)", (T["kStaged64Lanes"] - 16, 16)),
        ("off sweep: frames", (T["kSweepMinLanesFps"], T["kSweepMinFrames"] - 1)),
        ("sweep, full blocks", (ROUND_LANES, 16)), ("sweep, full blocks, 2 per workgroup", (2 * ROUND_LANES, 16)),
        ("staged, 32 lanes per wave", (T["kStaged32Lanes"], 16)), ("staged, 16 lanes per wave", (T["kStaged32Lanes"] - 4, 16)),
        ("LDS-DMA", (ROUND_LANES, 15)), ("LDS-DMA, smallest launch", (T["kLdsMinWaves"] * K_WAVE - K_WAVE + 4, 15)),
        ("off LDS-DMA: waves", (T["kLdsMinWaves"] * K_WAVE - K_WAVE, 15)),
        ("register window", (1000, 15)),
        # the smallest lane counts (of a scan in steps of 4 and around every threshold) of the remaining combinations of a body and the lanes % 4 split
        ("lanes % 4 split of a sweep of wide blocks, rows off the grid", (40955, 16)),
        ("lanes % 4 split of an XCD-contiguous LDS-DMA body", (T["kSweepOffGridSmallMax"] + 5, 16)),
        ("lanes % 4 split of a sweep, 2 blocks per workgroup", (T["kLdsGridCap"] * K_FM_BLOCK + 5, 16)),
        ("round split on the sweep kernel + lanes % 4 split", (2 * ROUND_LANES + 5, 16)),
        ("sweep, 4 blocks per workgroup, rows off the grid", (151556, 16)), ("lanes % 4 split of a sweep, 4 blocks per workgroup", (196603, 16)),
    ]
    out = [_case(form, FM, l, f, b) for b, (l, f) in rows]
    # rows off the 64-byte grid: x and y 16 bytes into their allocations
    out += [
        _case(form, FM, 32768, 16, "sweep, XCD-contiguous", 16, 16),
        _case(form, FM, T["kSweepOffGridSmallMax"], 16, "sweep off the grid, most lanes of the small window", 16, 16),
        _case(form, FM, T["kSweepOffGridSmallMax"] + 4, 16, "off the small window: XCD-contiguous LDS-DMA", 16, 16),
        _case(form, FM, T["kLdsGridCap"] * K_FM_BLOCK, 16, "off the grid up to the largest single-round LDS-DMA grid", 16, 16),
        _case(form, FM, T["kLdsGridCap"] * K_FM_BLOCK + 4, 16, "off the grid above it: the sweep again", 16, 16),
        _case(form, FM, T["kPairMaxLanes"], T["kPairMinFrames"], "off pair: rows off the 64-byte grid", 16, 16),
        _case(form, FM, T["kStaged32Lanes"], 16, "staged off the 64-byte grid", 16, 16),
    ]
    return out


def _heavy_fm(form):
    T = THR
    step = 4 if TRAITS[form].in_bytes == 4 else 2  # whole 16-byte pieces per row
    lo, hi = T["kStagedHeavyMinLanes"], T["kStagedHeavyMaxLanes"]
    out = [
        _case(form, FM, lo, 16, "staged, first lane count of the heavy window"), _case(form, FM, lo - step, 16, "off staged: below the heavy window"),
        _case(form, FM, hi - step, 16, "staged, last lane count of the heavy window"), _case(form, FM, hi, 16, "off staged: above the heavy window"),
        _case(form, FM, lo, 15, "off staged: frames"), _case(form, FM, 1000, 15, "register window"),
    ]
    if form == "rpll":
        out += [_case(form, FM, 24577, 16, "off staged: rows of no whole 16-byte pieces"), _case(form, FM, 3, 64, "no few kernel for 8-byte samples")]
    else:
        out += [_case(form, FM, 24577, 16, "lanes % 4 split with a staged body"), _case(form, FM, 3, 64, "few"), _case(form, FM, 3, 63, "off few: frames"),
                _case(form, FM, ODD_MIN_BODY + 1, 16, "lanes % 4 split with a register-window body")]
    return out


def _lane_major_cases(form):
    t, T = TRAITS[form], THR
    if not _lm_staged(t):
        return [_case(form, LM, 1000, 64, "tile kernel (the only one)"), _case(form, LM, 65, 33, "tile kernel, ragged tile"),
                _case(form, LM, T["kLmStaged64Lanes"], 16, "tile kernel at the staged kernel's 64-lane count")]
    wide = max(t.in_bytes if t.has_in else 0, t.out_bytes)
    F = K_LM_RUN // 4 // wide           # fewest frames of the staged kernel
    per16 = 16 // wide                  # frames per 16 bytes of a row
    out = [
        _case(form, LM, 1000, F, "staged, fewest frames"), _case(form, LM, 1000, F - 1, "off staged: frames"),
        _case(form, LM, 1000, F - per16, "off staged: frames, rows of whole 16-byte pieces"),
        _case(form, LM, 1000, F + 1, "off staged: row bytes no multiple of 16"),
        _case(form, LM, T["kLmStaged64Lanes"], F, "staged, 64 lanes per wave"), _case(form, LM, T["kLmStaged64Lanes"] - 4, F, "staged, 32 lanes per wave"),
        _case(form, LM, T["kLmStaged32Lanes"], F, "staged, 32 lanes per wave, fewest lanes"),
        _case(form, LM, T["kLmStaged32Lanes"] - 4, F, "staged, below the 32-lane count"),
        _case(form, LM, 65, 2 * F + per16 + 1, "tile kernel, ragged tiles"), _case(form, LM, 65, 4 * F + per16, "staged, ragged wave and last tile"),
    ]
    return out


def _frame_major_cases(form):
    t = TRAITS[form]
    if _four_four(t) and t.cost <= LDS_COST:
        return _cheap_fm(form)
    if _fm_staged(t):
        return _heavy_fm(form)
    # 4 in / 8 out and the generator: the register-window kernel, one wave or four per workgroup (1024 waves), deep or shallow window (2048 waves)
    return [_case(form, FM, 1000, 15, "register window"), _case(form, FM, 3, 64, "register window (no few kernel)"),
            _case(form, FM, 1024 * K_WAVE - K_WAVE, 16, "register window, single waves"), _case(form, FM, 1024 * K_WAVE, 16, "register window, 256-thread blocks"),
            _case(form, FM, 2048 * K_WAVE + 4, 16, "register window, shallow window"), _case(form, FM, THR["kStagedHeavyMinLanes"], 16, "register window inside the heavy window")]


CASES = [c for form in FORMS for c in _frame_major_cases(form) + _lane_major_cases(form)]

# Branches of launch_stream that a form's default dispatch cannot reach, with the condition that excludes them (tests/test_stream_proc_cases.py
# holds each to a scan of expected_kernel).  (forms, layout, kernel-name prefix never returned, why)
UNREACHABLE = [
    (("clamp", "unwrap0"), FM, "stream_frame_major_staged[64 lanes/wave]<",
     "from kStaged64Lanes (= kSweepMinLanesFps) lanes up a call of 16+ frames and lanes % 4 == 0 goes to the sweep kernel, on the grid and — up to "
     "kSweepOffGridSmallMax lanes — off it; the form only runs unnamed, as the remainder of a round split"),
    (("clamp", "unwrap0"), FM, "stream_frame_major_sweep[8 blocks/workgroup",
     "SWEEP_MAX_LPT is 4 for processors that do not declare it"),
    (("pll0", "pll1", "rpll"), FM, "stream_frame_major_staged[64 lanes/wave]<", "COST > 120: always 32 lanes per wave"),
    (("pll0", "pll1", "rpll"), FM, "stream_frame_major_staged[16 lanes/wave]<", "COST > 120: always 32 lanes per wave"),
    (("pll0", "pll1", "rpll"), FM, "stream_frame_major_sweep", "LDS_ELIGIBLE defaults to COST <= 120; rpll also has 8-byte inputs"),
    (("pll0", "pll1", "rpll"), FM, "stream_frame_major_lds", "LDS_ELIGIBLE defaults to COST <= 120; rpll also has 8-byte inputs"),
    (("pll0", "pll1", "rpll"), FM, "stream_frame_major_pair", "COST > kPairMaxCost"),
    (("pll0", "pll1"), FM, "stream_frame_major_sweep + ", "the round split needs COST <= 120"),
    (("rpll",), FM, "stream_frame_major_few<", "4-byte samples only"),
    (("unwrap1", "pll2", "sweep"), FM, "stream_frame_major_", "FmStagedOf needs equal sample sizes and an input; unwrap1 is LDS_ELIGIBLE = false, pll2 has COST 160, "
     "the generator has no input: the register-window kernel is all there is"),
    (("unwrap1", "pll2"), LM, "stream_lane_major_staged", "LmStagedOf needs an input of the output's size"),
    (("pll0", "pll1", "rpll"), LM, "stream_lane_major_staged[16 lanes/wave]<", "COST > 120: 32 lanes per wave below kLmStaged64Lanes"),
]
# sides of thresholds that expected_kernel evaluates but that cannot be reached: (threshold, on or above it, why)
UNREACHABLE_SIDES = [
    ("kStaged64Lanes", True, "see UNREACHABLE: the sweep kernel takes those lane counts first"),
    ("kStaged64LanesOffGrid", True, "see UNREACHABLE: off the grid the sweep kernel takes 24576 .. kSweepOffGridSmallMax lanes, and the staged kernel ends at kStagedMaxLanes"),
    ("kStaged64LanesOffGrid", False, "the same: the lane counts next to it go to the sweep kernel"),
    ("kStagedMaxLanes", True, "cheap processors: calls of 16+ frames next to it go to the sweep kernel (on the grid, and off it up to kSweepOffGridSmallMax lanes)"),
    ("kStagedMaxLanes", False, "the same"),
]


# ------------------------------------------------------------------------------------------------ inputs and specification
def sweep_population(rng, lanes, frames):
    """[7, lanes] uint32, lane l of kind l % 8: four fresh fit-derived sweeps and one under way that outlast the call (kinds 0, 2, 3, 5, 7), one that
    ends inside the call (1), one that had ended (4), one whose last sample is the call's last frame (6): three lanes in eight have ended by the last frame"""
    rate_k, tail = WS.kat_tail()
    assert frames < WS.TAIL
    tail = np.array(tail, dtype=np.int64)
    fits = [WS.fit(*WS.KAT_FIT), WS.fit(0.5, 1e6, 1.0), WS.fit(0.01, 7.0, 123.0), WS.fit(0.25, 100000.0, 2.9)]
    l = np.arange(lanes)
    kind, turn = l % 8, l // 8
    state = np.zeros(lanes, np.int64)
    rate = np.full(lanes, rate_k, np.int64)
    for k, (r, s) in zip((0, 2, 5, 7), fits):
        state[kind == k], rate[kind == k] = s, r
    state[kind == 1] = tail[1 + turn % max(frames - 1, 1)][kind == 1]
    state[kind == 3] = tail[frames + 1 + turn % (WS.TAIL - frames)][kind == 3]
    state[kind == 4] = tail[0]
    state[kind == 6] = tail[frames]
    st = rng.integers(0, 1 << 32, size=(WS.WORDS, lanes), dtype=np.uint64).astype(np.uint32)  # accu: random
    u = state.view(np.uint64)
    st[0], st[1] = (u & np.uint64(0xFFFFFFFF)).astype(np.uint32), (u >> np.uint64(32)).astype(np.uint32)
    st[4] = rate.astype(np.int32).view(np.uint32)
    em = np.array([0, 5, WS.M32, WS.M32 - 2, (1 << 64) - 1, (1 << 64) - 3, 1 << 40], dtype=np.uint64)[rng.integers(0, 7, size=lanes)]
    st[5], st[6] = (em & np.uint64(0xFFFFFFFF)).astype(np.uint32), (em >> np.uint64(32)).astype(np.uint32)
    return st


def make_inputs(form, lanes, frames, seed):
    """-> (cfg, x, st): x [frames, lanes(, 2)] int32 or None (the generator), st [words, lanes] uint32"""
    rng = np.random.default_rng(seed)
    if form.startswith("pll"):
        ba = PS.random_ba(rng)
        return ba, PS.adversarial_phases(rng, frames, lanes), PS.random_state(rng, PS.PLL_WORDS, lanes)
    if form == "rpll":
        cfg = RS.CONFIGS[(lanes + frames) % len(RS.CONFIGS)]
        return cfg, RS.adversarial_ts(rng, frames, lanes), RS.random_state(rng, lanes)
    if form == "sweep":
        return None, None, sweep_population(rng, lanes, frames)
    return None, PS.adversarial_phases(rng, frames, lanes), PS.random_state(rng, 2, lanes)


def spec_run(form, cfg, st, x, frames=None):
    """the specification on x [frames, lanes(, 2)]; st updated; -> [frames, lanes(, 2)]"""
    if form.startswith("pll"):
        return PS.pll_np(cfg, st, x, output=int(form[-1]))
    if form.startswith("unwrap"):
        return PS.unwrap_np(st, x, mode=int(form[-1]))
    if form == "clamp":
        return PS.clamp_wrap_np(st, x)
    if form == "rpll":
        return RS.rpll_np(cfg, st, x)
    return WS.osc_np(st, frames)


def case_seed(form, lanes, frames):
    return 100003 * FORMS.index(form) + 31 * lanes + frames


@functools.lru_cache(maxsize=4)
def reference(form, lanes, frames):
    """-> (cfg, x, state before, state after, output) of the specification on the case's inputs; shared, never modified"""
    cfg, x, st = make_inputs(form, lanes, frames, case_seed(form, lanes, frames))
    after = st.copy()
    out = spec_run(form, cfg, after, x, frames)
    for a in (x, st, after, out):
        if a is not None:
            a.setflags(write=False)
    return cfg, x, st, after, out


# ------------------------------------------------------------------------------------------------ through the C ABI
def _ptr(t):
    return C.c_void_p(t.data_ptr())


def to_layout(a, layout):
    """[frames, lanes(, w)] -> the flat array of `layout`"""
    return np.ascontiguousarray(a if layout == FM else np.swapaxes(a, 0, 1))


def from_layout(flat, layout, frames, lanes, width=1):
    """the flat output of `layout` -> [frames, lanes] (width 1) or [frames, lanes, width]"""
    tail = () if width == 1 else (width,)
    a = flat.reshape(((frames, lanes) if layout == FM else (lanes, frames)) + tail)
    return np.ascontiguousarray(a if layout == FM else np.swapaxes(a, 0, 1))


def call_form(gpu, form, cfg, sd, xd, yd, lanes, frames, layout, stream=None):
    """the entry of `form` on device pointers (ctypes c_void_p or int); -> the return code"""
    s = None if stream is None else C.c_void_p(stream)
    p = lambda v: v if isinstance(v, C.c_void_p) else C.c_void_p(v)  # noqa: E731
    if form.startswith("pll"):
        return gpu.fn["pll_i32"]((C.c_int32 * 3)(*cfg), p(sd), p(xd), p(yd), lanes, frames, layout, int(form[-1]), s)
    if form == "rpll":
        return gpu.fn["rpll_i32"](C.byref(_abi.Rpll(*cfg)), p(sd), p(xd), p(yd), lanes, frames, layout, s)
    if form == "sweep":
        return gpu.fn["sweep_i32"](p(sd), p(yd), lanes, frames, layout, s)
    return gpu.fn[TRAITS[form].entry](p(sd), p(xd), p(yd), lanes, frames, layout, s)


def out_width(form):
    """int32 words per output element as the tests see it: unwrap1 is one int64"""
    return 2 if form in ("pll2", "rpll", "sweep") else 1


def run_form(gpu, form, cfg, st, x, frames, layout, inplace=False, chunks=None, off=(0, 0, 0), record=None):
    """`form` through the C ABI on guarded buffers (tests/_guard.py), outputs poisoned; st [words, lanes] uint32 is updated.
    chunks: frame counts of consecutive calls on one state (their sum = frames); off: bytes between the 512-byte grid and x, y, state;
    record(n, kernel) is called after every call.  Returns the output as [frames, lanes(, 2)]."""
    import torch

    from tests._guard import Guards

    t = TRAITS[form]
    lanes = st.shape[1]
    gs = Guards(DEV)  # the state of all chunks
    sd = gs.upload("state", st, off=off[2])
    outs, f0 = [], 0
    for n in chunks or [frames]:
        g = Guards(DEV)
        xd = g.upload("x", to_layout(x[f0:f0 + n], layout), off=off[0], readonly=not inplace) if t.has_in else None
        if inplace:
            assert form in FOUR_BYTE and t.has_in
            yd = xd
        elif form == "unwrap1":
            yd = g.full("y", lanes * n, torch.int64, POISON, off=off[1])
        else:
            yd = g.full("y", lanes * n * out_width(form), torch.int32, POISON, off=off[1])
        rc = call_form(gpu, form, cfg, _ptr(sd), None if xd is None else _ptr(xd), _ptr(yd), lanes, n, layout)
        assert rc == 0, gpu.err()
        torch.cuda.synchronize()
        k = gpu.last_kernel()
        if record:
            record(n, k)
        g.check((form, cfg, layout, lanes, n, off, k))
        gs.check((form, cfg, layout, lanes, n, off, k))
        outs.append(from_layout(yd.cpu().numpy().reshape(-1), layout, n, lanes, out_width(form)))
        f0 += n
    assert f0 == frames
    st[...] = sd.cpu().numpy().view(np.uint32).reshape(st.shape)
    return np.concatenate(outs)
