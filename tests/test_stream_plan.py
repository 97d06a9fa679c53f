"""The dispatch of `launch_stream` without a GPU: `plan_stream` (idsp_amd/csrc/stream_plan.h) run through build/stream_plan_cli
(tests/cpp/stream_plan_cli.cpp, plain g++).

  * every row of tests/_dispatch_cases.py, with the assertions of tests/test_gpu_dispatch_table.py (which pins the real processors to the same
    rows on the GPU: a wrong hand-written trait set of the program shows up as a mismatch between the two);
  * the conditions that table does not reach — frame minima, every lane threshold of dispatch_thresholds.h at value - 4 and value, the two
    splits, rows off the 16- and the 64-byte grid, the switches the GPU tests use, sweep_geometry, duo_wanted.  The expectations were read
    off the launcher as it stood before the choice moved into stream_plan.h (`lane_stream.h:N` / `fm_sweep.h:N` below are line numbers of
    that revision, the parent of the commit that added this file);
  * the same function against the independent restatement of the dispatch in tests/_stream_proc_cases.py (`expected_kernel`, pinned on the
    GPU by tests/test_gpu_stream_proc_dispatch.py), over lane counts around every threshold.

Reference loop nests the launcher replaces: dsp-process/src/compose.rs:468-494 (`Lanes`), process.rs:122-141."""
import os
import subprocess

import pytest

from tests import _dispatch_cases as D
from tests import _stream_proc_cases as SP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = SP.THR
SWEEP, ODD = D.SWEEP, D.ODD
WINDOW, LDS, LDS_X = "stream_frame_major<", "stream_frame_major_lds<", "stream_frame_major_lds[XCD-contiguous blocks]<"
STAGED = "stream_frame_major_staged[%d lanes/wave]<"
PAIR = "stream_frame_major_pair[compute + mover wave per 32 lanes]<"
ROUNDS = "stream_frame_major_%s + stream_frame_major_staged (remainder, second stream)<"
SWEEP_X = SWEEP + "%s/workgroup, XCD-contiguous]<"
CHEAP, HEAVY = "i32_df1", "pll"


@pytest.fixture(scope="module")
def cli():
    subprocess.run(["make", "-s", "build/stream_plan_cli"], cwd=ROOT, check=True)
    exe = os.path.join(ROOT, "build", "stream_plan_cli")

    def run(lines):
        r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stderr
        out = r.stdout.split("\n")[:-1]
        assert len(out) == len(lines) and not any(o.startswith("error") for o in out), [o for o in out if o.startswith("error")][:3]
        return out

    return run


def plan(traits, lanes, frames=32, layout="FM", xo=0, yo=0, px=0, py=0, *flags):
    return "plan %s %d %d %s %d %d %d %d %s" % (traits, lanes, frames, layout, xo, yo, px, py, " ".join(flags))


def names(cli, lines):
    return [o.split("\t")[0] for o in cli(lines)]


def details(cli, lines):
    return [dict(kv.split("=") for kv in o.split("\t")[1].split(" ")) for o in cli(lines)]


def check(cli, rows):
    """rows: (plan line, expected start of the name, expected end or None) — the assertion of test_gpu_dispatch_table.py"""
    got = names(cli, [r[0] for r in rows])
    for (line, start, end), k in zip(rows, got):
        assert k.startswith(start) and (end is None or k.endswith(end)) and (end is not None or not k.endswith(ODD)), (line, k)


# ------------------------------------------------------------------------------------------------ the GPU table
def test_i32_df1_frame_major_lane_counts(cli):
    check(cli, [(plan(CHEAP, lanes), start, end) for lanes, start, end in D.I32_FM])


@pytest.mark.parametrize("table", [D.C5_AND_LANE_MAJOR, D.SEVERAL_SWEEPS], ids=["c5_and_lane_major", "several_sweeps"])
def test_other_biquad_rows(cli, table):
    got = names(cli, [plan(tr, lanes, frames, layout) for tr, lanes, frames, layout, _, _ in table])
    for (tr, lanes, frames, layout, start, taken), k in zip(table, got):
        assert k.startswith(start) == taken, (tr, lanes, k)


# ------------------------------------------------------------------------------------------------ frame minima
def test_frame_minima(cli):
    pf = T["kPairMinFrames"]
    check(cli, [
        # lane_stream.h:1712 `lanes <= 3 && frames >= 64`
        (plan(CHEAP, 3, 63), WINDOW, None), (plan(CHEAP, 3, 64), "stream_frame_major_few<", None), (plan(CHEAP, 4, 64), STAGED % 16, None),
        # lane_stream.h:1779 `frames >= thr::kPairMinFrames`
        (plan(CHEAP, 16384, pf - 1), STAGED % 32, None), (plan(CHEAP, 16384, pf), PAIR, None),
        # lane_stream.h:1826 staged `frames >= 16` (below: 256 waves of whole blocks, the round-3 LDS-DMA kernel)
        (plan(CHEAP, 16384, 15), LDS, None), (plan(CHEAP, 16384, 16), STAGED % 32, None),
        # lane_stream.h:1808 sweep `frames >= thr::kSweepMinFrames`
        (plan(CHEAP, 65536, 15), LDS, None), (plan(CHEAP, 65536, 16), SWEEP + "1 block/workgroup]<", None),
        # lane_stream.h:1744 rounds split `frames >= 16`, :1718 lanes % 4 split `frames >= 16`
        (plan(CHEAP, 65552, 15), LDS, None), (plan(CHEAP, 65552, 16), ROUNDS % "sweep", None),
        (plan(CHEAP, 8193, 15), WINDOW, None), (plan(CHEAP, 8193, 16), STAGED % 32, ODD),
        # lane_stream.h:1649 LaneMajor staged `frames * wide >= kLmRun / 4` = 128 bytes (rows of 32 elements either way)
        (plan(CHEAP, 65536, 31, "LM", 0, 0, 32, 32), "stream_lane_major<", None), (plan(CHEAP, 65536, 32, "LM", 0, 0, 32, 32), "stream_lane_major_staged<", None),
    ])


# ------------------------------------------------------------------------------------------------ lane thresholds, value - 4 and value
def test_lane_thresholds_cheap(cli):
    ns, ds = "IDSP_DIAG=1", "IDSP_NO_SWEEP=1"
    check(cli, [
        # kSweepMinLanesFps (lane_stream.h:1796, :1808); below it the staged kernel, rows off the 64-byte grid (24572 * 4 % 64 = 48)
        (plan(CHEAP, 24572), STAGED % 32, None), (plan(CHEAP, 24576), SWEEP + "1 block/workgroup]<", None),
        # kSweepMinLanes is the 8-byte outputs' (no LDS-eligible 8-byte processor among the trait sets); for 4-byte outputs 49152 is
        # kStagedMaxLanes (lane_stream.h:1825), reached with the sweep switched off
        (plan(CHEAP, 49148), SWEEP_X % "1 block", None), (plan(CHEAP, 49152), SWEEP + "1 block/workgroup]<", None),
        (plan(CHEAP, 49148, 32, "FM", 0, 0, 0, 0, ns, ds), STAGED % 64, None), (plan(CHEAP, 49152, 32, "FM", 0, 0, 0, 0, ns, ds), LDS, None),
        # kSweepOffGridSmallMax (lane_stream.h:1807), rows off the grid by pitch / by lane count
        (plan(CHEAP, 53244), SWEEP_X % "1 block", None), (plan(CHEAP, 53248, 32, "FM", 0, 0, 53252, 53252), SWEEP_X % "1 block", None),
        (plan(CHEAP, 53252), LDS_X, None),
        # kLdsGridCap * 256 = 98304 (lane_stream.h:1804, :1807 `lanes > off_grid_min`)
        (plan(CHEAP, 98300), LDS_X, None), (plan(CHEAP, 98304, 32, "FM", 0, 0, 98308, 98308), LDS_X, None), (plan(CHEAP, 98304), SWEEP + "2 blocks/workgroup]<", None),
        (plan(CHEAP, 98308), SWEEP_X % "2 blocks", None),
        # kStagedHeavyMinLanes / MaxLanes do not bind a cheap processor (lane_stream.h:1825)
        (plan(CHEAP, 12284), STAGED % 32, None), (plan(CHEAP, 12288), STAGED % 32, None),
        (plan(CHEAP, 40956), SWEEP_X % "1 block", None), (plan(CHEAP, 40960), SWEEP + "1 block/workgroup]<", None),
        # kStaged64Lanes on the 64-byte grid, kStaged64LanesOffGrid off it, kStaged32Lanes (lane_stream.h:1834)
        (plan(CHEAP, 24560, 32, "FM", 0, 0, 0, 0, ns, ds), STAGED % 32, None), (plan(CHEAP, 24576, 32, "FM", 0, 0, 0, 0, ns, ds), STAGED % 64, None),
        (plan(CHEAP, 24576, 32, "FM", 0, 0, 24580, 24580, ns, ds), STAGED % 32, None),
        (plan(CHEAP, 25596, 32, "FM", 0, 0, 0, 0, ns, ds), STAGED % 32, None), (plan(CHEAP, 25600, 32, "FM", 0, 0, 25604, 25604, ns, ds), STAGED % 64, None),
        (plan(CHEAP, 8188), STAGED % 16, None), (plan(CHEAP, 8192), STAGED % 32, None),
        # kPairMaxLanes (lane_stream.h:1775, :1779), rows on the 64-byte grid
        (plan(CHEAP, 24560, 512), PAIR, None), (plan(CHEAP, 24576, 512), PAIR, None), (plan(CHEAP, 24592, 512), SWEEP + "1 block/workgroup]<", None),
        (plan(CHEAP, 24580, 512), SWEEP_X % "1 block", None),
        # kLdsMinWaves = 256 waves (lane_stream.h:1871), 15 frames: no staged kernel
        (plan(CHEAP, 16320, 15), WINDOW, None), (plan(CHEAP, 16384, 15), LDS, None),
        # the lanes % 4 split's body (lane_stream.h:1718 `body >= 8192`)
        (plan(CHEAP, 8189), WINDOW, None), (plan(CHEAP, 8193), STAGED % 32, ODD),
        # LaneMajor: kLmStaged64Lanes, kLmStaged32Lanes (lane_stream.h:1659)
        (plan(CHEAP, 49148, 4096, "LM"), "stream_lane_major_staged[32 lanes/wave]<", None), (plan(CHEAP, 49152, 4096, "LM"), "stream_lane_major_staged<", None),
        (plan(CHEAP, 24572, 4096, "LM"), "stream_lane_major_staged[16 lanes/wave]<", None), (plan(CHEAP, 24576, 4096, "LM"), "stream_lane_major_staged[32 lanes/wave]<", None),
    ])


def test_lane_thresholds_heavy(cli):
    """PllProc: COST 160 — no split, no pair, not LDS-eligible: the staged kernel inside its window (32 lanes per wave only), else the register window"""
    check(cli, [
        (plan(HEAVY, 24572), STAGED % 32, None), (plan(HEAVY, 24576), STAGED % 32, None), (plan(HEAVY, 24576, 512), STAGED % 32, None),
        (plan(HEAVY, 49148), WINDOW, None), (plan(HEAVY, 49152), WINDOW, None), (plan(HEAVY, 53244), WINDOW, None), (plan(HEAVY, 53248), WINDOW, None),
        (plan(HEAVY, 98300), WINDOW, None), (plan(HEAVY, 98304), WINDOW, None), (plan(HEAVY, 65536 + T["kSplitTailMax"]), WINDOW, None),
        # kStagedHeavyMinLanes, kStagedHeavyMaxLanes (lane_stream.h:1825)
        (plan(HEAVY, 12284), WINDOW, None), (plan(HEAVY, 12288), STAGED % 32, None), (plan(HEAVY, 40956), STAGED % 32, None), (plan(HEAVY, 40960), WINDOW, None),
        (plan(HEAVY, 8188), WINDOW, None), (plan(HEAVY, 8192), WINDOW, None), (plan(HEAVY, 16384, 15), WINDOW, None),
        # the lanes % 4 split takes any 4-byte processor the staged kernel takes (lane_stream.h:1718)
        (plan(HEAVY, 12289), STAGED % 32, ODD), (plan(HEAVY, 8193), WINDOW, ODD),
        # LaneMajor (lane_stream.h:1659, :1678-1684): 32 lanes per wave below kLmStaged64Lanes, never 16
        (plan(HEAVY, 49148, 4096, "LM"), "stream_lane_major_staged[32 lanes/wave]<", None), (plan(HEAVY, 49152, 4096, "LM"), "stream_lane_major_staged<", None),
        (plan(HEAVY, 24572, 4096, "LM"), "stream_lane_major_staged[32 lanes/wave]<", None), (plan(HEAVY, 24576, 4096, "LM"), "stream_lane_major_staged[32 lanes/wave]<", None),
    ])
    # the register-window kernel's own thresholds (lane_stream.h:1955, :1964): 64-thread workgroups below 1024 waves, the deep window up to 2048
    d = details(cli, [plan(HEAVY, 65472), plan(HEAVY, 65476), plan(HEAVY, 131072), plan(HEAVY, 131076)])
    assert [(x["block"], x["deep_window"]) for x in d] == [("64", "1"), ("256", "1"), ("256", "1"), ("256", "0")], d


def test_other_processors(cli):
    check(cli, [
        # 8-byte output, not LDS-eligible, no staged kernel (sample sizes differ): the register window, the tile kernel
        (plan("unwrap_i64", 65536), WINDOW, None), (plan("unwrap_i64", 16384), WINDOW, None), (plan("unwrap_i64", 65537), WINDOW, None),
        (plan("unwrap_i64", 65536, 4096, "LM"), "stream_lane_major<", None),
        # IN_DIV == 2: two threads per input lane — none of the 4-byte kernels (x rows hold lanes / 2 samples)
        (plan("lockin_split", 65536), WINDOW, None), (plan("lockin_split", 3, 64), WINDOW, None), (plan("lockin_split", 65537), WINDOW, None),
        (plan("lockin_split", 65536, 4096, "LM"), "stream_lane_major<", None),
        # 8-byte samples in and out: the staged kernel takes them (whole 16-byte pieces: an even lane count), nothing else does
        (plan("rpll", 16384), STAGED % 32, None), (plan("rpll", 16385), WINDOW, None), (plan("rpll", 65536), WINDOW, None),
    ])


# ------------------------------------------------------------------------------------------------ the two splits
def test_rounds_split(cli):
    tail = T["kSplitTailMax"]
    check(cli, [
        # lane_stream.h:1744 `tail <= kSplitTailMax`
        (plan(CHEAP, 65536 + tail), ROUNDS % "sweep", None), (plan(CHEAP, 65536 + tail + 4), LDS_X, None),
        # :1743 whole rounds on the sweep kernel only as 1, 2, 4, 8, 16: three rounds are one sweep over everything
        (plan(CHEAP, 3 * 65536 + 8192), SWEEP + "4 blocks/workgroup]<", None), (plan(CHEAP, 2 * 65536 + 8192), ROUNDS % "sweep", None),
        # ... a processor the sweep does not take at `head` lanes (4 blocks per workgroup at most: 5 x 65536 lanes would be two narrow sweeps) keeps the split
        (plan("clamp_wrap", 5 * 65536 + 8192), ROUNDS % "lds", None),
        # :1744 `!diag_on()`; :1746 no second stream: the unsplit forms
        (plan(CHEAP, 65552, 32, "FM", 0, 0, 0, 0, "IDSP_DIAG=1"), SWEEP + "2 blocks/workgroup]<", None),
        (plan(CHEAP, 65552, 32, "FM", 0, 0, 0, 0, "no_side_stream"), SWEEP + "2 blocks/workgroup]<", None),
        (plan(CHEAP, 65537, 32, "FM", 0, 0, 0, 0, "no_side_stream"), WINDOW, None),
        # :1779 `!split_remainder_flag()`: the remainder of a split keeps the staged kernel where the same call alone takes the pair kernel
        (plan(CHEAP, 16384, 512), PAIR, None), (plan(CHEAP, 16384, 512, "FM", 0, 0, 0, 0, "remainder"), STAGED % 32, None),
        # whole rounds whose rows are off the 64-byte grid (dense 65540 / 131076 lanes): round 3's kernel below 98304 lanes, the sweep above
        (plan(CHEAP, 65540), ROUNDS % "lds", None), (plan(CHEAP, 131076), ROUNDS % "sweep", None),
    ])
    d = details(cli, [plan(CHEAP, 65536 + tail), plan(CHEAP, 131076)])
    assert [(x["head"], x["tail"]) for x in d] == [("65536", str(tail)), ("131072", "4")], d


# ------------------------------------------------------------------------------------------------ rows off the grids
def test_rows_off_the_grids(cli):
    rows = []
    want = {16384: STAGED % 32, 32768: SWEEP_X % "1 block", 65536: LDS_X, 131072: SWEEP_X % "2 blocks"}
    for lanes, k in want.items():
        # by base: off the 64-byte grid, off the 16-byte grid (x, then y); by pitch: + 1 and + 4 elements (lane_stream.h:1707-1709, :1799-1808, :1831, :1932)
        rows += [(plan(CHEAP, lanes, 32, "FM", 16, 0), k, None), (plan(CHEAP, lanes, 32, "FM", 4, 0), k, None), (plan(CHEAP, lanes, 32, "FM", 0, 12), k, None),
                 (plan(CHEAP, lanes, 32, "FM", 0, 0, lanes + 1, lanes + 1), k, None), (plan(CHEAP, lanes, 32, "FM", 0, 0, lanes + 4, lanes + 4), k, None),
                 (plan(CHEAP, lanes, 32, "FM", 0, 0, lanes, lanes + 4), k, None)]
        # dense tensors of lanes + 1 lanes: the last lane beside the rest
        rows.append((plan(CHEAP, lanes + 1), k, ODD))
    rows += [
        # dense tensors of lanes + 4 lanes
        (plan(CHEAP, 16388), STAGED % 32, None), (plan(CHEAP, 32772), SWEEP_X % "1 block", None), (plan(CHEAP, 65540), ROUNDS % "lds", None),
        (plan(CHEAP, 131076), ROUNDS % "sweep", None),
        # the pair kernel wants the 64-byte grid (lane_stream.h:1778)
        (plan(CHEAP, 16384, 512, "FM", 16, 0), STAGED % 32, None), (plan(CHEAP, 16384, 512, "FM", 0, 0, 16388, 16388), STAGED % 32, None),
        # IDSP_ALIGN16_ONLY (lane_stream.h:1706-1709): rows off the 16-byte grid on the register-window kernel, no lanes % 4 split
        (plan(CHEAP, 65536, 32, "FM", 4, 0, 0, 0, "IDSP_DIAG=1", "IDSP_ALIGN16_ONLY=1"), WINDOW, None),
        (plan(CHEAP, 65536, 32, "FM", 16, 0, 0, 0, "IDSP_DIAG=1", "IDSP_ALIGN16_ONLY=1"), LDS_X, None),
        (plan(CHEAP, 65537, 32, "FM", 0, 0, 0, 0, "IDSP_DIAG=1", "IDSP_ALIGN16_ONLY=1"), WINDOW, None),
        # LaneMajor (lane_stream.h:1648-1650): 16-byte pieces need 16-byte aligned rows
        (plan(CHEAP, 65536, 4096, "LM", 16, 0), "stream_lane_major_staged<", None), (plan(CHEAP, 65536, 4096, "LM", 4, 0), "stream_lane_major<", None),
        (plan(CHEAP, 65536, 4096, "LM", 0, 8), "stream_lane_major<", None), (plan(CHEAP, 65536, 4096, "LM", 0, 0, 4097, 4097), "stream_lane_major<", None),
        (plan(CHEAP, 65536, 4096, "LM", 0, 0, 4100, 4100), "stream_lane_major_staged<", None),
        # ... of less than 64 MiB (:1648), FrameMajor staged rows of less than 256 MiB (:1827)
        (plan(CHEAP, 64, 1 << 24, "LM"), "stream_lane_major<", None), (plan(CHEAP, 64, (1 << 24) - 4, "LM"), "stream_lane_major_staged[16 lanes/wave]<", None),
        (plan(CHEAP, 16384, 32, "FM", 0, 0, 1 << 26, 1 << 26), LDS, None), (plan(CHEAP, 16384, 32, "FM", 0, 0, (1 << 26) - 16, (1 << 26) - 16), STAGED % 32, None),
    ]
    check(cli, rows)
    # several frames per segment: 32768 lanes in 256 blocks of 128 (fm_sweep.h:594-599), brought down by the 32-bit guard on rows of gigabytes
    got = names(cli, [plan(CHEAP, 32768, 32, "FM", 16, 0), plan(CHEAP, 32768), plan(CHEAP, 32768, 32, "FM", 0, 0, 1 << 27, 1 << 27), plan(CHEAP, 65536)])
    assert got[0].endswith(" [2 frames/segment]") and got[1].endswith(" [2 frames/segment]") and got[2].endswith(" [1 frame/segment]") and got[3].endswith(">"), got
    # the staged kernel off the 64-byte grid: XCD-contiguous lane blocks from 64 workgroups, plain accesses (lane_stream.h:1846)
    d = details(cli, [plan(CHEAP, 16384), plan(CHEAP, 16384, 32, "FM", 16, 0), plan(CHEAP, 1024, 32, "FM", 16, 0)])
    assert [(x["grid"], x["staged_flags"]) for x in d] == [("512", "0"), ("512", "3"), ("64", "3")], d
    d = details(cli, [plan(CHEAP, 1008, 32, "FM", 16, 0)])
    assert (d[0]["grid"], d[0]["staged_flags"]) == ("63", "2"), d


# ------------------------------------------------------------------------------------------------ switches
def test_switches(cli):
    def sw(traits, lanes, frames, layout, *flags):
        return plan(traits, lanes, frames, layout, 0, 0, 0, 0, "IDSP_DIAG=1", *flags)

    check(cli, [
        # IDSP_LDS_COST=n: `COST <= n` instead of LDS_ELIGIBLE, and no sweep kernel (lane_stream.h:1797, :1863-1865)
        (sw("unwrap_i64", 65536, 32, "FM"), WINDOW, None), (sw("unwrap_i64", 65536, 32, "FM", "IDSP_LDS_COST=120"), LDS, None),
        (sw(CHEAP, 65536, 32, "FM", "IDSP_LDS_COST=120"), LDS, None), (sw(CHEAP, 65536, 32, "FM", "IDSP_LDS_COST=10"), WINDOW, None),
        # IDSP_LDS_MIN_WAVES (lane_stream.h:1589, :1871)
        (sw(CHEAP, 8192, 15, "FM"), WINDOW, None), (sw(CHEAP, 8192, 15, "FM", "IDSP_LDS_MIN_WAVES=128"), LDS, None),
        # IDSP_LM_LANES_PER_WAVE (lane_stream.h:1653, :1678-1684: a heavy processor has no 16-lane form)
        (sw(CHEAP, 65536, 4096, "LM"), "stream_lane_major_staged<", None), (sw(CHEAP, 65536, 4096, "LM", "IDSP_LM_LANES_PER_WAVE=16"), "stream_lane_major_staged[16 lanes/wave]<", None),
        (sw(CHEAP, 16384, 4096, "LM", "IDSP_LM_LANES_PER_WAVE=64"), "stream_lane_major_staged<", None),
        (sw(HEAVY, 65536, 4096, "LM", "IDSP_LM_LANES_PER_WAVE=16"), "stream_lane_major_staged[32 lanes/wave]<", None),
        (sw(CHEAP, 65536, 4096, "LM", "IDSP_NO_LM_STAGED=1"), "stream_lane_major<", None),
        # IDSP_FM_LANES_PER_WAVE forces the staged kernel at any lane count (lane_stream.h:1822, :1826) — behind the sweep, which comes first
        (sw(CHEAP, 16384, 32, "FM", "IDSP_FM_LANES_PER_WAVE=64"), STAGED % 64, None), (sw(CHEAP, 16384, 32, "FM", "IDSP_FM_LANES_PER_WAVE=16"), STAGED % 16, None),
        (sw(CHEAP, 65536, 32, "FM", "IDSP_FM_LANES_PER_WAVE=16"), SWEEP, None), (sw(CHEAP, 65536, 32, "FM", "IDSP_FM_LANES_PER_WAVE=16", "IDSP_NO_SWEEP=1"), STAGED % 16, None),
        (sw(HEAVY, 65536, 32, "FM", "IDSP_FM_LANES_PER_WAVE=16"), STAGED % 32, None),
        # IDSP_NO_FM_PAIR, IDSP_FM_PAIR_MAX_LANES (lane_stream.h:1774-1775)
        (sw(CHEAP, 16384, 512, "FM"), PAIR, None), (sw(CHEAP, 16384, 512, "FM", "IDSP_NO_FM_PAIR=1"), STAGED % 32, None),
        (sw(CHEAP, 16384, 512, "FM", "IDSP_FM_PAIR_MAX_LANES=8192"), STAGED % 32, None),
        # IDSP_NO_FM_STAGED (lane_stream.h:1821), IDSP_NO_FM_FEW (:1711)
        (sw(CHEAP, 16384, 32, "FM", "IDSP_NO_FM_STAGED=1"), LDS, None), (sw(CHEAP, 3, 64, "FM", "IDSP_NO_FM_FEW=1"), WINDOW, None),
        # IDSP_NO_LDS_PATH: neither LDS-DMA kernel (lane_stream.h:1797, :1867), IDSP_NO_SWEEP (:1795)
        (sw(CHEAP, 65536, 32, "FM", "IDSP_NO_LDS_PATH=1"), WINDOW, None), (sw(CHEAP, 65536, 32, "FM", "IDSP_NO_SWEEP=1"), LDS, None),
        # IDSP_SWEEP_MAX_GRID (fm_sweep.h:570-572, :589): 64 workgroups cover 65536 lanes with 4 blocks each; capped, several narrow sweeps are taken too
        (sw(CHEAP, 65536, 32, "FM", "IDSP_SWEEP_MAX_GRID=64"), SWEEP + "4 blocks/workgroup]<", None),
        (sw("i32_df1_x3", 1 << 18, 32, "FM", "IDSP_SWEEP_MAX_GRID=255"), SWEEP + "2 blocks/workgroup]<", None),
        # IDSP_SWEEP_MIN_LANES (lane_stream.h:1796), IDSP_SWEEP_OFFGRID_MIN_LANES (:1804), IDSP_SWEEP_GRID64_ONLY (:1798)
        (sw(CHEAP, 16384, 32, "FM", "IDSP_SWEEP_MIN_LANES=16384"), SWEEP + "1 block/workgroup]<", None),
        (sw(CHEAP, 32768, 32, "FM", "IDSP_SWEEP_MIN_LANES=49152"), STAGED % 64, None),
        (plan(CHEAP, 65536, 32, "FM", 16, 0, 0, 0, "IDSP_DIAG=1"), LDS_X, None),
        (plan(CHEAP, 65536, 32, "FM", 16, 0, 0, 0, "IDSP_DIAG=1", "IDSP_SWEEP_OFFGRID_MIN_LANES=32768"), SWEEP_X % "1 block", None),
        (plan(CHEAP, 131072, 32, "FM", 16, 0, 0, 0, "IDSP_DIAG=1", "IDSP_SWEEP_GRID64_ONLY=1"), LDS_X, None),
        # block order (fm_sweep.h:583-585; lane_stream.h:1931, :1961)
        (plan(CHEAP, 131072, 32, "FM", 16, 0, 0, 0, "IDSP_DIAG=1", "IDSP_SWEEP_NO_XCDC=1"), SWEEP + "2 blocks/workgroup]<", None),
        (sw(CHEAP, 131072, 32, "FM", "IDSP_SWEEP_FORCE_XCDC=1"), SWEEP_X % "2 blocks", None),
        (plan(CHEAP, 65536, 32, "FM", 16, 0, 0, 0, "IDSP_DIAG=1", "IDSP_LDS_NO_XCDC=1"), LDS, None),
        (sw(HEAVY, 65536, 32, "FM", "IDSP_FM_XCDC=1"), "stream_frame_major[XCD-contiguous blocks]<", None),
        # ... from 64 workgroups on the register-window kernel (lane_stream.h:1962), from 8 on the sweep kernel (fm_sweep.h:608): 64 lanes off the
        # grid are 4 blocks of 16, 128 lanes 8
        (sw(HEAVY, 4032, 32, "FM", "IDSP_FM_XCDC=1"), WINDOW, None), (sw(HEAVY, 4096, 32, "FM", "IDSP_FM_XCDC=1"), "stream_frame_major[XCD-contiguous blocks]<", None),
        (plan(CHEAP, 64, 32, "FM", 16, 0, 0, 0, "IDSP_DIAG=1", "IDSP_SWEEP_MIN_LANES=16"), SWEEP + "1 block/workgroup]<", None),
        (plan(CHEAP, 128, 32, "FM", 16, 0, 0, 0, "IDSP_DIAG=1", "IDSP_SWEEP_MIN_LANES=16"), SWEEP_X % "1 block", None),
    ])
    # a switch without IDSP_DIAG=1 is not honoured (common.h `diag_env`)
    check(cli, [(plan(CHEAP, 16384, 512, "FM", 0, 0, 0, 0, "IDSP_NO_FM_PAIR=1"), PAIR, None), (plan(CHEAP, 16384, 512, "FM", 0, 0, 0, 0, "IDSP_DIAG=0", "IDSP_NO_FM_PAIR=1"), PAIR, None)])
    # IDSP_LDS_GRID (lane_stream.h:1879, :1897-1902): 512 blocks are a persistent grid of 256 workgroups — on 7 tiles for a processor tuned to
    # another ring depth (:1944) — unless the switch asks for one workgroup per block (0) or another cap
    base = ("IDSP_DIAG=1", "IDSP_NO_SWEEP=1")
    d = details(cli, [plan(CHEAP, 131072, 32, "FM", 0, 0, 0, 0, *base), plan("i32_df1_x2", 131072, 32, "FM", 0, 0, 0, 0, *base),
                      plan("i32_df1_x2", 131072, 32, "FM", 0, 0, 0, 0, *base, "IDSP_LDS_GRID=0"), plan("i32_df1_x2", 131072, 32, "FM", 0, 0, 0, 0, *base, "IDSP_LDS_GRID=128"),
                      plan("i32_df1_x2", 98304, 32, "FM", 0, 0, 0, 0, *base), plan("i32_df1_x2", 98560, 32, "FM", 0, 0, 0, 0, *base)])
    assert [(x["grid"], x["deep_ring"]) for x in d] == [("256", "0"), ("256", "1"), ("512", "0"), ("128", "1"), ("384", "0"), ("193", "1")], d
    # IDSP_SWEEP_NO_FPS (fm_sweep.h:593)
    got = names(cli, [sw(CHEAP, 32768, 32, "FM"), sw(CHEAP, 32768, 32, "FM", "IDSP_SWEEP_NO_FPS=1")])
    assert got[0].endswith(" [2 frames/segment]") and got[1].endswith(">"), got


# ------------------------------------------------------------------------------------------------ sweep_geometry, duo_wanted
def test_sweep_geometry_and_duo(cli):
    # the three shapes the sweep kernel's header comment quotes (fm_sweep.h:20)
    assert cli(["geom 65536 16", "geom 100000 16", "geom 1048576 16", "geom 12 16", "geom 1048576 8"]) == \
        ["256 x 1 x 256, 1", "241 x 2 x 208, 1", "256 x 16 x 256, 1", "none", "256 x 8 x 256, 2"]
    lo, hi4 = T["kDuoMinLanes"], T["kDuo4MaxLanes"]
    # lane_stream.h:1988-1993
    assert cli(["duo 5 %d FM" % (lo - 4), "duo 5 %d FM" % lo, "duo 4 %d FM" % lo, "duo 3 %d FM" % lo, "duo 4 %d FM" % hi4, "duo 4 %d FM" % (hi4 + 4), "duo 8 %d FM" % (hi4 + 4),
                "duo 5 %d LM" % lo, "duo 5 %d FM IDSP_DIAG=1 IDSP_NO_DUO=1" % lo, "duo 5 %d FM IDSP_NO_DUO=1" % lo]) == ["0", "1", "1", "0", "1", "0", "1", "0", "0", "1"]


# ------------------------------------------------------------------------------------------------ against the Python restatement
FORMS = {"clamp": "clamp_wrap", "pll0": "pll", "unwrap1": "unwrap_i64", "rpll": "rpll"}  # form of _stream_proc_cases.py -> trait set of the program


def test_agrees_with_the_python_restatement(cli):
    """`expected_kernel` of tests/_stream_proc_cases.py was written from the launcher's source before the choice moved, and the GPU holds the
    real processors to it: plan_stream has to give the same name, suffix included, for dense calls around every threshold"""
    lanes_near = sorted({t + d for t in (4, 8192, 12288, 16384, 24576, 25600, 32768, 40960, 49152, 53248, 65536, 65536 + T["kSplitTailMax"], 98304, 131072,
                                        196608, 262144, 327680, 1 << 20) for d in (-4, -3, -1, 0, 1, 4)} | {1, 2, 3, 1000, 100000})
    cases = [(f, lay, lanes, frames, xo, yo) for f in FORMS for lay in ("FM", "LM") for lanes in lanes_near
             for frames in ((1, 15, 16, 63, 64, 511, 512) if lay == "FM" else (16, 31, 32, 4096))
             for xo, yo in ((0, 0), (16, 0), (0, 4)) if lanes > 0]
    got = names(cli, [plan(FORMS[f], lanes, frames, lay, xo, yo) for f, lay, lanes, frames, xo, yo in cases])
    bad = []
    for (f, lay, lanes, frames, xo, yo), k in zip(cases, got):
        e = SP.expected_kernel(f, SP.FM if lay == "FM" else SP.LM, lanes, frames, xo, yo)
        want = str(e) + FORMS[f] + ">" + e.suffix
        if k != want:
            bad.append(((f, lay, lanes, frames, xo, yo), k, want))
    assert not bad, (len(bad), bad[:5])
