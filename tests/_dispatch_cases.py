"""The shape tables of the dispatch tests: which kernel `launch_stream` takes at every BASELINE shape and on both sides of every lane-count
cliff of idsp_amd/csrc/dispatch_thresholds.h.  tests/test_gpu_dispatch_table.py pins them on the GPU through `idsp_last_kernel()` with the real
processors; tests/test_stream_plan.py pins the same rows without one, through `plan_stream` (idsp_amd/csrc/stream_plan.h) and the hand-written
trait sets of tests/cpp/stream_plan_cli.cpp — so a wrong trait there shows up as a mismatch between the two.  Test infrastructure only."""

SWEEP = "stream_frame_major_sweep["
ODD = " + stream_frame_major_few (lanes % 4, second stream)"
# (lanes, expected start of the kernel name, expected end or None): i32 DF1, FrameMajor, dense rows
I32_FM = [
    (65536, SWEEP + "1 block/workgroup]<", None),                       # C2
    (131072, SWEEP + "2 blocks/workgroup]<", None),                     # C5 shard at 8 GPUs
    (262144, SWEEP + "4 blocks/workgroup]<", None),
    (524288, SWEEP + "8 blocks/workgroup]<", None),
    (1048576, SWEEP + "16 blocks/workgroup]<", None),                   # C5
    (100000, SWEEP + "2 blocks/workgroup]<", None),                     # narrow blocks (208 lanes)
    (65552, "stream_frame_major_sweep + stream_frame_major_staged (remainder, second stream)<", None),  # a little above one round
    (65537, "stream_frame_major_lds[XCD-contiguous blocks]<", ODD),     # cliff: rows off the grid, last lane beside
    (131073, SWEEP + "2 blocks/workgroup, XCD-contiguous]<", ODD),      # cliff: off the grid beyond 98304 lanes
    (49152, SWEEP + "1 block/workgroup]<", None),
    (32768, SWEEP + "1 block/workgroup]<", None),                       # several frames per segment
    (32769, SWEEP + "1 block/workgroup, XCD-contiguous]<", ODD),        # cliff: rows off the grid, several frames per segment up to 53248 lanes
    (24576, SWEEP + "1 block/workgroup]<", None),
    (24560, "stream_frame_major_staged[32 lanes/wave]<", None),         # below kSweepMinLanesFps
    (16384, "stream_frame_major_staged[32 lanes/wave]<", None),
    (8192, "stream_frame_major_staged[32 lanes/wave]<", None),
    (8176, "stream_frame_major_staged[16 lanes/wave]<", None),
]

# The rows of the other biquad tests of test_gpu_dispatch_table.py, as (trait set of stream_plan_cli.cpp, lanes, frames, layout, expected start,
# taken): `taken` False = the name must NOT start so.
# test_c5_and_lane_major_biquads
C5_AND_LANE_MAJOR = [
    ("f32_df2t", 1 << 20, 32, "FM", SWEEP + "16 blocks/workgroup]<", True),
    ("f32_df2t", 1 << 17, 32, "FM", SWEEP + "2 blocks/workgroup]<", True),
    ("i32_df1", 65536, 4096, "LM", "stream_lane_major_staged<", True),
    ("i32_df1", 32768, 4096, "LM", "stream_lane_major_staged[32 lanes/wave]<", True),
    ("i32_df1", 16384, 4096, "LM", "stream_lane_major_staged[16 lanes/wave]<", True),
]
# test_several_sweeps_per_launch_only_when_eight_blocks_wide (two-section chains: 8 blocks per workgroup, three: 2)
SEVERAL_SWEEPS = [
    ("i32_df1_x2", 1 << 19, 32, "FM", SWEEP + "8 blocks/workgroup]<", True),
    ("i32_df1_x2", 1 << 20, 32, "FM", SWEEP + "8 blocks/workgroup]<", True),   # two sweeps
    ("i32_df1_x3", 1 << 17, 32, "FM", SWEEP + "2 blocks/workgroup]<", True),
    ("i32_df1_x3", 1 << 18, 32, "FM", SWEEP, False),                           # would be two narrow sweeps
]
