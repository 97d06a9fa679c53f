// dispatch_thresholds.h — every lane-count / frame-count threshold the launchers of the lane-streaming families branch on, in ONE place
// (round 5; VERDICT round 4, "upkeep").  Each was measured on MI355X boxes that differ by 3-5 %, so none of them is sharp; the file each
// comes from is named, profiles/NOTES.md has the numbers, and tests/test_gpu_dispatch_table.py pins the kernel taken at every BASELINE
// shape and on both sides of every cliff listed here; tests/test_stream_plan.py pins the same table and both sides of every threshold without
// a GPU, through `plan_stream` (stream_plan.h), which is the one reader of what follows — but for the lock-in section, whose one reader is
// `plan_lockin` (lockin_plan.h; tests/test_lockin_plan.py pins both sides of each of its names the same way), for the half-band and Cic
// sections, read by `plan_hbf` / `plan_cic` (resample_plan.h; tests/test_resample_plan.py), and for the last section, read by `plan_fm_disc` /
// `plan_dds` (readout_plan.h; tests/test_fm_disc_plan.py), which also read the stagger section's window and its kFmDiscStaggerTicks.
#pragma once

#include <cstddef>
#include <cstdint>

namespace idsp {
namespace thr {

// ---- FrameMajor, 4-byte inputs (launch_stream, lane_stream.h) ----------------------------------------------------------------------
// dense-sweep LDS-DMA kernel (fm_sweep.h) from this many lanes up: 8-byte outputs / 4-byte outputs (several frames per segment)
constexpr size_t kSweepMinLanes = 49152, kSweepMinLanesFps = 24576;
// ... and from this many frames up (shorter calls: the round-3 LDS-DMA kernel or the staged kernel)
constexpr size_t kSweepMinFrames = 16;
// ... and only when the launch is one sweep, or its sweeps are at least this many blocks per workgroup wide (fm_sweep.h `sweep_takes`; a processor's
// largest count is its SWEEP_MAX_LPT: 16 single biquad sections, 8 `Normal` / per-lane banks / two-section chains, 4 and 2 cascades and longer chains)
constexpr int kSweepMinLptSeveralSweeps = 8;
// rows off the 64-byte grid take the sweep kernel only above the largest single-round grid of the round-3 LDS-DMA kernel
constexpr size_t kLdsGridCap = 384;  // workgroups of 256 lanes: 98304 lanes
// ... and up to this many lanes (below: several frames per segment against the staged single-wave kernel; in between round 3's XCD-contiguous LDS-DMA kernel)
constexpr size_t kSweepOffGridSmallMax = 53248;
// "whole rounds + remainder on a second stream": remainders up to this many lanes, whole rounds of 1, 2, 4, 8 or 16 x 65536 lanes
constexpr size_t kSplitTailMax = 20480;
// staged single-wave kernel below kSweepMinLanes*: cheap processors below this lane count, heavy ones (COST > 120) inside the window
constexpr size_t kStagedMaxLanes = 49152, kStagedHeavyMinLanes = 12288, kStagedHeavyMaxLanes = 40960;
// ... lanes per wave: 64 from here (rows on / off the 64-byte grid), 32 from here, else 16
constexpr size_t kStaged64Lanes = 24576, kStaged64LanesOffGrid = 25600, kStaged32Lanes = 8192;
// compute + mover pair kernel (stream_frame_major_pair, round 6): cheap sections (COST <= kPairMaxCost) UP TO this lane count — 768 workgroups of 32 lanes and
// 32 KiB of LDS, three per CU, ahead of the sweep kernel's several-frames-per-segment form (24576 lanes 0.175 against 0.192 ms; 28672 lanes would be a second
// generation: 0.217 against 0.194) — from this many frames (four tiles; 512 frames 0.0174 against 0.0194 ms at 16384 lanes: profiles/r06_exp_fm_pair.txt)
constexpr size_t kPairMaxLanes = 24576, kPairMinFrames = 512;
constexpr int kPairMaxCost = 60;
// smallest launch (in 64-lane waves) of the round-3 LDS-DMA kernel
constexpr size_t kLdsMinWaves = 256;
// two-wave chain kernel (stream_frame_major_duo): from this many lanes, chains of 5+ sections (4 sections up to kDuo4MaxLanes)
constexpr size_t kDuoMinLanes = 40960, kDuo4MaxLanes = 98304;

// a processor is "heavy" (VALU-bound: half-empty waves cost arithmetic) above this COST estimate; also the default LDS-DMA eligibility
constexpr int kHeavyCost = 120;
// one to three lanes in all on stream_frame_major_few, from this many frames (a tile is 256)
constexpr size_t kFewMaxLanes = 3, kFewMinFrames = 64;
// "lanes % 4 on a second stream": bodies from this many lanes, calls from this many frames
constexpr size_t kOddSplitMinBody = 8192, kOddSplitMinFrames = 16;
// "whole rounds + remainder": from this many frames; whole rounds on the sweep kernel only as a power of two up to this many rounds of 65536 lanes
constexpr size_t kRoundsSplitMinFrames = 16, kRoundsSplitMaxRounds = 16;
// staged single-wave kernel: from this many frames; XCD-contiguous lane blocks on rows off the 64-byte grid from this many workgroups
constexpr size_t kStagedMinFrames = 16, kStagedXcdcMinGrid = 64;
// sweep kernel: XCD-contiguous block order from this many workgroups; several frames per segment up to this many lanes per block
constexpr size_t kSweepXcdcMinGrid = 8, kSweepFpsMaxBlockLanes = 128;
// register-window kernel: 256-thread workgroups from this many waves (below: one wave per workgroup, to reach all 256 CUs), the deep
// prefetch window up to this many waves, XCD-contiguous blocks (a diagnostic switch) from this many workgroups
constexpr size_t kWindowBlockMinWaves = 1024, kWindowDeepMaxWaves = 2048, kWindowXcdcMinGrid = 64;

// ---- LaneMajor (launch_stream) -----------------------------------------------------------------------------------------------------
// staged kernel, lanes per wave: 64 from here, 32 from here (or COST > 120), else 16
constexpr size_t kLmStaged64Lanes = 49152, kLmStaged32Lanes = 24576;
// ... from this many bytes per row on the wider side (a quarter of the staged kernel's 512-byte run: below, the tile kernel has less to set up)
constexpr size_t kLmStagedMinRowBytes = 128;

// ---- start-up stagger of the line-wise LaneMajor kernels (lockin_waves.h, fm_disc.hip; MI355X in SPX mode only: stagger_tuned_device()) --
constexpr unsigned kStaggerMinWorkgroups = 512;                     // launches of at least two workgroups per CU
constexpr size_t kStaggerMinFrames = 2048, kStaggerMaxFrames = 8192;  // long enough to pay, short enough not to drift apart anyway
constexpr unsigned kLockinStaggerTicks = 600, kFmDiscStaggerTicks = 1200;  // 10 ns ticks between the four CU groups of an XCD

// ---- half-band (plan_hbf, resample_plan.h; tests/test_resample_plan.py pins both sides of each name of this section and the next) ----
// Kernel geometry, not measured cliffs: what the kernels of the two resampling families are built for.  (Fixed-width types: the constants of the
// other sections, `size_t` / `int` / `unsigned`, are what tests/_stream_proc_cases.py collects as the stream launcher's thresholds.)
// the vector kernels of both resampling families move whole 16-byte pieces: the wide buffer (x of a decimator, y of an interpolator)
// starts on this grid, and so does every LaneMajor row of it
constexpr uint64_t kPieceBytes = 16;
// kernels of one workgroup per lane (or per lane group) keep the lane count inside a 31-bit grid; the lane-per-thread kernels take the rest
constexpr uint64_t kGridMaxLanes = 0x7fffffff;
// FrameMajor: a frame of at least one piece, 2^stages floats — from this many stages; one stage stays on the generic kernel
constexpr int32_t kHbfFmMinStages = 2;
// the LDS-DMA ring decimator (hbf_ring.h) exists for /16 only, on whole groups of this many lanes
constexpr int32_t kHbfRingStages = 4;
constexpr uint64_t kHbfRingLanes = 16;
// hbf_dec_block_fm / hbf_int_block_fm (hbf_wave.h): whole workgroups of this many lanes, else the wave-per-lane kernel
constexpr uint64_t kHbfBlockLanes = 4;

// ---- Cic (plan_cic, resample_plan.h) ---------------------------------------------------------------------------------------------------
// wave-per-lane ring kernels (cic_ring.h): a chunk of rate + 1 samples is 1, 2, 4 or 8 whole pieces, at least one whole block of 64 chunks
// (below that the lane-per-thread kernels have as much parallelism and less to set up); FrameMajor (interpolator) on whole groups of 16 lanes
constexpr uint64_t kCicRingMinChunkBytes = 16, kCicRingMaxChunkBytes = 128;
constexpr uint64_t kCicRingMinFrames = 64;
constexpr uint64_t kCicRingFmLanes = 16;
// lane-per-thread kernels (cic_kernels.h): blocks of 64 lanes; chunks of 1, 2, 4, 8 or 16 whole vectors are moved as vectors, and the
// LaneMajor tile form moves 64 lanes x 16 vectors through LDS: whole blocks, at least one whole tile
constexpr uint64_t kCicBlockLanes = 64;
constexpr uint64_t kCicTileVecs = 16;

// ---- lock-in (plan_lockin, lockin_plan.h; the measurements are quoted where each is read) ------------------------------------------
// largest lane count that still runs the I and Q arms on two threads of the stream kernels (IDSP_SPLIT_MAX_LANES overrides); the multi-wave
// kernel's 16-frame batches and the six-wave form of the `arg` read-out end at the same count
constexpr size_t kSplitMaxLanes = 40960;
// FrameMajor up to one workgroup per CU: six waves per 64 lanes with 16-frame batches; the stage-wave kernel with one lane group per workgroup
constexpr size_t kLockinSixWavesMaxLanes = 16384, kLockinStagesOneGroupMaxLanes = 16384;
// ... above, six waves for the `arg` read-out only while an arm is lighter than this many second-order equivalents (order x cascade)
constexpr int kLockinSixWavesArmWeight = 6;
// four workgroups per CU (above the first, up to the second): 16-frame batches again
constexpr size_t kLockinB16MinLanes = 49152, kLockinB16MaxLanes = 65536;
// the multi-wave kernels keep 32-bit thread offsets inside a row: fewer lanes than this (2^28)
constexpr size_t kLockinWavesMaxLanes = 268435456;
// LaneMajor rows that are not whole batches: body on the multi-wave kernel + tail on a stream kernel from this many frames
constexpr size_t kLockinTailMinFrames = 32;

// ---- FM discriminator and DDS (plan_fm_disc / plan_dds, readout_plan.h; tests/test_fm_disc_plan.py pins both sides of each name) -------
// (Fixed-width types, as in the half-band section.  plan_fm_disc also reads kPieceBytes for the two addresses and the stagger section.)
// FrameMajor role waves (fm_disc_waves_kernel, fm_disc.hip) UP TO this many lanes: beyond, the stream kernel has two waves per SIMD itself
// and fewer instructions per sample (no LDS hand-over, no second read of the previous row): 131072 lanes 1.40 ms against 1.52
// (profiles/r03_perf_fm_disc.jsonl)
constexpr uint64_t kFmDiscWavesMaxLanes = 81920;
// ... from this many frames: what one front wave takes of a tile
constexpr uint64_t kFmDiscFmMinFrames = 8;
// LaneMajor role waves (fm_disc_waves_lm_kernel) take whole tiles of this many frames, so rows of at least one ...
constexpr uint64_t kFmDiscLmTile = 32;
// ... of any multiple of this many frames (the last 16 of a row that is not whole tiles go to the tile kernel behind): multiples of 16 keep
// the input lines on the 128-byte grid; rows off it lose more to straddled lines than the role waves win (65536 lanes x 4100 / 4104 / 4124
// frames: 1.52 / 1.37 / 1.51 ms against 1.29 on the tile kernel; 4112 frames: 1.01)
constexpr uint64_t kFmDiscLmRowMultiple = 16;
// ... and keep 32-bit thread offsets inside a row: fewer lanes than this (2^28)
constexpr uint64_t kFmDiscLmMaxLanes = 268435456;
// DDS: the full-circle cossin table (16 KiB of LDS, filled at the start of every workgroup) for FrameMajor calls from this many frames,
// on the two-threads-per-lane form only (up to kSplitMaxLanes, lock-in section): one thread per lane runs 65536 lanes x 4096 in 0.36-0.37 ms
// on the 512-byte table and 0.46 on this one (profiles/r03_perf_dds_circle.jsonl, r03_perf_dds_one_circle.jsonl)
constexpr uint64_t kDdsCircleMinFrames = 256;

}  // namespace thr
}  // namespace idsp
