// stream_plan.h — which kernel a call of `launch_stream<P>()` (lane_stream.h) takes, as ONE pure function.
//
// `plan_stream` reads three plain structs — what the launcher knows about the processor at compile time (StreamTraits), the call
// (StreamCall) and the diagnostic switches (StreamSwitches) — and returns the decision (StreamPlan).  The launcher does what the plan
// says and records the name `stream_plan_name` gives it; tests/test_stream_plan.py runs the same function through
// tests/cpp/stream_plan_cli.cpp without a GPU.  No HIP here: this header compiles with a plain C++17 host compiler.
// The measurements behind each branch: profiles/NOTES.md (the round each one came from is named there); thresholds: dispatch_thresholds.h.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstdlib>  // strtoull: the switches that carry a number

#include "idsp_hip.h"
#include "dispatch_thresholds.h"

namespace idsp {

constexpr size_t kPlanWave = 64, kPlanBlock = 256;        // lanes per wave / per LDS-DMA block (lane_stream.h asserts kWave / kFmBlock)
constexpr size_t kPlanRound = 256 * kPlanBlock;           // one round of the LDS-DMA kernels: a 256-lane block on each of 256 CUs
constexpr size_t kPlanSweepSegments = 8;                  // one-KiB segments per sweep tile (fm_sweep.h asserts kSweepT)

// What the choice reads from a processor P (lane_stream.h `traits_of<P>()` fills it from P and the detectors there)
struct StreamTraits {
    bool has_in = true;
    int in_div = 1;
    size_t in_bytes = 4, out_bytes = 4;
    int cost = 0;
    bool lds_eligible = true;     // LdsEligibleOf
    int lds_ring = 8;             // LdsRingOf
    bool fm_staged = true;        // FmStagedOf
    bool lm_staged = true;        // LmStagedOf
    bool lm_one_form = false;     // LmOneFormOf
    int sweep_max_lpt = 4;        // SweepMaxLptOf
    // one 4-byte sample in, one out: what the few / pair kernels and both splits take
    constexpr bool four_four() const { return has_in && in_div == 1 && in_bytes == 4 && out_bytes == 4; }
    // one 4-byte sample in: what the LDS-DMA kernels (round 3 and the sweep) take
    constexpr bool lds_input() const { return has_in && in_div == 1 && in_bytes == 4; }
    constexpr bool heavy() const { return cost > thr::kHeavyCost; }
};

struct StreamCall {
    size_t lanes = 0, frames = 0;
    int layout = IDSP_FRAME_MAJOR;
    uintptr_t x = 0, y = 0;               // the two addresses
    size_t pitch_x = 0, pitch_y = 0;      // elements between rows; 0 = dense
    size_t state_pitch = 0;               // lanes between the state planes; 0 = `lanes`
    bool remainder_of_split = false;      // this call is the remainder of a "whole rounds + remainder" split
    bool no_side_stream = false;          // the second stream is not to be had: the unsplit forms
};

// Where the rows of x and y sit, computed once per call.  (Every condition of the launcher that asked this before had fixed element sizes,
// so all of them were these predicates: see `stream_rows`.)
struct StreamRows {
    bool grid16 = false, grid64 = false;  // both base addresses and both byte pitches are multiples of 16 / 64
    bool below_2_26 = false;              // both byte pitches < 64 MiB: 32-bit offsets inside a LaneMajor wave's 64 rows
    bool below_2_28 = false;              // both byte pitches < 256 MiB: 32-bit offsets over up to 15 FrameMajor rows + 1 KiB
};
// (a processor without an input has no x rows: the LaneMajor staged kernel is the only reader for one)
inline StreamRows stream_rows(const StreamTraits &t, uintptr_t x, uintptr_t y, size_t xl, size_t yl)
{
    const size_t xb = t.has_in ? xl * t.in_bytes : 0, yb = yl * t.out_bytes;
    const uintptr_t xa = t.has_in ? x : 0;
    StreamRows r;
    r.grid16 = xa % 16 == 0 && y % 16 == 0 && xb % 16 == 0 && yb % 16 == 0;
    r.grid64 = xa % 64 == 0 && y % 64 == 0 && xb % 64 == 0 && yb % 64 == 0;
    r.below_2_26 = xb < (size_t(1) << 26) && yb < (size_t(1) << 26);
    r.below_2_28 = xb < (size_t(1) << 28) && yb < (size_t(1) << 28);
    return r;
}

// Every kernel-selection switch of the launcher (profiles/NOTES.md, "Kernel-selection switches"), with the default dispatch as
// initialisers.  Honoured only with IDSP_DIAG=1: lane_stream.h `stream_switches()` reads them once per process through `diag_env`.
struct StreamSwitches {
    bool diag_on = false;                       // IDSP_DIAG: nothing may assume which kernel a shape takes
    // LaneMajor
    bool no_lm_staged = false;                  // IDSP_NO_LM_STAGED: always the tile kernel
    size_t lm_lanes_per_wave = 0;               // IDSP_LM_LANES_PER_WAVE = 64 / 32 / 16 forces one
    size_t lm_skew = 0, lm_skew_shift = 8, lm_skew_mod = 2;  // IDSP_LM_SKEW, _SHIFT, _MOD: start-up skew of the staged kernel (arguments, not a choice)
    // FrameMajor
    bool align16_only = false;                  // IDSP_ALIGN16_ONLY: round 2's rule — 16-byte aligned rows or the register-window kernel
    bool no_fm_few = false;                     // IDSP_NO_FM_FEW
    bool no_fm_pair = false;                    // IDSP_NO_FM_PAIR: the staged single-wave kernel
    size_t fm_pair_max_lanes = thr::kPairMaxLanes;  // IDSP_FM_PAIR_MAX_LANES
    bool no_sweep = false;                      // IDSP_NO_SWEEP: the round-4 dispatch
    size_t sweep_min_lanes_4 = thr::kSweepMinLanesFps, sweep_min_lanes_8 = thr::kSweepMinLanes;  // IDSP_SWEEP_MIN_LANES sets both (4- / 8-byte outputs)
    bool sweep_grid64_only = false;             // IDSP_SWEEP_GRID64_ONLY: rows off the 64-byte grid stay on round 3's kernel
    size_t sweep_offgrid_min_lanes = thr::kLdsGridCap * kPlanBlock;  // IDSP_SWEEP_OFFGRID_MIN_LANES
    size_t sweep_max_grid = 256;                // IDSP_SWEEP_MAX_GRID: at most n workgroups (small tensors reach every LPT and several sweeps: tests)
    bool sweep_no_xcdc = false, sweep_force_xcdc = false;  // IDSP_SWEEP_NO_XCDC / IDSP_SWEEP_FORCE_XCDC: the block order
    bool sweep_no_fps = false;                  // IDSP_SWEEP_NO_FPS: one frame per segment
    bool no_fm_staged = false;                  // IDSP_NO_FM_STAGED: never
    size_t fm_lanes_per_wave = 0;               // IDSP_FM_LANES_PER_WAVE = 64 / 32 / 16 forces the staged form at any lane count
    bool staged_no_xcdc = false;                // IDSP_STAGED_NO_XCDC: the plain block order on rows off the 64-byte grid
    bool staged_nt = false;                     // IDSP_STAGED_NT: nontemporal accesses everywhere
    bool lds_cost_forced = false;               // IDSP_LDS_COST=n replaces LDS_ELIGIBLE by `COST <= n` (and keeps the sweep kernel out)
    int lds_cost = thr::kHeavyCost;
    bool no_lds_path = false;                   // IDSP_NO_LDS_PATH: neither LDS-DMA kernel
    size_t lds_min_waves = thr::kLdsMinWaves;   // IDSP_LDS_MIN_WAVES
    size_t lds_max_waves = size_t(1) << 40;     // IDSP_LDS_MAX_WAVES
    size_t lds_grid = ~size_t(0);               // IDSP_LDS_GRID: workgroups at most (0: one per block)
    bool lds_no_xcdc = false;                   // IDSP_LDS_NO_XCDC: the plain block order on rows off the 64-byte grid
    bool fm_xcdc = false;                       // IDSP_FM_XCDC: XCD-contiguous blocks on the register-window kernel
    bool no_duo = false;                        // IDSP_NO_DUO: never the two-wave chain kernel
};

// `env(name)`: the variable's text or NULL (the launcher passes `diag_env`)
template <class Env>
StreamSwitches read_stream_switches(Env env)
{
    StreamSwitches s;
    auto on = [&](const char *name) { return env(name) != nullptr; };
    auto size = [&](const char *name, size_t dflt) {
        const char *e = env(name);
        return e ? size_t(strtoull(e, nullptr, 10)) : dflt;
    };
    s.diag_on = on("IDSP_DIAG");
    s.no_lm_staged = on("IDSP_NO_LM_STAGED");
    s.lm_lanes_per_wave = size("IDSP_LM_LANES_PER_WAVE", s.lm_lanes_per_wave);
    s.lm_skew = size("IDSP_LM_SKEW", s.lm_skew), s.lm_skew_shift = size("IDSP_LM_SKEW_SHIFT", s.lm_skew_shift), s.lm_skew_mod = size("IDSP_LM_SKEW_MOD", s.lm_skew_mod);
    s.align16_only = on("IDSP_ALIGN16_ONLY");
    s.no_fm_few = on("IDSP_NO_FM_FEW");
    s.no_fm_pair = on("IDSP_NO_FM_PAIR");
    s.fm_pair_max_lanes = size("IDSP_FM_PAIR_MAX_LANES", s.fm_pair_max_lanes);
    s.no_sweep = on("IDSP_NO_SWEEP");
    s.sweep_min_lanes_4 = size("IDSP_SWEEP_MIN_LANES", s.sweep_min_lanes_4), s.sweep_min_lanes_8 = size("IDSP_SWEEP_MIN_LANES", s.sweep_min_lanes_8);
    s.sweep_grid64_only = on("IDSP_SWEEP_GRID64_ONLY");
    s.sweep_offgrid_min_lanes = size("IDSP_SWEEP_OFFGRID_MIN_LANES", s.sweep_offgrid_min_lanes);
    s.sweep_max_grid = unsigned(size("IDSP_SWEEP_MAX_GRID", s.sweep_max_grid));
    s.sweep_no_xcdc = on("IDSP_SWEEP_NO_XCDC"), s.sweep_force_xcdc = on("IDSP_SWEEP_FORCE_XCDC");
    s.sweep_no_fps = on("IDSP_SWEEP_NO_FPS");
    s.no_fm_staged = on("IDSP_NO_FM_STAGED");
    s.fm_lanes_per_wave = size("IDSP_FM_LANES_PER_WAVE", s.fm_lanes_per_wave);
    s.staged_no_xcdc = on("IDSP_STAGED_NO_XCDC");
    s.staged_nt = on("IDSP_STAGED_NT");
    s.lds_cost_forced = on("IDSP_LDS_COST");
    s.lds_cost = int(size("IDSP_LDS_COST", size_t(s.lds_cost)));
    s.no_lds_path = on("IDSP_NO_LDS_PATH");
    s.lds_min_waves = size("IDSP_LDS_MIN_WAVES", s.lds_min_waves);
    s.lds_max_waves = size("IDSP_LDS_MAX_WAVES", s.lds_max_waves);
    s.lds_grid = size("IDSP_LDS_GRID", s.lds_grid);
    s.lds_no_xcdc = on("IDSP_LDS_NO_XCDC");
    s.fm_xcdc = on("IDSP_FM_XCDC");
    s.no_duo = on("IDSP_NO_DUO");
    return s;
}

// ------------------------------------------------------------------------------------------------------------ the sweep kernel's geometry
struct SweepGeom {
    int lpt = 1;             // sub-blocks per workgroup
    unsigned grid = 0;       // workgroups
    unsigned bw = 256;       // lanes per sub-block (multiple of 16, <= 256)
    unsigned rounds = 1;     // sweeps inside the launch
    unsigned fps = 1;        // frames per one-KiB segment (LPT = 1 and bw <= 128: plan_stream sets it for 4-byte outputs)
    size_t round_lanes = 0;  // lanes per sweep (the last one may hold fewer)
};

// Geometry for `lanes` lanes (a multiple of 4) with at most `max_lpt` sub-blocks per workgroup; false: not coverable
// (fewer than 16 lanes).  Waste (lanes of capacity beyond the last lane) costs duplicate traffic of at most one
// workgroup; a grid below 256 leaves CUs idle — scored 4 : 1 (tools/exp_fm_sweep.hip sweeps the alternatives).
inline bool sweep_geometry(size_t lanes, int max_lpt, SweepGeom &out, unsigned max_grid = 256)
{
    if (lanes < 16 || max_lpt < 1) return false;
    const size_t cap = size_t(max_grid) * size_t(max_lpt) * 256;
    const size_t rounds = (lanes + cap - 1) / cap;
    size_t lr = (lanes + rounds - 1) / rounds;
    lr = (lr + 15) / 16 * 16;
    int lpt = 1;
    while (lpt < max_lpt && size_t(max_grid) * size_t(lpt) * 256 < lr) lpt *= 2;
    double best = 1e30;
    for (unsigned bw = 256; bw >= 16; bw -= 16) {
        const size_t per = size_t(lpt) * bw, g = (lr + per - 1) / per;
        if (g > max_grid) continue;
        const double waste = double(g * per - lr) / double(lr), idle = double(max_grid - g) / double(max_grid);
        const double score = waste + 0.25 * idle + (256 - bw) * 1e-5;
        if (score < best) best = score, out.bw = bw, out.grid = unsigned(g);
    }
    if (best >= 1e30) return false;
    out.lpt = lpt, out.rounds = unsigned(rounds), out.round_lanes = lr;
    return true;
}

// Whether the sweep kernel is the one to take for `lanes` lanes of a processor instantiated up to `max_lpt` blocks per workgroup (`g`: the
// geometry): when the launch is ONE sweep, or when its sweeps are at least 8 blocks per workgroup wide (2 MiB of every row).  Several narrower
// sweeps per launch are the panel walk again (rows at a stride, 1 MiB or less of each): 2^20 lanes in four sweeps of 4 blocks per workgroup
// 0.54-0.57 of the HBM peak for every family against 0.60-0.62 on round 4's dispatch, which those launches keep (profiles/r05_perf_big_lanes.txt).
inline bool sweep_takes(int max_lpt, size_t lanes, const StreamSwitches &sw, SweepGeom *g = nullptr)
{
    SweepGeom geom;
    const unsigned max_grid = unsigned(sw.sweep_max_grid);
    if (!sweep_geometry(lanes, max_lpt, geom, max_grid ? max_grid : 256u)) return false;
    if (g) *g = geom;
    return geom.rounds == 1 || geom.lpt >= thr::kSweepMinLptSeveralSweeps || max_grid != 256;  // (a capped grid is the tests' way to reach several sweeps per launch at small sizes)
}

// When a chain of m sections (per launch) goes to the two-wave kernel (stream_frame_major_duo).  Measured at 4096 frames (tools/exp_duo.hip,
// profiles/r03_exp_duo.jsonl): i32 chain of 4 at 65536 lanes 0.483 -> 0.426 ms, at 131072 lanes 0.829 -> 0.909; i32 cascade of 8 at
// 32768 / 65536 / 131072 lanes 0.583 / 0.661 / 1.250 -> 0.482 / 0.578 / 1.066; and five to eight sections of a plain chain are ONE pass over
// HBM instead of two.
inline bool duo_wanted(size_t m, size_t lanes, int layout, const StreamSwitches &sw)
{
    if (sw.no_duo || layout != IDSP_FRAME_MAJOR || lanes < thr::kDuoMinLanes) return false;
    return m >= 5 || (m == 4 && lanes <= thr::kDuo4MaxLanes);
}

// ------------------------------------------------------------------------------------------------------------ the decision
enum class StreamForm {
    LmTile,          // stream_lane_major
    LmStaged,        // stream_lane_major_staged: lanes_per_wave
    FmFew,           // stream_frame_major_few: one to three lanes in all
    FmOddBeside,     // the last lanes % 4 on the second stream (few kernel) beside the body: body, odd
    FmRoundsBeside,  // whole rounds, and the remainder beside them on the second stream: head, tail
    FmPair,          // stream_frame_major_pair
    FmSweep,         // stream_frame_major_sweep (fm_sweep.h): geom, xcdc
    FmStaged,        // stream_frame_major_staged: lanes_per_wave, grid, staged_flags
    FmLds,           // stream_frame_major_lds: grid, deep_ring, xcdc
    FmWindow,        // stream_frame_major (register window): grid, block, deep_window, xcdc
};

struct StreamPlan {
    StreamForm form = StreamForm::FmWindow;
    size_t xl = 0, yl = 0;         // the row pitches, resolved
    int lanes_per_wave = 64;       // both staged kernels
    size_t body = 0, odd = 0;      // FmOddBeside
    size_t head = 0, tail = 0;     // FmRoundsBeside
    bool head_swept = false;       // FmRoundsBeside: the whole rounds went to the sweep kernel — the caller sets it from the head's own plan
    unsigned grid = 0;             // workgroups (FmStaged, FmLds, FmWindow; the sweep's are geom.grid)
    bool deep_ring = false;        // FmLds: 7 tiles and the indexed form (persistent grids)
    bool xcdc = false;             // XCD-contiguous block order (FmSweep, FmLds, FmWindow)
    int staged_flags = 0;          // FmStaged: bit 0 XCD-contiguous lane blocks, bit 1 plain instead of nontemporal accesses
    unsigned block = 0;            // FmWindow: threads per workgroup
    bool deep_window = true;       // FmWindow: the processor's full prefetch depth (else at most 8)
    SweepGeom geom;                // FmSweep
    bool fps_form = false;         // FmSweep: several frames per segment (geom.fps of them: 1 where the 32-bit guard brought them down)
};

// The call for lanes [first, first + n) of `c`, whose plan is `p`: a lane block of the same tensors (4-byte samples: both splits are
// four_four() only), at the call's row and state pitches
inline StreamCall lane_block(const StreamCall &c, const StreamPlan &p, size_t first, size_t n, bool remainder)
{
    StreamCall b = c;
    b.lanes = n, b.x = c.x + first * 4, b.y = c.y + first * 4;
    b.pitch_x = p.xl, b.pitch_y = p.yl, b.state_pitch = c.state_pitch ? c.state_pitch : c.lanes;
    b.remainder_of_split = remainder;
    return b;
}

inline StreamPlan plan_lane_major(const StreamTraits &t, const StreamCall &c, const StreamSwitches &sw)
{
    StreamPlan p;
    p.form = StreamForm::LmTile;
    p.xl = c.pitch_x ? c.pitch_x : c.frames, p.yl = c.pitch_y ? c.pitch_y : c.frames;
    p.grid = unsigned((c.lanes + kPlanWave - 1) / kPlanWave);
    if (!t.lm_staged) return p;
    // 16-byte pieces need 16-byte aligned rows (of less than 64 MiB: 32-bit offsets inside a wave's 64 rows); below a quarter tile of
    // frames the 4-byte tile kernel has less to set up
    const StreamRows rows = stream_rows(t, c.x, c.y, p.xl, p.yl);
    const size_t isz = t.has_in ? t.in_bytes : 0, wide = isz > t.out_bytes ? isz : t.out_bytes;
    if (sw.no_lm_staged || c.frames * wide < thr::kLmStagedMinRowBytes || !rows.grid16 || !rows.below_2_26) return p;
    // lanes per wave: 64 when that already gives every SIMD a wave, else 32 or 16 (tools/tune_lm.hip).  Measured
    // (profiles/r02_tune_lm_lanes_per_wave.jsonl, 4096 frames): i32 DF1 at 16384 lanes 0.168 / 0.157 / 0.136 ms with 64 / 32 / 16 lanes per
    // wave, at 32768 lanes 0.232 / 0.216 / 0.213, at 65536 0.382 / 0.393 / 0.446; the 8-section cascade (heavy) 0.57 / 0.45 / 0.52 at 16384
    // and 0.61 / 0.91 / 1.56 at 65536
    const size_t lw = sw.lm_lanes_per_wave ? sw.lm_lanes_per_wave
                      : c.lanes >= thr::kLmStaged64Lanes ? 64 : (c.lanes >= thr::kLmStaged32Lanes || t.heavy()) ? 32 : 16;
    // forms instantiated per processor: all three for the cheap ones, 64 / 32 for the heavy ones, 64 only for LM_ONE_FORM (build time)
    p.form = StreamForm::LmStaged;
    p.lanes_per_wave = t.lm_one_form ? 64 : (lw == 16 && !t.heavy()) ? 16 : lw <= 32 ? 32 : 64;
    p.grid = unsigned((c.lanes + size_t(p.lanes_per_wave) - 1) / size_t(p.lanes_per_wave));
    return p;
}

// FrameMajor, top to bottom: few lanes -> the two splits over a second stream -> pair -> sweep -> staged -> round-3 LDS-DMA -> register window
inline StreamPlan plan_frame_major(const StreamTraits &t, const StreamCall &c, const StreamSwitches &sw)
{
    StreamPlan p;
    const size_t lanes = c.lanes, frames = c.frames;
    const size_t xl = p.xl = c.pitch_x ? c.pitch_x : lanes / size_t(t.in_div), yl = p.yl = c.pitch_y ? c.pitch_y : lanes;
    const size_t waves = (lanes + kPlanWave - 1) / kPlanWave;
    const StreamRows rows = stream_rows(t, c.x, c.y, xl, yl);
    // Rows that are only 4-byte aligned (a dense tensor of 65537 lanes, an odd pitch, a base off the 16-byte grid): the 16-byte requests and
    // stores of the LDS-DMA and staged kernels only need dword alignment, so those kernels run on such rows as they are
    // (profiles/r03_exp_fm_unaligned4.jsonl: 65536 lanes at pitch 65537 0.65 of the HBM peak against 0.41 on the register-window kernel).
    const bool rows_ok = rows.grid16 || !sw.align16_only;

    if (t.four_four()) {
        // one to three lanes in all: one wave moves 256 frames per tile with all its threads (~90 ns per frame on the register-window kernel)
        if (lanes <= thr::kFewMaxLanes && frames >= thr::kFewMinFrames && !sw.no_fm_few) {
            p.form = StreamForm::FmFew;
            return p;
        }
        // What those kernels do need is whole 16-byte pieces per row, i.e. a multiple of 4 lanes: the last lanes % 4 run beside the rest
        p.odd = lanes % 4, p.body = lanes - p.odd;
        if (p.odd && !sw.align16_only && p.body >= thr::kOddSplitMinBody && frames >= thr::kOddSplitMinFrames && (t.fm_staged || t.lds_eligible) &&
            !c.no_side_stream) {
            p.form = StreamForm::FmOddBeside;
            return p;
        }
    }
    if (t.fm_staged && t.four_four() && !t.heavy()) {
        // Whole rounds + remainder.  The LDS-DMA kernels run one 256-lane block per CU and round; 65540 lanes are 257 blocks — one CU with
        // two workgroups, both at half speed — and 73728 lanes 288: 0.58 of the HBM peak where 65536 run at 0.78.  The lanes beyond the last
        // whole round run BESIDE the whole rounds on the staged single-wave kernel: 69632 lanes 0.57 -> 0.65, 73728 0.58 -> 0.69, 81920
        // 0.59 -> 0.63; no gain from a 24576-lane remainder up (profiles/r03_exp_split_streams.jsonl).
        // Whole rounds on the SWEEP kernel: only 1, 2, 4, 8 or 16 of them (full 256-lane blocks; three or five rounds would be narrow blocks
        // themselves, and the call is one sweep over all its lanes instead).  A processor the sweep does not take at `head` lanes keeps the
        // split for any number of rounds (3 x 65536 + 8192 lanes of a 3-section chain: 0.65 against 0.57 as one launch).
        p.head = lanes / kPlanRound * kPlanRound, p.tail = lanes - p.head;
        const size_t head_rounds = p.head / kPlanRound;
        const bool head_on_sweep = t.lds_eligible && p.head != 0 && sweep_takes(t.sweep_max_lpt, p.head, sw);
        const bool rounds_ok = !head_on_sweep || ((head_rounds & (head_rounds - 1)) == 0 && head_rounds <= thr::kRoundsSplitMaxRounds);
        if (p.head && p.tail && p.tail <= thr::kSplitTailMax && rounds_ok && lanes % 4 == 0 && frames >= thr::kRoundsSplitMinFrames && t.lds_eligible &&
            !sw.diag_on && rows_ok && rows.below_2_28 && !c.no_side_stream) {
            p.form = StreamForm::FmRoundsBeside;
            return p;
        }
    }
    if (t.fm_staged && t.four_four() && t.cost <= thr::kPairMaxCost) {
        // Few lanes, long calls, cheap single sections: one wave computes, one wave moves.  Rows on the 64-byte grid only: off it the staged
        // kernel's plain accesses and XCD-contiguous order win (16384 lanes of a 16385-lane tensor 0.315 ms here against 0.186 there).  The
        // remainder of a split keeps the staged kernel: beside the sweep kernel's whole rounds the pair kernel costs 6-10 % (69632 lanes
        // 0.413 -> 0.454 ms, profiles/r06_exp_fm_pair.txt).
        if (!sw.no_fm_pair && !c.remainder_of_split && lanes <= sw.fm_pair_max_lanes && frames >= thr::kPairMinFrames && lanes % 4 == 0 && rows.grid64 &&
            rows.below_2_28) {
            p.form = StreamForm::FmPair;
            return p;
        }
    }
    if (t.lds_input() && t.lds_eligible) {
        // ONE dense sweep for any lane count (fm_sweep.h): whole multiples of 65536, ragged counts, 2^20 lanes alike.  (Lane counts a little
        // above a multiple of 65536 were split above: 65552 lanes 0.77 of the HBM peak against 0.54 as one sweep of half-empty blocks.)
        // Rows off the 64-byte grid take the same sweep with the blocks dealt to the XCDs in contiguous eighths — from the lane count up where
        // round 3's XCD-contiguous kernel would walk panels on a persistent grid (131076 dense lanes 0.56 -> 0.61; below it that kernel is a
        // single round itself: 65000 dense lanes 0.745), and, 4-byte outputs, up to kSweepOffGridSmallMax lanes, where the alternative is the
        // staged single-wave kernel (40000 lanes at pitch + 4 0.51 -> 0.72 of the peak, 32768 0.52 -> 0.61; 57344: 0.69 either way).
        const bool off_grid_ok = !sw.sweep_grid64_only && rows_ok &&
                                 (lanes > sw.sweep_offgrid_min_lanes || (t.out_bytes == 4 && lanes <= thr::kSweepOffGridSmallMax));
        const size_t sweep_min = t.out_bytes == 4 ? sw.sweep_min_lanes_4 : sw.sweep_min_lanes_8;
        if (!sw.no_sweep && !sw.lds_cost_forced && !sw.no_lds_path && (rows.grid64 || off_grid_ok) && lanes % 4 == 0 && lanes >= sweep_min &&
            frames >= thr::kSweepMinFrames && sweep_takes(t.sweep_max_lpt, lanes, sw, &p.geom)) {
            p.form = StreamForm::FmSweep;
            p.xcdc = ((!rows.grid64 && !sw.sweep_no_xcdc) || sw.sweep_force_xcdc) && p.geom.grid >= thr::kSweepXcdcMinGrid;
            // few lanes per workgroup (below 32768 + lanes in all): several frames per one-KiB segment, so that a tile stays 8 KiB of real samples
            p.fps_form = p.geom.lpt == 1 && t.out_bytes == 4 && p.geom.bw <= thr::kSweepFpsMaxBlockLanes && !sw.sweep_no_fps;
            if (p.fps_form) {
                unsigned f = 256u / p.geom.bw;
                while (f > 1 && (size_t(f - 1) * kPlanSweepSegments * (xl > yl ? xl : yl) + 256) * 4 >= (size_t(1) << 32)) f--;  // per-thread byte offsets are 32-bit
                p.geom.fps = f;
            }
            return p;
        }
    }
    if (t.fm_staged) {
        // Few lanes (the chip is not full and every FrameMajor kernel below runs at its per-lane latency): the staged single-wave kernel
        // (profiles/r02_tune_fm_small.jsonl; i32 DF1 x 4096 frames: 16384 lanes 0.147 ms against 0.211 / 0.335 on the register-window / LDS-DMA
        // kernel, 32768 lanes 0.211 against 0.243 / 0.332, 65536 lanes 0.43 against 0.41 / 0.335).  Heavy processors gain only around
        // 16384-32768 lanes (8-section cascade 0.44 against 0.48) and lose elsewhere.
        const size_t sz = t.in_bytes;
        const bool in_range = t.heavy() ? (lanes >= thr::kStagedHeavyMinLanes && lanes < thr::kStagedHeavyMaxLanes) : lanes < thr::kStagedMaxLanes;
        if (!sw.no_fm_staged && (sw.fm_lanes_per_wave || in_range) && frames >= thr::kStagedMinFrames && (lanes * sz) % 16 == 0 && rows_ok && rows.below_2_28) {
            // rows off the 64-byte grid: a 32-lane wave's 128-byte row pieces each straddle two lines, so 64 lanes per wave a little later
            // (with plain accesses there the 32-lane form wins up to ~25000 lanes: 16385 lanes 0.217 -> 0.182 ms, 24580 0.249 -> 0.223;
            // 26628 0.255 with 64 against 0.268 with 32 — profiles/r03_exp_fm_unaligned_small.jsonl)
            const bool off64 = !rows.grid64;
            const size_t lw = sw.fm_lanes_per_wave ? sw.fm_lanes_per_wave : t.heavy() ? 32
                              : lanes >= (off64 ? thr::kStaged64LanesOffGrid : thr::kStaged64Lanes) ? 64 : lanes >= thr::kStaged32Lanes ? 32 : 16;
            p.form = StreamForm::FmStaged;
            p.lanes_per_wave = t.heavy() ? 32 : lw == 16 ? 16 : lw == 64 ? 64 : 32;  // (heavy processors: the 32-lane form only)
            p.grid = unsigned((lanes + size_t(p.lanes_per_wave) - 1) / size_t(p.lanes_per_wave));
            // rows off the 64-byte grid: XCD-contiguous lane blocks, and plain instead of nontemporal accesses
            p.staged_flags = (!sw.staged_no_xcdc && p.grid >= thr::kStagedXcdcMinGrid && off64 ? 1 : 0) | (!sw.staged_nt && off64 ? 2 : 0);
            return p;
        }
    }
    if (t.lds_input()) {
        // Round 3's LDS-DMA kernel: cheap per-sample arithmetic (the extra LDS hop and the two barriers per tile cost issue slots) — LDS_ELIGIBLE
        // where the processor says so (profiles/r02_tune_lds_heavy*.jsonl), else the cost estimate — and whole 256-lane blocks or, for
        // one-word outputs, any multiple of 4 lanes: the kernel's last block may be ragged
        const bool eligible = sw.lds_cost_forced ? t.cost <= sw.lds_cost : t.lds_eligible;
        const size_t ow = t.out_bytes / 4;
        if (!sw.no_lds_path && eligible && waves >= sw.lds_min_waves && waves <= sw.lds_max_waves && (lanes % kPlanBlock == 0 || (ow == 1 && lanes % 4 == 0)) &&
            rows_ok) {
            // Grid (profiles/r02_exp_c5_*.jsonl).  Up to kLdsGridCap workgroups: one per 256-lane block.  Beyond: a persistent grid of <= 256
            // workgroups (one per CU) that walks the lane blocks in column panels of equal rounds.
            const size_t nblocks = (lanes + kPlanBlock - 1) / kPlanBlock;
            size_t grid = nblocks;
            if (sw.lds_grid != ~size_t(0)) {
                if (sw.lds_grid && nblocks > sw.lds_grid) grid = sw.lds_grid;
            } else if (nblocks > thr::kLdsGridCap) {
                const size_t rounds = (nblocks + 255) / 256;
                grid = (nblocks + rounds - 1) / rounds;
            }
            p.form = StreamForm::FmLds;
            p.grid = unsigned(grid);
            // rows that do not start on 64-byte boundaries (dense 65000-lane tensors, odd pitches): adjacent lane blocks on one XCD
            // (0.67-0.71 of the peak on such rows instead of 0.58-0.64)
            p.xcdc = !rows.grid64 && !sw.lds_no_xcdc;
            // Ring depth: the processor's tuned depth for single-pass launches; persistent launches keep 7 tiles and the indexed form for
            // every processor — depths 3-5 lose 15-20 % there (profiles/r02_exp_c5_matrix7.jsonl: 0.56 vs 0.68 at 2^20 lanes)
            p.deep_ring = grid < nblocks && t.lds_ring != 7;
            return p;
        }
    }
    // The register-window kernel.  A CU's L1 moves ~10 B/cycle, so a launch must reach all 256 CUs: below 1024 waves (= 256 workgroups of 4)
    // one wave per workgroup (16384 lanes in 256-thread blocks would run on 64 CUs).  Prefetch depth by occupancy: at <= 2 waves/SIMD nothing
    // else hides HBM latency, so go deep; with many resident waves keep the register budget low.  XCD-contiguous blocks HURT this kernel
    // (65537 dense lanes 0.81 ms against 0.69, profiles/r03_perf_ragged_xcdc.jsonl): a diagnostic switch only.
    p.form = StreamForm::FmWindow;
    p.block = unsigned(waves < thr::kWindowBlockMinWaves ? kPlanWave : kPlanBlock);
    p.grid = unsigned((lanes + p.block - 1) / p.block);
    p.xcdc = sw.fm_xcdc && p.grid >= thr::kWindowXcdcMinGrid;
    p.deep_window = waves <= thr::kWindowDeepMaxWaves;
    return p;
}

inline StreamPlan plan_stream(const StreamTraits &t, const StreamCall &c, const StreamSwitches &sw)
{
    return c.layout == IDSP_LANE_MAJOR ? plan_lane_major(t, c, sw) : plan_frame_major(t, c, sw);
}

// ------------------------------------------------------------------------------------------------------------ names
// What idsp_last_kernel() reports for a plan: the launcher records exactly these strings.  FmOddBeside has no name of its own: the body's
// launch records one, and `stream_plan_also` is appended to it.
inline const char *stream_plan_name(const StreamPlan &p)
{
    const int lw = p.lanes_per_wave;
    switch (p.form) {
        case StreamForm::LmTile: return "stream_lane_major";
        case StreamForm::LmStaged:
            return lw == 64 ? "stream_lane_major_staged" : lw == 32 ? "stream_lane_major_staged[32 lanes/wave]" : "stream_lane_major_staged[16 lanes/wave]";
        case StreamForm::FmFew: return "stream_frame_major_few";
        case StreamForm::FmOddBeside: return "";
        case StreamForm::FmRoundsBeside:
            return p.head_swept ? "stream_frame_major_sweep + stream_frame_major_staged (remainder, second stream)"
                                : "stream_frame_major_lds + stream_frame_major_staged (remainder, second stream)";
        case StreamForm::FmPair: return "stream_frame_major_pair[compute + mover wave per 32 lanes]";
        case StreamForm::FmSweep: {
            static const char *const names[] = {"stream_frame_major_sweep[1 block/workgroup]", "stream_frame_major_sweep[2 blocks/workgroup]",
                                                "stream_frame_major_sweep[4 blocks/workgroup]", "stream_frame_major_sweep[8 blocks/workgroup]",
                                                "stream_frame_major_sweep[16 blocks/workgroup]"};
            static const char *const names_x[] = {"stream_frame_major_sweep[1 block/workgroup, XCD-contiguous]", "stream_frame_major_sweep[2 blocks/workgroup, XCD-contiguous]",
                                                  "stream_frame_major_sweep[4 blocks/workgroup, XCD-contiguous]", "stream_frame_major_sweep[8 blocks/workgroup, XCD-contiguous]",
                                                  "stream_frame_major_sweep[16 blocks/workgroup, XCD-contiguous]"};
            int k = 0;
            while ((1 << k) < p.geom.lpt) k++;
            return p.xcdc ? names_x[k] : names[k];
        }
        case StreamForm::FmStaged:
            return lw == 64 ? "stream_frame_major_staged[64 lanes/wave]" : lw == 32 ? "stream_frame_major_staged[32 lanes/wave]" : "stream_frame_major_staged[16 lanes/wave]";
        case StreamForm::FmLds:
            return p.xcdc ? "stream_frame_major_lds[XCD-contiguous blocks]" : "stream_frame_major_lds";
        case StreamForm::FmWindow: return p.xcdc ? "stream_frame_major[XCD-contiguous blocks]" : "stream_frame_major";
    }
    return "";
}

// The suffix a plan appends to the recorded name (NULL: none): the sweep's frames per segment — 1 where the 32-bit guard brought them down,
// tests pin both sides of it — and the second stream's kernel of the lanes % 4 split
inline const char *stream_plan_also(const StreamPlan &p)
{
    if (p.form == StreamForm::FmOddBeside) return " + stream_frame_major_few (lanes % 4, second stream)";
    if (p.form == StreamForm::FmSweep && p.fps_form) {
        static const char *const fps[] = {" [1 frame/segment]",   " [2 frames/segment]",  " [3 frames/segment]",  " [4 frames/segment]",
                                          " [5 frames/segment]",  " [6 frames/segment]",  " [7 frames/segment]",  " [8 frames/segment]",
                                          " [9 frames/segment]",  " [10 frames/segment]", " [11 frames/segment]", " [12 frames/segment]",
                                          " [13 frames/segment]", " [14 frames/segment]", " [15 frames/segment]", " [16 frames/segment]"};
        return fps[(p.geom.fps - 1) & 15];  // 256 / bw with bw >= 16
    }
    return nullptr;
}

}  // namespace idsp
