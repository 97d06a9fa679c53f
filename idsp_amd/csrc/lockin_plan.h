// lockin_plan.h — which kernel a call of one of the eight lock-in entries takes, as ONE pure function (as stream_plan.h is for launch_stream).
//
// `plan_lockin` reads the call (LockinCall) and the diagnostic switches (LockinSwitches) and returns the decision (LockinPlan): the entries
// (lockin_phase.hip, lockin_generic.hip) and the launchers of lockin_waves.h do what it says; tests/test_lockin_plan.py runs the same function
// through tests/cpp/stream_plan_cli.cpp without a GPU.  No HIP here: plain C++17.  Thresholds: dispatch_thresholds.h, "lock-in".
#pragma once

#include "stream_plan.h"

namespace idsp {

enum { MODE_IQ = 0, MODE_ARG = 1, MODE_NORM_SQR = 2 };                // read-out: `Complex<i32>`, `arg()`, `norm_sqr()`
enum { IN_FM_REG = 0, IN_FM_DMA = 1, IN_LM_REG = 2, IN_LM_DMA = 3 };  // input form of lockin_waves_kernel (lockin_waves.h)
constexpr int kLwB = 8;     // frames per batch, FrameMajor
constexpr int kLwBLm = 16;  // LaneMajor: 16 frames = one whole 128-byte line of 8-byte output elements per lane and batch
constexpr int kLsB = 16;    // the stage-wave kernel's batch

enum class LockinArms { Lowpass, Biquad };      // `[Lowpass<order>; cascade]` or `[Biquad; n]` (n is not read by the choice)
enum class LockinLo { Phase, Buffer, Accu };    // internal phase accumulator, caller's LO buffer, the RPLL's `Accu` rows

struct LockinCall {
    LockinArms arms = LockinArms::Lowpass;
    int order = 1, cascade = 1;
    LockinLo lo = LockinLo::Phase;
    int readout = MODE_IQ;
    size_t lanes = 0, frames = 0;
    int layout = IDSP_FRAME_MAJOR;
    uintptr_t x = 0, y = 0;     // the two addresses (the LO forms test these too, not `lo`)
    bool tuned_device = false;  // stagger_tuned_device(), common.h
};

// Every kernel-selection switch of the lock-in family (profiles/NOTES.md, "Kernel-selection switches").  Honoured only with IDSP_DIAG=1:
// dds_dev.h `lockin_switches()` reads them once per process through `diag_env`.
struct LockinSwitches {
    bool no_waves = false;       // IDSP_LOCKIN_NO_WAVES: everything on the one- / two-thread-per-lane stream kernels
    int waves = 0;               // IDSP_LOCKIN_WAVES = 4 / 6 forces one (lowpass arms on the internal phase only)
    bool no_lm_tail = false;     // IDSP_LOCKIN_NO_LM_TAIL: no body + tail (the three lowpass phase entries only)
    bool no_stages = false;      // IDSP_LOCKIN_NO_STAGES: never the stage-wave kernel
    int stage_groups = 0;        // IDSP_LOCKIN_STAGE_GROUPS = 1 / 2: always (when the shape allows)
    bool no_skew = false;        // IDSP_LOCKIN_NO_SKEW: no start-up stagger
    bool no_dma = false;         // IDSP_LOCKIN_NO_DMA: register-prefetch input
    int batch = 0;               // IDSP_LOCKIN_B = 8 / 16 forces a batch length (FrameMajor DMA form)
    size_t split_max_lanes = thr::kSplitMaxLanes;  // IDSP_SPLIT_MAX_LANES (read_dds_switches of readout_plan.h reads it too, for idsp_dds_i32)
};

// `env(name)`: the variable's text or NULL (the library passes `diag_env`)
template <class Env>
LockinSwitches read_lockin_switches(Env env)
{
    LockinSwitches s;
    auto on = [&](const char *name) { return env(name) != nullptr; };
    auto num = [&](const char *name, size_t dflt) {
        const char *e = env(name);
        return e ? size_t(strtoull(e, nullptr, 10)) : dflt;
    };
    s.no_waves = on("IDSP_LOCKIN_NO_WAVES");
    s.waves = int(num("IDSP_LOCKIN_WAVES", 0));
    s.no_lm_tail = on("IDSP_LOCKIN_NO_LM_TAIL");
    s.no_stages = on("IDSP_LOCKIN_NO_STAGES");
    s.stage_groups = int(num("IDSP_LOCKIN_STAGE_GROUPS", 0));
    s.no_skew = on("IDSP_LOCKIN_NO_SKEW");
    s.no_dma = on("IDSP_LOCKIN_NO_DMA");
    s.batch = int(num("IDSP_LOCKIN_B", 0));
    s.split_max_lanes = num("IDSP_SPLIT_MAX_LANES", s.split_max_lanes);
    return s;
}

enum class LockinForm {
    Stream,     // the one- / two-thread-per-lane stream kernels (launch_stream names them)
    Waves,      // lockin_waves_kernel
    WavesTail,  // lockin_waves_kernel on the whole batches of every LaneMajor row, a stream kernel on the last frames % 16
    Stages,     // lockin_stages_kernel
};

struct LockinPlan {
    LockinForm form = LockinForm::Stream;
    int waves = 0;       // per 64 lanes: 4 / 6 (Waves, WavesTail)
    int groups = 0;      // lane groups per workgroup: 1 / 2 (Stages)
    int batch = 0;       // frames per batch (Waves, WavesTail)
    int in = -1;         // IN_* (Waves, WavesTail)
    unsigned skew = 0;   // start-up stagger in 10 ns ticks, a kernel argument
    size_t body = 0;     // frames the multi-wave / stage-wave kernel takes: all of them, or all whole batches (WavesTail)
    bool split = false;  // Stream: the I and Q arms on two threads
};

inline const char *lockin_waves_name(int waves) { return waves == 6 ? "lockin_waves_kernel[6 waves per 64 lanes]" : "lockin_waves_kernel[4 waves per 64 lanes]"; }
// what note_kernel records for the plan ("stream_": the stream launcher records its own, stream_plan_name; every one of them begins so)
inline const char *lockin_plan_name(const LockinPlan &p)
{
    switch (p.form) {
        case LockinForm::Stages: return p.groups == 2 ? "lockin_stages_kernel[16 waves per 128 lanes]" : "lockin_stages_kernel[8 waves per 64 lanes]";
        case LockinForm::Waves: return lockin_waves_name(p.waves);
        case LockinForm::WavesTail: return "lockin_waves_kernel + stream kernel (last frames % 16)";
        default: return "stream_";
    }
}

inline LockinPlan plan_lockin(const LockinCall &c, const LockinSwitches &sw)
{
    LockinPlan p;
    const bool lm = c.layout == IDSP_LANE_MAJOR, lowpass_phase = c.arms == LockinArms::Lowpass && c.lo == LockinLo::Phase;
    const bool aligned = (c.x | c.y) % 16 == 0, arg = c.readout == MODE_ARG;
    // too few lanes to give every SIMD a wave: the I and Q arms on separate threads — idsp_lockin_i32_process alone among the phase forms
    // (its stream processor is the one with a split twin), and idsp_lockin_i32_accu_process
    p.split = c.arms == LockinArms::Lowpass && c.lo != LockinLo::Buffer && c.readout == MODE_IQ && c.lanes <= sw.split_max_lanes;
    // (the lowpass phase entries reach this with frames == 0 — they return early for lanes == 0 only — and call the stream path, which
    // launches nothing; the other entries return before they plan)
    if (c.lo == LockinLo::Accu || c.frames == 0) return p;

    // The multi-wave kernels take FrameMajor always and LaneMajor for whole 16-frame batches on 16-byte aligned rows.
    // Wave count per 64 lanes, 0 = not theirs.  Biquad arms and every external-LO form: four, whatever IDSP_LOCKIN_WAVES says.
    const auto waves_for = [&](size_t frames) {
        if (sw.no_waves || c.lanes >= thr::kLockinWavesMaxLanes) return 0;  // 32-bit thread offsets inside a row (8-byte elements, 3 input rows of 4 lanes bytes)
        if (lm && !(frames % kLwBLm == 0 && aligned)) return 0;
        if (!lowpass_phase) return 4;
        if (sw.waves == 4 || sw.waves == 6) return sw.waves;
        // FrameMajor up to one workgroup per CU: six waves (four read-out waves) with 16-frame batches — the read-out path is what an interval
        // waits for there (`[Lowpass<1>; 1]` 0.183 -> 0.156 ms, `[Lowpass<2>; 1]`->arg 0.324 -> 0.283 at 16384 lanes x 4096, profiles/r03_perf_c4small.jsonl;
        // `[Lowpass<N>; 2]` is the stage-wave kernel's at these lane counts).  Two 6-wave workgroups with 16-frame batches do not share a CU, so not above.
        if (!lm && c.lanes <= thr::kLockinSixWavesMaxLanes) return 6;
        // measured at 4096 frames (arg read-out): 6 waves 0.64 ms at 32768 lanes (4 waves: 0.73), 4 waves 1.07 ms at 65536 (6: 1.12)
        // (with six and more second-order-equivalents per arm the arm waves are the longer path again and the four-wave form with 16-frame
        // batches wins: `[Lowpass<2>; 4]` -> arg at 32768 lanes 0.58 against 0.74 ms, profiles/r03_perf_c4small_32768.jsonl)
        return arg && c.lanes <= sw.split_max_lanes && c.order * c.cascade < thr::kLockinSixWavesArmWeight ? 6 : 4;
    };
    p.body = c.frames;
    p.waves = waves_for(p.body);
    p.form = LockinForm::Waves;
    if (!p.waves) {
        // LaneMajor rows that are not whole 16-frame batches (round 4): the multi-wave kernel takes the whole batches of every row at the call's
        // row pitch and a stream kernel the last frames % 16 behind it (same stream; the state carries over as between two calls).  Rows
        // must keep their 16-byte alignment: frames % 4 == 0.  (IDSP_LOCKIN_NO_LM_TAIL: lockin_lm_body of what is now lockin_phase.hip read it, lm_body of
        // lockin_generic.hip did not.)  The tail is never the two-thread split.
        const bool tail = lm && !(lowpass_phase && sw.no_lm_tail) && c.frames >= thr::kLockinTailMinFrames && c.frames % 4 == 0 && c.frames % kLwBLm != 0;
        p.body = tail ? c.frames - c.frames % kLwBLm : 0;
        p.waves = tail ? waves_for(p.body) : 0;
        p.form = p.waves ? LockinForm::WavesTail : LockinForm::Stream;
        if (!p.waves) return p.body = 0, p;
    }
    p.split = false;

    // The stage-wave kernel (lockin_waves.h: measured there): K = 2 lowpass arms on the internal phase, whole 64-lane groups, whole
    // batches, aligned rows, FrameMajor.  Up to 16384 lanes one group per workgroup for every read-out; above, the `arg` read-out only, two groups.
    if (lowpass_phase && c.cascade == 2 && !sw.no_stages && !lm && p.body % kLsB == 0 && c.lanes % kPlanWave == 0 && c.x % 16 == 0) {
        const bool pairs = c.lanes % (2 * kPlanWave) == 0;
        p.groups = sw.stage_groups == 1 || (sw.stage_groups == 2 && pairs) ? sw.stage_groups
                   : c.lanes <= thr::kLockinStagesOneGroupMaxLanes   ? 1
                   : arg && pairs                                    ? 2
                                                                     : 0;
        if (p.groups) return p.form = LockinForm::Stages, p.waves = 0, p;
    }

    // 16-frame batches halve the barriers per frame: 0.37 -> 0.35 ms (Complex<i32>), 0.61 -> 0.59 ms (arg) at 32768 lanes x 4096
    // frames, but 1.06 -> 1.19 ms (arg) at 65536 lanes, where the longer intervals cost more than the barriers.
    // The 6-wave form keeps 8-frame batches above one workgroup per CU: with 16 (66 KiB of LDS) only ONE 6-wave workgroup runs on a CU at a
    // time — every second workgroup started after the first had finished (tools/exp_lockin_trace.hip) although the occupancy API promises two.
    // Four workgroups per CU (49152 < lanes <= 65536) also take 16-frame batches: two co-resident workgroups in two rounds, where the 8-frame
    // form's three leave a round of one (0.649 against 0.581 of the HBM peak at 65536 lanes; 49152: 0.557 against 0.654, 98304: 0.649 against 0.666,
    // profiles/r03_exp_lockin_batch_v2.jsonl)
    const bool b16 = sw.batch == 16 ||
                     (sw.batch != 8 && (p.waves == 4 ? c.lanes <= sw.split_max_lanes || (c.lanes > thr::kLockinB16MinLanes && c.lanes <= thr::kLockinB16MaxLanes)
                                                     : c.lanes <= thr::kLockinSixWavesMaxLanes));
    if (lm) {
        // input by DMA (whole 128-byte lines, each requested once) for the 4-wave I/Q and norm_sqr forms: 0.48 -> 0.43-0.44 ms
        // at 32768 lanes x 4096 frames, 0.94 -> 0.86 at 65536; its 32 KiB ring halves the workgroups a CU can hold, which
        // costs the 6-wave form and the arg read-out more than the input gains (tools/exp_lockin_lm.py)
        p.in = !sw.no_dma && p.waves == 4 && !arg ? IN_LM_DMA : IN_LM_REG;
        p.batch = kLwBLm;
        // start-up stagger (lockin_waves.h, kLwSkewTicks): LaneMajor launches that fill the chip, long enough for the wait to pay
        // (one workgroup per CU: 16384 x 4096 0.217 -> 0.225 ms with it; 32768 lanes x 2048 frames 0.187 -> 0.179, x 4096 0.350 -> 0.323,
        // x 16384 1.335 -> 1.358: long calls drift apart by themselves; 65536 x 4096 0.696 -> 0.640)
        const bool stagger = !sw.no_skew && (c.lanes + kPlanWave - 1) / kPlanWave >= thr::kStaggerMinWorkgroups && p.body >= thr::kStaggerMinFrames &&
                             p.body <= thr::kStaggerMaxFrames && c.tuned_device;
        p.skew = stagger ? thr::kLockinStaggerTicks : 0u;
    } else if (!sw.no_dma && c.lanes % kPlanWave == 0 && c.x % 16 == 0) {
        p.in = IN_FM_DMA;
        p.batch = b16 ? 16 : kLwB;
    } else {
        p.in = IN_FM_REG;
        p.batch = kLwB;
    }
    return p;
}

}  // namespace idsp
