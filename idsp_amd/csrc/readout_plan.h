// readout_plan.h — which kernel a call of idsp_fm_disc_i32 and of idsp_dds_i32 takes, as ONE pure function each (as lockin_plan.h is for
// the lock-in entries and resample_plan.h for the half-band and Cic ones): `plan_fm_disc` / `plan_dds` read the call and the diagnostic
// switches and return the decision; the entries (fm_disc.hip, dds.hip) switch on it and launch.  tests/test_fm_disc_plan.py runs the same
// functions through tests/cpp/stream_plan_cli.cpp without a GPU.  No HIP here: plain C++17.  Thresholds: dispatch_thresholds.h,
// "FM discriminator and DDS", and kFmDiscStaggerTicks with the window of the "start-up stagger" section.
#pragma once

#include <cstdint>

#include "stream_plan.h"

namespace idsp {

// ------------------------------------------------------------------------------------------------------------ FM discriminator
struct FmDiscCall {
    size_t lanes = 0, frames = 0;  // neither is 0: the entry returns first
    int layout = IDSP_FRAME_MAJOR;
    uintptr_t x = 0, y = 0;     // the two addresses
    bool tuned_device = false;  // stagger_tuned_device(), common.h (the entry asks for LaneMajor calls only)
};

// The kernel-selection switches of idsp_fm_disc_i32 (profiles/NOTES.md, "Kernel-selection switches"), honoured only with IDSP_DIAG=1.
struct FmDiscSwitches {
    static constexpr size_t kNotForced = ~size_t(0);
    size_t waves = kNotForced;     // IDSP_FM_DISC_WAVES (FrameMajor): 0 the one-thread-per-lane stream kernel, 3 three front waves, anything else four
    bool no_lm_waves = false;      // IDSP_FM_DISC_LM_WAVES=0: LaneMajor never on the line-wise role kernel
    size_t skew = kNotForced;      // IDSP_FMD_SKEW: start-up stagger in 10 ns ticks, whatever the shape and the device
    unsigned skew_shift = 4, skew_mod = 4;  // IDSP_FMD_SKEW_SHIFT (0..31), IDSP_FMD_SKEW_MOD (at least 1): workgroup b waits ((b >> shift) % mod) * skew
};

// `env(name)`: the variable's text or NULL (the library passes `diag_env`).  The one reader of these five.
template <class Env>
FmDiscSwitches read_fm_disc_switches(Env env)
{
    const auto num = [&](const char *name, size_t dflt) {
        const char *e = env(name);
        return e ? size_t(strtoull(e, nullptr, 10)) : dflt;
    };
    FmDiscSwitches s;
    s.waves = num("IDSP_FM_DISC_WAVES", s.waves);
    s.no_lm_waves = num("IDSP_FM_DISC_LM_WAVES", 1) == 0;
    s.skew = num("IDSP_FMD_SKEW", s.skew);
    s.skew_shift = unsigned(num("IDSP_FMD_SKEW_SHIFT", s.skew_shift)) & 31u;
    s.skew_mod = unsigned(num("IDSP_FMD_SKEW_MOD", s.skew_mod));
    if (s.skew_mod == 0) s.skew_mod = 1;
    return s;
}

enum class FmDiscForm {
    Stream,       // launch_stream<FmDiscProc>: one thread per lane (the stream launcher records its own name)
    WavesFm,      // fm_disc_waves_kernel<front_waves>: FrameMajor, the discriminator on front waves, the deemphasis biquad on one more
    WavesLm,      // fm_disc_waves_lm_kernel: LaneMajor rows of whole 32-frame tiles
    WavesLmTail,  // ... on the whole tiles of every row, the stream kernel on the last frames % 32 behind it
};

struct FmDiscPlan {
    FmDiscForm form = FmDiscForm::Stream;
    int front_waves = 0;       // 3 / 4 (WavesFm)
    unsigned grid = 0;         // workgroups of 64 lanes (the three role-wave forms)
    size_t body = 0, tail = 0;  // frames of every row on the role kernel / behind it on the stream kernel (WavesLm, WavesLmTail)
    unsigned skew = 0, skew_shift = 0, skew_mod = 1;  // start-up stagger: kernel arguments (WavesLm, WavesLmTail)
};

// what note_kernel records for the plan (Stream: the stream launcher's own name, stream_plan_name; every one of them begins so)
inline const char *fm_disc_plan_name(const FmDiscPlan &p)
{
    switch (p.form) {
        case FmDiscForm::WavesFm: return p.front_waves == 3 ? "fm_disc_waves_kernel<3>" : "fm_disc_waves_kernel<4>";
        case FmDiscForm::WavesLm: return "fm_disc_waves_lm_kernel";
        case FmDiscForm::WavesLmTail: return "fm_disc_waves_lm_kernel + stream_lane_major (last frames % 32)";
        default: return "stream_";
    }
}

inline FmDiscPlan plan_fm_disc(const FmDiscCall &c, const FmDiscSwitches &sw)
{
    FmDiscPlan p;
    const unsigned grid = unsigned((c.lanes + kPlanWave - 1) / kPlanWave);
    if (c.layout == IDSP_FRAME_MAJOR) {
        // The discriminator on four front waves, the deemphasis biquad on a fifth (IDSP_FM_DISC_WAVES = 0: the one-thread-per-lane stream
        // kernel; = 3: three front waves).  Up to kFmDiscWavesMaxLanes: beyond, the stream kernel has two waves per SIMD itself and fewer
        // instructions per sample (no LDS hand-over, no second read of the previous row).  A front wave takes eight frames of a tile.
        const size_t waves = sw.waves != FmDiscSwitches::kNotForced ? sw.waves : c.lanes <= thr::kFmDiscWavesMaxLanes ? 4 : 0;
        if (waves && c.frames >= thr::kFmDiscFmMinFrames) p.form = FmDiscForm::WavesFm, p.front_waves = waves == 3 ? 3 : 4, p.grid = grid;
        return p;
    }
    // LaneMajor, the line-wise role kernel: rows of any multiple of 16 frames from one 32-frame tile up, 16-byte aligned, 32-bit thread
    // offsets inside a row — the whole tiles on it, the last 16 frames of a row that is not whole tiles on the tile kernel behind it (same
    // stream, rows at the call's pitch, the state carries over as between two calls).  Multiples of 16 keep the input lines on the 128-byte
    // grid; rows off it lose more to straddled lines than the role waves win (65536 lanes x 4100 / 4104 / 4124 frames: 1.52 / 1.37 / 1.51 ms
    // against 1.29 on the tile kernel; 4112 frames: 1.01).
    if (sw.no_lm_waves || c.frames < thr::kFmDiscLmTile || c.frames % thr::kFmDiscLmRowMultiple != 0 || c.lanes >= thr::kFmDiscLmMaxLanes ||
        (c.x | c.y) % thr::kPieceBytes != 0)
        return p;
    p.tail = c.frames % thr::kFmDiscLmTile;
    p.body = c.frames - p.tail;
    p.form = p.tail ? FmDiscForm::WavesLmTail : FmDiscForm::WavesLm;
    p.grid = grid;
    // Start-up stagger (lockin_waves.h, "lanes in phase"): arithmetic alone 0.535 ms at 65536 lanes x 4096 frames, with the requests
    // 0.60, with the stores 0.555 — and with both 0.92: every lane reads and writes the same offset of its rows at the same time.
    // Four groups of CUs 12 us apart: 0.926 -> 0.834 ms (6 us 0.884, 24 us 0.827, 48 us 0.97; groups per XCD or per
    // workgroup pair nothing; tools/exp_fm_disc_skew.sh).  The window is the lock-in's (plan_lockin), on the frames of the whole call.
    const bool stagger = grid >= thr::kStaggerMinWorkgroups && c.frames >= thr::kStaggerMinFrames && c.frames <= thr::kStaggerMaxFrames && c.tuned_device;
    p.skew = sw.skew != FmDiscSwitches::kNotForced ? unsigned(sw.skew) : stagger ? thr::kFmDiscStaggerTicks : 0u;
    p.skew_shift = sw.skew_shift, p.skew_mod = sw.skew_mod;
    return p;
}

// ------------------------------------------------------------------------------------------------------------------------- DDS
struct DdsCall {
    size_t lanes = 0, frames = 0;
    int layout = IDSP_FRAME_MAJOR;
};

struct DdsSwitches {
    bool no_circle = false;                        // IDSP_DDS_NO_CIRCLE: the 512-byte cossin table everywhere
    size_t split_max_lanes = thr::kSplitMaxLanes;  // IDSP_SPLIT_MAX_LANES: the lock-in family's (lockin_plan.h reads it too)
};

template <class Env>
DdsSwitches read_dds_switches(Env env)
{
    DdsSwitches s;
    s.no_circle = env("IDSP_DDS_NO_CIRCLE") != nullptr;
    if (const char *e = env("IDSP_SPLIT_MAX_LANES")) s.split_max_lanes = size_t(strtoull(e, nullptr, 10));
    return s;
}

struct DdsPlan {
    bool split = false;   // the re and im of a lane on two threads (DdsSplitProcT) — too few lanes to give every SIMD a wave otherwise
    bool circle = false;  // cossin through the full-circle table (dds_dev.h cossin_circle; the split form only)
};

inline DdsPlan plan_dds(const DdsCall &c, const DdsSwitches &sw)
{
    DdsPlan p;
    p.split = c.lanes <= sw.split_max_lanes;
    // The full-circle table is 16 KiB of LDS per workgroup, filled at the start of every workgroup: FrameMajor calls long enough to pay for
    // the fill (LaneMajor: the staged kernel needs the LDS for the 32 KiB tile slot of every wave).  One thread per lane keeps the 512-byte
    // table: 65536 lanes x 4096 run 0.36-0.37 ms with it and 0.46 with the full-circle table, 24- or 16-byte entries alike
    // (profiles/r03_perf_dds_circle.jsonl, r03_perf_dds_one_circle.jsonl)
    p.circle = p.split && !sw.no_circle && c.layout == IDSP_FRAME_MAJOR && c.frames >= thr::kDdsCircleMinFrames;
    return p;
}

}  // namespace idsp
