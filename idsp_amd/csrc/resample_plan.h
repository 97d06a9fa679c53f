// resample_plan.h — which kernel a call of idsp_hbf_{dec,int}_f32 and of idsp_cic_{dec,int}_{i32,i64} takes, as ONE pure function each
// (as lockin_plan.h is for the lock-in entries): `plan_hbf` / `plan_cic` read the call and the diagnostic switches and return the decision;
// the entries (hbf.hip `launch_hbf`, cic_kernels.h `run`) switch on its form, and the launchers of hbf_blk.h, hbf_ring.h, hbf_wave.h,
// cic_ring_{dec,int}.hip and cic_kernels.h only launch.  tests/test_resample_plan.py runs the same functions through
// tests/cpp/stream_plan_cli.cpp without a GPU.  No HIP here: plain C++17.  Thresholds: dispatch_thresholds.h, "half-band" and "Cic".
#pragma once

#include <cstdint>

#include "dispatch_thresholds.h"
#include "idsp_hip.h"

namespace idsp {

// ------------------------------------------------------------------------------------------------------------------- half-band
struct HbfCall {
    bool dec = true;
    int tap_set = -1, stages = 1;  // 0 = HBF_TAPS, 1 = HBF_TAPS_98 (hbf_taps.h), bit for bit; -1 = not a built-in set
    size_t lanes = 0, frames = 0;  // frames at the low rate
    int layout = IDSP_FRAME_MAJOR;
    uintptr_t wide = 0;  // the high-rate buffer: x of a decimator, y of an interpolator
};

// The kernel-selection switches of the half-band entries (profiles/NOTES.md, "Kernel-selection switches"), honoured only with IDSP_DIAG=1.
struct HbfSwitches {
    bool generic = false;      // IDSP_HBF_GENERIC: the generic-tap kernels for the built-in cascades too
    bool no_blk = false;       // IDSP_HBF_NO_BLK: no register-blocked LaneMajor decimator — the generic kernel then (nothing else takes those)
    bool no_ring = false;      // IDSP_HBF_NO_RING: no FrameMajor /16 ring decimator: block_fm or the wave kernel
    bool no_block_fm = false;  // IDSP_HBF_NO_BLOCK_FM: no 4-lane FrameMajor workgroups: the wave-per-lane kernels
};

// `env(name)`: the variable's text or NULL (the library passes `diag_env`).  The one reader of these four.
template <class Env>
HbfSwitches read_hbf_switches(Env env)
{
    const auto on = [&](const char *name) { return env(name) != nullptr; };
    HbfSwitches s{on("IDSP_HBF_GENERIC"), on("IDSP_HBF_NO_BLK"), on("IDSP_HBF_NO_RING"), on("IDSP_HBF_NO_BLOCK_FM")};
#ifdef IDSP_HBF_BLK_OFF  // A/B harness (tools/exp_hbf_ab.py, tools/exp_hbf_blk.sh): a library whose LaneMajor decimators never take hbf_blk.h
    s.no_blk = true;
#endif
    return s;
}

enum class HbfForm {
    Generic,  // hbf_dec_kernel / hbf_int_kernel of hbf.hip: run-time taps, a workgroup per lane
    BlkLm,    // hbf_dec_blk_lm (hbf_blk.h): LaneMajor decimators
    RingFm,   // hbf_dec_ring_fm (hbf_ring.h): FrameMajor /16 decimators on whole 16-lane groups
    BlockFm,  // hbf_dec_block_fm / hbf_int_block_fm (hbf_wave.h): FrameMajor on whole 4-lane groups
    WaveFm,   // hbf_dec_wave / hbf_int_wave<false>: FrameMajor, a wave per lane
    WaveLm,   // hbf_int_wave<true>: LaneMajor interpolators
};

struct HbfPlan {
    HbfForm form = HbfForm::Generic;
    bool dec = true;
    unsigned grid = 0;  // workgroups
};

// what note_kernel records for the plan, before the `<typeid>` detail of the specialised kernels
inline const char *hbf_plan_name(const HbfPlan &p)
{
    switch (p.form) {
        case HbfForm::BlkLm: return "hbf_dec_blk[LaneMajor]";
        case HbfForm::RingFm: return "hbf_dec_ring[FrameMajor]";
        case HbfForm::BlockFm: return p.dec ? "hbf_dec_block_fm" : "hbf_int_block_fm";
        case HbfForm::WaveFm: return p.dec ? "hbf_dec_wave[FrameMajor]" : "hbf_int_wave[FrameMajor]";
        case HbfForm::WaveLm: return "hbf_int_wave[LaneMajor]";
        default: return p.dec ? "hbf_dec_kernel (generic taps)" : "hbf_int_kernel (generic taps)";
    }
}

// grid of a kernel that gives XCD b % 8 a contiguous run of its `n` lanes or lane groups: a multiple of 8 workgroups (hbf_wave.h xcd_lane())
inline unsigned xcd_grid(size_t n) { return unsigned(8 * ((n + 7) / 8)); }

inline HbfPlan plan_hbf(const HbfCall &c, const HbfSwitches &sw)
{
    HbfPlan p{HbfForm::Generic, c.dec, 0};
    const bool lm = c.layout == IDSP_LANE_MAJOR;
    const auto take = [&](HbfForm form, size_t grid) { return p.form = form, p.grid = unsigned(grid), p; };
    // The specialised kernels: the reference's own cascades, when every 16-byte access they make is aligned — the wide buffer, LaneMajor
    // rows of whole pieces, FrameMajor frames of at least one.  f32 slices are 4-byte aligned in the reference; the generic kernels' 8- and
    // 16-byte global accesses are legal at that alignment on gfx950 (unaligned access mode), so they take anything else (custom taps, odd shapes).
    const bool fast = !sw.generic && c.tap_set >= 0 && c.wide % thr::kPieceBytes == 0 &&
                      (lm ? ((c.frames * sizeof(float)) << c.stages) % thr::kPieceBytes == 0 : c.stages >= thr::kHbfFmMinStages);
    if (fast && lm) {
        if (!c.dec) return take(HbfForm::WaveLm, c.lanes);
        // decimators: the register-blocked kernel, one workgroup per lane — and nothing behind it: neither the ring nor the wave kernels
        // have a LaneMajor decimator any more, so IDSP_HBF_NO_BLK ends on the generic kernel
        if (!sw.no_blk && c.lanes <= thr::kGridMaxLanes) return take(HbfForm::BlkLm, c.lanes);
    } else if (fast) {
        if (c.dec && !sw.no_ring && c.stages == thr::kHbfRingStages && c.lanes % thr::kHbfRingLanes == 0)
            return take(HbfForm::RingFm, xcd_grid(c.lanes / thr::kHbfRingLanes));
        if (!sw.no_block_fm && c.lanes % thr::kHbfBlockLanes == 0) return take(HbfForm::BlockFm, xcd_grid(c.lanes / thr::kHbfBlockLanes));
        return take(HbfForm::WaveFm, xcd_grid(c.lanes));
    }
    return take(HbfForm::Generic, lm ? c.lanes : xcd_grid(c.lanes));
}

// ------------------------------------------------------------------------------------------------------------------------- Cic
struct CicCall {
    bool dec = true;
    int elem_bytes = 4, order = 1;  // 4 / 8: i32 / i64 samples; the order is read by the launchers' ladder, not by the choice
    uint32_t rate = 0;              // a chunk is rate + 1 high-rate samples
    size_t lanes = 0, frames = 0;
    int layout = IDSP_FRAME_MAJOR;
    uintptr_t x = 0, y = 0;
};

struct CicSwitches {
    bool no_ring = false;      // IDSP_CIC_NO_RING: never the wave-per-lane kernels of cic_ring.h
    bool no_lm_tiles = false;  // IDSP_CIC_NO_LM_TILES: LaneMajor without the 64-lane x 16-vector LDS tiles
};

template <class Env>
CicSwitches read_cic_switches(Env env)
{
    const auto on = [&](const char *name) { return env(name) != nullptr; };
    return CicSwitches{on("IDSP_CIC_NO_RING"), on("IDSP_CIC_NO_LM_TILES")};
}

enum class CicForm {
    RingLm,     // cic_dec_ring_lm / cic_int_ring_lm (cic_ring.h): a wave per lane
    RingFm,     // cic_int_ring_fm: 16 waves per workgroup, interpolators only
    LaneTiles,  // cic_dec_lm_kernel / cic_int_lm_kernel (cic_kernels.h): a lane per thread, 64 lanes x 16 vectors through LDS
    Lane,       // cic_dec_kernel / cic_int_kernel: a lane per thread
};

struct CicPlan {
    CicForm form = CicForm::Lane;
    bool dec = true;
    int ppt = 0, vpc = 0;  // 16-byte pieces per chunk, 1 2 4 8 (ring forms) / vectors per chunk, 1 .. 16 or 0 = by element (lane forms)
    unsigned grid = 0;
};

// what note_kernel records; the two lane forms share a name
inline const char *cic_plan_name(const CicPlan &p)
{
    switch (p.form) {
        case CicForm::RingLm: return p.dec ? "cic_dec_ring[LaneMajor]" : "cic_int_ring[LaneMajor]";
        case CicForm::RingFm: return "cic_int_ring[FrameMajor]";
        default: return p.dec ? "cic_dec_kernel" : "cic_int_kernel";
    }
}

inline CicPlan plan_cic(const CicCall &c, const CicSwitches &sw)
{
    CicPlan p{CicForm::Lane, c.dec, 0, 0, 0};
    const bool lm = c.layout == IDSP_LANE_MAJOR;
    // a chunk of whole pieces in an aligned high-rate tensor (x of a decimator, y of an interpolator), how many of them, and a power of two
    const size_t chunk = (size_t(c.rate) + 1) * size_t(c.elem_bytes), pieces = chunk / thr::kPieceBytes;
    const bool whole = chunk % thr::kPieceBytes == 0 && (c.dec ? c.x : c.y) % thr::kPieceBytes == 0 && (pieces & (pieces - 1)) == 0;
    // one wave per lane (the decimator in LaneMajor only): whole blocks of chunks, a workgroup per lane or per group of 16 within the grid limit
    if (whole && !sw.no_ring && (lm || !c.dec) && chunk >= thr::kCicRingMinChunkBytes && chunk <= thr::kCicRingMaxChunkBytes &&
        c.frames >= thr::kCicRingMinFrames && c.lanes <= thr::kGridMaxLanes && (lm || c.lanes % thr::kCicRingFmLanes == 0)) {
        p.form = lm ? CicForm::RingLm : CicForm::RingFm;
        p.ppt = int(pieces);
        p.grid = lm ? unsigned(c.lanes) : xcd_grid(c.lanes / thr::kCicRingFmLanes);
        return p;
    }
    if (whole && pieces <= thr::kCicTileVecs) p.vpc = int(pieces);
    // LaneMajor tile kernels: whole blocks of lanes, at least one whole tile, both tensors aligned (their rows then are: whole vectors per chunk)
    const bool tiles = lm && p.vpc > 0 && !sw.no_lm_tiles && c.lanes % thr::kCicBlockLanes == 0 && c.frames >= thr::kCicTileVecs / size_t(p.vpc) &&
                       (c.x | c.y) % thr::kPieceBytes == 0;
    p.form = tiles ? CicForm::LaneTiles : CicForm::Lane;
    p.grid = unsigned((c.lanes + thr::kCicBlockLanes - 1) / thr::kCicBlockLanes);
    return p;
}

}  // namespace idsp
