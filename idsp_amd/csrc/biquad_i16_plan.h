// biquad_i16_plan.h — which kernel form of biquad_i16_kernels.h a pass of idsp_biquad_i16_df1 / _df1_clamp takes, and on what grid: a
// pure function of the shape, the two addresses and the two pitches.  No HIP in this header: tests/cpp/biquad_i16_plan_cli.cpp
// compiles it with plain g++ and tests/test_biquad_i16_plan.py pins the table on the CPU.
//
// The element is 2 bytes, so a form is about how a wave's memory request gets its width:
//   FRAME_MAJOR  one form     a thread owns one lane and moves one 16-bit element per frame: 128 B per wave and frame, on lanes / 64
//                             waves.  Any lane count, any 2-byte-aligned address, any pitch.  (Lane pairs on dwords were built,
//                             measured and dropped: biquad_i16_kernels.h.)
//   LANE_MAJOR   dword runs   a dword holds two consecutive frames of one lane; a 64-lane x 128-frame tile moves as 64 dwords per
//                             lane.  Needs every lane's row on the 4-byte grid: x and y on it, even pitches.  An odd frame count
//                             is fine: the last element of a lane moves as a 16-bit access.
//                half runs    the same tile through 16-bit accesses, for every other address and pitch.
#pragma once

#include <cstddef>
#include <cstdint>

namespace idsp {
namespace bq16 {

constexpr int kWave = 64;
// (sections fused per launch, bq16::kMaxChain: biquad_pass_plan.h)
// Threads per FRAME_MAJOR workgroup.  One wave, so that few waves still spread over all CUs, until the waves fill every SIMD of a 256-CU
// part once; from there four.  Measured at 4096 frames with 64 / 256: 16384 lanes 0.158 / 0.162 ms, 65536 lanes 0.208 / 0.199
// (profiles/NOTES.md, "Biquad i16"); nothing between or beyond was measured.
constexpr unsigned kFmBlockSmall = 64, kFmBlockBig = 256;
constexpr size_t kFmBigMinLanes = 65536;

enum Form { kFmPlain = 1, kLmDwordRuns = 2, kLmHalfRuns = 3 };

// what a measurement may override (IDSP_DIAG=1 only, common.h: diag_env)
struct Switches {
    unsigned fm_block = 0;  // IDSP_BQ16_FM_BLOCK: threads per FRAME_MAJOR workgroup, 64..256 in whole waves; 0: the rule above
};

struct Plan {
    Form form;
    unsigned grid, block;
    const char *name;  // what idsp_last_kernel() reports
};

// both rows of a pass keep element 2 i of every row in the low half of an aligned dword
inline bool on_dword_grid(uintptr_t x, uintptr_t y, size_t xl, size_t yl) { return x % 4 == 0 && y % 4 == 0 && xl % 2 == 0 && yl % 2 == 0; }

// xl / yl: elements between row starts (never 0 here: the entry has replaced a dense 0 by the row length)
inline Plan plan_biquad_i16(bool lane_major, size_t lanes, uintptr_t x, uintptr_t y, size_t xl, size_t yl, const Switches &sw = {})
{
    const bool grid4 = on_dword_grid(x, y, xl, yl);
    if (lane_major) {
        const unsigned grid = unsigned((lanes + kWave - 1) / kWave);
        return grid4 ? Plan{kLmDwordRuns, grid, unsigned(kWave), "biquad_i16_lane_major[dword runs]"}
                     : Plan{kLmHalfRuns, grid, unsigned(kWave), "biquad_i16_lane_major[half runs]"};
    }
    unsigned block = lanes >= kFmBigMinLanes ? kFmBlockBig : kFmBlockSmall;
    if (sw.fm_block >= 64 && sw.fm_block <= 256 && sw.fm_block % 64 == 0) block = sw.fm_block;
    return Plan{kFmPlain, unsigned((lanes + block - 1) / block), block, "biquad_i16_frame_major"};
}

// idsp_biquad_i16_df1_bylane / _df1_clamp_bylane (biquad_i16_bylane.hip): the same form on the same grid — where a section's
// coefficients come from changes nothing about how rows move —, on kernels of their own, which idsp_last_kernel() tells apart
inline const char *bylane_name(Form form)
{
    switch (form) {
    case kLmDwordRuns: return "biquad_i16_bylane_lane_major[dword runs]";
    case kLmHalfRuns: return "biquad_i16_bylane_lane_major[half runs]";
    default: return "biquad_i16_bylane_frame_major";
    }
}
inline Plan plan_biquad_i16_bylane(bool lane_major, size_t lanes, uintptr_t x, uintptr_t y, size_t xl, size_t yl, const Switches &sw = {})
{
    Plan pl = plan_biquad_i16(lane_major, lanes, x, y, xl, yl, sw);
    pl.name = bylane_name(pl.form);
    return pl;
}

}  // namespace bq16
}  // namespace idsp
