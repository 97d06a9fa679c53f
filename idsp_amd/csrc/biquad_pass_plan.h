// biquad_pass_plan.h — how the n sections of a biquad-family call are cut into launches, and which of those launches go to the
// two-wave kernel (lane_stream.h, stream_frame_major_duo) in what split: ONE pure function for the section chains, the per-lane banks,
// the cascade, the Wdf chain and the 16-bit chains.  The entries (biquad_host.h, normal_wdf.hip, biquad_i16*.hip) ask `next_pass`,
// launch what it says and advance; tests/test_biquad_pass_plan.py runs the same function through tests/cpp/stream_plan_cli.cpp
// without a GPU.  No HIP here: plain C++17.  `duo_wanted` and its lane thresholds: stream_plan.h.
#pragma once

#include "stream_plan.h"

namespace idsp {

namespace bq {
constexpr int kMaxChain = 4;        // sections fused per launch; longer chains run in passes
constexpr int kMaxChainDuo = 8;     // ... per launch of the two-wave kernel: five to eight sections are ONE pass over HBM instead of two
constexpr int kMaxChainByLane = 2;  // per-lane banks: coefficient registers come on top of the state
constexpr int kMaxCascade = 8;      // Cascade<[Biquad; N]> shares delay lines: single launch
}  // namespace bq
namespace bq16 {
constexpr int kMaxChain = 4;  // sections fused per launch; longer chains run in passes, in place on y
}
constexpr int kWdfMaxSections = 4;  // sections fused per launch; longer chains run in passes

// What tells one family's schedule from another's
struct PassRules {
    int max_single;    // the largest launch on one wave (launch_stream)
    int max_duo;       // the largest launch on the two-wave kernel; 0: the family has no two-wave form
    int duo_min;       // the smallest section count of a launch that asks for the two-wave form
    bool four_capped;  // a launch of exactly 4 asks as duo_wanted(4, ...) — the kDuo4MaxLanes cap applies —, every other count as duo_wanted(5, ...)
};

// Shared-coefficient chains (`[C] x [S]`): 4-byte samples have the two-wave instantiations.  Four sections take them for the plain
// forms of up to 4 state words only (+9 % for plain i32 DF1, +20 % for the f32 forms, -1 % / -5 % for the clamp / wide forms, which stay)
constexpr PassRules chain_rules(size_t sample_bytes, bool clamp, int state_words)
{
    return sample_bytes == 4 ? PassRules{bq::kMaxChain, bq::kMaxChainDuo, !clamp && state_words <= 4 ? 4 : 5, true} : PassRules{bq::kMaxChain, 0, 0, false};
}
// `ByLane` banks: three or four sections of a bank in one pass on the two-wave kernel, two sections per wave
constexpr PassRules bylane_rules(size_t sample_bytes)
{
    return sample_bytes == 4 ? PassRules{bq::kMaxChainByLane, 2 * bq::kMaxChainByLane, 3, false} : PassRules{bq::kMaxChainByLane, 0, 0, false};
}
// `Cascade`: one launch whatever its length (4 sections stay on the LDS-DMA kernel: 0.69 against 0.62)
constexpr PassRules cascade_rules(size_t sample_bytes)
{
    return sample_bytes == 4 ? PassRules{bq::kMaxCascade, bq::kMaxCascade, 5, false} : PassRules{bq::kMaxCascade, 0, 0, false};
}
// `Wdf` sections: two waves from two sections up (the entry keeps a pass that holds an order above 4 on one wave)
constexpr PassRules wdf_rules() { return PassRules{kWdfMaxSections, kWdfMaxSections, 2, false}; }
// `Biquad<Q16<F>>`: never two waves
constexpr PassRules i16_rules() { return PassRules{bq16::kMaxChain, 0, 0, false}; }

// nb == 0: one launch of na sections on launch_stream; else the two-wave kernel with na sections on wave 0 and nb on wave 1
struct Pass {
    int na, nb;
};

// The next launch of a call with `remaining` sections to go.  The widest two-wave pass is tried first; where it is refused, the pass is
// the widest single-wave one, and the pass after it is decided afresh.
inline Pass next_pass(const PassRules &r, size_t remaining, size_t lanes, int layout, const StreamSwitches &sw)
{
    const int md = int(remaining < size_t(r.max_duo) ? remaining : size_t(r.max_duo));
    if (md && md >= r.duo_min && duo_wanted(md == 4 && r.four_capped ? 4 : 5, lanes, layout, sw)) return Pass{(md + 1) / 2, md / 2};
    return Pass{int(remaining < size_t(r.max_single) ? remaining : size_t(r.max_single)), 0};
}

}  // namespace idsp
