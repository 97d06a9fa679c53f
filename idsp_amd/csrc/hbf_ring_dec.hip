// hbf_ring_dec.hip — instantiates the LDS-DMA ring decimator cascades of hbf_ring.h (FrameMajor /16).
#include "hbf_ring.h"

namespace idsp {
int hbf_ring_launch(const HbfCall &c, const HbfPlan &p, uint32_t *st, const float *x, float *y, hipStream_t stream)
{
    return for_cascade(c.tap_set, c.stages, [&](auto ts, auto s) {
        if constexpr (decltype(s)::value == thr::kHbfRingStages)
            return hbfr::launch_ring<decltype(ts)::value, decltype(s)::value>(p, st, x, y, c.lanes, c.frames, stream);
        else
            return fail(IDSP_EINVAL, "no %s for %d stages", hbf_plan_name(p), c.stages);
    });
}
}  // namespace idsp
