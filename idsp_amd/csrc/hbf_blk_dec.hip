// hbf_blk_dec.hip — instantiates the register-blocked half-band decimator cascades of hbf_blk.h.
#include "hbf_blk.h"

namespace idsp {
int hbf_blk_launch(const HbfCall &c, const HbfPlan &p, uint32_t *st, const float *x, float *y, hipStream_t stream)
{
    return for_cascade(c.tap_set, c.stages, [&](auto ts, auto s) {
        return hbfb::launch_blk<decltype(ts)::value, decltype(s)::value>(p, st, x, y, c.lanes, c.frames, stream);
    });
}
}  // namespace idsp
