// hbf_wave_int.hip — instantiates the specialised interpolator cascades of hbf_wave.h.
#include "hbf_wave.h"

namespace idsp {
int hbf_wave_int_launch(const HbfCall &c, const HbfPlan &p, uint32_t *st, const float *x, float *y, hipStream_t stream)
{
    return hbfw::launch_waves<false>(c, p, st, x, y, stream);
}
}  // namespace idsp
