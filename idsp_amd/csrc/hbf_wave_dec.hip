// hbf_wave_dec.hip — instantiates the specialised decimator cascades of hbf_wave.h.
#include "hbf_wave.h"

namespace idsp {
int hbf_wave_dec_launch(const HbfCall &c, const HbfPlan &p, uint32_t *st, const float *x, float *y, hipStream_t stream)
{
    return hbfw::launch_waves<true>(c, p, st, x, y, stream);
}
}  // namespace idsp
