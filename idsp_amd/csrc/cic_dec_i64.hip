// cic_dec_i64.hip — C-ABI entry point idsp_cic_dec_i64 (include/idsp_hip.h) and its kernels for orders 1..3;
// orders 4..6 are instantiated in cic_dec_i64_hi.hip.  Device code in cic_kernels.h.
#include "cic_kernels.h"

namespace idsp {
namespace cic {
extern template int run_orders<int64_t, true, 4>(const CicPlan &, const idsp_cic *, uint32_t *, const int64_t *, int64_t *, size_t, size_t, int, hipStream_t);
}  // namespace cic
}  // namespace idsp

extern "C" int idsp_cic_dec_i64(const idsp_cic *cfg, void *state, const int64_t *x, int64_t *y, size_t lanes, size_t frames, int layout,
                                void *stream)
{
    return idsp::cic::run<int64_t, true>(cfg, state, x, y, lanes, frames, layout, stream);
}
