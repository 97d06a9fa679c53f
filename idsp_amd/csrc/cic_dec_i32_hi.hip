// cic_dec_i32_hi.hip — kernels of idsp_cic_dec_i32 for orders 4..6 (entry point in cic_dec_i32.hip).
#include "cic_kernels.h"

namespace idsp {
namespace cic {
template int run_orders<int32_t, true, 4>(const CicPlan &, const idsp_cic *, uint32_t *, const int32_t *, int32_t *, size_t, size_t, int, hipStream_t);
}  // namespace cic
}  // namespace idsp
