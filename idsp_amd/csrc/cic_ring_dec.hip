// cic_ring_dec.hip — host side and instantiations of the wave-per-lane Cic decimator (cic_ring.h).
#include "cic_ring_host.h"

namespace idsp {

using namespace cicr;
using namespace cicr_host;

template <class T>
int cic_ring_dec_launch(const CicPlan &p, const idsp_cic *cfg, uint32_t *st, const T *x, T *y, size_t lanes, size_t frames, hipStream_t stream)
{
    return for_order_pieces(cfg->order, p.ppt, [&](auto n, auto pieces) {
        constexpr int N = decltype(n)::value, PPT = decltype(pieces)::value;
        const ScanCoef<T, N> coef = scan_coef<T, N>(size_t(PPT) * 16 / sizeof(T));
        constexpr size_t bytes = 2 * size_t(PPT) * 1024;
        if (const int rc = ensure_dyn_lds<&cic_dec_ring_lm<T, N, PPT>>(bytes)) return rc;
        note_kernel(cic_plan_name(p));
        hipLaunchKernelGGL((cic_dec_ring_lm<T, N, PPT>), dim3(p.grid), dim3(kW), bytes, stream, coef, int(cfg->comb_delay), st, x, y, lanes, frames);
        return launch_status();
    });
}

template int cic_ring_dec_launch<int32_t>(const CicPlan &, const idsp_cic *, uint32_t *, const int32_t *, int32_t *, size_t, size_t, hipStream_t);
template int cic_ring_dec_launch<int64_t>(const CicPlan &, const idsp_cic *, uint32_t *, const int64_t *, int64_t *, size_t, size_t, hipStream_t);

}  // namespace idsp
