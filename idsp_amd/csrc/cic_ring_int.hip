// cic_ring_int.hip — host side and instantiations of the wave-per-lane Cic interpolator (cic_ring.h).
#include "cic_ring_host.h"

namespace idsp {

using namespace cicr;
using namespace cicr_host;

template <class T>
int cic_ring_int_launch(const CicPlan &p, const idsp_cic *cfg, uint32_t *st, const T *x, T *y, size_t lanes, size_t frames, hipStream_t stream)
{
    return for_order_pieces(cfg->order, p.ppt, [&](auto n_, auto pieces) {
        constexpr int N = decltype(n_)::value, PPT = decltype(pieces)::value;
        using UT = typename std::make_unsigned<T>::type;
        constexpr size_t R = size_t(PPT) * 16 / sizeof(T);
        IntCoef<T, N> coef{};
        coef.scan = scan_coef<T, N>(R);
        // h = the chain after R steps on constant input 1 from zero (src/cic.rs:174-180), wrapping
        uint64_t z[N] = {};
        for (size_t s = 0; s < R; s++) {
            uint64_t v = 1;
            for (int n = 0; n < N; n++) {
                z[n] += v;
                v = z[n];
            }
        }
        for (int n = 0; n < N; n++) coef.h[n] = UT(z[n]);
        note_kernel(cic_plan_name(p));
        // FrameMajor: whole groups of 16 lanes whose rows of y start on 16-byte boundaries (they do: whole pieces per chunk)
        if (p.form == CicForm::RingFm) {
            constexpr size_t fbytes = size_t(kW) * (kFmLanes * PPT + 1) * 16 + size_t(kW) * (kFmLanes + 1) * sizeof(T);
            static_assert(fbytes <= 160 * 1024, "one workgroup per CU at least");
            if (const int rc = ensure_dyn_lds<&cic_int_ring_fm<T, N, PPT>>(fbytes)) return rc;
            hipLaunchKernelGGL((cic_int_ring_fm<T, N, PPT>), dim3(p.grid), dim3(kFmLanes * kW), fbytes, stream, coef, int(cfg->comb_delay), st, x, y, lanes, frames);
            return launch_status();
        }
        constexpr size_t bytes = size_t(kW) * (PPT + 1) * 16;
        if (const int rc = ensure_dyn_lds<&cic_int_ring_lm<T, N, PPT>>(bytes)) return rc;
        hipLaunchKernelGGL((cic_int_ring_lm<T, N, PPT>), dim3(p.grid), dim3(kW), bytes, stream, coef, int(cfg->comb_delay), st, x, y, lanes, frames);
        return launch_status();
    });
}

template int cic_ring_int_launch<int32_t>(const CicPlan &, const idsp_cic *, uint32_t *, const int32_t *, int32_t *, size_t, size_t, hipStream_t);
template int cic_ring_int_launch<int64_t>(const CicPlan &, const idsp_cic *, uint32_t *, const int64_t *, int64_t *, size_t, size_t, hipStream_t);

}  // namespace idsp
