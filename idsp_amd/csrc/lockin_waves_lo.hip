// lockin_waves_lo.hip — `Lockin<[Lowpass<N>; K]>` fed by a per-sample oscillator (src/lockin.rs:17-27; idsp_lockin_i32_lo_process)
// on the multi-wave lock-in kernel: `LpBank<N, K>` with the LO taken from the caller's buffer instead of `Accu` -> cossin.
#include "lockin_waves.h"

namespace idsp {
namespace {

template <int N, int K>
struct LpLoBank : LpBank<N, K> {
    static constexpr bool kExtLo = true, kSixWaves = false;
    static const char *name() { return "[Lowpass<N>; K], LO"; }
};

}  // namespace

int lockin_waves_lowpass_lo(const idsp_lockin_i32 *cfg, void *state, const int32_t *x, const int32_t *lo, int32_t *y, size_t lanes, const LockinPlan &plan,
                            hipStream_t s, size_t pitch)
{
    const LpParams p = lp_params(cfg);
    return for_nk(cfg, [&](auto n, auto k) {
        return launch_lockin_waves_bank<MODE_IQ, LpLoBank<decltype(n)::value, decltype(k)::value>>(p, static_cast<uint32_t *>(state), x, reinterpret_cast<Cplx *>(y),
                                                                                                  lanes, plan, s, lo, pitch);
    });
}

}  // namespace idsp
