// lockin_waves_biquad.hip — `Lockin<[Biquad<C>; n]>` on the multi-wave lock-in kernel of lockin_waves.h: the biquad chain is one more
// arm functor (`Bank`) beside `[Lowpass<N>; K]`.  Phase form (src/lockin.rs:30-39 over src/iir/biquad.rs:366-383) for i32, and the
// external-oscillator form (src/lockin.rs:17-27) for i32 and f32 — the latter is the mix -> lowpass graph of
// examples/ddc_lockin.rs:35-42.  Round 4; the one-thread-per-lane forms (lockin_generic.hip) stay for the shapes this does not take.
#include "biquad_sections.h"
#include "lockin_waves.h"

namespace idsp {
namespace {

// n serial DF1 sections, state words {x0, x1, y0, y1} per section at `word0` (the record of idsp_lockin_biquad_state_words)
template <int NS>
struct BqBank : bq::SectionState<NS> {
    using Params = bq::ChainParams<bq::SecI32, NS>;
    static constexpr int kArmWords = 4 * NS;
    static constexpr bool kSixWaves = false;  // four waves per 64 lanes only: the arm waves are the long path with biquad arms
    static constexpr bool kExtLo = false;
    static __device__ __forceinline__ int32_t mix(int32_t lo, int32_t x) { return __mulhi(lo, x); }
    static const char *name() { return NS == 1 ? "[Biquad; 1]" : NS == 2 ? "[Biquad; 2]" : NS == 3 ? "[Biquad; 3]" : "[Biquad; 4]"; }
    __device__ __forceinline__ int32_t step(const Params &p, int32_t x)
    {
#pragma unroll
        for (int k = 0; k < NS; k++) x = bq::Df1I32<false>::step(p.sec[k], this->s[k], x);
        return x;
    }
};

// the same arms fed by a per-sample oscillator
template <int NS>
struct BqLoBank : BqBank<NS> {
    static constexpr bool kExtLo = true;
    static const char *name() { return NS == 1 ? "[Biquad; 1], LO" : NS == 2 ? "[Biquad; 2], LO" : NS == 3 ? "[Biquad; 3], LO" : "[Biquad; 4], LO"; }
};
// `[Biquad<f32>; n]` x `[DirectForm1<f32>; n]` arms on bit patterns: rows, samples and oscillator travel as 32-bit words
template <int NS>
struct BqLoBankF32 : bq::SectionState<NS> {
    using Params = bq::ChainParams<bq::SecF32, NS>;
    static constexpr int kArmWords = 4 * NS;
    static constexpr bool kSixWaves = false, kExtLo = true;
    static const char *name() { return NS == 1 ? "[Biquad<f32>; 1], LO" : NS == 2 ? "[Biquad<f32>; 2], LO" : NS == 3 ? "[Biquad<f32>; 3], LO" : "[Biquad<f32>; 4], LO"; }
    static __device__ __forceinline__ int32_t mix(int32_t lo, int32_t x) { return __float_as_int(__int_as_float(x) * __int_as_float(lo)); }
    __device__ __forceinline__ int32_t step(const Params &p, int32_t xb)
    {
        float x = __int_as_float(xb);
#pragma unroll
        for (int k = 0; k < NS; k++) x = bq::Df1F32<false>::step(p.sec[k], this->s[k], x);
        return __float_as_int(x);
    }
};

// `Bank<n>` with its sections filled, on the kernel the plan names (samples and oscillator as 32-bit words)
template <template <int> class Bank, class Fill>
int run(size_t n, const Fill &fill, void *state, const void *x, const void *lo, void *y, size_t lanes, const LockinPlan &plan, hipStream_t s, size_t pitch)
{
    return for_sections(n, [&](auto ns) {
        using B = Bank<decltype(ns)::value>;
        typename B::Params p;
        bq::fill_sections(fill, p.sec);
        return launch_lockin_waves_bank<MODE_IQ, B>(p, static_cast<uint32_t *>(state), static_cast<const int32_t *>(x), static_cast<Cplx *>(y), lanes, plan, s,
                                                    static_cast<const int32_t *>(lo), pitch);
    });
}

}  // namespace

// the caller (lockin_generic.hip) has validated the arguments and asked plan_lockin() whether the shape is the kernel's
int lockin_waves_biquad_iq(const idsp_biquad_i32 *sec, size_t n, void *state, const int32_t *x, int32_t *y, size_t lanes, const LockinPlan &plan, hipStream_t s,
                           size_t pitch)
{
    return run<BqBank>(n, bq::Fill{sec}, state, x, nullptr, y, lanes, plan, s, pitch);
}
int lockin_waves_biquad_lo(const idsp_biquad_i32 *sec, size_t n, void *state, const int32_t *x, const int32_t *lo, int32_t *y, size_t lanes,
                           const LockinPlan &plan, hipStream_t s, size_t pitch)
{
    return run<BqLoBank>(n, bq::Fill{sec}, state, x, lo, y, lanes, plan, s, pitch);
}
int lockin_waves_biquad_lo_f32(const idsp_biquad_f32 *sec, size_t n, void *state, const float *x, const float *lo, float *y, size_t lanes,
                               const LockinPlan &plan, hipStream_t s, size_t pitch)
{
    return run<BqLoBankF32>(n, bq::Fill{sec}, state, x, lo, y, lanes, plan, s, pitch);
}

}  // namespace idsp
