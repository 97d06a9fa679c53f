// rpll_procs.h — the reciprocal PLL of the reference (`RPLLConfig` x `RPLL`, src/rpll.rs:13-78) as a stream processor (processor
// contract: lane_stream.h).  All wrapping u32 / i32 / u64 arithmetic, one lane per thread, the four state words in registers for
// the call; the library is built with -fwrapv (phase_procs.h).
#pragma once
#include "lane_stream.h"

namespace idsp {
namespace {

// `RPLLConfig` (:23-36) with everything that depends on the shifts alone worked out on the host: kernarg, i.e. SGPR, values.
struct RpllParams {
    int32_t dt2;      // `f >> dt2` (:70)
    int32_t sf;       // `>> shift_frequency` (:61), 1..32
    int32_t sdy;      // `shift_phase - dt2` (:72), 0..31
    uint32_t half;    // `1u32 << (shift_frequency - 1)` (:60)
    uint32_t p_ref;   // `1u32 << (32 + dt2 - shift_frequency)` (:64)
    uint32_t dt_mask; // `(1 << dt2) - 1` (:68)
};

// `Option<W<i32>>` as two adjacent words { some, x } and `Accu<W<i32>>` as { state, step }
typedef int32_t rpll_pair __attribute__((ext_vector_type(2)));

// `RPLLConfig::process` (src/rpll.rs:47-77).  `some` differs from lane to lane, so the `if let Some` is a select on the three
// state words it guards (y moves either way): both sides are computed, there is no divergent branch.
// :58 `state.ff.0 as u64 * dx.0 as u64`: `dx.0 as u64` SIGN-extends an i32, and the product wraps modulo 2^64.  Its low 64 bits
// are ff * (u32)dx — one v_mad_u64_u32, the rounding bias of :60 riding in the addend — minus ff << 32 when dx < 0: a select
// and a subtract on the high word, no 64 x 64 multiply (PllProc's low-half term, phase_procs.h, is the same trick).
struct RpllProc {
    using In = rpll_pair;
    using Out = rpll_pair;
    static constexpr bool HAS_IN = true;
    static constexpr int LDS_WORDS = 0;
    static constexpr int IN_DIV = 1;
    // one v_mad_u64_u32 and one v_mul_lo_u32 (quarter rate: 16 cycles per wave each) + ~30 full-rate instructions (the 64-bit
    // shift, the three selects), one serial chain: PllProc's estimate (160) with two multiplies fewer and the selects more
    static constexpr int COST = 150;
    using Params = RpllParams;
    int32_t x0, y;
    uint32_t ff, f;
    __device__ __forceinline__ void load(const Params &, const uint32_t *st, size_t lanes, size_t lane)
    {
        x0 = int32_t(st[lane]);
        ff = st[lanes + lane];
        f = st[2 * lanes + lane];
        y = int32_t(st[3 * lanes + lane]);
    }
    __device__ __forceinline__ void store(const Params &, uint32_t *st, size_t lanes, size_t lane) const
    {
        st[lane] = uint32_t(x0);
        st[lanes + lane] = ff;
        st[2 * lanes + lane] = f;
        st[3 * lanes + lane] = uint32_t(y);
    }
    __device__ __forceinline__ Out step(const Params &p, In in)
    {
        const bool some = in.x != 0;
        const int32_t x = in.y;
        y += int32_t(f);                                                               // :51
        const uint32_t dx = uint32_t(x) - uint32_t(x0);                                // :54
        uint64_t p64 = uint64_t(ff) * uint64_t(dx) + uint64_t(p.half);                 // :58, :60
        p64 -= uint64_t(int32_t(dx) < 0 ? ff : 0u) << 32;                              // :58 the sign extension of dx
        const uint32_t p_sig = uint32_t(p64 >> p.sf);                                  // :61-62 logical shift, truncation
        const uint32_t nff = ff + (p.p_ref - p_sig);                                   // :66
        const uint32_t dt = (0u - uint32_t(x)) & p.dt_mask;                            // :68
        const uint32_t y_ref = (f >> p.dt2) * dt;                                      // :70 the OLD f
        const int32_t dy = int32_t(y_ref - uint32_t(y)) >> p.sdy;                      // :72 y already advanced; arithmetic shift
        const uint32_t nf = nff + uint32_t(dy);                                        // :74 the NEW ff
        x0 = some ? x : x0;                                                            // :56
        ff = some ? nff : ff;
        f = some ? nf : f;
        return Out{y, int32_t(f)};                                                     // :76
    }
};

}  // namespace
}  // namespace idsp
