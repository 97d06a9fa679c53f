// phase_procs.h — the phase consumers behind the lock-in / atan2 / discriminator outputs as stream processors (processor contract:
// lane_stream.h): `ClampWrap<W<i32>>` and `Unwrapper<i64>` (src/unwrap.rs) and the `PLL` (src/pll.rs).  All wrapping integer
// arithmetic, one lane per thread, the whole per-lane state in registers for the call; the library is built with -fwrapv, so plain
// signed arithmetic has the semantics of a Rust release build (as in dds_dev.h, lowpass_step).
#pragma once
#include "lane_stream.h"

namespace idsp {
namespace {

// `ClampWrap<W<i32>>::process` (src/unwrap.rs:184-193) on `overflowing_sub` (:73-80) and `Wrap + Wrap` (:49-55).
// `clamp` holds the `Wrap` discriminant -1 / 0 / 1.
__device__ __forceinline__ int32_t clamp_wrap_step(int32_t &x0, int32_t &clamp, int32_t x)
{
    const int32_t delta = int32_t(uint32_t(x) - uint32_t(x0));            // :77 y.wrapping_sub(&x)
    const int32_t wrap = int32_t(delta >= 0) - int32_t(x >= x0);          // :78 (delta >= 0).cmp(&(y >= x)): false < true
    x0 = x;                                                                // :186
    const int32_t c = clamp + wrap;                                        // :53 (self as i32 + rhs as i32).cmp(&0)
    clamp = int32_t(c > 0) - int32_t(c < 0);
    return clamp == 0 ? x : (INT32_MAX ^ (clamp >> 31));                   // :188-192 Negative -> MIN, None -> x, Positive -> MAX
}

// (no configuration: a one-word kernarg POD keeps the processor contract's `Params` by value)
struct NoParams {
    int32_t reserved;
};

struct ClampWrapProc {
    using In = int32_t;
    using Out = int32_t;
    static constexpr bool HAS_IN = true;
    static constexpr int LDS_WORDS = 0;
    static constexpr int IN_DIV = 1;
    static constexpr int COST = 40;  // ~10 full-rate VALU instructions per sample
    using Params = NoParams;
    int32_t x0, clamp;
    __device__ __forceinline__ void load(const Params &, const uint32_t *st, size_t lanes, size_t lane)
    {
        x0 = int32_t(st[lane]);
        clamp = int32_t(st[lanes + lane]);
    }
    __device__ __forceinline__ void store(const Params &, uint32_t *st, size_t lanes, size_t lane) const
    {
        st[lane] = uint32_t(x0);
        st[lanes + lane] = uint32_t(clamp);
    }
    __device__ __forceinline__ Out step(const Params &, In x) { return clamp_wrap_step(x0, clamp, x); }
};

// `Unwrapper<i64>` fed `i32` (src/unwrap.rs:151-155).  MODE 0: the wrapped difference `dx` (what `process` returns);
// MODE 1: the running `y` (`phase::<i64>()`, :130-136) after the sample.
template <int MODE>
struct UnwrapProc {
    using In = int32_t;
    using Out = std::conditional_t<MODE == 0, int32_t, int64_t>;
    static constexpr bool HAS_IN = true;
    static constexpr int LDS_WORDS = 0;
    static constexpr int IN_DIV = 1;
    static constexpr int COST = 16;  // sub, sign extension, 64-bit add
    // two-word outputs: on the register-window kernel, like every other 4-byte-in / 8-byte-out processor of the library
    // (`Lockin` -> Complex<i32>, -> norm_sqr); by its cost alone this would be the first to take the sweep kernel with them
    static constexpr bool LDS_ELIGIBLE = MODE == 0;
    using Params = NoParams;
    int64_t y;
    __device__ __forceinline__ void load(const Params &, const uint32_t *st, size_t lanes, size_t lane)
    {
        y = int64_t(uint64_t(st[lane]) | (uint64_t(st[lanes + lane]) << 32));
    }
    __device__ __forceinline__ void store(const Params &, uint32_t *st, size_t lanes, size_t lane) const
    {
        st[lane] = uint32_t(uint64_t(y));
        st[lanes + lane] = uint32_t(uint64_t(y) >> 32);
    }
    __device__ __forceinline__ Out step(const Params &, In x)
    {
        const int32_t dx = int32_t(uint32_t(x) - uint32_t(uint64_t(y)));  // :152 x.wrapping_sub(&self.y.as_())
        y += int64_t(dx);                                                  // :153 self.y.wrapping_add(&dx.as_())
        if constexpr (MODE == 0)
            return dx;
        else
            return y;
    }
};

struct PllParams {
    int32_t ba[3];  // `PLL::ba` as `Q32<32>` bits (src/pll.rs:37)
};

// `{ process(), frequency() }` of one sample, adjacent like Complex<i32>
struct PhaseFreq {
    int32_t phase, frequency;
};
static_assert(sizeof(PhaseFreq) == 8, "two adjacent words");

// `PLL::process` (src/pll.rs:90-107) on `PLLState` (:62-75).  MODE 0: the phase `process` returns; MODE 1: `frequency()` (:84-86)
// after the sample; MODE 2: both.
// `Q32<32> * i32` is the widened product `Q<i64, i32, 32>` (dsp-fixedpoint/src/ops.rs:91-97 -> src/lib.rs:310-312), so the three
// products and their sum are i64 — one v_mad_i64_i32 each, chained through the addend.  The low-half term
// `(a1 as i64 * f0 as u32 as i64) >> 32` is a signed x unsigned 32-bit product: its high half is
// mulhi_u32(a1, lo) - (a1 < 0 ? lo : 0), a value that fits i32 — one v_mul_hi_u32 and a subtract, no 64 x 64 multiply.
template <int MODE>
struct PllProc {
    using In = int32_t;
    using Out = std::conditional_t<MODE == 2, PhaseFreq, int32_t>;
    static constexpr bool HAS_IN = true;
    static constexpr int LDS_WORDS = 0;
    static constexpr int IN_DIV = 1;
    // three v_mad_i64_i32 and one v_mul_hi_u32 (quarter rate: 16 cycles per wave each) + ~24 full-rate instructions; about twice
    // `[Lowpass<2>; 1]` (80), and as serially dependent
    static constexpr int COST = 160;
    using Params = PllParams;
    int32_t x0, clamp, z0, y0, y;
    int64_t f0, f;
    __device__ __forceinline__ void load(const Params &, const uint32_t *st, size_t lanes, size_t lane)
    {
        auto w = [&](int i) { return st[size_t(i) * lanes + lane]; };
        x0 = int32_t(w(0));
        clamp = int32_t(w(1));
        z0 = int32_t(w(2));
        y0 = int32_t(w(3));
        f0 = int64_t(uint64_t(w(4)) | (uint64_t(w(5)) << 32));
        f = int64_t(uint64_t(w(6)) | (uint64_t(w(7)) << 32));
        y = int32_t(w(8));
    }
    __device__ __forceinline__ void store(const Params &, uint32_t *st, size_t lanes, size_t lane) const
    {
        auto w = [&](int i, uint32_t v) { st[size_t(i) * lanes + lane] = v; };
        w(0, uint32_t(x0));
        w(1, uint32_t(clamp));
        w(2, uint32_t(z0));
        w(3, uint32_t(y0));
        w(4, uint32_t(uint64_t(f0)));
        w(5, uint32_t(uint64_t(f0) >> 32));
        w(6, uint32_t(uint64_t(f)));
        w(7, uint32_t(uint64_t(f) >> 32));
        w(8, uint32_t(y));
    }
    __device__ __forceinline__ Out step(const Params &p, In x)
    {
        y += int32_t(f >> 32);                                               // :92 state.y += state.frequency()
        const int32_t z = clamp_wrap_step(x0, clamp, x + y) >> 1;            // :94 clamp.process(x + state.y).0 >> 1
        const int32_t yn = z + z0;                                           // :96
        z0 = z;                                                              // :97
        const uint32_t lo = uint32_t(uint64_t(f0));
        const int32_t low = int32_t(__umulhi(uint32_t(p.ba[2]), lo) - (p.ba[2] < 0 ? lo : 0u));  // :102
        int64_t d = int64_t(low);
        d += int64_t(p.ba[2]) * int64_t(int32_t(f0 >> 32));                  // :100 ba[2] * (state.f0 >> 32) as i32
        d += int64_t(p.ba[1]) * int64_t(y0);                                 // :100 ba[1] * state.y0
        d += int64_t(p.ba[0]) * int64_t(yn);                                 // :100 ba[0] * y0
        f0 += d;                                                             // :99
        y0 = yn;                                                             // :103
        f += f0;                                                             // :105
        if constexpr (MODE == 0)
            return y;                                                        // :106
        else if constexpr (MODE == 1)
            return int32_t(f >> 32);                                         // :85
        else
            return PhaseFreq{y, int32_t(f >> 32)};
    }
};

}  // namespace
}  // namespace idsp
