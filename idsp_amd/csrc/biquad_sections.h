// biquad_sections.h — iir::Biquad / BiquadClamp / Cascade over many lanes
// (reference: src/iir/biquad.rs; fixed-point semantics dsp-fixedpoint/src).
//
// Each section type is a small device functor operating on the per-lane state
// words of include/idsp_hip.h held in registers; `Chain<Sec, N>` folds N
// serial sections sample-major, which yields the same values as the
// reference's stage-major slice composition (dsp-process/src/compose.rs:43-77)
// because every section is a causal function of its own input sequence.
// The extern "C" entry points live in biquad_*.hip (one translation unit per
// family so the many template instances compile in parallel); their host side —
// checks, the passes of a long chain, the launches — is biquad_host.h.
//
// Integer paths are bit-exact restatements of Rust release (wrapping)
// arithmetic: i32 x i32 -> i64 products (v_mad_i64_i32), wrapping i64 sums,
// arithmetic `>> F`, truncating casts.  Float paths keep the reference's
// left-to-right association with every product and sum rounded separately
// (the library is compiled with -ffp-contract=off; f32 denormals enabled).
#pragma once

#include <limits>
#include <type_traits>

#include "lane_stream.h"

namespace idsp {
namespace bq {

__device__ __forceinline__ int64_t mulw(int32_t c, int32_t v) { return int64_t(c) * int64_t(v); }
__device__ __forceinline__ int64_t wadd(int64_t a, int64_t b) { return int64_t(uint64_t(a) + uint64_t(b)); }
// low 32 bits of (acc >> f) for 0 <= f < 32: one v_alignbit_b32
__device__ __forceinline__ int32_t shr_lo(int64_t acc, int f)
{
    return int32_t(__builtin_amdgcn_alignbit(uint32_t(uint64_t(acc) >> 32), uint32_t(uint64_t(acc)), uint32_t(f)));
}
__device__ __forceinline__ int32_t clampi(int32_t v, int32_t lo, int32_t hi) { return v < lo ? lo : (v > hi ? hi : v); }
// num_traits::clamp on floats: NaN input passes through
__device__ __forceinline__ float clampf(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ------------------------------------------------------------ parameter PODs
struct SecI32 {
    int32_t ba[5];
    int32_t frac;
    int32_t u, mn, mx;
};
struct SecF32 {
    float ba[5];
    float u, mn, mx;
};
struct SecF64 {
    double ba[5];
    double u, mn, mx;
};
template <class S, int N>
struct ChainParams {
    S sec[N];
};
// Section k of a host config array (include/idsp_hip.h) into its POD.  `Fill` takes idsp_biquad_{i32,f32,f64} — no offset, no limits —,
// `FillClamp` idsp_biquad_clamp_{i32,f32,f64}; `frac` where the config has one.
template <class Cfg, class = void>
struct HasFrac : std::false_type {};
template <class Cfg>
struct HasFrac<Cfg, std::void_t<decltype(Cfg::frac)>> : std::true_type {};
template <class Cfg>
struct Fill {
    const Cfg *c;
    template <class S>
    void operator()(S &d, size_t k) const
    {
        using V = decltype(d.u);
        using L = std::numeric_limits<V>;
        for (int i = 0; i < 5; i++) d.ba[i] = c[k].ba[i];
        if constexpr (HasFrac<Cfg>::value) d.frac = c[k].frac;
        d.u = V(0);
        d.mn = L::has_infinity ? -L::infinity() : L::lowest();
        d.mx = L::has_infinity ? L::infinity() : L::max();
    }
};
template <class Cfg>
struct FillClamp {
    const Cfg *c;
    template <class S>
    void operator()(S &d, size_t k) const
    {
        for (int i = 0; i < 5; i++) d.ba[i] = c[k].ba[i];
        if constexpr (HasFrac<Cfg>::value) d.frac = c[k].frac;
        d.u = c[k].u;
        d.mn = c[k].min;
        d.mx = c[k].max;
    }
};
template <class Cfg>
Fill(const Cfg *) -> Fill<Cfg>;
template <class Cfg>
FillClamp(const Cfg *) -> FillClamp<Cfg>;
template <class CfgFill, class S, int N>
inline void fill_sections(const CfgFill &fill, S (&sec)[N])
{
    for (int k = 0; k < N; k++) fill(sec[k], size_t(k));
}

// What a section type that says nothing hands `Chain` / `ChainByLane` below; the section structs derive from it and shadow what they tune
struct SecDefaults {
    static constexpr int LDS_RING = 8;       // LDS-DMA ring depth of a one-section processor
    static constexpr bool LDS_RUN = false;
    // Section count up to which a chain of this section type runs faster on the LDS-DMA kernel than on the register-window
    // kernel at the C2 shape, both at their worst output placement (tools/tune_lds.hip): i32 DF1 x3 0.77 vs 0.62, x4 0.61 vs
    // 0.68; wide x2 0.73 vs 0.65; f32 DF1 / DF2T x2 0.75-0.77 vs 0.60-0.69, x3 0.70 vs 0.71, x4 0.54-0.57 vs 0.57-0.62;
    // Normal x2 0.77-0.81 vs 0.66-0.70, x4 0.51 vs 0.53.
    static constexpr int LDS_MAX_N = 0;      // f64 sections: 8-byte samples never take the LDS-DMA kernel
    // largest number of sub-blocks per workgroup a single section is instantiated with on the sweep kernel: 16 (2^20 lanes in one sweep) for the
    // biquad sections proper (Normal: 8)
    static constexpr int SWEEP_LPT = 16;
    // sections whose single-section processors run 8 / 16 blocks per workgroup of the sweep kernel on its two-barrier schedule (fm_sweep.h)
    static constexpr bool SWEEP_BIG_TWO_BARRIER = false;
    // sections whose full blocks the sweep kernel runs WITHOUT the `s_sleep` pacing although they are cheap: `Normal` f32 — and the clamped ones, which
    // `Chain` adds (65536 lanes: f32 DF1 clamp 0.67 of the peak paced, 0.76 unpaced; f32 DF2T clamp 0.69 / 0.75; i32 DF1 clamp 0.73 / 0.75; Normal f32
    // 0.73 / 0.75 — the unclamped ones 0.77-0.80 / 0.76)
    static constexpr bool SWEEP_UNPACED = false;
    static constexpr bool HAS_TILE = false;  // a `tile` member (Df1I32)
};

// The state of NS serial sections of W words each on one lock-in arm (lockin_generic.hip, lockin_waves_biquad.hip): words
// `word0 + k W + w` of the lane's record, section-major
template <int NS, int W = 4>
struct SectionState {
    uint32_t s[NS][W];
    __device__ __forceinline__ void load(const uint32_t *st, size_t lanes, size_t lane, int word0)
    {
#pragma unroll
        for (int k = 0; k < NS; k++)
#pragma unroll
            for (int w = 0; w < W; w++) s[k][w] = st[size_t(word0 + k * W + w) * lanes + lane];
    }
    __device__ __forceinline__ void store(uint32_t *st, size_t lanes, size_t lane, int word0) const
    {
#pragma unroll
        for (int k = 0; k < NS; k++)
#pragma unroll
            for (int w = 0; w < W; w++) st[size_t(word0 + k * W + w) * lanes + lane] = s[k][w];
    }
};

// ------------------------------------------------------------ i32 sections
// src/iir/biquad.rs:366-383 (C = Q<i32,i64,F>): acc = b0*x0 + b1*x1 + b2*x2 +
// a1*y1 + a2*y2 in i64, y0 = (acc >> F) as i32.
__device__ __forceinline__ int64_t sum5(const SecI32 &c, int32_t x0, int32_t x1, int32_t x2, int32_t y1, int32_t y2)
{
    int64_t acc = mulw(c.ba[0], x0);
    acc = wadd(acc, mulw(c.ba[1], x1));
    acc = wadd(acc, mulw(c.ba[2], x2));
    acc = wadd(acc, mulw(c.ba[3], y1));
    acc = wadd(acc, mulw(c.ba[4], y2));
    return acc;
}

template <bool CLAMP>
struct Df1I32 : SecDefaults {
    static constexpr bool kClamp = CLAMP;
    static constexpr bool SWEEP_BIG_TWO_BARRIER = !CLAMP;
    static constexpr int LDS_RING = CLAMP ? 4 : 7;   // tools/tune_lds.hip: best worst-case over four output placements (plain: 5, 6, 7 within 1.5 %)
    static constexpr int LDS_MAX_N = 3;     // serial sections up to which the LDS-DMA kernel beats the register window
    using T = int32_t;
    using Sec = SecI32;
    static constexpr int W = 4;  // x0 x1 y0 y1
    static constexpr int COST = 50;  // ~VALU cycles per sample and wave (5 quarter-rate 64-bit MADs)
    static __device__ __forceinline__ int32_t step(const SecI32 &c, uint32_t (&s)[W], int32_t x0)
    {
        int32_t y0 = shr_lo(sum5(c, x0, int32_t(s[0]), int32_t(s[1]), int32_t(s[2]), int32_t(s[3])), c.frac);
        if (CLAMP) y0 = clampi(int32_t(uint32_t(y0) + uint32_t(c.u)), c.mn, c.mx);  // biquad.rs:394-404
        s[1] = s[0];
        s[0] = uint32_t(x0);
        s[3] = s[2];
        s[2] = uint32_t(y0);
        return y0;
    }
    // A whole tile of samples at once (round 5): SB independent lanes (states st[0 .. SB)), R consecutive samples of each, x and y in the
    // order g = r SB + lane.  step() is ONE chain of five dependent v_mad_i64_i32 per sample, and an in-order wave that has nothing else
    // to issue pays the ~10-cycle latency of each (86 cycles per sample measured where the arithmetic is 25).  The wrapping i64 sum of
    // biquad.rs:366-383 is associative and commutative mod 2^64, so the same bits come out of any order: here the three feed-forward
    // products of ALL samples go first, term by term across the tile (independent chains, back to back), and only a1 y1 — with a2 y2
    // issued beside it — and the shift stay on the per-sample chain.
    static constexpr bool HAS_TILE = true;
    template <int SB, int R, class StateOf>
    static __device__ __forceinline__ void tile(const SecI32 &c, StateOf &&state_of, const int32_t (&x)[SB * R], int32_t (&y)[SB * R])
    {
        int64_t acc[SB * R];
#pragma unroll
        for (int g = 0; g < SB * R; g++) acc[g] = mulw(c.ba[0], x[g]);
#pragma unroll
        for (int g = 0; g < SB * R; g++) acc[g] = wadd(acc[g], mulw(c.ba[1], g >= SB ? x[g - SB] : int32_t(state_of(g % SB)[0])));
#pragma unroll
        for (int g = 0; g < SB * R; g++)
            acc[g] = wadd(acc[g], mulw(c.ba[2], g >= 2 * SB ? x[g - 2 * SB] : int32_t(state_of(g % SB)[g >= SB ? 0 : 1])));
#pragma unroll
        for (int r = 0; r < R; r++) {
#pragma unroll
            for (int l = 0; l < SB; l++) {
                const int g = r * SB + l;
                acc[g] = wadd(acc[g], mulw(c.ba[4], r >= 2 ? y[g - 2 * SB] : int32_t(state_of(l)[r == 1 ? 2 : 3])));
            }
#pragma unroll
            for (int l = 0; l < SB; l++) {
                const int g = r * SB + l;
                acc[g] = wadd(acc[g], mulw(c.ba[3], r >= 1 ? y[g - SB] : int32_t(state_of(l)[2])));
            }
#pragma unroll
            for (int l = 0; l < SB; l++) {
                const int g = r * SB + l;
                int32_t y0 = shr_lo(acc[g], c.frac);
                if (CLAMP) y0 = clampi(int32_t(uint32_t(y0) + uint32_t(c.u)), c.mn, c.mx);
                y[g] = y0;
            }
        }
#pragma unroll
        for (int l = 0; l < SB; l++) {
            uint32_t(&s)[W] = state_of(l);
            const uint32_t nx1 = R >= 2 ? uint32_t(x[(R - 2) * SB + l]) : s[0], ny1 = R >= 2 ? uint32_t(y[(R - 2) * SB + l]) : s[2];
            s[1] = nx1, s[0] = uint32_t(x[(R - 1) * SB + l]);
            s[3] = ny1, s[2] = uint32_t(y[(R - 1) * SB + l]);
        }
    }
};

// src/iir/biquad.rs:511-538 (first-order error feedback)
template <bool CLAMP>
struct DitherI32 : SecDefaults {
    static constexpr bool kClamp = CLAMP;
    static constexpr int LDS_RING = CLAMP ? 4 : 7;   // tools/tune_lds.hip: best worst-case over four output placements
    static constexpr int LDS_MAX_N = 2;     // serial sections up to which the LDS-DMA kernel beats the register window
    using T = int32_t;
    using Sec = SecI32;
    static constexpr int W = 5;  // x0 x1 y0 y1 e
    static constexpr int COST = 60;
    static __device__ __forceinline__ int32_t step(const SecI32 &c, uint32_t (&s)[W], int32_t x0)
    {
        int64_t acc = wadd(int64_t(uint64_t(s[4])), sum5(c, x0, int32_t(s[0]), int32_t(s[1]), int32_t(s[2]), int32_t(s[3])));
        const int sh = 32 - c.frac;  // 1..32
        const uint64_t a = uint64_t(acc) << sh;
        // `(acc as u32) >> (32 - F)`: low word of a; F == 0 leaves a zero low word
        s[4] = c.frac == 0 ? 0u : (uint32_t(a) >> sh);
        int32_t y0 = int32_t(uint32_t(a >> 32));
        if (CLAMP) y0 = clampi(int32_t(uint32_t(y0) + uint32_t(c.u)), c.mn, c.mx);
        s[1] = s[0];
        s[0] = uint32_t(x0);
        s[3] = s[2];
        s[2] = uint32_t(y0);
        return y0;
    }
};

// src/iir/biquad.rs:456-480 (64-bit y state)
template <bool CLAMP>
struct WideI32 : SecDefaults {
    static constexpr bool kClamp = CLAMP;
    using T = int32_t;
    static constexpr int LDS_RING = CLAMP ? 4 : 5;   // tools/tune_lds.hip: best worst-case over four output placements
    static constexpr bool LDS_RUN = !CLAMP;
    static constexpr int LDS_MAX_N = 2;     // serial sections up to which the LDS-DMA kernel beats the register window
    using Sec = SecI32;
    static constexpr int W = 6;  // x0 x1 y0.lo y0.hi y1.lo y1.hi
    static constexpr int COST = 100;
    static __device__ __forceinline__ int32_t step(const SecI32 &c, uint32_t (&s)[W], int32_t x0)
    {
        int64_t acc = mulw(c.ba[0], x0);
        acc = wadd(acc, mulw(c.ba[1], int32_t(s[0])));
        acc = wadd(acc, mulw(c.ba[2], int32_t(s[1])));
        s[1] = s[0];
        s[0] = uint32_t(x0);
        // (y.lo as u32 as i64 * a) >> 32, then (y >> 32) as i32 as i64 * a
        acc = wadd(acc, (int64_t(uint64_t(s[2])) * int64_t(c.ba[3])) >> 32);
        acc = wadd(acc, mulw(int32_t(s[3]), c.ba[3]));
        acc = wadd(acc, (int64_t(uint64_t(s[4])) * int64_t(c.ba[4])) >> 32);
        acc = wadd(acc, mulw(int32_t(s[5]), c.ba[4]));
        const uint64_t a = uint64_t(acc) << (32 - c.frac);
        s[4] = s[2];
        s[5] = s[3];
        s[2] = uint32_t(a);
        s[3] = uint32_t(a >> 32);
        int32_t y0 = int32_t(s[3]);
        if (CLAMP) {
            y0 = clampi(int32_t(uint32_t(y0) + uint32_t(c.u)), c.mn, c.mx);
            s[3] = uint32_t(y0);  // y[0] = (y0 << 32) | y[0] as u32
        }
        return y0;
    }
};

// ------------------------------------------------------------ f32 sections
// src/iir/biquad.rs:366-383 (C = T = A = f32)
template <bool CLAMP>
struct Df1F32 : SecDefaults {
    static constexpr bool kClamp = CLAMP;
    static constexpr int LDS_RING = CLAMP ? 4 : 5;   // tools/tune_lds.hip: best worst-case over four output placements
    static constexpr int LDS_MAX_N = 2;     // serial sections up to which the LDS-DMA kernel beats the register window
    using T = float;
    using Sec = SecF32;
    static constexpr int W = 4;
    static constexpr int COST = 24;  // 9 full-rate f32 ops + moves
    static __device__ __forceinline__ float step(const SecF32 &c, uint32_t (&s)[W], float x0)
    {
        float acc = c.ba[0] * x0;
        acc = acc + c.ba[1] * __uint_as_float(s[0]);
        acc = acc + c.ba[2] * __uint_as_float(s[1]);
        acc = acc + c.ba[3] * __uint_as_float(s[2]);
        acc = acc + c.ba[4] * __uint_as_float(s[3]);
        if (CLAMP) acc = clampf(acc + c.u, c.mn, c.mx);
        s[1] = s[0];
        s[0] = __float_as_uint(x0);
        s[3] = s[2];
        s[2] = __float_as_uint(acc);
        return acc;
    }
};

// src/iir/biquad.rs:418-440
template <bool CLAMP>
struct Df2tF32 : SecDefaults {
    static constexpr bool kClamp = CLAMP;
    static constexpr bool SWEEP_BIG_TWO_BARRIER = !CLAMP;
    static constexpr int LDS_RING = CLAMP ? 4 : 7;   // tools/tune_lds.hip: best worst-case over four output placements
    static constexpr int LDS_MAX_N = 2;     // serial sections up to which the LDS-DMA kernel beats the register window
    using T = float;
    using Sec = SecF32;
    static constexpr int W = 2;  // s0 s1
    static constexpr int COST = 22;
    static __device__ __forceinline__ float step(const SecF32 &c, uint32_t (&s)[W], float x0)
    {
        float y0 = __uint_as_float(s[0]) + c.ba[0] * x0;
        if (CLAMP) y0 = clampf(y0 + c.u, c.mn, c.mx);
        const float n0 = (__uint_as_float(s[1]) + c.ba[1] * x0) + c.ba[3] * y0;
        const float n1 = c.ba[2] * x0 + c.ba[4] * y0;
        s[0] = __float_as_uint(n0);
        s[1] = __float_as_uint(n1);
        return y0;
    }
};

// ------------------------------------------------------------ f64 sections
// Same generic impls with C = T = A = f64; a value is two state words (low first).
__device__ __forceinline__ double ldd(const uint32_t *s, int i)
{
    return __builtin_bit_cast(double, uint64_t(s[2 * i]) | (uint64_t(s[2 * i + 1]) << 32));
}
__device__ __forceinline__ void std_(uint32_t *s, int i, double v)
{
    const uint64_t u = __builtin_bit_cast(uint64_t, v);
    s[2 * i] = uint32_t(u), s[2 * i + 1] = uint32_t(u >> 32);
}
__device__ __forceinline__ double clampd(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }

template <bool CLAMP>
struct Df1F64 : SecDefaults {
    static constexpr bool kClamp = CLAMP;
    using T = double;
    using Sec = SecF64;
    static constexpr int W = 8;
    static constexpr int COST = 60;
    static __device__ __forceinline__ double step(const SecF64 &c, uint32_t (&s)[W], double x0)
    {
        double acc = c.ba[0] * x0;
        acc = acc + c.ba[1] * ldd(s, 0);
        acc = acc + c.ba[2] * ldd(s, 1);
        acc = acc + c.ba[3] * ldd(s, 2);
        acc = acc + c.ba[4] * ldd(s, 3);
        if (CLAMP) acc = clampd(acc + c.u, c.mn, c.mx);
        s[2] = s[0], s[3] = s[1];
        std_(s, 0, x0);
        s[6] = s[4], s[7] = s[5];
        std_(s, 2, acc);
        return acc;
    }
};

template <bool CLAMP>
struct Df2tF64 : SecDefaults {
    static constexpr bool kClamp = CLAMP;
    using T = double;
    using Sec = SecF64;
    static constexpr int W = 4;
    static constexpr int COST = 55;
    static __device__ __forceinline__ double step(const SecF64 &c, uint32_t (&s)[W], double x0)
    {
        double y0 = ldd(s, 0) + c.ba[0] * x0;
        if (CLAMP) y0 = clampd(y0 + c.u, c.mn, c.mx);
        const double n0 = (ldd(s, 1) + c.ba[1] * x0) + c.ba[3] * y0;
        const double n1 = c.ba[2] * x0 + c.ba[4] * y0;
        std_(s, 0, n0);
        std_(s, 1, n1);
        return y0;
    }
};

// ------------------------------------------------------------ normal form
// `Normal<C>` x `DirectForm1<T>` (src/iir/normal.rs:37-58); ba = [b0, b1, b2, p.re, p.im], state words
// {x0, x1, y0, y1}: y1' = (b0 x0 + b1 x1 + b2 x2 + re y1 + (-im) y0).as_(), y0' = (im y1 + re y0).as_().
struct NormalI32 : SecDefaults {
    static constexpr int SWEEP_LPT = 8;
    using T = int32_t;
    static constexpr int LDS_RING = 5;   // tools/tune_lds.hip: best worst-case over four output placements
    static constexpr bool LDS_RUN = true;
    static constexpr int LDS_MAX_N = 2;     // serial sections up to which the LDS-DMA kernel beats the register window
    using Sec = SecI32;
    static constexpr bool kClamp = false;
    static constexpr int W = 4;
    static constexpr int COST = 70;
    static __device__ __forceinline__ int32_t step(const SecI32 &c, uint32_t (&s)[W], int32_t x0)
    {
        const int32_t y0o = int32_t(s[2]), y1o = int32_t(s[3]);
        int64_t acc = mulw(c.ba[0], x0);
        acc = wadd(acc, mulw(c.ba[1], int32_t(s[0])));
        acc = wadd(acc, mulw(c.ba[2], int32_t(s[1])));
        acc = wadd(acc, mulw(c.ba[3], y1o));
        acc = wadd(acc, mulw(int32_t(0u - uint32_t(c.ba[4])), y0o));  // `-self.p.im()` wraps like Neg on Q
        const int32_t y1 = shr_lo(acc, c.frac);
        const int32_t y0 = shr_lo(wadd(mulw(c.ba[4], y1o), mulw(c.ba[3], y0o)), c.frac);
        s[1] = s[0];
        s[0] = uint32_t(x0);
        s[2] = uint32_t(y0);
        s[3] = uint32_t(y1);
        return y0;
    }
};
struct NormalF32 : SecDefaults {
    static constexpr int SWEEP_LPT = 8;
    static constexpr bool SWEEP_BIG_TWO_BARRIER = true;
    static constexpr bool SWEEP_UNPACED = true;
    using T = float;
    static constexpr int LDS_RING = 5;   // tools/tune_lds.hip: best worst-case over four output placements
    static constexpr bool LDS_RUN = true;
    static constexpr int LDS_MAX_N = 2;     // serial sections up to which the LDS-DMA kernel beats the register window
    using Sec = SecF32;
    static constexpr bool kClamp = false;
    static constexpr int W = 4;
    static constexpr int COST = 30;
    static __device__ __forceinline__ float step(const SecF32 &c, uint32_t (&s)[W], float x0)
    {
        const float y0o = __uint_as_float(s[2]), y1o = __uint_as_float(s[3]);
        float acc = c.ba[0] * x0;
        acc = acc + c.ba[1] * __uint_as_float(s[0]);
        acc = acc + c.ba[2] * __uint_as_float(s[1]);
        acc = acc + c.ba[3] * y1o;
        acc = acc + (-c.ba[4]) * y0o;
        const float y0 = c.ba[4] * y1o + c.ba[3] * y0o;
        s[1] = s[0];
        s[0] = __float_as_uint(x0);
        s[2] = __float_as_uint(y0);
        s[3] = __float_as_uint(acc);
        return y0;
    }
};
struct NormalF64 : SecDefaults {
    using T = double;
    using Sec = SecF64;
    static constexpr bool kClamp = false;
    static constexpr int W = 8;
    static constexpr int COST = 70;
    static __device__ __forceinline__ double step(const SecF64 &c, uint32_t (&s)[W], double x0)
    {
        const double y0o = ldd(s, 2), y1o = ldd(s, 3);
        double acc = c.ba[0] * x0;
        acc = acc + c.ba[1] * ldd(s, 0);
        acc = acc + c.ba[2] * ldd(s, 1);
        acc = acc + c.ba[3] * y1o;
        acc = acc + (-c.ba[4]) * y0o;
        const double y0 = c.ba[4] * y1o + c.ba[3] * y0o;
        s[2] = s[0], s[3] = s[1];
        std_(s, 0, x0);
        std_(s, 2, y0);
        std_(s, 3, acc);
        return y0;
    }
};

// ------------------------------------------------------------ processors
// N independent sections in series (`[C] x [S]`, compose.rs:43-77).
template <class Sec, int N>
struct Chain {
    using In = typename Sec::T;
    using Out = typename Sec::T;
    static constexpr bool HAS_IN = true;
    static constexpr int LDS_WORDS = 0;
    static constexpr int IN_DIV = 1;
    static constexpr int COST = N * Sec::COST;
    static constexpr int LDS_RING = N == 1 ? Sec::LDS_RING : 4;  // N >= 2: tools/tune_lds.hip (worst placement 0.75-0.77 against 0.68 at 8 tiles for N = 2)
    static constexpr bool LDS_RUN = N == 1 && Sec::LDS_RUN;
    static constexpr bool LDS_ELIGIBLE = N <= Sec::LDS_MAX_N;
    static constexpr int SWEEP_MAX_LPT = N == 1 ? Sec::SWEEP_LPT : N == 2 ? 8 : 2;  // sub-blocks per workgroup on the sweep kernel (fm_sweep.h)
    static constexpr bool SWEEP_BIG_TWO_BARRIER = N == 1 && Sec::SWEEP_BIG_TWO_BARRIER;
    static constexpr bool SWEEP_UNPACED = Sec::SWEEP_UNPACED || Sec::kClamp;
    using Params = ChainParams<typename Sec::Sec, N>;
    uint32_t s[N][Sec::W];

    __device__ __forceinline__ void load(const Params &, const uint32_t *st, size_t lanes, size_t lane)
    {
#pragma unroll
        for (int k = 0; k < N; k++)
#pragma unroll
            for (int w = 0; w < Sec::W; w++) s[k][w] = st[size_t(k * Sec::W + w) * lanes + lane];
    }
    __device__ __forceinline__ void store(const Params &, uint32_t *st, size_t lanes, size_t lane)
    {
#pragma unroll
        for (int k = 0; k < N; k++)
#pragma unroll
            for (int w = 0; w < Sec::W; w++) st[size_t(k * Sec::W + w) * lanes + lane] = s[k][w];
    }
    __device__ __forceinline__ Out step(const Params &p, In x)
    {
#pragma unroll
        for (int k = 0; k < N; k++) x = Sec::step(p.sec[k], s[k], x);
        return x;
    }
    // tile form of a single section that has one (Sec::tile; lane_stream.h: HasTileOf): `p` points at SB chains of independent lanes
    static constexpr bool HAS_TILE = N == 1 && Sec::HAS_TILE;
    template <int SB, int R>
    static __device__ __forceinline__ void tile(const Params &prm, Chain *p, const In (&x)[SB * R], Out (&y)[SB * R])
    {
        if constexpr (HAS_TILE) {
            Sec::template tile<SB, R>(prm.sec[0], [&](int l) -> uint32_t(&)[Sec::W] { return p[l].s[0]; }, x, y);
        } else {
#pragma unroll
            for (int g = 0; g < SB * R; g++) y[g] = p[g % SB].step(prm, x[g]);
        }
    }
};

// `Cascade<[Biquad<C>; N]>` x `DirectForm<T, N>` (biquad.rs:339-364): the input
// history of section k is the output history of section k-1.
// Values: h[0..1] = x, h[2+2k..3+2k] = y[k]; sizeof(T)/4 state words per value.
template <class T, int N>
struct CascadeDf1 {
    using In = T;
    using Out = T;
    static constexpr bool HAS_IN = true;
    static constexpr int LDS_WORDS = 0;
    static constexpr int IN_DIV = 1;
    static constexpr bool kFloat = std::is_floating_point<T>::value;
    static constexpr int COST = N * (std::is_same<T, float>::value ? 24 : (kFloat ? 60 : 50));
    static constexpr int LDS_RING = 4;  // tools/tune_lds.hip: worst placement 0.76-0.78 (N = 2) against 0.67-0.68 at 8 tiles
    // LDS-DMA kernel against register window at the C2 shape: i32 x3 0.78 vs 0.59, x4 0.69 vs 0.65, x8 0.42 vs 0.50;
    // f32 x2 0.76 vs 0.70, x4 0.59 vs 0.62
    static constexpr bool LDS_ELIGIBLE = std::is_same<T, int32_t>::value ? N <= 4 : (std::is_same<T, float>::value && N <= 2);
    static constexpr int SWEEP_MAX_LPT = N == 1 ? 4 : 2;
    using SecT = typename std::conditional<std::is_same<T, float>::value, SecF32,
                                           typename std::conditional<kFloat, SecF64, SecI32>::type>::type;
    using Params = ChainParams<SecT, N>;
    static constexpr int V = 2 + 2 * N;       // values
    static constexpr int VW = sizeof(T) / 4;  // words per value
    T h[V];

    __device__ __forceinline__ void load(const Params &, const uint32_t *st, size_t lanes, size_t lane)
    {
#pragma unroll
        for (int v = 0; v < V; v++) {
            uint32_t w[VW];
#pragma unroll
            for (int k = 0; k < VW; k++) w[k] = st[size_t(v * VW + k) * lanes + lane];
            h[v] = words_to<T>(w);
        }
    }
    __device__ __forceinline__ void store(const Params &, uint32_t *st, size_t lanes, size_t lane)
    {
#pragma unroll
        for (int v = 0; v < V; v++) {
            uint32_t w[VW];
            to_words<T>(h[v], w);
#pragma unroll
            for (int k = 0; k < VW; k++) st[size_t(v * VW + k) * lanes + lane] = w[k];
        }
    }
    __device__ __forceinline__ Out step(const Params &p, In x0)
    {
#pragma unroll
        for (int k = 0; k < N; k++) {
            T *xh = &h[2 * k];
            const T *yh = &h[2 * k + 2];
            T y0;
            if constexpr (kFloat) {
                const SecT &c = p.sec[k];
                T acc = c.ba[0] * x0;
                acc = acc + c.ba[1] * xh[0];
                acc = acc + c.ba[2] * xh[1];
                acc = acc + c.ba[3] * yh[0];
                acc = acc + c.ba[4] * yh[1];
                y0 = acc;
            } else {
                const SecI32 &c = p.sec[k];
                y0 = shr_lo(sum5(c, x0, xh[0], xh[1], yh[0], yh[1]), c.frac);
            }
            xh[1] = xh[0];
            xh[0] = x0;
            x0 = y0;
        }
        h[2 * N + 1] = h[2 * N];
        h[2 * N] = x0;
        return x0;
    }
};

// `ByLane<[C; lanes]>` (dsp-process/src/compose.rs:363-390): every lane filters with its
// own coefficients.  Coefficient planes are lane-contiguous like the state planes:
// value v of section k of lane l is coef[(k * CV + v) * lanes + l] (an i32/f32/f64),
// CV = 5 (ba) or 8 (ba, u, min, max); they are read once into registers.
template <class S, class T>
__device__ __forceinline__ void unpack_sec(S &c, const T *v, int nv, T lo, T hi)
{
#pragma unroll
    for (int i = 0; i < 5; i++) c.ba[i] = v[i];
    c.u = nv == 8 ? v[5] : T(0);
    c.mn = nv == 8 ? v[6] : lo;
    c.mx = nv == 8 ? v[7] : hi;
}
__device__ __forceinline__ void unpack_sec(SecI32 &c, const int32_t *v, int nv, int32_t frac)
{
    unpack_sec(c, v, nv, INT32_MIN, INT32_MAX);
    c.frac = frac;
}
__device__ __forceinline__ void unpack_sec(SecF32 &c, const float *v, int nv, int32_t)
{
    unpack_sec(c, v, nv, -__builtin_inff(), __builtin_inff());
}
__device__ __forceinline__ void unpack_sec(SecF64 &c, const double *v, int nv, int32_t)
{
    unpack_sec(c, v, nv, -__builtin_inf(), __builtin_inf());
}

struct ByLaneParams {
    const void *coef;
    int32_t frac;
};

template <class Sec, int N>
struct ChainByLane {
    using In = typename Sec::T;
    using Out = typename Sec::T;
    static constexpr bool HAS_IN = true;
    static constexpr int LDS_WORDS = 0;
    static constexpr int IN_DIV = 1;
    static constexpr int COST = N * Sec::COST;
    static constexpr int LDS_RING = N == 1 ? Sec::LDS_RING : 4;  // N >= 2: tools/tune_lds.hip (worst placement 0.75-0.77 against 0.68 at 8 tiles for N = 2)
    static constexpr bool LDS_RUN = N == 1 && Sec::LDS_RUN;
    static constexpr bool LDS_ELIGIBLE = N <= Sec::LDS_MAX_N;
    static constexpr int CV = Sec::kClamp ? 8 : 5;
    // sub-blocks per workgroup on the sweep kernel (fm_sweep.h): every lane carries its own coefficients in registers beside its state
    static constexpr int SWEEP_MAX_LPT = N == 1 ? 8 : 2;
    static constexpr bool SWEEP_BIG_TWO_BARRIER = N == 1 && Sec::SWEEP_BIG_TWO_BARRIER && std::is_same<typename Sec::T, float>::value;  // (i32 DF1 by lane: one barrier)
    // never paced: with the coefficient registers the paced schedule is bimodal on some boxes (65536 lanes, i32 DF1 / f32 DF2T by lane: launches of 0.345 and of
    // 0.41-0.43 ms in one process, median 0.41; unpaced 0.35-0.36 every time; other boxes 0.34 paced)
    static constexpr bool SWEEP_UNPACED = true;
    using Params = ByLaneParams;
    uint32_t s[N][Sec::W];
    typename Sec::Sec c[N];

    __device__ __forceinline__ void load(const Params &p, const uint32_t *st, size_t lanes, size_t lane)
    {
#pragma unroll
        for (int k = 0; k < N; k++) {
#pragma unroll
            for (int w = 0; w < Sec::W; w++) s[k][w] = st[size_t(k * Sec::W + w) * lanes + lane];
            In cv[CV];
#pragma unroll
            for (int v = 0; v < CV; v++) cv[v] = static_cast<const In *>(p.coef)[size_t(k * CV + v) * lanes + lane];
            unpack_sec(c[k], cv, CV, p.frac);
        }
    }
    __device__ __forceinline__ void store(const Params &, uint32_t *st, size_t lanes, size_t lane)
    {
#pragma unroll
        for (int k = 0; k < N; k++)
#pragma unroll
            for (int w = 0; w < Sec::W; w++) st[size_t(k * Sec::W + w) * lanes + lane] = s[k][w];
    }
    __device__ __forceinline__ Out step(const Params &, In x)
    {
#pragma unroll
        for (int k = 0; k < N; k++) x = Sec::step(c[k], s[k], x);
        return x;
    }
};


// What `Chain` (N = 1 .. 4) and `ChainByLane` (N = 1, 2; not Normal) make of every section type they are instantiated with: the values the launcher
// reads (lane_stream.h, fm_sweep.h), written out by hand so that a default of SecDefaults or a shadowing member cannot move one unseen.
//   ring / run: LDS_RING, LDS_RUN of one section (N >= 2: 4, false)    maxn: LDS_ELIGIBLE = N <= maxn    tile: HAS_TILE of one section
//   lpt: SWEEP_MAX_LPT of one section (Chain N = 2: 8, N >= 3: 2; ChainByLane: 8, 2)
//   two: SWEEP_BIG_TWO_BARRIER of one section (ChainByLane: f32 only)  unpaced: SWEEP_UNPACED (ChainByLane: always)
template <class P, int N, int RING, bool RUN, int MAXN, int LPT, bool TWO, bool UNPACED>
constexpr bool chain_is = P::LDS_RING == (N == 1 ? RING : 4) && P::LDS_RUN == (N == 1 && RUN) && P::LDS_ELIGIBLE == (N <= MAXN) && P::SWEEP_MAX_LPT == LPT &&
                          P::SWEEP_BIG_TWO_BARRIER == (N == 1 && TWO) && P::SWEEP_UNPACED == UNPACED;
#define IDSP_CHAIN_IS(SEC, RING, RUN, MAXN, LPT, TWO, UNPACED, TILE, BYLANE, TWO_BYLANE)                                                                      \
    static_assert(chain_is<Chain<SEC, 1>, 1, RING, RUN, MAXN, LPT, TWO, UNPACED> && chain_is<Chain<SEC, 2>, 2, RING, RUN, MAXN, 8, TWO, UNPACED> &&           \
                      chain_is<Chain<SEC, 3>, 3, RING, RUN, MAXN, 2, TWO, UNPACED> && chain_is<Chain<SEC, 4>, 4, RING, RUN, MAXN, 2, TWO, UNPACED> &&         \
                      Chain<SEC, 1>::HAS_TILE == TILE && !Chain<SEC, 2>::HAS_TILE && !Chain<SEC, 3>::HAS_TILE && !Chain<SEC, 4>::HAS_TILE,                   \
                  "Chain<" #SEC ", N>");                                                                                                                     \
    static_assert(!BYLANE || (chain_is<ChainByLane<SEC, 1>, 1, RING, RUN, MAXN, 8, TWO_BYLANE, true> &&                                                      \
                              chain_is<ChainByLane<SEC, 2>, 2, RING, RUN, MAXN, 2, TWO_BYLANE, true>),                                                       \
                  "ChainByLane<" #SEC ", N>");
//            section          ring run  maxn lpt two    unpaced tile  | by lane: two
IDSP_CHAIN_IS(Df1I32<false>,    7, false, 3, 16, true,  false, true,   true, false)
IDSP_CHAIN_IS(Df1I32<true>,     4, false, 3, 16, false, true,  true,   true, false)
IDSP_CHAIN_IS(DitherI32<false>, 7, false, 2, 16, false, false, false,  true, false)
IDSP_CHAIN_IS(DitherI32<true>,  4, false, 2, 16, false, true,  false,  true, false)
IDSP_CHAIN_IS(WideI32<false>,   5, true,  2, 16, false, false, false,  true, false)
IDSP_CHAIN_IS(WideI32<true>,    4, false, 2, 16, false, true,  false,  true, false)
IDSP_CHAIN_IS(Df1F32<false>,    5, false, 2, 16, false, false, false,  true, false)
IDSP_CHAIN_IS(Df1F32<true>,     4, false, 2, 16, false, true,  false,  true, false)
IDSP_CHAIN_IS(Df2tF32<false>,   7, false, 2, 16, true,  false, false,  true, true)
IDSP_CHAIN_IS(Df2tF32<true>,    4, false, 2, 16, false, true,  false,  true, false)
IDSP_CHAIN_IS(Df1F64<false>,    8, false, 0, 16, false, false, false,  true, false)
IDSP_CHAIN_IS(Df1F64<true>,     8, false, 0, 16, false, true,  false,  true, false)
IDSP_CHAIN_IS(Df2tF64<false>,   8, false, 0, 16, false, false, false,  true, false)
IDSP_CHAIN_IS(Df2tF64<true>,    8, false, 0, 16, false, true,  false,  true, false)
IDSP_CHAIN_IS(NormalI32,        5, true,  2, 8,  false, false, false,  false, false)
IDSP_CHAIN_IS(NormalF32,        5, true,  2, 8,  true,  true,  false,  false, false)
IDSP_CHAIN_IS(NormalF64,        8, false, 0, 16, false, false, false,  false, false)
#undef IDSP_CHAIN_IS

}  // namespace bq
}  // namespace idsp
