// sweep_procs.h — the exponential swept sine of the reference (src/sweptsine.rs) as a stream processor (processor contract:
// lane_stream.h): `AccuOsc<Sweep>` with `Osc` for `W<i32>` (:22-32, :180-188; idsp_sweep_i32).  All integer and bit-exact,
// one lane per thread; the library is built with -fwrapv, so plain signed arithmetic wraps as a Rust release build does.
//
// A lane can END: `Sweep::next` is `state.checked_add(rate * ((state + BIAS) >> 32))?`.  Whether it has is a pure function of
// (state, rate) — the state does not move once the sum leaves i64 — so no flag is stored and every frame evaluates the test again.
// The test is a select, not a branch: an ended lane runs the same instructions and keeps its old words.
#pragma once
#include "dds_dev.h"

namespace idsp {
namespace {

// state words per lane (include/idsp_hip.h): { state lo, hi, accu lo, hi, rate, emitted lo, hi }
struct SweepCore {
    int64_t state, accu;
    uint64_t emitted;
    int32_t rate;
    __device__ __forceinline__ void load(const uint32_t *st, size_t lanes, size_t lane)
    {
        auto w = [&](int i) { return uint64_t(st[size_t(i) * lanes + lane]); };
        state = int64_t(w(0) | (w(1) << 32));
        accu = int64_t(w(2) | (w(3) << 32));
        rate = int32_t(w(4));
        emitted = w(5) | (w(6) << 32);
    }
    // (the rate never changes)
    __device__ __forceinline__ void store(uint32_t *st, size_t lanes, size_t lane) const
    {
        auto w = [&](int i, uint64_t v) { st[size_t(i) * lanes + lane] = uint32_t(v); };
        w(0, uint64_t(state)), w(1, uint64_t(state) >> 32);
        w(2, uint64_t(accu)), w(3, uint64_t(accu) >> 32);
        w(5, emitted), w(6, emitted >> 32);
    }
    // One frame: `Sweep::next` (:26-31, post-increment) into `Integrator` (dsp-process/src/basic.rs:461-466: add, then read).
    // Returns whether the lane emitted; `phase` is the oscillator's argument `(accu >> 32) as i32` (meaningless if it did not).
    __device__ __forceinline__ bool next(int32_t &phase)
    {
        const int64_t s = state;
        const int32_t t = int32_t((uint64_t(s) + 0x80000000ull) >> 32);  // `(s + BIAS) >> 32`, the sum wrapping (release build)
        const int64_t ns = int64_t(rate) * int64_t(t) + s;               // one v_mad_i64_i32; the product is exact
        // `checked_add`: s + p leaves i64 iff s and p share a sign that the wrapped sum does not.  The sign of the exact product is
        // that of rate ^ t unless the product is 0, and then ns == s.  High words only.
        const int32_t sh = int32_t(s >> 32), nh = int32_t(ns >> 32);
        const bool live = ((sh ^ nh) & (rate ^ t ^ nh)) >= 0;
        const int64_t na = accu + s;
        state = live ? ns : s;
        accu = live ? na : accu;
        emitted += live ? 1u : 0u;
        phase = int32_t(na >> 32);
        return live;
    }
};

// (no configuration: a one-word kernarg POD keeps the processor contract's `Params` by value)
struct SweepParams {
    int32_t reserved;
};

// `AccuOsc<Sweep>` (:180-188).  An ended lane writes (0, 0), which cossin never returns.
struct SweepProc {
    using In = int32_t;  // unused
    using Out = Cplx;
    static constexpr bool HAS_IN = false;
    static constexpr int LDS_WORDS = 1 << kCossinDepth;
    static constexpr int IN_DIV = 1;
    static constexpr int COST = 120;  // DdsProc (100) + one quarter-rate multiply-add and ~14 full-rate instructions
    using Params = SweepParams;
    const uint32_t *lut;
    SweepCore c;
    static __device__ __forceinline__ void fill_shared(uint32_t *sh, int tid, int n) { fill_cossin(sh, tid, n); }
    __device__ __forceinline__ void set_shared(const uint32_t *sh) { lut = sh; }
    __device__ __forceinline__ void load(const Params &, const uint32_t *st, size_t lanes, size_t lane) { c.load(st, lanes, lane); }
    __device__ __forceinline__ void store(const Params &, uint32_t *st, size_t lanes, size_t lane) { c.store(st, lanes, lane); }
    // The recurrence is short and serial, cossin long and free of it: four frames' table reads and interpolations in flight at once
    // (lane_stream.h, BATCH).  Without, the FrameMajor kernel — one sample per trip, one wave per SIMD at 65536 lanes — waits out
    // every LDS read: 0.72 ms at 65536 x 4096 against 0.46 with the batch (idsp_dds_i32: 0.36; profiles/NOTES.md, "Swept sine").
    static constexpr int BATCH = 4;
    using Pre = Cplx;
    __device__ __forceinline__ Pre pre(const Params &)
    {
        int32_t ph;
        const bool live = c.next(ph);
        const Cplx v = cossin_dev(ph, lut);
        return Cplx{live ? v.re : 0, live ? v.im : 0};
    }
    __device__ __forceinline__ Out step(const Params &, In, const Pre &v) { return v; }
};

}  // namespace
}  // namespace idsp
