// lockin_accu_procs.h — the lock-in whose LO is iterated from the RPLL's `Accu` rows inside the kernel: idsp_accu_lo_i32 followed by
// idsp_lockin_i32_lo_process (src/accu.rs:34-54 -> src/complex.rs:237-240 -> src/lockin.rs:17-39) with the LO never stored, as stream
// processors (processor contract: lane_stream.h).  They are LockinProc / LockinSplitProc (lockin_stream_procs.h) with the phase
// accumulator re-seeded once per 2^k frames from the lane's next { state, step } pair:
//     phase(t) = state * h + offset + (j + 1) * ((u32)step >> k) * h,   t = u 2^k + j,   { state, step } = accu[u, lane]
// i.e. `acc = state * h + offset; inc = ((u32)step >> k) * h` when j wraps, then LockinProc's `acc += inc` (all wrapping).
// The stream kernels call pre() once per frame in frame order and every thread of a wave is at the same frame, so the frame
// counter is wave-uniform and the reload is a uniform branch (the counter is read with readfirstlane: the compiler cannot see
// that).  Nothing assumes that a batch, a tile or a tail of the kernels starts on an update; k = 0 reloads on every frame.
#pragma once
#include "dds_dev.h"

namespace idsp {
namespace {

typedef uint32_t accu_pair __attribute__((ext_vector_type(2)));  // { state, step }

// where a lane's `Accu` rows are: pair (u, lane) at accu[lane * lane_stride + u * row_stride] (FrameMajor: 1, lanes; LaneMajor:
// updates, 1).  A side pointer computed from the lane index of the WHOLE call: launch_stream's lane splits must not take these
// parameters, and the member is called `xw` so that lane_stream.h's HasSideWalk sees it and shift_lanes() refuses to compile.
struct AccuWalk {
    const void *accu;
    size_t lane_stride, row_stride, updates;
};
struct LpAccuParams {
    LpParams lp;
    AccuWalk xw;
    uint32_t harmonic, offset;  // `Accu * harmonic + Accu::new(offset, 0)` (src/accu.rs:40-54)
    uint32_t k, jmask;          // batch_log2, 2^k - 1
};

// The LO phase of one lane: shared by the two processors.
// Where the `Accu` pairs are loaded decides the speed.  A load issued INSIDE the reload branch has an age the compiler cannot know
// when the branch is next taken, so it guards the use with `s_waitcnt vmcnt(0)` — which drains the register window of x loads the
// FrameMajor kernel keeps in flight, once per update.  So the loads sit at a fixed place instead: the END of every batch of
// kAccuBatch frames requests what the NEXT batch may reload from (request()) and the reload branch only reads registers.  The wait
// before it is then counted from straight-line code: it leaves the x loads and the stores of one batch in flight, which is why the
// batch is eight frames and not LockinProc's four.  A frame taken on its own (next(): the kernels' tails) loads its pair on the
// spot and leaves `pend` stale.  CONTRACT: within one call a processor sees batches first and single frames after them, never a
// batch after a single frame — what every stream kernel does (stream_frame_major: window loop, then drain; stream_lane_major: full
// tiles, then the last partial one; stream_frame_major_lds: single frames only).
constexpr int kAccuBatch = 8, kAccuBatchLog2 = 3;
struct AccuPhase {
    const accu_pair *base;  // the lane's pair of update 0
    size_t un;              // the update the next reload seeds           } the same in every thread of a wave
    uint32_t j;             // frames into the current update; 0: reload  }
    uint32_t acc, inc;
    accu_pair pend[kAccuBatch];  // requested by the previous batch (by start() for the first)
    // a wave-uniform value as the compiler can see it: scalar arithmetic from here on
    static __device__ __forceinline__ size_t uniform(size_t v)
    {
        const uint32_t lo = __builtin_amdgcn_readfirstlane(int(uint32_t(v))), hi = __builtin_amdgcn_readfirstlane(int(uint32_t(v >> 32)));
        return size_t(lo) | (size_t(hi) << 32);
    }
    __device__ __forceinline__ accu_pair pair_at(const LpAccuParams &p, size_t u) const
    {
        const size_t us = uniform(u);  // a request past the last row reads the last row again
        return nt_load<false>(base + (us < p.xw.updates ? us : p.xw.updates - 1) * p.xw.row_stride);
    }
    __device__ __forceinline__ bool wraps() const { return __builtin_amdgcn_readfirstlane(int(j)) == 0; }
    __device__ __forceinline__ void seed(const LpAccuParams &p, const accu_pair a)
    {
        acc = a.x * p.harmonic + p.offset;  // `Mul` then `Add` of the states
        inc = (a.y >> p.k) * p.harmonic;    // the logical shift of accu_lo_kernel, then `Mul`
        un++;
    }
    __device__ __forceinline__ uint32_t advance(const LpAccuParams &p)
    {
        j = (j + 1) & p.jmask;
        acc += inc;  // the pre-incrementing `next()` (src/accu.rs:34-37)
        return acc;
    }
    // What the next batch may reload from: one pair when 2^k >= kAccuBatch (at most one update starts within that many frames,
    // wherever they lie), one pair per frame below.  Frame i of the batch reloads (if it does) after
    // c(i) = ceil((j + i) / 2^k) - ceil(j / 2^k) earlier reloads; c(0) = 0, and with 2^k >= kAccuBatch the one reload there can be
    // is the first.  (One `if` without an `else`: two branches that both end in a store to `pend` are merged into one store at a
    // variable offset, and the processor then lives on the stack.)
    __device__ __forceinline__ void request(const LpAccuParams &p)
    {
        pend[0] = pair_at(p, un);
        if (p.k < kAccuBatchLog2) {
            const uint32_t j0 = uint32_t(__builtin_amdgcn_readfirstlane(int(j))), c0 = (j0 + p.jmask) >> p.k;
#pragma unroll
            for (uint32_t i = 1; i < kAccuBatch; i++) pend[i] = pair_at(p, un + (((j0 + i + p.jmask) >> p.k) - c0));
        }
    }
    __device__ __forceinline__ void start(const LpAccuParams &p, size_t lane)
    {
        base = static_cast<const accu_pair *>(p.xw.accu) + lane * p.xw.lane_stride;
        un = 0;
        acc = inc = j = 0;
        request(p);
    }
    // the phase of the next frame, on its own
    __device__ __forceinline__ uint32_t next(const LpAccuParams &p)
    {
        if (wraps()) seed(p, pair_at(p, un));
        return advance(p);
    }
    // the phases of the next kAccuBatch frames
    __device__ __forceinline__ void next_batch(const LpAccuParams &p, uint32_t (&phase)[kAccuBatch])
    {
#pragma unroll
        for (int i = 0; i < kAccuBatch; i++) {
            // (values, not `one ? pend[0] : pend[i]`: a select between two lvalues is a select of addresses and puts the processor on the stack)
            const bool one = p.k >= kAccuBatchLog2;
            if (wraps()) seed(p, accu_pair{one ? pend[0].x : pend[i].x, one ? pend[0].y : pend[i].y});
            phase[i] = advance(p);
        }
        request(p);
    }
};

// one thread per lane
template <int N, int K>
struct LockinAccuProc {
    using In = int32_t;
    using Out = Cplx;
    static constexpr bool HAS_IN = true;
    static constexpr int LDS_WORDS = 1 << kCossinDepth;
    static constexpr int IN_DIV = 1;
    static constexpr int COST = 110 + 80 * N * K;
    using Params = LpAccuParams;
    const uint32_t *lut;
    AccuPhase ph;
    LpBank<N, K> bi, bq;
    static __device__ __forceinline__ void fill_shared(uint32_t *sh, int tid, int n) { fill_cossin(sh, tid, n); }
    __device__ __forceinline__ void set_shared(const uint32_t *sh) { lut = sh; }
    __device__ __forceinline__ void load(const Params &p, const uint32_t *st, size_t lanes, size_t lane)
    {
        ph.start(p, lane);
        bi.load(st, lanes, lane, 0);
        bq.load(st, lanes, lane, 2 * N * K);
    }
    __device__ __forceinline__ void store(const Params &, uint32_t *st, size_t lanes, size_t lane)
    {
        bi.store(st, lanes, lane, 0);
        bq.store(st, lanes, lane, 2 * N * K);
    }
    static constexpr int BATCH = kAccuBatch;
    using Pre = Cplx;  // the frame's LO
    __device__ __forceinline__ Pre pre(const Params &p) { return cossin_dev(int32_t(ph.next(p)), lut); }
    __device__ __forceinline__ void pre_batch(const Params &p, Pre (&out)[BATCH])
    {
        uint32_t phase[BATCH];
        ph.next_batch(p, phase);
#pragma unroll
        for (int i = 0; i < BATCH; i++) out[i] = cossin_dev(int32_t(phase[i]), lut);
    }
    __device__ __forceinline__ Out step(const Params &p, In x, const Pre &lo)
    {
        return Cplx{bi.step(p.lp, __mulhi(lo.re, x)), bq.step(p.lp, __mulhi(lo.im, x))};
    }
};

// I/Q arms on two adjacent threads (virtual lanes 2 * lane + iq), as LockinSplitProc: both threads walk the same `Accu` rows
template <int N, int K>
struct LockinAccuSplitProc {
    using In = int32_t;
    using Out = int32_t;
    static constexpr bool HAS_IN = true;
    static constexpr int LDS_WORDS = 1 << kCossinDepth;
    static constexpr int IN_DIV = 2;
    static constexpr int COST = 70 + 40 * N * K;
    using Params = LpAccuParams;
    const uint32_t *lut;
    AccuPhase ph;
    bool q;
    LpBank<N, K> b;
    static __device__ __forceinline__ void fill_shared(uint32_t *sh, int tid, int n) { fill_cossin(sh, tid, n); }
    __device__ __forceinline__ void set_shared(const uint32_t *sh) { lut = sh; }
    __device__ __forceinline__ void load(const Params &p, const uint32_t *st, size_t vlanes, size_t vlane)
    {
        const size_t lanes = vlanes / 2, lane = vlane / 2;
        q = vlane & 1;
        ph.start(p, lane);
        b.load(st, lanes, lane, q ? 2 * N * K : 0);
    }
    __device__ __forceinline__ void store(const Params &, uint32_t *st, size_t vlanes, size_t vlane)
    {
        const size_t lanes = vlanes / 2, lane = vlane / 2;
        b.store(st, lanes, lane, q ? 2 * N * K : 0);
    }
    static constexpr int BATCH = kAccuBatch;
    using Pre = int32_t;  // this arm's LO component
    __device__ __forceinline__ Pre pre(const Params &p)
    {
        const Cplx lo = cossin_dev(int32_t(ph.next(p)), lut);
        return q ? lo.im : lo.re;
    }
    // The phases of the batch come from the closed form one after the other (an add each, a reload where an update
    // starts); the two threads of a lane then evaluate cossin of alternate frames (thread q: frames 2 i + q) and swap the
    // component the partner needs with one DPP move, as LockinSplitProc::pre_batch does.
    __device__ __forceinline__ void pre_batch(const Params &p, Pre (&out)[BATCH])
    {
        uint32_t phase[BATCH];
        ph.next_batch(p, phase);
#pragma unroll
        for (int i = 0; i < BATCH / 2; i++) {
            const Cplx lo = cossin_dev(int32_t(q ? phase[2 * i + 1] : phase[2 * i]), lut);
            const int32_t mine = q ? lo.im : lo.re, other = q ? lo.re : lo.im;
            const int32_t recv = pair_swap(other);
            out[2 * i] = q ? recv : mine;
            out[2 * i + 1] = q ? mine : recv;
        }
    }
    __device__ __forceinline__ Out step(const Params &p, In x, const Pre &lo) { return b.step(p.lp, __mulhi(lo, x)); }
};

}  // namespace
}  // namespace idsp
