// lane_stream.h — the two streaming kernels every per-lane recurrence of the
// hot path runs through (biquad family, lowpass, DDS, lock-in).
//
// Replaces "L2 block loop x L3 process body x N lanes" of the reference
// (dsp-process/src/process.rs:122-127,137-141 driven by Lanes,
// dsp-process/src/compose.rs:468-494) by ONE launch:
//   * one lane per thread; the serially dependent recurrence state lives in
//     VGPRs for the whole call and is read/written once (word-plane-major
//     state, include/idsp_hip.h);
//   * the shared configuration arrives as a kernarg POD, i.e. in SGPRs —
//     uniform across the wave, no LDS or vector loads on the hot loop;
//   * FRAME_MAJOR: a wave reads one 256-byte row segment per frame through a
//     rotating register window that requests frame f+U before frame f is
//     consumed, so a wave keeps U row segments in flight at all times (HBM
//     latency >> per-sample work, and at 64k lanes there is exactly one wave
//     per SIMD — no other wave hides it);
//   * LANE_MAJOR: adjacent lanes are `frames` elements apart, so a wave moves
//     64-lane x TS-sample tiles through a padded LDS tile: row-contiguous
//     (coalesced) global accesses on one side, conflict-free column walks by
//     the owning thread on the other.
//
// A processor P provides:
//   using In / Out;            element types (Out may be a 2-word struct)
//   static constexpr bool HAS_IN;
//   struct Params;             POD, passed by value as kernarg
//   load(prm, st, lanes, lane) / store(...)   state <-> registers
//   Out step(prm, In x)        one sample of the reference `process()`
//   static constexpr int LDS_WORDS;   read-only table words (0 = none), filled
//   by static fill_shared(uint32_t*) with the whole block and handed to the
//   processor through set_shared(const uint32_t*).
//   static constexpr int BATCH; Pre pre(prm); Out step(prm, x, pre)   (optional,
//   BATCH > 1): the part of a sample's work that does not depend on the
//   recurrence state (the DDS phase -> cossin chain) is evaluated for BATCH
//   consecutive frames back to back, which gives the scheduler independent
//   dependency chains to interleave — at one wave per SIMD the per-frame
//   dependent-chain latency, not throughput, is what bounds these kernels.
//   Within one call every kernel here runs a lane's whole batches first and its remaining frames one by one (pre()) after them,
//   never a batch after a single frame: lockin_accu_procs.h relies on that order.
//   static constexpr int IN_DIV;      FRAME_MAJOR only: IN_DIV adjacent threads
//   ("virtual lanes") share one input lane — used to split the I and Q arms of
//   the lock-in / DDS over two threads when there are too few lanes to give
//   every SIMD a wave; `lanes` then counts virtual lanes.
#pragma once

#include <atomic>
#include <cstdlib>
#include <type_traits>
#include <typeinfo>

#include "common.h"
#include "dispatch_thresholds.h"
#include "lds_dma.h"

namespace idsp {

template <class P, class = void>
struct BatchOf {
    static constexpr int value = 1;
};
template <class P>
struct BatchOf<P, std::void_t<decltype(P::BATCH)>> {
    static constexpr int value = P::BATCH;
};

// Processors with a large per-sample body (many uniform branches) cap the register-window depth so that the
// unrolled loop stays inside the instruction cache: `static constexpr int MAX_U`.
template <class P, class = void>
struct MaxU {
    static constexpr int value = 24;
};
template <class P>
struct MaxU<P, std::void_t<decltype(P::MAX_U)>> {
    static constexpr int value = P::MAX_U;
};

// BATCH pre-stage values: processors may provide pre_batch(prm, Pre (&)[BATCH]) (e.g. to share
// the work between the IN_DIV threads of a lane); the default evaluates pre() BATCH times.
template <class P, class = void>
struct HasPreBatch : std::false_type {};
template <class P>
struct HasPreBatch<P, std::void_t<decltype(&P::pre_batch)>> : std::true_type {};

// Processors with a tile form — P::tile<SB, R>(prm, P *lanes, x, y): SB independent lanes x R consecutive samples in one call, the
// state-independent part of all samples issued ahead of the per-sample chains (biquad_sections.h, Df1I32::tile) — declare HAS_TILE.
template <class P, class = void>
struct HasTileOf : std::false_type {};
template <class P>
struct HasTileOf<P, std::void_t<decltype(P::HAS_TILE)>> : std::integral_constant<bool, P::HAS_TILE> {};

template <class P, int B>
__device__ __forceinline__ void pre_all(P &p, const typename P::Params &prm, typename P::Pre (&pre)[B])
{
    if constexpr (HasPreBatch<P>::value) {
        p.pre_batch(prm, pre);
    } else {
#pragma unroll
        for (int b = 0; b < B; b++) pre[b] = p.pre(prm);
    }
}

// one sample through processors with or without a state-independent pre-stage
template <class P>
__device__ __forceinline__ typename P::Out step1(P &p, const typename P::Params &prm, typename P::In v)
{
    if constexpr (BatchOf<P>::value > 1)
        return p.step(prm, v, p.pre(prm));
    else
        return p.step(prm, v);
}

// (a function of its own: inside the kernels' generic lambdas a discarded `if constexpr` branch is still checked against P)
template <class P, int SB, int R>
__device__ __forceinline__ void tile_of(const typename P::Params &prm, P *lanes, const typename P::In (&x)[SB * R], typename P::Out (&y)[SB * R])
{
    if constexpr (HasTileOf<P>::value) {
        P::template tile<SB, R>(prm, lanes, x, y);
    } else {
#pragma unroll
        for (int g = 0; g < SB * R; g++) y[g] = step1(lanes[g % SB], prm, x[g]);
    }
}

// words <-> sample helpers (1- or 2-word element types)
template <class T>
__device__ __forceinline__ T words_to(const uint32_t *w)
{
    if constexpr (sizeof(T) == 4) {
        return __builtin_bit_cast(T, w[0]);
    } else {
        const uint64_t u = uint64_t(w[0]) | (uint64_t(w[1]) << 32);
        return __builtin_bit_cast(T, u);
    }
}
template <class T>
__device__ __forceinline__ void to_words(const T &v, uint32_t *w)
{
    if constexpr (sizeof(T) == 4) {
        w[0] = __builtin_bit_cast(uint32_t, v);
    } else {
        const uint64_t u = __builtin_bit_cast(uint64_t, v);
        w[0] = uint32_t(u), w[1] = uint32_t(u >> 32);
    }
}

// streamed-once data: nontemporal loads/stores (struct outputs go out as a 2-word vector).
// NT = false for arithmetic-bound processors, where the longer nontemporal load latency
// showed up as a slowdown (8-section cascade) instead of a bandwidth gain.
// (Both name the GLOBAL address space: a pointer rebuilt from a wave-uniform integer base is a generic one otherwise and the access a
// `flat_*` instruction, which counts on lgkmcnt beside vmcnt — tools/check_flat.py keeps the library free of them.)
// a 4-, 8- or 16-byte object as a vector of words (class types have no copy operations in a named address space)
template <int BYTES>
struct WordsOf;
template <>
struct WordsOf<4> {
    using type = uint32_t;
};
template <>
struct WordsOf<8> {
    typedef uint32_t type __attribute__((ext_vector_type(2)));
};
template <>
struct WordsOf<16> {
    typedef uint32_t type __attribute__((ext_vector_type(4)));
};
template <bool NT, class T>
__device__ __forceinline__ T nt_load(const T *p)
{
    using W = typename WordsOf<int(sizeof(T))>::type;
    const auto *g = reinterpret_cast<const __attribute__((address_space(1))) W *>(reinterpret_cast<uintptr_t>(p));
    if constexpr (NT)
        return __builtin_bit_cast(T, __builtin_nontemporal_load(g));
    else
        return __builtin_bit_cast(T, *g);
}
template <bool NT, class T>
__device__ __forceinline__ void nt_store(T *p, const T &v)
{
    using W = typename WordsOf<int(sizeof(T))>::type;
    auto *g = reinterpret_cast<__attribute__((address_space(1))) W *>(reinterpret_cast<uintptr_t>(p));
    if constexpr (NT)
        __builtin_nontemporal_store(__builtin_bit_cast(W, v), g);
    else
        *g = __builtin_bit_cast(W, v);
}

constexpr int kWave = 64;
constexpr int kFmBlock = 256;  // 4 waves: one per SIMD of a CU, 1 KiB row segment per block

// ---------------------------------------------------------------- FRAME_MAJOR
template <class P, int U>
__global__ __launch_bounds__(kFmBlock) void stream_frame_major(
    const typename P::Params prm, uint32_t *st, const typename P::In *x, typename P::Out *y,
    const size_t lanes, const size_t frames, const size_t xl, const size_t yl, const int xcd_contiguous, const size_t slanes_ = 0)
{
    using In = typename P::In;
    using Out = typename P::Out;
    // slanes: pitch of the state (and per-lane coefficient) planes in lanes; 0 = `lanes` (not a lane block of a larger call)
    const size_t slanes = slanes_ ? slanes_ : lanes;
    __shared__ uint32_t ptab[P::LDS_WORDS ? P::LDS_WORDS : 1];
    // launched with 256-thread workgroups when that still gives every CU one, else with single waves
    if constexpr (P::LDS_WORDS > 0) {
        P::fill_shared(ptab, threadIdx.x, int(blockDim.x));
        __syncthreads();
    }
    // xcd_contiguous (rows that do not start on 64-byte boundaries, see stream_frame_major_lds XCDC): workgroup blockIdx runs
    // on XCD blockIdx % 8; give XCD j the j-th contiguous eighth of the lane blocks so that the lines two neighbouring blocks
    // share are fetched and written through one L2
    size_t wg = blockIdx.x;
    if (xcd_contiguous) {
        const size_t q = gridDim.x / 8, r = gridDim.x % 8, j = blockIdx.x % 8;
        wg = j * q + (j < r ? j : r) + blockIdx.x / 8;
    }
    const size_t lane = wg * blockDim.x + threadIdx.x;
    if (lane >= lanes) return;

    P p;
    if constexpr (P::LDS_WORDS > 0) p.set_shared(ptab);
    p.load(prm, st, slanes, lane);

    constexpr bool kNT = P::COST <= 220;
    // xl / yl: elements between consecutive frames of x / y (dense: lanes / IN_DIV and lanes — IN_DIV virtual
    // lanes share an input lane)
    const In *xp = x + lane / P::IN_DIV;
    Out *yp = y + lane;

    if constexpr (P::HAS_IN) {
        // Rotating register window: frame f + U is requested right before frame
        // f is consumed, so U row segments per wave are in flight at all
        // times (vmcnt is in-order: the wait for frame f tolerates the U-1
        // younger loads and the interleaved stores).  Reads always run ahead of
        // this thread's writes, so y == x is safe.
        // (The sub-word families share this walk as subword_rows.h: window_walk; this one keeps its own for BATCH / `pre`.)
        In ring[U];
#pragma unroll
        for (int u = 0; u < U; u++)
            if (size_t(u) < frames) ring[u] = nt_load<kNT>(xp + size_t(u) * xl);
        size_t f = 0;
        for (; f + 2 * U <= frames; f += U) {
            const In *xn = xp + (f + U) * xl;
            Out *yn = yp + f * yl;
            constexpr int B = BatchOf<P>::value;
            static_assert(U % B == 0, "window depth must be a multiple of the batch");
#pragma unroll
            for (int u0 = 0; u0 < U; u0 += B) {
                if constexpr (B > 1) {
                    typename P::Pre pre[B];
                    pre_all<P, B>(p, prm, pre);
#pragma unroll
                    for (int b = 0; b < B; b++) {
                        const int u = u0 + b;
                        const In v = ring[u];
                        ring[u] = nt_load<kNT>(xn + size_t(u) * xl);
                        nt_store<kNT>(yn + size_t(u) * yl, p.step(prm, v, pre[b]));
                    }
                } else {
                    const int u = u0;
                    const In v = ring[u];
                    ring[u] = nt_load<kNT>(xn + size_t(u) * xl);
                    nt_store<kNT>(yn + size_t(u) * yl, p.step(prm, v));
                }
            }
        }
        // drain: fewer than 2U frames left, predicates are wave-uniform
#pragma unroll
        for (int u = 0; u < U; u++) {
            const size_t fr = f + u;
            if (fr < frames) {
                const In v = ring[u];
                if (fr + U < frames) ring[u] = nt_load<kNT>(xp + (fr + U) * xl);
                nt_store<kNT>(yp + fr * yl, step1(p, prm, v));
            }
        }
        f += U;
#pragma unroll
        for (int u = 0; u < U; u++) {
            const size_t fr = f + u;
            if (fr < frames) nt_store<kNT>(yp + fr * yl, step1(p, prm, ring[u]));
        }
    } else {
        constexpr int B = BatchOf<P>::value;
        size_t f = 0;
        if constexpr (B > 1) {
            for (; f + B <= frames; f += B) {
                typename P::Pre pre[B];
                pre_all<P, B>(p, prm, pre);
#pragma unroll
                for (int b = 0; b < B; b++) nt_store<kNT>(yp + size_t(b) * yl, p.step(prm, In{}, pre[b]));
                yp += size_t(B) * yl;
            }
        }
        for (; f < frames; f++) {
            nt_store<kNT>(yp, step1(p, prm, In{}));
            yp += yl;
        }
    }
    p.store(prm, st, slanes, lane);
}

// ------------------------------------------------- FRAME_MAJOR through LDS (DMA)
// At <= 2 waves per SIMD the register-window kernel above is limited by what a
// 4-byte-per-lane access stream can pull from HBM (~5.3-5.5 TB/s measured at 65536
// lanes).  This variant moves the same rows with 16-byte-per-lane accesses while
// keeping one lane per thread (all four SIMDs of a CU compute): a 256-thread
// block owns 256 lanes (1 KiB per frame row); its waves pull whole rows straight
// into an LDS ring with `global_load_lds_dwordx4` (no VGPR staging, NB tiles of T
// rows in flight), every thread then walks its own column with conflict-free
// ds_read_b32, and results leave through a double-buffered LDS tile as
// row-contiguous dwordx4 stores.  +10 % at C2 (6.07 vs 5.52 TB/s, tools/exp_lds.hip).
//
// The DMA loads are issued from inline asm (the compiler neither counts nor
// drains them), so their completion is tracked by hand: vmcnt is in-order, and
// in steady state exactly kYoung younger operations (this wave's later DMA rows
// and its dwordx4 stores) are allowed to remain outstanding when tile i is
// needed; start-up, drain and ragged tiles simply wait for everything.
constexpr int kLdsT = 8;    // frames per tile
// Ring depth (input tiles in flight, 8 KiB each at 256 lanes): 8 unless the processor names another (P::LDS_RING).  It sets
// how far the DMA reads run ahead of the stores.  Measured at C2 (65536 lanes, 256 KiB rows; tools/probe_xy_offset.py over
// output placements y - x = 1 GiB + delta and in place), plain i32 DF1: 8 tiles 0.348-0.412 ms depending on delta (in
// place 0.39), 9 tiles 0.347-0.393, 7 tiles 0.333-0.354 (in place 0.34), 6 tiles 0.343-0.363, 5 tiles 0.340-0.354: with 8
// (and 9) the read and the write stream sit 16 (18) MiB apart and collide on the HBM channels unless y happens to sit at
// a lucky offset from x.  The clamp / wide / multi-section processors are the other way round (8 tiles 0.35-0.40 ms by
// placement, 7 or fewer a flat 0.41-0.46 ms), so only DF1 i32, dither and f32 DF2T without clamp take 7.
constexpr int kLdsNB = 8;
// Largest non-persistent grid of the LDS-DMA kernel; launches with more workgroups walk their lane blocks persistently.
constexpr size_t kLdsGridCap = thr::kLdsGridCap;
// LDS-DMA path or register-window kernel (launch_stream): P::LDS_ELIGIBLE if the processor declares it, else COST <= 120.
template <class P, class = void>
struct LdsEligibleOf {
    static constexpr bool value = P::COST <= 120;
};
template <class P>
struct LdsEligibleOf<P, std::void_t<decltype(P::LDS_ELIGIBLE)>> {
    static constexpr bool value = P::LDS_ELIGIBLE;
};
template <class P, class = void>
struct LdsRingOf {
    static constexpr int value = kLdsNB;
};
template <class P>
struct LdsRingOf<P, std::void_t<decltype(P::LDS_RING)>> {
    static constexpr int value = P::LDS_RING;
};
// Addressing form of the LDS-DMA kernel per processor (see the kernel): indexed unless the processor asks for the running
// form (P::LDS_RUN).  Ring depth and form per section type come from tools/tune_lds.hip (profiles/r02_tune_lds.jsonl).
template <class P, class = void>
struct LdsRunOf {
    static constexpr bool value = false;
};
template <class P>
struct LdsRunOf<P, std::void_t<decltype(P::LDS_RUN)>> {
    static constexpr bool value = P::LDS_RUN;
};

// tools/exp_lm_ablate.sh: stream_lane_major_staged and stream_frame_major_lds without their loads / stores (conditions never true at run time: timing only)
#ifdef IDSP_EXP_LM_NOLOAD
#define IDSP_EXP_LM_LD_ON (frames == 1)
#else
#define IDSP_EXP_LM_LD_ON true
#endif
#ifdef IDSP_EXP_LM_NOSTORE
#define IDSP_EXP_LM_ST_ON (frames == 1)
#else
#define IDSP_EXP_LM_ST_ON true
#endif
template <int N, class F>
__device__ __forceinline__ void static_for(F &&f)
{
    if constexpr (N > 0) {
        static_for<N - 1>(f);
        f(std::integral_constant<int, N - 1>{});
    }
}

// One lane per thread: a workgroup of 256 threads owns a block of 256 adjacent lanes, and a tile is kLdsT frames of that
// block: kLdsT one-KiB row segments.  (Several lanes per thread, a choice of block orders and plain instead of nontemporal
// accesses were measured and retired: profiles/NOTES.md, "LDS-DMA kernel: forms retired".)
// XCDC (round 3): rows that do not start on 64-byte boundaries — dense rows of 65000 or 65532 lanes, odd pitches.  The 1 KiB
// row segments of adjacent lane blocks then share the 64-byte pieces at their boundaries, and with consecutive blocks dealt
// round-robin to the 8 XCDs (each with its own L2) both halves of every shared piece are fetched — and partially written —
// through two different L2s: 0.58-0.64 of the HBM peak against 0.77 on aligned rows (tools/exp_fm_pitch.py: same lanes, same
// kernel, pitch 65536 + {4, 8, 16, 32} lanes -> 0.59 / 0.64 / 0.76 / 0.75).  XCDC gives every XCD a CONTIGUOUS eighth of the
// lane blocks, so that neighbours meet in one L2: 65000 dense lanes 0.62 -> 0.71, pitch 65540 0.59 -> 0.67, aligned rows
// 0.78 -> 0.77 (tools/exp_fm_misaligned.hip, profiles/r03_exp_fm_misaligned.jsonl) — used for misaligned rows only.
// Built, bit-exact and removed again: rotating the piece -> thread assignment per row so that every 16-lane quad of a
// `dwordx4` request starts on a 64-byte boundary (the LDS-DMA destination is fixed by the hardware lane, so the row sits
// rotated in LDS and the owning thread reads its column through the rotation) ran at 0.56 on EVERY pitch, aligned ones
// included: the straddling quads were not the cost.
template <class P, int NB = LdsRingOf<P>::value, bool RUN = LdsRunOf<P>::value, bool XCDC = false>
__global__ __launch_bounds__(kFmBlock) void stream_frame_major_lds(
    const typename P::Params prm, uint32_t *st, const typename P::In *x, typename P::Out *y,
    const size_t lanes, const size_t frames, const size_t xl, const size_t yl, const size_t slanes)
{
    // slanes: pitch of the state (and per-lane coefficient) planes, in lanes — `lanes` unless this launch is a lane block of
    // a larger call (launch_stream splits a call into whole rounds here + a remainder on the staged kernel)
    using In = typename P::In;
    using Out = typename P::Out;
    static_assert(P::HAS_IN && P::IN_DIV == 1 && sizeof(In) == 4, "LDS path: one 4-byte input per lane and frame");
    constexpr int OW = sizeof(Out) / 4, B = BatchOf<P>::value;
    constexpr int TS = kLdsT;    // frames per tile = 1 KiB row segments per tile: segment g is frame g of the tile
    constexpr int RPW = TS / 4;  // segments per wave and tile
    constexpr int kYoung = RPW * OW + (NB - 1) * (RPW + RPW * OW);
    static_assert(kYoung <= 63 && TS % 4 == 0 && TS % B == 0, "vmcnt range / tile shape");
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    uint32_t *tin = smem;                               // [NB][TS][256]
    uint32_t *tout = smem + NB * TS * kFmBlock;         // [2][TS][256 * OW]
    uint32_t *ptab = tout + 2 * TS * kFmBlock * OW;     // [P::LDS_WORDS]
    const int tid = threadIdx.x, lid = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t lds_base = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint32_t *)smem;

    P p;
    if constexpr (P::LDS_WORDS > 0) {
        P::fill_shared(ptab, tid, kFmBlock);  // published by the first tile barrier
        for (int once = 0; once < 1; once++) p.set_shared(ptab);  // one trip: see the state load below
    }
    // Persistent over lane blocks: a workgroup walks its 256-lane blocks one after the other (state load, the whole frame
    // walk, state store per block).
    // One-word outputs also take a ragged last block (lanes % 256 != 0, lanes % 4 == 0: whole 16-byte pieces): a thread whose
    // piece of the 1 KiB row segment lies beyond the last lane acts as a CLONE of an in-range thread — it requests
    // that thread's piece again and stores that thread's results to that thread's address (same bytes, twice) — so
    // the steady-state loop carries no predicate and every wave still issues exactly RPW loads and RPW * OW stores
    // per tile (the vmcnt bookkeeping below).  Its own column computes on whatever the clone's piece holds and is
    // dropped; only the state store is predicated.
    const size_t nblocks = (lanes + size_t(kFmBlock) - 1) / size_t(kFmBlock);
    // (a workgroup that owns ADJACENT blocks instead — blocks [w rounds, (w + 1) rounds) — was measured slower: 0.58 vs
    // 0.68 of peak at 2^20 lanes, profiles/r02_exp_c5_matrix6.jsonl: the panel order keeps the concurrently active
    // columns in one contiguous 256 KiB piece of every row)
    // Order in which a persistent workgroup visits its column panels.  All workgroups advance through the frames in
    // lockstep, so if workgroup w simply walked the blocks w, w + grid, w + 2 grid, ... the whole launch would touch the same
    // few rows of ONE 256 KiB panel at any instant.  Here the upper half of the grid starts half way through its panels,
    // which keeps two panels active: over nine placements of the output buffer 0.71-0.77 against 0.68-0.72 at 131072 lanes,
    // 0.67-0.71 against 0.65-0.67 at 262144, 0.61-0.72 against 0.64-0.70 at 2^20 (profiles/r03_exp_c5_order.jsonl).
    // Single-round launches (C2) are the same walk either way.
    const size_t rounds_ = (nblocks + gridDim.x - 1) / gridDim.x;
    for (size_t k_ = 0; k_ < rounds_; k_++) {
    const size_t rr_ = (k_ + (blockIdx.x >= gridDim.x / 2 ? rounds_ / 2 : 0)) % rounds_;
    // XCDC: workgroups are dealt to the XCDs round-robin (blockIdx % 8); give XCD j the j-th contiguous eighth of the blocks
    // (XCD j hosts the workgroups blockIdx = j, j + 8, ...: grid / 8 of them, one more on the first grid % 8 XCDs)
    const size_t q_ = gridDim.x / 8, r_ = gridDim.x % 8, j_ = blockIdx.x % 8;
    const size_t wg_ = XCDC ? j_ * q_ + (j_ < r_ ? j_ : r_) + blockIdx.x / 8 : blockIdx.x;
    const size_t blk = wg_ + rr_ * gridDim.x;
    if (blk >= nblocks) continue;
    const size_t lane0 = blk * size_t(kFmBlock);
    const size_t avail = lanes - lane0;  // lanes of this block that exist (>= 4)
    const bool ragged_block = OW == 1 && avail < size_t(kFmBlock);
    const int lid4 = ragged_block && size_t(lid * 4) >= avail ? int(size_t(lid * 4) % avail) : lid * 4;  // first lane of this thread's piece
    const bool lane_ok = !ragged_block || size_t(tid) < avail;
    // set_shared above, the state load and the state store each sit in a loop of ONE trip on purpose: DO NOT FLATTEN them without
    // a codegen diff (tools/diff_codegen.py) and a measurement.  As plain statements the load's address arithmetic dominates the
    // store's, the optimiser shares it and then hoists the store's addresses out of `if (lane_ok)`, and that moves registers and
    // spills in most instantiations (plain i32 DF1: only a branch in the drain loop; the lock-in processors: 2 VGPRs fewer, 2 SGPR
    // spills more).  A helper function around the loop does not keep the code either.  The measured code is the one with the loops.
    for (int once = 0; once < 1; once++) p.load(prm, st, slanes, lane_ok ? lane0 + tid : lanes - 1);
    // The state loads must have landed HERE, in a way the compiler's wait-count pass sees: it cannot see the DMA
    // requests of glds16(), and if it first needs a state register inside the steady-state loop it protects that use
    // with `s_waitcnt vmcnt(0)` on every iteration — which drains the whole prefetch ring each tile (0.52 instead of
    // 0.34 ms at C2 when a refactoring moved the first use).  vmcnt(0), expcnt / lgkmcnt untouched:
    __builtin_amdgcn_s_waitcnt(0x0F70);

    const size_t ntiles = (frames + TS - 1) / TS;
    const size_t nfull = frames / TS;  // tiles [0, nfull) have all their rows
    // a ragged tile holds nseg(v) segments
    auto nseg = [&](size_t v) { return int(frames - v * TS < size_t(TS) ? frames - v * TS : size_t(TS)); };
    // Two forms of the per-tile addressing, chosen per processor (P::LDS_RUN) by measurement — these kernels sit on a
    // timing edge where the scalar instructions between the barriers decide how the DMA requests and the stores
    // interleave (profiles/r02_exp_c2_clamp*.jsonl, tools/exp_c2_clamp.sh: C2 shape, four placements of y):
    //   RUN = false  ring slot = tile % NB, addresses from the tile index: plain DF1 / dither / f32 DF2T at ring 7
    //                run 0.796-0.805 of peak this way and 0.71-0.77 the other way;
    //   RUN = true   running ring slot, x / y pointers advanced per tile: the clamp forms (two more dependent
    //                operations per sample) run 0.77-0.78 at ring 5 this way in every placement, against 0.67-0.68
    //                (ring 5-7) or 0.67 / 0.75 by placement (ring 8) the other way.
    const size_t xstep = size_t(TS) * xl, ystep = size_t(TS) * yl * OW;
    const In *xq = x + lane0 + lid4;                                          // RUN: tile about to be requested
    uint32_t *yq = reinterpret_cast<uint32_t *>(y) + lane0 * OW + lid4;       // RUN: tile about to be stored
    int slot_run = 0;                                                         // RUN: i % NB
    auto issue = [&](size_t v, auto full) {
        constexpr bool FULL = decltype(full)::value;
        const int slot = RUN ? slot_run : int(v % NB), ns = FULL ? TS : nseg(v);
#pragma unroll
        for (int j = 0; j < RPW; j++) {
            const int g = wave + 4 * j;
            if ((FULL || g < ns) && IDSP_EXP_LM_LD_ON) {
                const In *src = RUN ? xq + size_t(g) * xl : x + (v * TS + g) * xl + lane0 + lid4;
                glds16(src, lds_base + uint32_t((slot * TS + g) * kFmBlock * 4));
            }
        }
        if constexpr (RUN) xq += xstep;
    };
    auto store = [&](size_t v, auto full) {
        constexpr bool FULL = decltype(full)::value;
        const uint32_t *o = tout + (v & 1) * TS * kFmBlock * OW;
        const int ns = FULL ? TS : nseg(v);
        uint32_t *yw = reinterpret_cast<uint32_t *>(y);
#pragma unroll
        for (int j = 0; j < RPW; j++) {
            const int g = wave + 4 * j;
            if ((FULL || g < ns) && IDSP_EXP_LM_ST_ON) {
#pragma unroll
                for (int h = 0; h < OW; h++) {
                    const u32x4 v4 = *reinterpret_cast<const u32x4 *>(o + (g * OW + h) * kFmBlock + lid4);
                    uint32_t *dst = RUN ? yq + size_t(g) * yl * OW + h * kFmBlock : yw + ((v * TS + g) * yl + lane0) * OW + h * kFmBlock + lid4;
                    __builtin_nontemporal_store(v4, reinterpret_cast<u32x4 *>(dst));
                }
            }
        }
        if constexpr (RUN) {
            yq += ystep;
            slot_run = slot_run + 1 == NB ? 0 : slot_run + 1;  // the tile is done: its slot went to tile v + NB in issue()
        }
    };
    auto compute = [&](size_t v, auto full) {
        constexpr bool FULL = decltype(full)::value;
        const uint32_t *in = tin + (RUN ? slot_run : int(v % NB)) * TS * kFmBlock;
        uint32_t *o = tout + (v & 1) * TS * kFmBlock * OW;
        const int ns = FULL ? TS : nseg(v);
        if constexpr (B > 1) {
#pragma unroll
            for (int r0 = 0; r0 < TS; r0 += B) {
                if (!FULL && r0 >= ns) break;
                typename P::Pre pre[B];
#pragma unroll
                for (int b = 0; b < B; b++)
                    if (FULL || r0 + b < ns) pre[b] = p.pre(prm);
#pragma unroll
                for (int b = 0; b < B; b++) {
                    const int r = r0 + b;
                    if (FULL || r < ns) to_words<Out>(p.step(prm, __builtin_bit_cast(In, in[r * kFmBlock + tid]), pre[b]), o + (r * kFmBlock + tid) * OW);
                }
            }
        } else {
            static_for<TS>([&](auto gg) {
                constexpr int g = decltype(gg)::value;
                if (FULL || g < ns) to_words<Out>(p.step(prm, __builtin_bit_cast(In, in[g * kFmBlock + tid])), o + (g * kFmBlock + tid) * OW);
            });
        }
    };

    using Full = std::true_type;
    using Ragged = std::false_type;
    for (size_t t = 0; t < size_t(NB) && t < ntiles; t++) {
        slot_run = int(t);
        issue(t, Ragged{});
    }
    slot_run = 0;
    size_t i = 0;
    auto slow_iter = [&]() {  // start-up, drain and ragged tiles: wait for everything
        wait_vmcnt<0>();
        lds_barrier();
        compute(i, Ragged{});
        lds_barrier();
        if (i + NB < ntiles) issue(i + NB, Ragged{});
        store(i, Ragged{});
    };
    for (; i < ntiles && i < size_t(NB); i++) slow_iter();
    // steady state: all tiles involved are full, and every wave has issued exactly RPW loads
    // and RPW*OW stores per past tile, so kYoung younger operations may stay in flight
    for (; i + NB < nfull; i++) {
        wait_vmcnt<kYoung>();
        lds_barrier();  // all four waves' segments of tile i have landed
        compute(i, Full{});
        lds_barrier();  // out tile complete; ring slot i % NB is free again
        issue(i + NB, Full{});
        store(i, Full{});
    }
    for (; i < ntiles; i++) slow_iter();
    for (int once = 0; once < 1; once++)  // one trip: see the state load
        if (lane_ok) p.store(prm, st, slanes, lane0 + tid);
    // No barrier needed here: the next block's first lds_barrier() (after each wave's lgkmcnt wait) orders this
    // block's last output-tile reads before the compute() that overwrites the tile, and its first DMA rows only
    // touch input slots whose last readers passed the barrier after the final compute().
    }
}

// ----------------------------------------------------------------- LANE_MAJOR
// One wave per workgroup; tiles are wave-private, so the syncs below only
// order this wave's own LDS traffic (lds_wave_sync: no vmcnt drain, the next
// tile's global loads stay in flight).
template <class P>
__global__ __launch_bounds__(kWave) void stream_lane_major(
    const typename P::Params prm, uint32_t *st, const typename P::In *x, typename P::Out *y,
    const size_t lanes, const size_t frames, const size_t xl, const size_t yl)
{
    // xl / yl: samples between the starts of consecutive lanes of x / y (dense: frames)
    using In = typename P::In;
    using Out = typename P::Out;
    // D = IN_DIV threads ("virtual lanes") share one lane: they read the same input sample and each
    // writes its own OW words of the lane's D*OW-word output sample; `lanes` counts virtual lanes.
    constexpr int D = P::IN_DIV;
    constexpr int IW = sizeof(In) / 4, OW = sizeof(Out) / 4, OWR = OW * D;  // words per input / output sample
    static_assert((IW == 1 || IW == 2) && (OWR == 1 || OWR == 2) && (D == 1 || D == 2), "samples are one or two 32-bit words");
    constexpr int MW = IW > OWR ? IW : OWR;
    constexpr int TS = kWave / MW;             // samples per tile and lane (widest row = 64 words)
    constexpr int RWI = TS * IW, RWO = TS * OWR;  // words per tile row
    constexpr int ROWS = kWave / D;            // lanes per wave
    constexpr int RPI = kWave / RWI;           // tile rows covered by one load instruction
    constexpr int NLD = ROWS / RPI;            // load instructions per tile
    constexpr bool kAlias = P::HAS_IN && RWI == RWO;

    __shared__ uint32_t tin[P::HAS_IN ? ROWS : 1][RWI + 1];
    __shared__ uint32_t tout_[kAlias ? 1 : ROWS][RWO + 1];
    uint32_t(*tout)[RWO + 1] = kAlias ? reinterpret_cast<uint32_t(*)[RWO + 1]>(tin) : tout_;

    const int lid = threadIdx.x;
    const size_t vlane = size_t(blockIdx.x) * kWave + lid;  // virtual lane of this thread
    const bool active = vlane < lanes;
    const size_t lane0 = size_t(blockIdx.x) * ROWS, rlanes = lanes / D;  // first lane of the wave, lane count
    const size_t nrows = rlanes - lane0 < size_t(ROWS) ? rlanes - lane0 : size_t(ROWS);
    const int trow = lid / D, tsub = lid % D;

    __shared__ uint32_t ptab[P::LDS_WORDS ? P::LDS_WORDS : 1];
    if constexpr (P::LDS_WORDS > 0) P::fill_shared(ptab, lid, kWave);  // published by the first tile sync

    P p;
    if constexpr (P::LDS_WORDS > 0) p.set_shared(ptab);
    if (active) p.load(prm, st, lanes, vlane);

    const uint32_t *xw = reinterpret_cast<const uint32_t *>(x);
    uint32_t *yw = reinterpret_cast<uint32_t *>(y);
    // word (row r, col c) handled by this thread in load instruction i: r = i*RPI + lrow, c = lcol
    const int lrow = lid / RWI, lcol = lid % RWI;

    uint32_t stage[NLD];
    auto fetch = [&](size_t t0) {
        if constexpr (P::HAS_IN) {
            const size_t nw = (frames - t0 < size_t(TS) ? frames - t0 : size_t(TS)) * IW;
#pragma unroll
            for (int i = 0; i < NLD; i++) {
                const size_t r = size_t(i) * RPI + lrow;
                stage[i] = (r < nrows && size_t(lcol) < nw) ? xw[((lane0 + r) * xl + t0) * IW + lcol] : 0u;
            }
        }
    };

    auto one = [&](size_t j) {
        In v{};
        if constexpr (P::HAS_IN) v = words_to<In>(&tin[trow][j * IW]);
        const Out o = step1(p, prm, v);
        to_words<Out>(o, &tout[trow][j * OWR + tsub * OW]);
    };

    fetch(0);
    for (size_t t0 = 0; t0 < frames; t0 += TS) {
        const size_t ncols = frames - t0 < size_t(TS) ? frames - t0 : size_t(TS);
        if constexpr (P::HAS_IN) {
#pragma unroll
            for (int i = 0; i < NLD; i++) tin[i * RPI + lrow][lcol] = stage[i];
        }
        lds_wave_sync();
        if (t0 + TS < frames) fetch(t0 + TS);  // next tile in flight during the arithmetic

        if (active) {
            if (ncols == size_t(TS)) {
                constexpr int B = BatchOf<P>::value;
                if constexpr (B > 1 && TS % B == 0) {
#pragma unroll
                    for (int j0 = 0; j0 < TS; j0 += B) {
                        typename P::Pre pre[B];
                        pre_all<P, B>(p, prm, pre);
#pragma unroll
                        for (int b = 0; b < B; b++) {
                            In v{};
                            if constexpr (P::HAS_IN) v = words_to<In>(&tin[trow][(j0 + b) * IW]);
                            to_words<Out>(p.step(prm, v, pre[b]), &tout[trow][(j0 + b) * OWR + tsub * OW]);
                        }
                    }
                } else if constexpr (MaxU<P>::value < 24) {
                    for (int j = 0; j < TS; j++) one(size_t(j));  // large body: keep the tile loop rolled
                } else {
#pragma unroll
                    for (int j = 0; j < TS; j++) one(size_t(j));
                }
            } else {
                for (size_t j = 0; j < ncols; j++) one(j);
            }
        }
        lds_wave_sync();
        // row-contiguous stores: one instruction = up to 64 consecutive words of one lane
        const size_t nw = ncols * OWR;
        for (size_t r = 0; r < nrows; r++) {
            if (size_t(lid) < nw) yw[((lane0 + r) * yl + t0) * OWR + lid] = tout[r][lid];
        }
        lds_wave_sync();
    }
    if (active) p.store(prm, st, lanes, vlane);
}

// ------------------------------------------- LANE_MAJOR, 16-byte pieces (staged)
// The kernel above moves a lane's row as 4-byte pieces (one 256-byte run of ONE lane per instruction): 64 loads, 64
// stores and 256 LDS accesses per 64 x 64 tile, all on the issue path of a single wave, and it asks HBM for 256-byte
// runs per lane.  This form moves 512-byte runs per lane with 16 bytes per thread in both directions:
//   * a tile is 64 lanes x kLmRun bytes (TF = 128 / W frames of W words, PCS = 32 pieces per lane); load instruction j
//     of a tile fetches the runs of the G = 2 lanes j and j + 32 — 32 threads per run — into VGPRs, and the whole tile
//     is handed to one 32 KiB LDS slot with linear ds_write_b128 (thread t's piece of instruction j at 1024 j + 16 t, so
//     lane l sits in slot row (l % PCS) G + l / PCS).  WHICH piece of the run a thread fetches is free: thread t takes
//     piece (t % PCS) ^ (j % 16), so the row of lane l holds piece k at 16 (k ^ (l % 16)) and the owning thread's
//     ds_read_b128 column walk is bank-conflict free without padding;
//   * thread l reads its pieces, runs the steps in registers, writes the results over the same pieces; the wave then
//     re-reads the slot linearly and stores whole runs.  The NEXT tile's loads are issued right after the hand-over,
//     so they are in flight during the arithmetic and the stores (the compiler counts them: plain loads).
//     Per 64 x 128 samples: 32 loads + 128 LDS + 32 stores instead of 128 + 512 + 128.
// What the run length is worth at 65536 lanes x 4096 frames (tools/tune_lm.hip, profiles/r02_tune_lm.jsonl; same
// arithmetic, i32 DF1): 128-byte runs 0.54 of the HBM peak whatever the prefetch depth, 256-byte 0.56-0.58, 512-byte
// 0.65-0.70 (this kernel; the 4-byte tile kernel 0.60-0.64), 1 KiB runs no better at the two waves per CU their LDS
// allows.  An LDS-DMA twin (global_load_lds_dwordx4 rings of 1-4 slots) ran the same rates per run length: the bound
// is the access pattern (65536 concurrent streams of short runs 16 KiB apart), not latency or issue.
// One wave per workgroup, no barriers.  Needs 16-byte aligned rows (base and pitch).  A last partial tile moves its
// whole 16-byte pieces the same way; the final frames % (4 / W) samples of every lane go sample by sample.  x == y is
// safe (a tile is stored after it has been read; the rows of one wave are touched by no other).
constexpr int kLmRun = 512;  // bytes per lane and tile on the wider of the two sides
// Processors the staged kernel takes: one lane per thread (IN_DIV == 1), 4- or 8-byte samples, no input or an input of the
// output's size, and a pre-stage batch of 1 or 4 frames.  The kernel itself also handles samples of different sizes (a tile
// is then 128 / max(words) frames: 512-byte runs on the wider side, 256-byte runs on the narrower, separate LDS slots), but
// its 48 KiB of LDS leave a CU three waves and those processors (fm_disc, the lock-in with Complex output) are VALU-bound:
// fm_disc LaneMajor 1.89 ms staged against 1.46 ms on the tile kernel at 65536 lanes x 4096, so they stay there.
// A processor can opt out (P::LM_STAGED = false): with 128 staging registers next to a large state the kernel spills
// (tools/check_scratch.py is the build check).
template <class P, class = void>
struct LmStagedAllowed : std::true_type {};
template <class P>
struct LmStagedAllowed<P, std::void_t<decltype(P::LM_STAGED)>> : std::integral_constant<bool, P::LM_STAGED> {};
template <class P, class = void>
struct LmStagedOf {
    static constexpr bool value = false;
};
template <class P>
struct LmStagedOf<P, std::enable_if_t<P::IN_DIV == 1 && (!P::HAS_IN || sizeof(typename P::In) == sizeof(typename P::Out)) &&
                                      (sizeof(typename P::Out) == 4 || sizeof(typename P::Out) == 8) &&
                                      (BatchOf<P>::value == 1 || BatchOf<P>::value == 4) && LmStagedAllowed<P>::value>> {
    static constexpr bool value = true;
};
template <class P, class = void>
struct LmOneFormOf : std::false_type {};
template <class P>
struct LmOneFormOf<P, std::void_t<decltype(P::LM_ONE_FORM)>> : std::integral_constant<bool, P::LM_ONE_FORM> {};
// bytes of LDS the kernel needs for P (slots + the processor's table)
template <class P, int LW, int LB = kLmRun>
constexpr size_t lm_staged_lds_bytes()
{
    constexpr int IW = P::HAS_IN ? int(sizeof(typename P::In)) / 4 : 0, OW = int(sizeof(typename P::Out)) / 4;
    constexpr int S = IW > OW ? IW : OW, TF = LB / 4 / S;
    constexpr int IB = TF * IW * 4, OB = TF * OW * 4;
    return size_t(LW) * (IB == OB ? OB : IB + OB) + size_t(P::LDS_WORDS) * 4;
}

// geometry of one side of a tile of LW lanes: RB bytes per lane, moved as PCS 16-byte pieces; one instruction covers G
// lanes, a tile takes NI instructions; instruction j covers lanes j, j + NI, ...; lane l sits in slot row (l % NI) G + l / NI
// with piece k at 16 (k ^ (l % 16))
template <int RB, int LW>
struct LmSide {
    static constexpr int PCS = RB / 16, G = PCS ? kWave / PCS : 1, NI = LW / G;
    static_assert(PCS == 0 || PCS == 16 || PCS == 32 || PCS == 64, "256-, 512- or 1024-byte runs");
};

// LW = lanes per wave (64, 32 or 16).  With fewer than 64 the wave still moves whole runs with all its threads, but only
// the first LW threads own a lane: a launch of few lanes then spreads over LW / 64 times as many waves (SIMDs) — below
// 65536 lanes a 64-lane wave per SIMD leaves most of the chip without a wave, and the per-lane recurrence is a serial
// chain that one wave cannot speed up.
template <class P, int LW = kWave, int LB = kLmRun>
__global__ __launch_bounds__(kWave) void stream_lane_major_staged(
    const typename P::Params prm, uint32_t *st, const typename P::In *x, typename P::Out *y,
    const size_t lanes, const size_t frames, const size_t xl, const size_t yl, const unsigned skew = 0, const unsigned skew_shift = 8)
{
    // Start-up skew (round 5 experiment; IDSP_DIAG=1 IDSP_LM_SKEW=ticks of 10 ns, IDSP_LM_SKEW_SHIFT): every wave of a launch issues its tile's 32
    // loads in one burst and its 32 stores in another, and all waves do so at the same time — a CU's memory pipe then serves a load burst
    // and a store burst one after the other (round 4: the kernel runs as the SUM of its directions).  Workgroups with an odd
    // (blockIdx >> shift) start `skew` ticks late, so that half the waves of a CU store while the other half load.
    // (round 6: `skew_shift` bits 8.. = number of phases, 0 = two: workgroup b of the first 1024 waits ((b >> shift) % phases) x skew ticks)
    const unsigned skew_ph = skew && blockIdx.x < 1024u ? (blockIdx.x >> (skew_shift & 31u)) % ((skew_shift >> 8) ? (skew_shift >> 8) : 2u) : 0u;
    if (skew_ph) {
        const long long d = (long long)(skew) * skew_ph, t0 = wall_clock64();
        for (long long spins = d / 8 + 16; spins > 0 && wall_clock64() - t0 < d; spins--) __builtin_amdgcn_s_sleep(8);
    }
    using In = typename P::In;
    using Out = typename P::Out;
    static_assert(LmStagedOf<P>::value, "one lane per thread, 4- or 8-byte samples, pre-stage batch 1 or 4");
    constexpr bool HAS_IN = P::HAS_IN;
    constexpr int IW = HAS_IN ? int(sizeof(In)) / 4 : 0, OW = int(sizeof(Out)) / 4;  // words per sample
    constexpr int S = IW > OW ? IW : OW;
    constexpr int TF = LB / 4 / S;                 // frames per tile (LB = bytes per lane and tile on the wider side)
    constexpr int IB = TF * IW * 4, OB = TF * OW * 4;  // bytes per lane and tile
    static_assert(LW == 64 || LW == 32 || LW == 16, "lanes per wave");
    using SI = LmSide<IB, LW>;
    using SO = LmSide<OB, LW>;
    constexpr int PI = SI::PCS, PO = SO::PCS;      // pieces per lane and tile
    constexpr int NII = HAS_IN ? SI::NI : 0, NIO = SO::NI;  // load / store instructions per tile
    constexpr bool kAlias = IB == OB;              // results overwrite the input pieces
    constexpr int NS = 16 / S;                     // samples per compute chunk (4 pieces of the wider side)
    constexpr int CI = NS * IW / 4, CO = NS * OW / 4;  // pieces per chunk
    constexpr int B = BatchOf<P>::value;
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    char *const slot_in = reinterpret_cast<char *>(smem);
    char *const slot_out = slot_in + (kAlias ? 0 : LW * IB);
    uint32_t *ptab = reinterpret_cast<uint32_t *>(slot_out + LW * OB);  // [P::LDS_WORDS]
    const int lid = threadIdx.x;

    const size_t lane0 = size_t(blockIdx.x) * LW;
    const size_t nrows = lanes - lane0 < size_t(LW) ? lanes - lane0 : size_t(LW);
    const bool active = size_t(lid) < nrows;

    P p;
    if constexpr (P::LDS_WORDS > 0) {
        P::fill_shared(ptab, lid, kWave);
        lds_wave_sync();
        p.set_shared(ptab);
    }
    if (active) p.load(prm, st, lanes, lane0 + lid);

    // Addresses = wave-uniform 64-bit base (the wave's first lane, instruction j, tile: SGPRs) + a 32-bit per-thread
    // byte offset (the lane of the instruction's group and the piece): the global_load / store `saddr` form.  With one
    // 64-bit pointer per instruction in VGPRs the source and destination pointers sat next to the staged pieces and
    // the kernel spilled.  (The launcher checks that 64 rows span less than 4 GiB.)
    const size_t xrowb = xl * sizeof(In), yrowb = yl * sizeof(Out);  // bytes between lanes
    const char *const xbase = reinterpret_cast<const char *>(x) + lane0 * xrowb;
    char *const ybase = reinterpret_cast<char *>(y) + lane0 * yrowb;
    // mover role on either side: in instruction j, lane mq + j of the tile, piece mpc ^ ((mq + j) % 16) of its run
    const int mqi = PI ? (lid / (PI ? PI : 1)) * NII : 0, mpci = PI ? lid % (PI ? PI : 1) : 0;
    const int mqo = (lid / PO) * NIO, mpco = lid % PO;
    const uint32_t xoff = uint32_t(mqi) * uint32_t(xrowb), yoff = uint32_t(mqo) * uint32_t(yrowb);
    // owner role (threads < LW): slot row of this thread's lane, and the byte offset of its piece k = own ^ (16 k)
    const int ol = lid % LW;
    const uint32_t owni = NII ? uint32_t((ol % (NII ? NII : 1)) * SI::G + ol / (NII ? NII : 1)) * IB + uint32_t(ol & 15) * 16 : 0;
    const uint32_t owno = uint32_t((ol % NIO) * SO::G + ol / NIO) * OB + uint32_t(ol & 15) * 16;

    const size_t nfull = frames / TF;
    const int nquad = int((frames - nfull * TF) / 4);  // whole groups of 4 samples of the last, partial tile
    u32x4 stage[NII ? NII : 1];
    // WHOLE: all 64 lanes of the wave exist; FULL: the whole tile exists (else nq groups of 4 samples)
    auto fetch = [&](size_t v, auto whole, auto full, int nq) __attribute__((always_inline)) {
        if constexpr (HAS_IN) {
            const char *src = xbase + v * size_t(IB);
#pragma unroll
            for (int j = 0; j < NII; j++) {
                const int pc = mpci ^ (NII % 16 == 0 ? j & 15 : (mqi + j) & 15);  // mqi is a multiple of NII: a constant when 16 | NII
                if ((decltype(whole)::value || size_t(mqi + j) < nrows) && (decltype(full)::value || pc < nq * IW) && IDSP_EXP_LM_LD_ON)
                    stage[j] = global_ld<u32x4, true>(src + j * xrowb, xoff + uint32_t(pc * 16));
            }
        }
    };
    auto hand_over = [&]() __attribute__((always_inline)) {
        if constexpr (HAS_IN) {
#pragma unroll
            for (int j = 0; j < NII; j++) *reinterpret_cast<u32x4 *>(slot_in + j * 1024 + lid * 16) = stage[j];
        }
    };
    // four consecutive samples: IW input pieces in, OW output pieces out
    auto quad = [&](const u32x4 *in, u32x4 *out) __attribute__((always_inline)) {
        uint32_t wi[IW ? 4 * IW : 1], wo[4 * OW];
        if constexpr (HAS_IN) {
#pragma unroll
            for (int h = 0; h < IW; h++)
#pragma unroll
                for (int e = 0; e < 4; e++) wi[4 * h + e] = in[h][e];
        }
        auto sample = [&](int b) __attribute__((always_inline)) {
            In v{};
            if constexpr (HAS_IN) v = words_to<In>(wi + b * IW);
            return v;
        };
        if constexpr (B == 4) {
            typename P::Pre pre[4];
            pre_all<P, 4>(p, prm, pre);
#pragma unroll
            for (int b = 0; b < 4; b++) to_words<Out>(p.step(prm, sample(b), pre[b]), wo + b * OW);
        } else {
#pragma unroll
            for (int b = 0; b < 4; b++) to_words<Out>(p.step(prm, sample(b)), wo + b * OW);
        }
#pragma unroll
        for (int h = 0; h < OW; h++) out[h] = u32x4{wo[4 * h], wo[4 * h + 1], wo[4 * h + 2], wo[4 * h + 3]};
    };
    auto in_piece = [&](int k) __attribute__((always_inline)) { return *reinterpret_cast<const u32x4 *>(slot_in + (owni ^ uint32_t(k * 16))); };
    auto out_piece = [&](int k, const u32x4 &v) __attribute__((always_inline)) { *reinterpret_cast<u32x4 *>(slot_out + (owno ^ uint32_t(k * 16))) = v; };
    auto compute = [&](auto full, int nq) __attribute__((always_inline)) {
        if (!active) return;
        if constexpr (!decltype(full)::value || MaxU<P>::value < 24) {
            for (int q = 0; q < nq; q++) {  // partial tile, or a large body: keep the loop rolled
                u32x4 in[IW ? IW : 1], out[OW];
#pragma unroll
                for (int h = 0; h < IW; h++) in[h] = in_piece(q * IW + h);
                quad(in, out);
#pragma unroll
                for (int h = 0; h < OW; h++) out_piece(q * OW + h, out[h]);
            }
        } else {
            // chunks of NS samples (4 pieces of the wider side): the next chunk's LDS reads are issued before the
            // current chunk's arithmetic, and a scheduling fence per chunk keeps the compiler from hoisting all reads
            // of the tile above the first step (which, next to the staged pieces of the next tile, overflowed the
            // register file into scratch)
            constexpr int NCH = TF / NS;
            u32x4 cur[CI ? CI : 1], nxt[CI ? CI : 1];
#pragma unroll
            for (int c = 0; c < CI; c++) cur[c] = in_piece(c);
#pragma unroll
            for (int g = 0; g < NCH; g++) {
                if (g + 1 < NCH) {
#pragma unroll
                    for (int c = 0; c < CI; c++) nxt[c] = in_piece((g + 1) * CI + c);
                }
                u32x4 out[CO];
                if constexpr (HasTileOf<P>::value && IW == 1 && OW == 1 && B == 1) {
                    In xin[NS];
                    Out yo[NS];
#pragma unroll
                    for (int q = 0; q < NS; q++) xin[q] = __builtin_bit_cast(In, uint32_t(cur[q / 4][q % 4]));
                    tile_of<P, 1, NS>(prm, &p, xin, yo);
#pragma unroll
                    for (int q = 0; q < NS / 4; q++)
                        out[q] = u32x4{__builtin_bit_cast(uint32_t, yo[4 * q]), __builtin_bit_cast(uint32_t, yo[4 * q + 1]), __builtin_bit_cast(uint32_t, yo[4 * q + 2]),
                                       __builtin_bit_cast(uint32_t, yo[4 * q + 3])};
                } else {
#pragma unroll
                    for (int q = 0; q < NS / 4; q++) quad(cur + q * IW, out + q * OW);
                }
#pragma unroll
                for (int c = 0; c < CO; c++) out_piece(g * CO + c, out[c]);
                asm volatile("" ::: "memory");
#pragma unroll
                for (int c = 0; c < CI; c++) cur[c] = nxt[c];
            }
        }
    };
    auto store = [&](size_t v, auto whole, auto full, int nq) __attribute__((always_inline)) {
        char *dst = ybase + v * size_t(OB);
#pragma unroll
        for (int j = 0; j < NIO; j++) {
            const int pc = mpco ^ (NIO % 16 == 0 ? j & 15 : (mqo + j) & 15);
            const u32x4 v4 = *reinterpret_cast<const u32x4 *>(slot_out + j * 1024 + lid * 16);
            if ((decltype(whole)::value || size_t(mqo + j) < nrows) && (decltype(full)::value || pc < nq * OW) && IDSP_EXP_LM_ST_ON)
                global_st<u32x4, true>(dst + j * yrowb, yoff + uint32_t(pc * 16), v4);
            if (j % 8 == 7) asm volatile("" ::: "memory");  // at most 8 pieces between LDS and the store (the staged tile holds PI)
        }
    };
    auto walk = [&](auto whole) __attribute__((always_inline)) {
        using Full = std::true_type;
        using Part = std::false_type;
        if (nfull > 0)
            fetch(0, whole, Full{}, TF / 4);
        else
            fetch(0, whole, Part{}, nquad);
        for (size_t i = 0; i < nfull; i++) {
            hand_over();
            lds_wave_sync();
            if (i + 1 < nfull)
                fetch(i + 1, whole, Full{}, TF / 4);
            else if (nquad > 0)
                fetch(i + 1, whole, Part{}, nquad);
            compute(Full{}, TF / 4);
            lds_wave_sync();
            store(i, whole, Full{}, TF / 4);
            lds_wave_sync();
        }
        if (nquad > 0) {
            hand_over();
            lds_wave_sync();
            compute(Part{}, nquad);
            lds_wave_sync();
            store(nfull, whole, Part{}, nquad);
        }
    };
    if (nrows == size_t(LW))
        walk(std::true_type{});
    else
        walk(std::false_type{});

    if (active) {  // the last frames % 4 samples of this lane's own row
        const In *xr = x + (lane0 + lid) * xl;
        Out *yr = y + (lane0 + lid) * yl;
        for (size_t f = nfull * TF + size_t(nquad) * 4; f < frames; f++) {
            In v{};
            if constexpr (HAS_IN) v = xr[f];
            yr[f] = step1(p, prm, v);
        }
        p.store(prm, st, lanes, lane0 + lid);
    }
}

// ------------------------------------------- FRAME_MAJOR, few lanes (staged)
// Below ~49152 lanes the FrameMajor kernels above stop being bandwidth-bound: a lane is a serial chain, the LDS-DMA
// kernel pays two workgroup barriers per 8 frames and the register-window kernel a global-load wait per frame, and both
// take the same ~0.33 ms for 4096 frames whatever the lane count (80 ns = 190 cycles per frame and wave), so the rate
// falls with the lanes: 0.61 of the HBM peak at 49152 lanes, 0.41 at 32768, 0.20 at 16384 — while the LaneMajor staged
// kernel, whose threads run 128 frames from LDS without a barrier, needs 36 ns per frame.  This kernel gives FrameMajor
// buffers the same structure: one wave per workgroup owns LW lanes (64 / 32 / 16, as in the LaneMajor kernel); a tile is
// 32 KiB = TF frames x LW lanes, fetched as 16-byte pieces (one instruction = 1 KiB = 1024 / (LW W 4) row pieces — the
// neighbouring waves read the neighbouring pieces of the same rows) into VGPRs one tile ahead, handed to LDS linearly
// (instruction j's 1 KiB at 1024 j: the slot is [frame][lane]), walked by the owning thread down its column (conflict
// free: consecutive lanes, consecutive banks; two frames per ds_read2st64), results written in place, the slot re-read
// linearly and stored as whole row pieces.  Rows must be 16-byte aligned (lanes and pitches multiples of 4 / W).
constexpr int kFmStagedTile = 32768;  // bytes per tile
template <class P, class = void>
struct FmStagedOf {
    static constexpr bool value = false;
};
template <class P>
struct FmStagedOf<P, std::enable_if_t<P::HAS_IN && P::IN_DIV == 1 && sizeof(typename P::In) == sizeof(typename P::Out) &&
                                      (sizeof(typename P::In) == 4 || sizeof(typename P::In) == 8) && BatchOf<P>::value == 1>> {
    static constexpr bool value = true;
};

template <class P, int LW>
__global__ __launch_bounds__(kWave) void stream_frame_major_staged(
    const typename P::Params prm, uint32_t *st, const typename P::In *x, typename P::Out *y,
    const size_t lanes, const size_t frames, const size_t xl, const size_t yl, const size_t slanes, const int xcd_contiguous = 0)
{
    using In = typename P::In;
    using Out = typename P::Out;
    static_assert(FmStagedOf<P>::value && (LW == 64 || LW == 32 || LW == 16), "one 4- or 8-byte input and output per lane and frame");
    constexpr int W = int(sizeof(In)) / 4;          // words per sample
    constexpr int RB = LW * W * 4;                  // bytes of a row piece (one frame of the wave's lanes)
    constexpr int TF = kFmStagedTile / RB;          // frames per tile
    constexpr int PPR = RB / 16;                    // 16-byte pieces per row piece
    constexpr int RPI = kWave / PPR;                // rows one instruction covers
    constexpr int NI = kFmStagedTile / 1024;        // instructions per tile
    constexpr int NS = 16;                          // frames per compute chunk
    static_assert(TF % NS == 0 && NI * RPI == TF, "tile shape");
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    using Word = std::conditional_t<W == 1, uint32_t, uint64_t>;

    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    char *const slot = reinterpret_cast<char *>(smem);
    uint32_t *ptab = smem + kFmStagedTile / 4;  // [P::LDS_WORDS]
    const int lid = threadIdx.x;

    // xcd_contiguous (rows off the 64-byte grid): XCD j = blockIdx % 8 takes the j-th contiguous eighth of the lane blocks, so that the
    // 128-byte lines two neighbouring waves share are fetched and written through one L2 (see stream_frame_major_lds, XCDC)
    size_t wg = blockIdx.x;
    if (xcd_contiguous & 1) {
        const size_t q = gridDim.x / 8, r = gridDim.x % 8, j = blockIdx.x % 8;
        wg = j * q + (j < r ? j : r) + blockIdx.x / 8;
    }
    const size_t lane0 = wg * LW;
    const size_t nrows = lanes - lane0 < size_t(LW) ? lanes - lane0 : size_t(LW);  // lanes of this wave (a multiple of 4 / W)
    const bool active = size_t(lid) < nrows;

    P p;
    if constexpr (P::LDS_WORDS > 0) {
        P::fill_shared(ptab, lid, kWave);
        lds_wave_sync();
        p.set_shared(ptab);
    }
    if (active) p.load(prm, st, slanes, lane0 + lid);

    // mover role: in instruction j, row j RPI + mrow of the tile, piece mpc of the row piece; addresses = wave-uniform base
    // (SGPRs, see uniform_ptr) + 32-bit thread offset
    const size_t xrowb = xl * sizeof(In), yrowb = yl * sizeof(Out);  // bytes between frames
    const int mrow = lid / PPR, mpc = lid % PPR;
    const bool mine = size_t(mpc) * 16 < nrows * sizeof(In);  // this thread's piece lies inside the wave's lanes
    const char *const xbase = reinterpret_cast<const char *>(x) + lane0 * sizeof(In);
    char *const ybase = reinterpret_cast<char *>(y) + lane0 * sizeof(Out);
    const uint32_t xoff = uint32_t(mrow) * uint32_t(xrowb) + uint32_t(mpc) * 16, yoff = uint32_t(mrow) * uint32_t(yrowb) + uint32_t(mpc) * 16;

    const size_t nfull = frames / TF;
    const int ntail = int(frames - nfull * TF);  // frames of the last, partial tile
    u32x4 stage[NI];
    // FULL: all TF frames of the tile exist (else nf of them).  `mine` masks the pieces of missing lanes (last wave only; one
    // code path for whole and partial waves: the predicate is a loop-invariant exec mask, and the kernel compiles once)
    auto fetch_as = [&](size_t v, auto full, int nf, auto nt) __attribute__((always_inline)) {
        const char *src = xbase + v * TF * xrowb;
#pragma unroll
        for (int j = 0; j < NI; j++)
            if (mine && (decltype(full)::value || j * RPI + mrow < nf))
                stage[j] = global_ld<u32x4, decltype(nt)::value>(src + size_t(j * RPI) * xrowb, xoff);
    };
    // Rows off the 64-byte grid (xcd_contiguous & 2): the 128-byte lines at both ends of a wave's row piece are shared with the
    // neighbouring waves, and with nontemporal accesses each of the two fetches them from memory and writes its part back alone;
    // plain loads and stores let the second wave hit, and the two parts meet, in the L2 the XCD-contiguous order gives them in
    // common: 32769 lanes x 4096 frames 0.363 -> 0.268 ms, 32772 0.351 -> 0.278, 40001 0.489 -> 0.356 (round 4; plain stores
    // alone 0.341 / 0.312 / 0.418; aligned rows lose 4 % with plain accesses and keep the nontemporal ones).
    const bool plain = (xcd_contiguous & 2) != 0;
    auto fetch = [&](size_t v, auto full, int nf) __attribute__((always_inline)) {
        if (plain)
            fetch_as(v, full, nf, std::false_type{});
        else
            fetch_as(v, full, nf, std::true_type{});
    };
    auto hand_over = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < NI; j++) *reinterpret_cast<u32x4 *>(slot + j * 1024 + lid * 16) = stage[j];
    };
    Word *const col = reinterpret_cast<Word *>(slot) + lid;  // this thread's column: frame f at col[f LW]
    auto one = [&](Word w) __attribute__((always_inline)) {
        uint32_t ww[W];
        ww[0] = uint32_t(w);
        if constexpr (W == 2) ww[1] = uint32_t(uint64_t(w) >> 32);
        to_words<Out>(p.step(prm, words_to<In>(ww)), ww);
        if constexpr (W == 2)
            return Word(uint64_t(ww[0]) | (uint64_t(ww[1]) << 32));
        else
            return Word(ww[0]);
    };
    auto compute = [&](auto full, int nf) __attribute__((always_inline)) {
        if (!active) return;
        if constexpr (!decltype(full)::value || MaxU<P>::value < 24) {
            for (int f = 0; f < nf; f++) col[f * LW] = one(col[f * LW]);  // partial tile, or a large body: keep the loop rolled
        } else {
            // chunks of NS frames: the next chunk's LDS reads are issued before the current chunk's arithmetic; the fence
            // keeps the compiler from hoisting all reads of the tile above the first step
            Word cur[NS], nxt[NS];
#pragma unroll
            for (int c = 0; c < NS; c++) cur[c] = col[c * LW];
#pragma unroll
            for (int g = 0; g < TF / NS; g++) {
                if (g + 1 < TF / NS) {
#pragma unroll
                    for (int c = 0; c < NS; c++) nxt[c] = col[((g + 1) * NS + c) * LW];
                }
                if constexpr (HasTileOf<P>::value && W == 1) {
                    In xin[NS];
                    Out yo[NS];
#pragma unroll
                    for (int c = 0; c < NS; c++) xin[c] = __builtin_bit_cast(In, cur[c]);
                    tile_of<P, 1, NS>(prm, &p, xin, yo);
#pragma unroll
                    for (int c = 0; c < NS; c++) col[(g * NS + c) * LW] = __builtin_bit_cast(Word, yo[c]);
                } else {
#pragma unroll
                    for (int c = 0; c < NS; c++) col[(g * NS + c) * LW] = one(cur[c]);
                }
                asm volatile("" ::: "memory");
#pragma unroll
                for (int c = 0; c < NS; c++) cur[c] = nxt[c];
            }
        }
    };
    auto store_as = [&](size_t v, auto full, int nf, auto nt) __attribute__((always_inline)) {
        char *dst = ybase + v * TF * yrowb;
#pragma unroll
        for (int j = 0; j < NI; j++) {
            const u32x4 v4 = *reinterpret_cast<const u32x4 *>(slot + j * 1024 + lid * 16);
            if (mine && (decltype(full)::value || j * RPI + mrow < nf)) {
                global_st<u32x4, decltype(nt)::value>(dst + size_t(j * RPI) * yrowb, yoff, v4);
            }
            if (j % 8 == 7) asm volatile("" ::: "memory");
        }
    };
    auto store = [&](size_t v, auto full, int nf) __attribute__((always_inline)) {
        if (plain)
            store_as(v, full, nf, std::false_type{});
        else
            store_as(v, full, nf, std::true_type{});
    };
    using Full = std::true_type;
    using Part = std::false_type;
    if (nfull > 0)
        fetch(0, Full{}, TF);
    else
        fetch(0, Part{}, ntail);
    for (size_t i = 0; i < nfull; i++) {
        hand_over();
        lds_wave_sync();
        if (i + 1 < nfull)
            fetch(i + 1, Full{}, TF);
        else if (ntail > 0)
            fetch(i + 1, Part{}, ntail);
        compute(Full{}, TF);
        lds_wave_sync();
        store(i, Full{}, TF);
        lds_wave_sync();
    }
    if (ntail > 0) {
        hand_over();
        lds_wave_sync();
        compute(Part{}, ntail);
        lds_wave_sync();
        store(nfull, Part{}, ntail);
    }
    if (active) p.store(prm, st, slanes, lane0 + lid);
}

// ------------------------------------------- FRAME_MAJOR, few lanes: one wave computes, one wave moves (round 6)
// Below ~24576 lanes a FrameMajor launch is a race against ONE wave's serial chain: 4096 frames x (39.5 cycles for the i32 DF1
// step at one wave per SIMD, tools/ubench_df1_step.hip) = 0.069 ms, where stream_frame_major_staged needs 0.139 ms at 16384 lanes
// and the f32 sections, whose chain is no longer, 0.157: the rest is its skeleton — the same in-order wave issues the tile's 32
// loads, hands them to LDS, walks its column, re-reads the tile and issues 32 stores — and a section that only copies takes 0.11 ms
// in it.  Here the two halves run side by side: a workgroup is TWO waves over LW = 32 lanes; wave 1 (the mover) brings tile k + 1 in
// by `global_load_lds_dwordx4` (8 row pieces of 128 bytes per request, straight into the tile: no staging registers) and takes
// tile k - 1 out (`ds_read_b128` + 16-byte stores) while wave 0 walks its column of tile k; two 16 KiB tiles (128 frames), ONE barrier
// per tile: at barrier k the mover has waited for tile k's requests and the compute wave has finished tile k - 1.  The compute wave's
// loop holds nothing but LDS reads (two frames per instruction), the processor's steps and LDS writes.
constexpr int kFmPairTile = 16384;  // bytes per tile: 128 frames x 32 lanes (32 KiB tiles: 16384 lanes 0.108 against 0.102 ms, and only two workgroups per CU)
template <class P, int TB = kFmPairTile>
__global__ __launch_bounds__(2 * kWave) void stream_frame_major_pair(
    const typename P::Params prm, uint32_t *st, const typename P::In *x, typename P::Out *y,
    const size_t lanes, const size_t frames, const size_t xl, const size_t yl, const size_t slanes)
{
    using In = typename P::In;
    using Out = typename P::Out;
    static_assert(FmStagedOf<P>::value && sizeof(In) == 4 && sizeof(Out) == 4, "one 4-byte input and output per lane and frame");
    constexpr int LW = 32;
    constexpr int RB = LW * 4;                      // bytes of a row piece (one frame of the workgroup's lanes)
    constexpr int TF = TB / RB;                     // frames per tile
    constexpr int PPR = RB / 16;                    // 16-byte pieces per row piece
    constexpr int RPI = kWave / PPR;                // rows one instruction covers
    constexpr int NI = TB / 1024;                   // instructions per tile
    constexpr int NS = 16;                          // frames per compute chunk
    static_assert(TF % NS == 0 && NI * RPI == TF, "tile shape");
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    char *const slots = reinterpret_cast<char *>(smem);       // two tiles
    uint32_t *ptab = smem + 2 * TB / 4;                       // [P::LDS_WORDS]
    const int lid = threadIdx.x % kWave;
    const bool mover = __builtin_amdgcn_readfirstlane(int(threadIdx.x / kWave)) != 0;
    const size_t lane0 = size_t(blockIdx.x) * LW;
    const size_t nrows = lanes - lane0 < size_t(LW) ? lanes - lane0 : size_t(LW);  // lanes of this workgroup (a multiple of 4)
    const size_t ntiles = (frames + TF - 1) / TF;
    const int ntail = int(frames - (ntiles - 1) * TF);  // frames of the last tile (1 .. TF)

    if (mover) {
        // in instruction j: row j RPI + mrow of the tile, piece mpc of the row piece
        const size_t xrowb = xl * sizeof(In), yrowb = yl * sizeof(Out);
        const int mrow = lid / PPR, mpc = lid % PPR;
        const bool mine = size_t(mpc) * 16 < nrows * sizeof(In);  // this thread's piece lies inside the workgroup's lanes
        const char *const xbase = reinterpret_cast<const char *>(x) + lane0 * sizeof(In);
        char *const ybase = reinterpret_cast<char *>(y) + lane0 * sizeof(Out);
        const uint32_t xoff = uint32_t(mrow) * uint32_t(xrowb) + uint32_t(mpc) * 16, yoff = uint32_t(mrow) * uint32_t(yrowb) + uint32_t(mpc) * 16;
        const uint32_t slots_lds = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char *)slots;
        auto load = [&](size_t k) __attribute__((always_inline)) {
            const char *src = xbase + k * TF * xrowb;
            const int nf = k + 1 == ntiles ? ntail : TF;
            const uint32_t dst = slots_lds + uint32_t(k & 1) * TB;
#pragma unroll
            for (int j = 0; j < NI; j++)
                if (mine && j * RPI + mrow < nf) glds16_s(uniform_ptr(src + size_t(j * RPI) * xrowb), xoff, dst + j * 1024);
        };
        auto store = [&](size_t k) __attribute__((always_inline)) {
            char *dst = ybase + k * TF * yrowb;
            const int nf = k + 1 == ntiles ? ntail : TF;
            const char *slot = slots + (k & 1) * TB;
#pragma unroll
            for (int j = 0; j < NI; j++) {
                const u32x4 v4 = *reinterpret_cast<const u32x4 *>(slot + j * 1024 + lid * 16);
                if (mine && j * RPI + mrow < nf) global_st<u32x4, true>(dst + size_t(j * RPI) * yrowb, yoff, v4);
                if (j % 8 == 7) asm volatile("" ::: "memory");
            }
        };
        load(0);
        for (size_t k = 0; k < ntiles; k++) {
            wait_vmcnt<0>();  // tile k has landed (and the stores of tile k - 2 are done)
            lds_barrier();    // barrier k: the compute wave has finished tile k - 1
            if (k >= 1) {
                store(k - 1);
                lds_wave_sync();  // its LDS reads are done: the tile may be overwritten
            }
            if (k + 1 < ntiles) load(k + 1);
        }
        lds_barrier();  // barrier ntiles: the last tile is computed
        store(ntiles - 1);
        return;
    }

    // ---- compute wave
    const bool active = size_t(lid) < nrows;
    P p;
    if constexpr (P::LDS_WORDS > 0) {
        P::fill_shared(ptab, lid, kWave);
        lds_wave_sync();
        p.set_shared(ptab);
    }
    if (active) p.load(prm, st, slanes, lane0 + lid);
    auto one = [&](uint32_t w) __attribute__((always_inline)) {
        uint32_t ww[1] = {w};
        to_words<Out>(p.step(prm, words_to<In>(ww)), ww);
        return ww[0];
    };
    for (size_t k = 0; k < ntiles; k++) {
        lds_barrier();  // barrier k: tile k has landed
        uint32_t *const col = reinterpret_cast<uint32_t *>(slots + (k & 1) * TB) + lid;  // frame f at col[f LW]
        if (!active) continue;
        if (k + 1 == ntiles && ntail != TF) {
            for (int f = 0; f < ntail; f++) col[f * LW] = one(col[f * LW]);
        } else if constexpr (MaxU<P>::value < 24) {
            for (int f = 0; f < TF; f++) col[f * LW] = one(col[f * LW]);  // a large body: keep the loop rolled
        } else {
            // chunks of NS frames: the next chunk's LDS reads are issued before the current chunk's arithmetic
            uint32_t cur[NS], nxt[NS];
#pragma unroll
            for (int c = 0; c < NS; c++) cur[c] = col[c * LW];
#pragma unroll 1
            for (int g = 0; g < TF / NS; g++) {
                if (g + 1 < TF / NS) {
#pragma unroll
                    for (int c = 0; c < NS; c++) nxt[c] = col[((g + 1) * NS + c) * LW];
                }
                if constexpr (HasTileOf<P>::value) {
                    In xin[NS];
                    Out yo[NS];
#pragma unroll
                    for (int c = 0; c < NS; c++) xin[c] = __builtin_bit_cast(In, cur[c]);
                    tile_of<P, 1, NS>(prm, &p, xin, yo);
#pragma unroll
                    for (int c = 0; c < NS; c++) col[(g * NS + c) * LW] = __builtin_bit_cast(uint32_t, yo[c]);
                } else {
#pragma unroll
                    for (int c = 0; c < NS; c++) col[(g * NS + c) * LW] = one(cur[c]);
                }
                asm volatile("" ::: "memory");
#pragma unroll
                for (int c = 0; c < NS; c++) cur[c] = nxt[c];
            }
        }
    }
    lds_barrier();  // barrier ntiles
    if (active) p.store(prm, st, slanes, lane0 + lid);
}

// ------------------------------------------------------------- FRAME_MAJOR, two waves per 64 lanes
// A serial chain of sections split over TWO waves (round 3).  A VALU-bound processor at one wave per SIMD — 65536 lanes are
// 1024 waves — runs at the issue rate of a single wave, and for the i32 sections that is one v_mad_i64_i32 per ~10 cycles
// where two waves on the SIMD get one per 5 (tools/ubench_valu.hip): a 4-section i32 chain sits at 0.58 of the HBM peak,
// the 8-section cascade at 0.47, both far from memory-bound.  Here a workgroup of two waves owns 64 lanes: wave 0 runs the
// first part of the chain (processor PA) on the input and leaves its output in an LDS tile of T frames, wave 1 runs the
// rest (PB) one tile behind and writes y; one workgroup barrier per tile, tiles double-buffered.  Twice the waves per SIMD
// and every lane still one thread per wave — and 8 sections are ONE pass over HBM instead of two.  Results are those of
// the single-wave kernels: both halves run the same per-sample functors on the same sample sequences.
// In place (y == x): wave 0 reads frame f at least a tile before wave 1 writes it.
template <class PA, class PB, int T = 32>
__global__ __launch_bounds__(2 * kWave) void stream_frame_major_duo(
    const typename PA::Params prmA, const typename PB::Params prmB, uint32_t *stA, uint32_t *stB, const typename PA::In *x,
    typename PB::Out *y, const size_t lanes, const size_t frames, const size_t xl, const size_t yl)
{
    using In = typename PA::In;
    using Mid = typename PA::Out;
    using Out = typename PB::Out;
    static_assert(std::is_same<Mid, typename PB::In>::value && PA::LDS_WORDS == 0 && PB::LDS_WORDS == 0 && PA::IN_DIV == 1 && PB::IN_DIV == 1,
                  "PB continues PA's sample stream; table-free processors");
    __shared__ Mid tile[2][T][kWave];
    const int wave = __builtin_amdgcn_readfirstlane(int(threadIdx.x) / kWave), lid = int(threadIdx.x) % kWave;
    const size_t lane = size_t(blockIdx.x) * kWave + lid;
    const bool active = lane < lanes;
    const size_t la = active ? lane : lanes - 1;  // idle threads of the last workgroup shadow a valid lane, stores masked
    const size_t nfull = frames / T;
    const int ntail = int(frames - nfull * T);  // frames of the last, partial tile
    if (wave == 0) {
        PA p;
        p.load(prmA, stA, lanes, la);
        const In *xp = x + la;
        In cur[T], nxt[T];
        // whole tiles: no per-frame predicates (wave-uniform runtime tests per frame fragment the loop into hundreds of blocks)
        auto fetch = [&](size_t k, In (&dst)[T], auto full) __attribute__((always_inline)) {
#pragma unroll
            for (int f = 0; f < T; f++)
                if (decltype(full)::value || f < ntail) dst[f] = nt_load<true>(xp + (k * T + f) * xl);
        };
        if (nfull)
            fetch(0, cur, std::true_type{});
        else
            fetch(0, cur, std::false_type{});
        for (size_t k = 0; k < nfull; k++) {
            if (k + 1 < nfull)
                fetch(k + 1, nxt, std::true_type{});
            else if (ntail)
                fetch(k + 1, nxt, std::false_type{});
#pragma unroll
            for (int f = 0; f < T; f++) tile[k & 1][f][lid] = p.step(prmA, cur[f]);
#pragma unroll
            for (int f = 0; f < T; f++) cur[f] = nxt[f];
            lds_barrier();  // tile k complete; wave 1 has finished tile k - 1 (it may be overwritten two tiles on)
        }
        if (ntail) {
            for (int f = 0; f < ntail; f++) tile[nfull & 1][f][lid] = p.step(prmA, cur[f]);
            lds_barrier();
        }
        lds_barrier();  // pairs with wave 1's last interval
        if (active) p.store(prmA, stA, lanes, lane);
    } else {
        PB p;
        p.load(prmB, stB, lanes, la);
        Out *yp = y + la;
        lds_barrier();  // tile 0
        for (size_t k = 0; k < nfull; k++) {
            Mid v[T];
#pragma unroll
            for (int f = 0; f < T; f++) v[f] = tile[k & 1][f][lid];
#pragma unroll
            for (int f = 0; f < T; f++) {
                // (no `if (active)`: an idle thread of the last workgroup shadows lane `lanes - 1` — same input, same state, the same
                // value to the same address — and a predicate per store is a branch per sample in the ISA)
                nt_store<true>(yp + (k * T + f) * yl, p.step(prmB, v[f]));
            }
            lds_barrier();
        }
        if (ntail) {
            for (int f = 0; f < ntail; f++) {
                const Out o = p.step(prmB, tile[nfull & 1][f][lid]);
                if (active) nt_store<true>(yp + (nfull * T + f) * yl, o);
            }
            lds_barrier();
        }
        if (active) p.store(prmB, stB, lanes, lane);
    }
}

// ------------------------------------------------------------- FRAME_MAJOR, one to three lanes
// The last lanes % 4 lanes of a call whose rows do not hold a whole number of 16-byte pieces (launch_stream runs them beside the
// rest on a second stream).  One thread per lane on the register-window kernel is a chain of frames at ~90 ns each — the load
// latency over the ring depth: 0.36-0.42 ms for 4096 frames, longer than the whole 65536-lane body beside it and three times
// a 16384-lane body.  Here ONE wave moves the samples of 256 frames per tile with all 64 threads (thread t: frames t, t + 64,
// t + 128, t + 192 of each lane), hands them over through LDS, threads 0 .. n - 1 walk their lane's 256 samples from there
// (the next tile's loads in flight), and all 64 threads store the results.
template <class P>
__global__ __launch_bounds__(kWave) void stream_frame_major_few(
    const typename P::Params prm, uint32_t *st, const typename P::In *x, typename P::Out *y,
    const int n, const size_t frames, const size_t xl, const size_t yl, const size_t slanes)
{
    using In = typename P::In;
    using Out = typename P::Out;
    static_assert(P::HAS_IN && P::IN_DIV == 1 && sizeof(In) == 4 && sizeof(Out) == 4, "one 4-byte sample in, one out");
    constexpr int K = 4, TF = K * kWave, ML = 3;
    __shared__ uint32_t tin[TF][4], tout[TF][4];
    __shared__ uint32_t ptab[P::LDS_WORDS ? P::LDS_WORDS : 1];
    const int t = threadIdx.x;
    if constexpr (P::LDS_WORDS > 0) {
        P::fill_shared(ptab, t, kWave);
        lds_wave_sync();
    }
    P p;
    if constexpr (P::LDS_WORDS > 0) p.set_shared(ptab);
    const bool own = t < n;
    if (own) p.load(prm, st, slanes, size_t(t));
    uint32_t cur[K][ML] = {};
    const size_t ntiles = (frames + TF - 1) / TF;
    auto fetch = [&](size_t tile) __attribute__((always_inline)) {
#pragma unroll
        for (int k = 0; k < K; k++) {
            const size_t f = tile * TF + size_t(k) * kWave + t;
            if (f < frames) {
#pragma unroll
                for (int j = 0; j < ML; j++)
                    if (j < n) cur[k][j] = __builtin_bit_cast(uint32_t, x[f * xl + j]);
            }
        }
    };
    fetch(0);
    for (size_t i = 0; i < ntiles; i++) {
#pragma unroll
        for (int k = 0; k < K; k++)
#pragma unroll
            for (int j = 0; j < ML; j++) tin[k * kWave + t][j] = cur[k][j];
        lds_wave_sync();
        if (i + 1 < ntiles) fetch(i + 1);
        if (own) {
            const size_t left = frames - i * TF;
            const int nf = left < size_t(TF) ? int(left) : TF;
            int f = 0;
            for (; f + 8 <= nf; f += 8) {
                uint32_t v[8];
#pragma unroll
                for (int u = 0; u < 8; u++) v[u] = tin[f + u][t];
#pragma unroll
                for (int u = 0; u < 8; u++) tout[f + u][t] = __builtin_bit_cast(uint32_t, step1(p, prm, __builtin_bit_cast(In, v[u])));
            }
            for (; f < nf; f++) tout[f][t] = __builtin_bit_cast(uint32_t, step1(p, prm, __builtin_bit_cast(In, tin[f][t])));
        }
        lds_wave_sync();
#pragma unroll
        for (int k = 0; k < K; k++) {
            const size_t f = i * TF + size_t(k) * kWave + t;
            if (f < frames) {
#pragma unroll
                for (int j = 0; j < ML; j++)
                    if (j < n) y[f * yl + j] = __builtin_bit_cast(Out, tout[k * kWave + t][j]);
            }
        }
        lds_wave_sync();
    }
    if (own) p.store(prm, st, slanes, size_t(t));
}

// a size from the environment (diagnostic switches: honoured only with IDSP_DIAG=1)
inline size_t diag_size(const char *name, size_t dflt)
{
    const char *e = diag_env(name);
    return e ? size_t(strtoull(e, nullptr, 10)) : dflt;
}

}  // namespace idsp
#include "stream_plan.h"  // which kernel a call takes: the pure half of the launcher below
#include "fm_sweep.h"     // the dense-sweep FrameMajor kernel (round 5): needs everything above, is needed by launch_stream below
namespace idsp {

// --------------------------------------------------------------------- launch
static_assert(kPlanWave == size_t(kWave) && kPlanBlock == size_t(kFmBlock) && kPlanSweepSegments == size_t(kSweepT) &&
                  thr::kLmStagedMinRowBytes == size_t(kLmRun) / 4 && thr::kLdsGridCap == kLdsGridCap,
              "stream_plan.h restates these");

// The kernel-selection switches of launch_stream and duo_wanted, read once per process (honoured only with IDSP_DIAG=1: diag_env)
inline const StreamSwitches &stream_switches()
{
    static const StreamSwitches sw = read_stream_switches(diag_env);
    return sw;
}

// What plan_stream reads from a processor
template <class P>
constexpr StreamTraits traits_of()
{
    StreamTraits t;
    t.has_in = P::HAS_IN, t.in_div = P::IN_DIV, t.in_bytes = sizeof(typename P::In), t.out_bytes = sizeof(typename P::Out), t.cost = P::COST;
    t.lds_eligible = LdsEligibleOf<P>::value, t.lds_ring = LdsRingOf<P>::value;
    t.fm_staged = FmStagedOf<P>::value, t.lm_staged = LmStagedOf<P>::value, t.lm_one_form = LmOneFormOf<P>::value;
    t.sweep_max_lpt = SweepMaxLptOf<P>::value;
    return t;
}

// Row pitches of a call: elements between consecutive frames (FRAME_MAJOR) or between the starts of consecutive
// lanes (LANE_MAJOR) of x and y; 0 = dense.  The `_pitch` entry points of the ABI pass them through.
struct Pitch {
    size_t x = 0, y = 0;
};

// Parameters of a lane block that starts `first` lanes into the call: per-lane coefficient planes (ByLaneParams::coef) move
// with the lanes, everything else is shared
template <class T, class = void>
struct HasCoefPlanes : std::false_type {};
template <class T>
struct HasCoefPlanes<T, std::void_t<decltype(std::declval<T>().coef)>> : std::true_type {};
// (parameters that carry a per-lane side pointer under the name `xw` — lockin_generic.hip's XWalk, lockin_accu_procs.h's AccuWalk, both
// computed from the lane index of the WHOLE call — cannot be shifted here: launch_stream's lane splits only take 4-byte-in / 4-byte-out processors, and this assert keeps it so)
template <class T, class = void>
struct HasSideWalk : std::false_type {};
template <class T>
struct HasSideWalk<T, std::void_t<decltype(std::declval<T>().xw)>> : std::true_type {};
template <class Params>
inline Params shift_lanes(Params p, size_t first, size_t elem)
{
    static_assert(!HasSideWalk<Params>::value, "lane split of a processor whose parameters hold a side pointer `xw` (XWalk, AccuWalk): shift it here first");
    if constexpr (HasCoefPlanes<Params>::value) p.coef = static_cast<const char *>(p.coef) + first * elem;
    return p;
}

// One call as the per-form launch functions below see it (`sp`: lanes between the state planes)
template <class P>
struct StreamArgs {
    const typename P::Params &prm;
    uint32_t *st;
    const typename P::In *x;
    typename P::Out *y;
    size_t lanes, frames, sp;
    hipStream_t s;
};

// One function per form of the plan: each notes the name stream_plan_name gives the plan and launches that kernel.  The `if constexpr` /
// `static_assert` conditions are those under which launch_call reaches them: a processor instantiates exactly the kernels it can take.
template <class P>
int launch_lm_tile(const StreamArgs<P> &a, const StreamPlan &p)
{
    note_kernel(stream_plan_name(p), typeid(P).name());
    hipLaunchKernelGGL((stream_lane_major<P>), dim3(p.grid), dim3(kWave), 0, a.s, a.prm, a.st, a.x, a.y, a.lanes, a.frames, p.xl, p.yl);
    return launch_status();
}

template <class P>
int launch_lm_staged(const StreamArgs<P> &a, const StreamPlan &p)
{
    auto go = [&](auto lw_tag) {
        constexpr int LW = decltype(lw_tag)::value;
        // the 32- and 16-lane forms move 1 KiB per lane and tile (the same 32 / 16 KiB slot and staging registers
        // as 512-byte runs would need at twice the lanes): 5-10 % faster at 16384 lanes and below, 10-20 % on rows
        // that are not 128-byte aligned, equal at 65536 lanes (profiles/r02_tune_lm_run1k.jsonl)
        constexpr int LB = LW == 64 ? kLmRun : 2 * kLmRun;
        constexpr size_t bytes = lm_staged_lds_bytes<P, LW, LB>();
        if (int rc = ensure_dyn_lds<&stream_lane_major_staged<P, LW, LB>>(bytes)) return rc;
        note_kernel(stream_plan_name(p), typeid(P).name());
        const StreamSwitches &sw = stream_switches();
        const unsigned lm_skew = unsigned(sw.lm_skew), lm_skew_shift = (unsigned(sw.lm_skew_shift) & 31u) | ((unsigned(sw.lm_skew_mod) & 255u) << 8);
        hipLaunchKernelGGL((stream_lane_major_staged<P, LW, LB>), dim3(p.grid), dim3(kWave), bytes, a.s, a.prm, a.st, a.x, a.y, a.lanes, a.frames, p.xl, p.yl,
                           lm_skew, lm_skew_shift);
        return launch_status();
    };
    // forms instantiated per processor: all three for the cheap ones, 64 / 32 for the heavy ones, 64 only for P::LM_ONE_FORM (plan_lane_major)
    if constexpr (!LmOneFormOf<P>::value) {
        if constexpr (!traits_of<P>().heavy()) {
            if (p.lanes_per_wave == 16) return go(std::integral_constant<int, 16>{});
        }
        if (p.lanes_per_wave == 32) return go(std::integral_constant<int, 32>{});
    }
    return go(std::integral_constant<int, 64>{});
}

// n = 1 ... 3 lanes from lane `first` of the call, on stream `s`
template <class P>
int launch_fm_few(const StreamArgs<P> &a, const StreamPlan &p, size_t first, size_t n, hipStream_t s)
{
    hipLaunchKernelGGL((stream_frame_major_few<P>), dim3(1), dim3(kWave), 0, s, shift_lanes(a.prm, first, sizeof(typename P::In)), a.st + first, a.x + first,
                       a.y + first, int(n), a.frames, p.xl, p.yl, a.sp);
    return launch_status();
}

template <class P>
int launch_fm_pair(const StreamArgs<P> &a, const StreamPlan &p)
{
    constexpr size_t bytes = 2 * size_t(kFmPairTile) + size_t(P::LDS_WORDS) * 4;
    if (int rc = ensure_dyn_lds<&stream_frame_major_pair<P>>(bytes)) return rc;
    note_kernel(stream_plan_name(p), typeid(P).name());
    hipLaunchKernelGGL((stream_frame_major_pair<P>), dim3(unsigned((a.lanes + 31) / 32)), dim3(2 * kWave), bytes, a.s, a.prm, a.st, a.x, a.y, a.lanes, a.frames,
                       p.xl, p.yl, a.sp);
    return launch_status();
}

template <class P>
int launch_fm_staged(const StreamArgs<P> &a, const StreamPlan &p)
{
    auto go = [&](auto lw_tag) {
        constexpr int LW = decltype(lw_tag)::value;
        constexpr size_t bytes = size_t(kFmStagedTile) + size_t(P::LDS_WORDS) * 4;
        if (int rc = ensure_dyn_lds<&stream_frame_major_staged<P, LW>>(bytes)) return rc;
        note_kernel(stream_plan_name(p), typeid(P).name());
        hipLaunchKernelGGL((stream_frame_major_staged<P, LW>), dim3(p.grid), dim3(kWave), bytes, a.s, a.prm, a.st, a.x, a.y, a.lanes, a.frames, p.xl, p.yl, a.sp,
                           p.staged_flags);
        return launch_status();
    };
    if constexpr (!traits_of<P>().heavy()) {
        if (p.lanes_per_wave == 16) return go(std::integral_constant<int, 16>{});
        if (p.lanes_per_wave == 64) return go(std::integral_constant<int, 64>{});
    }
    return go(std::integral_constant<int, 32>{});
}

template <class P>
int launch_fm_lds(const StreamArgs<P> &a, const StreamPlan &p)
{
    constexpr size_t ow = sizeof(typename P::Out) / 4;
    auto go = [&](auto deep, auto xcdc) {
        constexpr bool DEEP = decltype(deep)::value, XCDC = decltype(xcdc)::value;
        constexpr int NB = DEEP ? 7 : LdsRingOf<P>::value;
        constexpr bool RUN = DEEP ? false : LdsRunOf<P>::value;
        constexpr size_t bytes = (size_t(NB) * kLdsT * kFmBlock + 2 * size_t(kLdsT) * kFmBlock * ow + P::LDS_WORDS) * 4;
        if (int rc = ensure_dyn_lds<&stream_frame_major_lds<P, NB, RUN, XCDC>>(bytes)) return rc;
        note_kernel(stream_plan_name(p), typeid(P).name());
        hipLaunchKernelGGL((stream_frame_major_lds<P, NB, RUN, XCDC>), dim3(p.grid), dim3(kFmBlock), bytes, a.s, a.prm, a.st, a.x, a.y, a.lanes, a.frames, p.xl,
                           p.yl, a.sp);
        return launch_status();
    };
    using Yes = std::true_type;
    using No = std::false_type;
    if (p.xcdc) return go(Yes{}, Yes{});  // XCD-contiguous blocks: always the deep ring
    if (p.deep_ring) return go(Yes{}, No{});
    return go(No{}, No{});
}

template <class P>
int launch_fm_window(const StreamArgs<P> &a, const StreamPlan &p)
{
    constexpr int kDeep = MaxU<P>::value, kShallow = kDeep < 8 ? kDeep : 8;
    note_kernel(stream_plan_name(p), typeid(P).name());
    if (p.deep_window)
        hipLaunchKernelGGL((stream_frame_major<P, kDeep>), dim3(p.grid), dim3(p.block), 0, a.s, a.prm, a.st, a.x, a.y, a.lanes, a.frames, p.xl, p.yl, int(p.xcdc), a.sp);
    else
        hipLaunchKernelGGL((stream_frame_major<P, kShallow>), dim3(p.grid), dim3(p.block), 0, a.s, a.prm, a.st, a.x, a.y, a.lanes, a.frames, p.xl, p.yl, int(p.xcdc), a.sp);
    return launch_status();
}

// Plans the call `c` (x and y are its two addresses, typed) and launches what the plan says; `took`: the form it took
template <class P>
int launch_call(const typename P::Params &prm, uint32_t *st, const typename P::In *x, typename P::Out *y, StreamCall c, hipStream_t s, StreamForm *took = nullptr)
{
    constexpr StreamTraits t = traits_of<P>();
    const size_t sp = c.state_pitch ? c.state_pitch : c.lanes;  // lanes between the state planes (a lane block of a larger call keeps the call's)
    if (c.layout == IDSP_LANE_MAJOR && sp != c.lanes) return fail(IDSP_EINVAL, "internal: lane block with a state pitch on a LaneMajor kernel");
    StreamPlan p = plan_stream(t, c, stream_switches());
    SideStream *ss = nullptr;
    if (p.form == StreamForm::FmOddBeside || p.form == StreamForm::FmRoundsBeside) {
        // a caller whose stream lives on another device than the current one has no second stream: the unsplit forms
        if (!(ss = side_stream(s))) c.no_side_stream = true, p = plan_stream(t, c, stream_switches());
    }
    if (took) *took = p.form;
    const StreamArgs<P> a{prm, st, x, y, c.lanes, c.frames, sp, s};
    switch (p.form) {
        case StreamForm::LmTile: return launch_lm_tile<P>(a, p);
        case StreamForm::LmStaged:
            if constexpr (t.lm_staged) return launch_lm_staged<P>(a, p);
            break;
        case StreamForm::FmFew:
            if constexpr (t.four_four()) {
                note_kernel(stream_plan_name(p), typeid(P).name());
                return launch_fm_few<P>(a, p, 0, c.lanes, s);
            }
            break;
        case StreamForm::FmOddBeside:
            // the last lanes % 4 on the second stream, the body (a lane block of the caller's tensors) on the caller's
            if constexpr (t.four_four()) {
                IDSP_HIP_TRY(hipEventRecord(ss->fork, s));
                IDSP_HIP_TRY(hipStreamWaitEvent(ss->stream, ss->fork, 0));
                int rc = launch_fm_few<P>(a, p, p.body, p.odd, ss->stream);
                if (rc == IDSP_OK) rc = launch_call<P>(prm, st, x, y, lane_block(c, p, 0, p.body, false), s);
                IDSP_HIP_TRY(hipEventRecord(ss->join, ss->stream));
                IDSP_HIP_TRY(hipStreamWaitEvent(s, ss->join, 0));
                if (rc == IDSP_OK) note_kernel_also(stream_plan_also(p));
                return rc;
            }
            break;
        case StreamForm::FmRoundsBeside:
            // the whole rounds on the caller's stream, the remainder beside them on the second: both are lane blocks of the caller's
            // tensors (row pitches xl / yl, state and coefficient planes at the call's pitch)
            if constexpr (t.fm_staged && t.four_four() && !t.heavy()) {
                IDSP_HIP_TRY(hipEventRecord(ss->fork, s));
                IDSP_HIP_TRY(hipStreamWaitEvent(ss->stream, ss->fork, 0));
                // which kernel the whole rounds go to: the dense-sweep kernel, or the LDS-DMA panel walk for the processors / shapes the sweep does not take
                StreamForm head_form = StreamForm::FmLds;
                int rc = launch_call<P>(prm, st, x, y, lane_block(c, p, 0, p.head, false), s, &head_form);
                p.head_swept = head_form == StreamForm::FmSweep;
                if (rc == IDSP_OK)
                    rc = launch_call<P>(shift_lanes(prm, p.head, sizeof(typename P::In)), st + p.head, x + p.head, y + p.head, lane_block(c, p, p.head, p.tail, true),
                                        ss->stream);
                // join even after a failed launch: the caller's stream must not run ahead of whatever the side stream holds
                IDSP_HIP_TRY(hipEventRecord(ss->join, ss->stream));
                IDSP_HIP_TRY(hipStreamWaitEvent(s, ss->join, 0));
                if (rc == IDSP_OK) note_kernel(stream_plan_name(p), typeid(P).name());
                return rc;
            }
            break;
        case StreamForm::FmPair:
            if constexpr (t.fm_staged && t.four_four() && t.cost <= thr::kPairMaxCost) return launch_fm_pair<P>(a, p);
            break;
        case StreamForm::FmSweep:
            if constexpr (t.lds_input() && t.lds_eligible) return launch_sweep<P>(prm, st, x, y, c.lanes, c.frames, sp, p, s);
            break;
        case StreamForm::FmStaged:
            if constexpr (t.fm_staged) return launch_fm_staged<P>(a, p);
            break;
        case StreamForm::FmLds:
            if constexpr (t.lds_input()) return launch_fm_lds<P>(a, p);
            break;
        case StreamForm::FmWindow: return launch_fm_window<P>(a, p);
    }
    return fail(IDSP_EINVAL, "internal: the plan names a kernel this processor does not have");
}

template <class P>
int launch_stream(const typename P::Params &prm, void *state, const typename P::In *x,
                  typename P::Out *y, size_t lanes, size_t frames, int layout, hipStream_t s, Pitch pitch = {}, size_t state_pitch = 0)
{
    if (lanes == 0) return IDSP_OK;
    StreamCall c;
    c.lanes = lanes, c.frames = frames, c.layout = layout;
    c.x = reinterpret_cast<uintptr_t>(x), c.y = reinterpret_cast<uintptr_t>(y);
    c.pitch_x = pitch.x, c.pitch_y = pitch.y, c.state_pitch = state_pitch;
    return launch_call<P>(prm, static_cast<uint32_t *>(state), x, y, c, s);
}

// Two-wave launch of a chain split into PA (first sections) and PB (the rest): FRAME_MAJOR only, 4-byte samples
template <class PA, class PB>
int launch_duo(const typename PA::Params &pa, const typename PB::Params &pb, uint32_t *stA, uint32_t *stB, const typename PA::In *x,
               typename PB::Out *y, size_t lanes, size_t frames, hipStream_t s, Pitch pitch)
{
    const size_t xl = pitch.x ? pitch.x : lanes, yl = pitch.y ? pitch.y : lanes;
    note_kernel("stream_frame_major_duo", typeid(PB).name());
    hipLaunchKernelGGL((stream_frame_major_duo<PA, PB>), dim3(unsigned((lanes + kWave - 1) / kWave)), dim3(2 * kWave), 0, s, pa, pb, stA, stB, x, y, lanes,
                       frames, xl, yl);
    return launch_status();
}

// When a chain of m sections goes to it (stream_plan.h; IDSP_DIAG=1 IDSP_NO_DUO=1: never)
inline bool duo_wanted(size_t m, size_t lanes, int layout) { return duo_wanted(m, lanes, layout, stream_switches()); }

}  // namespace idsp
