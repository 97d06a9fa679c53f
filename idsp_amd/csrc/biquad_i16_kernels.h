// biquad_i16_kernels.h — `Biquad<Q16<F>>` x `DirectForm1<i16>` and `BiquadClamp<Q16<F>, i16>` of the reference per lane
// (src/iir/biquad.rs:366-383 and :394-404 with C = Q<i16, i32, F>, T = i16, A = Q<i32, i16, F>): i16 rows in, i16 rows out, in place
// if wanted.  Input AND output elements are half a 32-bit word (lane_stream.h asserts "samples are one or two 32-bit words" in
// every kernel), so these kernels move their own bytes, as dsm_kernels.h does for its byte output.
//
// Semantics, as a RELEASE build of the reference computes them (every i32 and i16 operation wraps):
//   * acc: i32 = b0 x0 + b1 x[0] + b2 x[1] + a1 y[0] + a2 y[1]; each product is i32(c) * i32(v) (dsp-fixedpoint/src/lib.rs:310-312,
//     ops.rs:91-97), the sum runs left to right in wrapping i32 (ops.rs:63-76).  Five products of up to 2^30 do leave i32: a debug
//     build panics there, here the sum wraps.  A wrapping sum is associative, so the order is free;
//   * y0 = (acc >> F) as i16: arithmetic shift of the i32, truncating cast (num_traits_impl.rs:74-90, lib.rs:270-299), 0 <= F < 32;
//   * clamp form: y0 = clamp(y0 + u, min, max), the `+` in wrapping i16, `num_traits::clamp` (min first, so min > max yields min
//     for anything below it and max for the rest above max), and y0 is what the state keeps (:400-401).
// The operands are 16-bit, so nothing needs the quarter-rate 64-bit multiply-adds of the i32 step.  A delay pair lives in ONE register,
// x[0] | x[1] << 16, beside the coefficient pairs b1 | b2 << 16 and a1 | a2 << 16, and the sum is three `v_dot2_i32_i16`
// (D = A.lo B.lo + A.hi B.hi + C in wrapping i32, full rate): b0 against the input word with a zero partner half, then the two pairs.
// A new value enters its pair by one `v_perm_b32`, which keeps its low 16 bits: the truncating cast of `.as_()` costs nothing.  (The
// first form of this step, five `v_mul_i32_i24` on sign-extended words and two `v_add3_u32`, was a third longer and took 0.260 ms
// where this one takes 0.208, FrameMajor 65536 lanes x 4096 frames: profiles/NOTES.md, "Biquad i16".)
// State (include/idsp_hip.h): W = 4 words per section and lane {x0, x1, y0, y1}, word-plane-major; an i16 sits in a 32-bit word that
// is read as its low half and written back sign-extended.
//
// Which alignments take which form: biquad_i16_plan.h.
#pragma once

#include "biquad_i16_plan.h"
#include "subword_rows.h"

namespace idsp {
namespace bq16 {

using subword::kFmU;  // depth of the rotating register window
static_assert(kWave == subword::kWave, "biquad_i16_plan.h (no HIP: it cannot include subword_rows.h) and the walkers agree on the wave");
constexpr int kLmTW = 64;          // dwords per lane and tile: 256-byte runs
constexpr int kLmTS = 2 * kLmTW;   // samples per lane and tile

// one section, packed on the host from the i16 fields of the ABI structs
struct Sec {
    uint32_t b0lo, b0hi;  // b0 in the low half / in the high half, the other half zero: picks the sample out of a word that holds two
    uint32_t b12, a12;    // b1 | b2 << 16, a1 | a2 << 16
    int32_t frac;
    int32_t u, mn, mx;    // sign-extended
};
template <int N>
struct Params {
    Sec sec[N];
};

// the measurement switches of biquad_i16_plan.h, read once per process
inline Switches switches()
{
    static const Switches sw = [] {
        Switches s;
        if (const char *e = diag_env("IDSP_BQ16_FM_BLOCK")) s.fm_block = unsigned(atoi(e));
        return s;
    }();
    return sw;
}

__device__ __forceinline__ int32_t lo16(uint32_t w) { return int32_t(int16_t(w)); }
__device__ __forceinline__ int32_t hi16(uint32_t w) { return int32_t(w) >> 16; }
typedef short short2v __attribute__((ext_vector_type(2)));
// a.lo * b.lo + a.hi * b.hi + c, the halves as i16, the sum in wrapping i32: v_dot2_i32_i16
__device__ __forceinline__ uint32_t dot2(uint32_t a, uint32_t b, uint32_t c)
{
    return uint32_t(__builtin_amdgcn_sdot2(__builtin_bit_cast(short2v, a), __builtin_bit_cast(short2v, b), int32_t(c), false));
}
// (lo & 0xFFFF) | hi << 16 — and, HI, (lo >> 16) | hi << 16: one v_perm_b32 (selector bytes 0..3 index `lo`, 4..7 index `hi`)
template <bool HI = false>
__device__ __forceinline__ uint32_t pack16(uint32_t lo, uint32_t hi)
{
    return __builtin_amdgcn_perm(hi, lo, HI ? 0x05040302u : 0x05040100u);
}

// N serial sections of one lane (`[C] x [S]`, dsp-process/src/compose.rs:43-77: sample-major here, the same values as the
// reference's stage-major slice composition because every section is a causal function of its own input)
template <int N, bool CLAMP>
struct Core {
    uint32_t xs[N], ys[N];  // x[0] | x[1] << 16, y[0] | y[1] << 16

    __device__ __forceinline__ void load(const uint32_t *st, size_t lanes, size_t lane)
    {
#pragma unroll
        for (int k = 0; k < N; k++) {
            xs[k] = pack16(st[size_t(k * 4 + 0) * lanes + lane], st[size_t(k * 4 + 1) * lanes + lane]);
            ys[k] = pack16(st[size_t(k * 4 + 2) * lanes + lane], st[size_t(k * 4 + 3) * lanes + lane]);
        }
    }
    __device__ __forceinline__ void store(uint32_t *st, size_t lanes, size_t lane) const
    {
#pragma unroll
        for (int k = 0; k < N; k++) {
            st[size_t(k * 4 + 0) * lanes + lane] = uint32_t(lo16(xs[k]));
            st[size_t(k * 4 + 1) * lanes + lane] = uint32_t(hi16(xs[k]));
            st[size_t(k * 4 + 2) * lanes + lane] = uint32_t(lo16(ys[k]));
            st[size_t(k * 4 + 3) * lanes + lane] = uint32_t(hi16(ys[k]));
        }
    }
    // v holds x0 in its low half, or, HI, in its high half (the other half is anything); the i16 result is the low half of the
    // word returned
    template <bool HI>
    __device__ __forceinline__ uint32_t step(const Params<N> &p, uint32_t v)
    {
#pragma unroll
        for (int k = 0; k < N; k++) {
            const Sec &c = p.sec[k];
            const bool hi = HI && k == 0;  // later sections take the low half of the y0 word
            // biquad.rs:373-378
            uint32_t acc = dot2(hi ? c.b0hi : c.b0lo, v, 0u);
            acc = dot2(c.b12, xs[k], acc);
            acc = dot2(c.a12, ys[k], acc);
            uint32_t y0 = uint32_t(int32_t(acc) >> c.frac);  // its low half is `as i16`
            if (CLAMP) {  // biquad.rs:400
                const int32_t t = lo16(y0 + uint32_t(c.u));
                y0 = uint32_t(t < c.mn ? c.mn : (t > c.mx ? c.mx : t));
            }
            xs[k] = hi ? pack16<true>(v, xs[k]) : pack16<false>(v, xs[k]);  // :379
            ys[k] = pack16(y0, ys[k]);                                      // :380, :401
            v = y0;
        }
        return v;
    }
};

// ---------------------------------------------------------------- FRAME_MAJOR
// One lane per thread, one 16-bit element per frame, any alignment: a wave moves 128 contiguous bytes per frame, on the rotating
// register window (subword::window_walk, which is also what makes y == x safe).  xl / yl: elements between consecutive frames.
// (A second form was built beside this one and measured: a thread owned the adjacent lanes 2 t and 2 t + 1 and moved one dword per
// frame, 256 B per wave, on half as many waves.  It was never faster — 65536 lanes x 4096 frames 0.207 ms against 0.199-0.208, 16384
// lanes 0.203 against 0.158 — and was taken out.  Loads and stores share the one 6-bit vmcnt counter, so a wave has at most 63 of them
// in flight whatever their width, and lanes x 2 bytes x 63 are in flight per frame row either way; the form with more waves issues
// them sooner.  profiles/NOTES.md, "Biquad i16".)
template <int N, bool CLAMP, int U>
__global__ __launch_bounds__(256) void biquad_i16_frame_major(const Params<N> prm, uint32_t *st, const int16_t *x, int16_t *y, const size_t lanes,
                                                              const size_t frames, const size_t xl, const size_t yl)
{
    const size_t lane = size_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (lane >= lanes) return;

    Core<N, CLAMP> p;
    p.load(st, lanes, lane);
    const uint32_t voff = uint32_t(lane) * 2u;  // the thread's bytes into a row (lanes <= 2^31); the row base is wave-uniform: SGPRs

    subword::window_walk<U>(
        frames, [&](size_t f) -> uint32_t { return global_ld<uint16_t, true>(x + f * xl, voff); },
        [&](uint32_t v, size_t f) { global_st<uint16_t, true>(y + f * yl, voff, uint16_t(p.template step<false>(prm, v))); });
    p.store(st, lanes, lane);
}

// ----------------------------------------------------------------- LANE_MAJOR
// A wave (one per workgroup) moves 64-lane x 128-sample tiles through one padded LDS tile of 64 x 64 dwords on the front end of
// subword_rows.h (WaveRows, fetch_dwords, deposit): a load instruction takes 64 consecutive dwords (128 samples) of ONE lane, the next
// tile's 64 loads are in flight during the arithmetic, the owning thread walks its row conflict-free and leaves the two outputs of a
// dword where the two inputs were, and a store instruction writes 64 dwords of one lane.
// `grid4` (x, y on the 4-byte grid and xl, yl even): whole tiles move as dwords.  Otherwise, and in the last, partial tile of a
// lane, every dword is put together from / taken apart into two 16-bit accesses, each predicated on its own sample: nothing outside
// the `frames` elements of a lane is read or written.  (With `grid4` the partial tile still moves dwords wherever both samples exist.)
// xl / yl: elements between the starts of consecutive lanes.  In place (y == x, yl == xl) a wave has read tile t + 1 of its lanes
// before it writes tile t, and the two do not overlap.
template <int N, bool CLAMP>
__global__ __launch_bounds__(kWave) void biquad_i16_lane_major(const Params<N> prm, uint32_t *st, const int16_t *x, int16_t *y, const size_t lanes,
                                                               const size_t frames, const size_t xl, const size_t yl, const int grid4)
{
    constexpr int TW = kLmTW, TS = kLmTS;
    static_assert(TW == kWave, "a load instruction covers one row of the tile");
    __shared__ uint32_t tile[kWave][TW + 1];

    const subword::WaveRows w(lanes);
    const int lid = w.lid;
    const size_t lane0 = w.lane0, lane = w.lane, nrows = w.nrows;
    const bool active = w.active;

    Core<N, CLAMP> p;
    if (active) p.load(st, lanes, lane);

    uint32_t stage[kWave];
    auto fetch = [&](size_t t0) {
        const size_t ns = frames - t0 < size_t(TS) ? frames - t0 : size_t(TS);
        if (grid4 && ns == size_t(TS)) {
            subword::fetch_dwords(stage, w, x, xl, t0, true);  // a whole tile: no column predicate
        } else {  // this family's own: rows off the 4-byte grid and the partial tile, a dword from two 16-bit loads
            const bool h0 = size_t(2 * lid) < ns, h1 = size_t(2 * lid + 1) < ns;
#pragma unroll
            for (int r = 0; r < kWave; r++) {
                uint32_t w = 0;
                if (size_t(r) < nrows) {
                    const int16_t *row = x + (lane0 + r) * xl + t0;
                    if (grid4 && h1) {
                        w = global_ld<uint32_t, true>(row, uint32_t(lid) * 4u);
                    } else {
                        if (h0) w = global_ld<uint16_t, true>(row, uint32_t(lid) * 4u);
                        if (h1) w |= uint32_t(global_ld<uint16_t, true>(row, uint32_t(lid) * 4u + 2u)) << 16;
                    }
                }
                stage[r] = w;
            }
        }
    };

    fetch(0);
    for (size_t t0 = 0; t0 < frames; t0 += TS) {
        const size_t ns = frames - t0 < size_t(TS) ? frames - t0 : size_t(TS);
        subword::deposit(tile, stage, lid);
        lds_wave_sync();
        if (t0 + TS < frames) fetch(t0 + TS);

        if (active) {
            if (ns == size_t(TS)) {
#pragma unroll 8
                for (int j = 0; j < TW; j++) {
                    const uint32_t w = tile[lid][j];
                    const uint32_t y0 = p.template step<false>(prm, w);
                    const uint32_t y1 = p.template step<true>(prm, w);
                    tile[lid][j] = pack16(y0, y1);
                }
            } else {
                for (size_t j = 0; 2 * j < ns; j++) {
                    const uint32_t w = tile[lid][j];
                    const uint32_t y0 = p.template step<false>(prm, w);
                    const uint32_t y1 = 2 * j + 1 < ns ? p.template step<true>(prm, w) : 0u;
                    tile[lid][j] = pack16(y0, y1);
                }
            }
        }
        lds_wave_sync();
        if (grid4 && ns == size_t(TS)) {
#pragma unroll 8
            for (int r = 0; r < kWave; r++)
                if (size_t(r) < nrows) global_st<uint32_t, true>(y + (lane0 + r) * yl + t0, uint32_t(lid) * 4u, tile[r][lid]);
        } else {
            const bool h0 = size_t(2 * lid) < ns, h1 = size_t(2 * lid + 1) < ns;
            for (size_t r = 0; r < nrows; r++) {
                int16_t *row = y + (lane0 + r) * yl + t0;
                const uint32_t w = tile[r][lid];
                if (grid4 && h1) {
                    global_st<uint32_t, true>(row, uint32_t(lid) * 4u, w);
                } else {
                    if (h0) global_st<uint16_t, true>(row, uint32_t(lid) * 4u, uint16_t(w));
                    if (h1) global_st<uint16_t, true>(row, uint32_t(lid) * 4u + 2u, uint16_t(w >> 16));
                }
            }
        }
        lds_wave_sync();
    }
    if (active) p.store(st, lanes, lane);
}

// ------------------------------------------------------------------- BY LANE
// `ByLane<[C; N]>` (dsp-process/src/compose.rs:363-390): lane l runs configuration l on state l.  The same step and the same two
// walkers; only the section's home changes, from the kernel arguments (SGPRs) to the thread's registers.  `coef`: i16 planes, value v
// of section k of lane l at coef[(k * CV + v) * lanes + l], CV = 5 {b0, b1, b2, a1, a2} or, CLAMP, 8 {.., u, min, max}
// (include/idsp_hip.h).  A thread reads its own lane of every plane once, before the first frame: 16-bit loads, 128 contiguous bytes per
// wave and plane wherever the plane begins (an odd lane count puts every other plane off the 4-byte grid), and packs them into the
// words of `Sec`.  A thread WITHOUT a lane must not come here: the planes end with the last lane.
// b0 for the odd sample of a dword (`step<true>`) is a second register, b0 << 16, as in the shared kernels: a shift of the sample word
// instead would be one more VALU instruction in every odd step of the LaneMajor loop, the register costs N VGPRs where these kernels
// are far from any occupancy step (profiles/NOTES.md, "Biquad i16 by lane").  FrameMajor never takes the odd step: b0hi is dead there.
template <int N, bool CLAMP>
__device__ __forceinline__ void load_sections(Params<N> &prm, const int16_t *coef, size_t lanes, size_t lane, int frac)
{
    constexpr int CV = CLAMP ? 8 : 5;
    auto at = [&](int k, int v) { return uint32_t(uint16_t(coef[size_t(k * CV + v) * lanes + lane])); };
#pragma unroll
    for (int k = 0; k < N; k++) {
        Sec &d = prm.sec[k];
        d.b0lo = at(k, 0), d.b0hi = d.b0lo << 16;
        d.b12 = pack16(at(k, 1), at(k, 2));
        d.a12 = pack16(at(k, 3), at(k, 4));
        d.frac = frac;  // one F for the bank: wave-uniform, it stays in an SGPR
        d.u = d.mn = d.mx = 0;
        if (CLAMP) d.u = lo16(at(k, 5)), d.mn = lo16(at(k, 6)), d.mx = lo16(at(k, 7));
    }
}

template <int N, bool CLAMP, int U>
__global__ __launch_bounds__(256) void biquad_i16_bylane_frame_major(const int16_t *coef, const int frac, uint32_t *st, const int16_t *x, int16_t *y,
                                                                     const size_t lanes, const size_t frames, const size_t xl, const size_t yl)
{
    const size_t lane = size_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (lane >= lanes) return;  // before any plane is read

    Params<N> prm;
    load_sections<N, CLAMP>(prm, coef, lanes, lane, frac);
    Core<N, CLAMP> p;
    p.load(st, lanes, lane);
    const uint32_t voff = uint32_t(lane) * 2u;

    subword::window_walk<U>(
        frames, [&](size_t f) -> uint32_t { return global_ld<uint16_t, true>(x + f * xl, voff); },
        [&](uint32_t v, size_t f) { global_st<uint16_t, true>(y + f * yl, voff, uint16_t(p.template step<false>(prm, v))); });
    p.store(st, lanes, lane);
}

// biquad_i16_lane_major with the sections in registers.  The body is that kernel's, line for line, and is spelled out a second time on
// purpose: the shared-coefficient kernel is what this one is measured against (profiles/NOTES.md, "Biquad i16 by lane"), and routing
// both through one inlined body was tried and changed ITS code — other register allocation, other s_waitcnt placement, 30-80
// instructions fewer of about 8000 —, which would have needed a measurement of its own against the kernel as it stood.
template <int N, bool CLAMP>
__global__ __launch_bounds__(kWave) void biquad_i16_bylane_lane_major(const int16_t *coef, const int frac, uint32_t *st, const int16_t *x, int16_t *y,
                                                                      const size_t lanes, const size_t frames, const size_t xl, const size_t yl,
                                                                      const int grid4)
{
    constexpr int TW = kLmTW, TS = kLmTS;
    static_assert(TW == kWave, "a load instruction covers one row of the tile");
    __shared__ uint32_t tile[kWave][TW + 1];

    const subword::WaveRows w(lanes);
    const int lid = w.lid;
    const size_t lane0 = w.lane0, lane = w.lane, nrows = w.nrows;
    const bool active = w.active;

    Params<N> prm = {};  // a thread of the ragged last wave has no lane: it moves rows and never steps
    Core<N, CLAMP> p;
    if (active) {  // the predicate of the state load: nothing is read past the last lane of a plane
        load_sections<N, CLAMP>(prm, coef, lanes, lane, frac);
        p.load(st, lanes, lane);
    }

    uint32_t stage[kWave];
    auto fetch = [&](size_t t0) {
        const size_t ns = frames - t0 < size_t(TS) ? frames - t0 : size_t(TS);
        if (grid4 && ns == size_t(TS)) {
            subword::fetch_dwords(stage, w, x, xl, t0, true);  // a whole tile: no column predicate
        } else {  // this family's own: rows off the 4-byte grid and the partial tile, a dword from two 16-bit loads
            const bool h0 = size_t(2 * lid) < ns, h1 = size_t(2 * lid + 1) < ns;
#pragma unroll
            for (int r = 0; r < kWave; r++) {
                uint32_t w = 0;
                if (size_t(r) < nrows) {
                    const int16_t *row = x + (lane0 + r) * xl + t0;
                    if (grid4 && h1) {
                        w = global_ld<uint32_t, true>(row, uint32_t(lid) * 4u);
                    } else {
                        if (h0) w = global_ld<uint16_t, true>(row, uint32_t(lid) * 4u);
                        if (h1) w |= uint32_t(global_ld<uint16_t, true>(row, uint32_t(lid) * 4u + 2u)) << 16;
                    }
                }
                stage[r] = w;
            }
        }
    };

    fetch(0);
    for (size_t t0 = 0; t0 < frames; t0 += TS) {
        const size_t ns = frames - t0 < size_t(TS) ? frames - t0 : size_t(TS);
        subword::deposit(tile, stage, lid);
        lds_wave_sync();
        if (t0 + TS < frames) fetch(t0 + TS);

        if (active) {
            if (ns == size_t(TS)) {
#pragma unroll 8
                for (int j = 0; j < TW; j++) {
                    const uint32_t w = tile[lid][j];
                    const uint32_t y0 = p.template step<false>(prm, w);
                    const uint32_t y1 = p.template step<true>(prm, w);
                    tile[lid][j] = pack16(y0, y1);
                }
            } else {
                for (size_t j = 0; 2 * j < ns; j++) {
                    const uint32_t w = tile[lid][j];
                    const uint32_t y0 = p.template step<false>(prm, w);
                    const uint32_t y1 = 2 * j + 1 < ns ? p.template step<true>(prm, w) : 0u;
                    tile[lid][j] = pack16(y0, y1);
                }
            }
        }
        lds_wave_sync();
        if (grid4 && ns == size_t(TS)) {
#pragma unroll 8
            for (int r = 0; r < kWave; r++)
                if (size_t(r) < nrows) global_st<uint32_t, true>(y + (lane0 + r) * yl + t0, uint32_t(lid) * 4u, tile[r][lid]);
        } else {
            const bool h0 = size_t(2 * lid) < ns, h1 = size_t(2 * lid + 1) < ns;
            for (size_t r = 0; r < nrows; r++) {
                int16_t *row = y + (lane0 + r) * yl + t0;
                const uint32_t w = tile[r][lid];
                if (grid4 && h1) {
                    global_st<uint32_t, true>(row, uint32_t(lid) * 4u, w);
                } else {
                    if (h0) global_st<uint16_t, true>(row, uint32_t(lid) * 4u, uint16_t(w));
                    if (h1) global_st<uint16_t, true>(row, uint32_t(lid) * 4u + 2u, uint16_t(w >> 16));
                }
            }
        }
        lds_wave_sync();
    }
    if (active) p.store(st, lanes, lane);
}


}  // namespace bq16
}  // namespace idsp
