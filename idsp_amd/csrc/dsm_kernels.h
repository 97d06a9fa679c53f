// dsm_kernels.h — the MASH-(1)^K delta-sigma modulator of the reference (`Dsm<K>`, src/dsm.rs:44-57) per lane: u32 samples in,
// one i8 per sample out.  The first kernels of the library whose output element is smaller than a 32-bit word (lane_stream.h asserts
// "samples are one or two 32-bit words" in every kernel), so they move their own bytes, on the walkers of subword_rows.h; the arithmetic
// is a few dozen full-rate VALU operations per sample against 5 bytes, and how the bytes leave is what the two kernels are about.
//
// Semantics, as a RELEASE build of the reference computes them (every u32 and i8 operation wraps):
//   * stage fold (:47-51): a[i], carry[i] = a[i].overflowing_add(v), v = x for stage 0 and the new a[i - 1] after it;
//   * recombination fold (:52-56): y = carry[K - 1]; for j = 0 .. K - 2: (y, c[j]) = (carry[K - 2 - j] + y - c[j], y) in wrapping
//     i8.  From `Dsm::default()` no i8 operation overflows and y stays inside 1 - 2^(K-1) ..= 2^(K-1); from arbitrary c words the
//     fold overflows i8 already at K = 3, where a debug build of the reference panics.  Here the values wrap, like `-i32::MIN` in
//     cordic.hip.  The fold is additions and subtractions only, so it runs on 32-bit registers and the low byte is taken where a
//     value leaves the lane (the output byte, the state word): the low byte of a wrapping 32-bit sum IS the wrapping 8-bit sum;
//   * c[K - 1] is part of the struct and never read or written (`take(K - 1)`): state word 2K - 1 is not touched;
//   * K = 1: the output is the carry.  K = 0: the output is the constant 0 and there is no state (`take(usize::MAX)` over an empty
//     array in a release build; the doc comment of the struct promises it).
// State (include/idsp_hip.h): word-plane-major, words 0..K-1 = a, words K..2K-1 = c; a c word is read as its low byte and written
// back sign-extended.
#pragma once

#include "subword_rows.h"

namespace idsp {
namespace dsm {

using subword::kFmU;  // depth of the rotating register window: measured on these kernels (subword_rows.h)
using subword::kWave;
constexpr int kFmBlock = 256;  // four waves, 256 lanes of a row: 1 KiB in, 256 bytes out per frame
constexpr int kLmTS = 64;  // samples per lane and input tile: 256-byte runs in
// Input tiles per output tile: outputs leave as runs of 64 kLmOT bytes per lane.  Measured with 1 / 2 / 4 at 65536 lanes x 4096 frames:
// K = 1 0.419 / 0.350 / 0.377 ms, K = 3 0.429 / 0.409 / 0.398, K = 8 0.520 / 0.503 / 0.506; at 16384 lanes the three are within 1 %
// except K = 1 with 4 (+ 12 %).  2: whole 128-byte lines where a lane's row starts on one.
constexpr int kLmOT = 2;

typedef __attribute__((address_space(1))) const uint32_t *gu32c;
typedef __attribute__((address_space(1))) uint32_t *gu32;
typedef __attribute__((address_space(1))) int8_t *gi8;

// streamed-once data, GLOBAL address space named (no flat_* accesses)
__device__ __forceinline__ uint32_t ld_word(const uint32_t *p)
{
    return __builtin_nontemporal_load(reinterpret_cast<gu32c>(reinterpret_cast<uintptr_t>(p)));
}
__device__ __forceinline__ void st_word(int8_t *p, uint32_t v)  // p is 4-byte aligned
{
    __builtin_nontemporal_store(v, reinterpret_cast<gu32>(reinterpret_cast<uintptr_t>(p)));
}
__device__ __forceinline__ void st_byte(int8_t *p, uint32_t v)
{
    __builtin_nontemporal_store(int8_t(v), reinterpret_cast<gi8>(reinterpret_cast<uintptr_t>(p)));
}

template <int K>
struct Core {
    uint32_t a[K > 0 ? K : 1];
    uint32_t c[K > 1 ? K - 1 : 1];  // i8 values, kept as wrapping 32-bit words (header)

    __device__ __forceinline__ void load(const uint32_t *st, size_t lanes, size_t lane)
    {
#pragma unroll
        for (int i = 0; i < K; i++) a[i] = st[size_t(i) * lanes + lane];
#pragma unroll
        for (int j = 0; j + 1 < K; j++) c[j] = uint32_t(int32_t(int8_t(st[size_t(K + j) * lanes + lane])));
    }
    __device__ __forceinline__ void store(uint32_t *st, size_t lanes, size_t lane) const
    {
#pragma unroll
        for (int i = 0; i < K; i++) st[size_t(i) * lanes + lane] = a[i];
#pragma unroll
        for (int j = 0; j + 1 < K; j++) st[size_t(K + j) * lanes + lane] = uint32_t(int32_t(int8_t(c[j])));
    }
    // `process` (:44-57); the i8 result is the low byte of the word returned
    __device__ __forceinline__ uint32_t step(uint32_t x)
    {
        if constexpr (K == 0) {
            return 0u;
        } else {
            uint32_t carry[K];
            uint32_t v = x;
#pragma unroll
            for (int i = 0; i < K; i++) {
                const uint32_t s = a[i] + v;  // `overflowing_add` (:48)
                carry[i] = s < v ? 1u : 0u;
                a[i] = s, v = s;
            }
            uint32_t y = carry[K - 1];  // `d & 1` (:52)
#pragma unroll
            for (int j = 0; j + 1 < K; j++) {
                const uint32_t n = carry[K - 2 - j] + y - c[j];  // (:54)
                c[j] = y, y = n;
            }
            return y;
        }
    }
};

// ---------------------------------------------------------------- FRAME_MAJOR
// One lane per thread on a rotating register window (frame f + U is requested right before frame f is consumed): one word load and one
// byte store per thread and frame, so a wave writes 64 contiguous bytes, whatever the alignment of y.  xl / yl: elements between
// consecutive frames of x / y.
// (A second store form was built beside this one and measured: a thread kept the bytes of four frames, the four threads of a quad
// transposed their 4 x 4 bytes with two quad_perm DPP moves and each stored one dword.  It took 1.10 to 1.23 times this form's time
// at 65536 and 16384 lanes x 4096 frames, K = 1, 3, 8 — profiles/NOTES.md, "Dsm" — and was taken out.)
template <int K, int U>
__global__ __launch_bounds__(kFmBlock) void dsm_frame_major(uint32_t *st, const uint32_t *x, int8_t *y, const size_t lanes, const size_t frames,
                                                            const size_t xl, const size_t yl)
{
    const size_t lane = size_t(blockIdx.x) * kFmBlock + threadIdx.x;
    if (lane >= lanes) return;

    Core<K> p;
    p.load(st, lanes, lane);
    const uint32_t *xp = x + lane;
    int8_t *yp = y + lane;

    // The window of subword::window_walk, written out: on the shared walker this kernel measured slower at 65536 lanes x 4096 frames in
    // both runs of an A/B against this form (K = 1 + 2.6 %, K = 3 and 8 + 0.3 %; profiles/NOTES.md, "Sub-word rows").
    uint32_t ring[U];
#pragma unroll
    for (int u = 0; u < U; u++)
        if (size_t(u) < frames) ring[u] = ld_word(xp + size_t(u) * xl);
    size_t f = 0;
    for (; f + 2 * U <= frames; f += U) {
        const uint32_t *xn = xp + (f + U) * xl;
        int8_t *yn = yp + f * yl;
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint32_t v = ring[u];
            ring[u] = ld_word(xn + size_t(u) * xl);
            st_byte(yn + size_t(u) * yl, p.step(v));
        }
    }
    // drain: fewer than 2 U frames left, predicates are wave-uniform
#pragma unroll
    for (int u = 0; u < U; u++) {
        const size_t fr = f + u;
        if (fr < frames) {
            const uint32_t v = ring[u];
            if (fr + U < frames) ring[u] = ld_word(xp + (fr + U) * xl);
            st_byte(yp + fr * yl, p.step(v));
        }
    }
    f += U;
#pragma unroll
    for (int u = 0; u < U; u++) {
        const size_t fr = f + u;
        if (fr < frames) st_byte(yp + fr * yl, p.step(ring[u]));
    }
    p.store(st, lanes, lane);
}

// ----------------------------------------------------------------- LANE_MAJOR
// A wave (one per workgroup) moves 64-lane x 64-sample tiles through a padded LDS tile on the front end of subword_rows.h (WaveRows,
// fetch_dwords, deposit): a load instruction takes 64 consecutive words of ONE lane (the next tile's 64 loads are in flight during the
// arithmetic), the owning thread walks its row conflict-free, packs four output bytes to a word and leaves 16 words per lane and
// input tile in the output tile.  The second, output tile is this family's own: it collects OT input tiles, so outputs leave as runs
// of 64 OT bytes per lane: as
// dwords where the runs are 4-byte aligned (`aligned`: y and yl multiples of 4; a run starts at a multiple of 64 samples), byte by
// byte otherwise (unaligned rows) and for the last frames % 4 bytes of a lane.
// xl / yl: elements between the starts of consecutive lanes of x / y.
template <int K, int OT>
__global__ __launch_bounds__(kWave) void dsm_lane_major(uint32_t *st, const uint32_t *x, int8_t *y, const size_t lanes, const size_t frames, const size_t xl,
                                                        const size_t yl, const int aligned)
{
    constexpr int TS = kLmTS, OW = TS / 4, OWR = OT * OW;  // output words per input tile / per output tile row
    static_assert(OWR <= kWave && kWave % OWR == 0, "a store instruction covers whole output rows");
    constexpr int RPS = kWave / OWR;  // rows per dword store instruction
    __shared__ uint32_t tin[kWave][TS + 1];
    __shared__ uint32_t tout[kWave][OWR + 1];

    const subword::WaveRows w(lanes);
    const int lid = w.lid;
    const size_t lane0 = w.lane0, lane = w.lane, nrows = w.nrows;
    const bool active = w.active;

    Core<K> p;
    if (active) p.load(st, lanes, lane);

    uint32_t stage[kWave];
    auto fetch = [&](size_t t0) {
        const size_t nw = frames - t0 < size_t(TS) ? frames - t0 : size_t(TS);
        subword::fetch_dwords(stage, w, x, xl, t0, size_t(lid) < nw);
    };

    fetch(0);
    size_t tile = 0;
    for (size_t t0 = 0; t0 < frames; t0 += TS, tile++) {
        const size_t ncols = frames - t0 < size_t(TS) ? frames - t0 : size_t(TS);
        const int part = int(tile % OT);  // which part of the output tile this input tile fills
        subword::deposit(tin, stage, lid);
        lds_wave_sync();
        if (t0 + TS < frames) fetch(t0 + TS);

        if (active) {
            if (ncols == size_t(TS)) {
#pragma unroll
                for (int j0 = 0; j0 < TS; j0 += 4) {
                    uint32_t w = 0;
#pragma unroll
                    for (int b = 0; b < 4; b++) w |= (p.step(tin[lid][j0 + b]) & 0xFFu) << (8 * b);
                    tout[lid][part * OW + j0 / 4] = w;
                }
            } else {
                for (size_t j0 = 0; j0 < ncols; j0 += 4) {
                    uint32_t w = 0;
                    for (int b = 0; b < 4; b++)
                        if (j0 + b < ncols) w |= (p.step(tin[lid][j0 + b]) & 0xFFu) << (8 * b);
                    tout[lid][part * OW + j0 / 4] = w;
                }
            }
        }
        lds_wave_sync();
        if (part == OT - 1 || t0 + TS >= frames) {
            // the output tile leaves: nb bytes per lane from sample tb on
            const size_t tb = t0 - size_t(part) * TS, nb = t0 + ncols - tb;
            size_t done = 0;  // bytes per lane stored as dwords
            if (aligned) {
                const size_t nd = nb / 4;
                done = nd * 4;
                // thread t of instruction i: word t % OWR of row RPS i + t / OWR
#pragma unroll
                for (int i = 0; i < kWave / RPS; i++) {
                    const size_t r = size_t(RPS * i + lid / OWR);
                    if (r < nrows && size_t(lid % OWR) < nd) st_word(y + (lane0 + r) * yl + tb + 4 * (lid % OWR), tout[r][lid % OWR]);
                }
            }
            if (done < nb) {
                for (size_t r = 0; r < nrows; r++)
                    for (size_t b = done + lid; b < nb; b += kWave)
                        global_st<int8_t, true>(y + (lane0 + r) * yl + tb, uint32_t(b), int8_t(tout[r][b / 4] >> (8 * (b % 4))));
            }
            lds_wave_sync();
        }
    }
    if (active) p.store(st, lanes, lane);
}

}  // namespace dsm
}  // namespace idsp
