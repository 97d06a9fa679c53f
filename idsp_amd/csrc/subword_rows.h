// subword_rows.h — what the kernels whose elements are smaller than a 32-bit word share (dsm_kernels.h: u32 in, i8 out;
// biquad_i16_kernels.h: i16 in and out; lane_stream.h asserts one or two 32-bit words per sample, so they move their own bytes).  What
// a load, a step and a store ARE stays with each family; here, once: the FRAME_MAJOR rotating register window, the front end of a
// 64-lane LANE_MAJOR wave, and the host-side row checks of an entry that takes a pitch for x and one for y.
#pragma once

#include "common.h"

namespace idsp {
namespace subword {

constexpr int kWave = 64;
// Depth of the rotating register window (frames in flight per thread): at one wave per SIMD or fewer nothing but the window hides the
// latency of a row.  Measured on Dsm with 16 / 32 / 48 at 4096 frames (profiles/NOTES.md, "Dsm": 48 is never slower at 16384 lanes and
// at K = 8); with 48 the Dsm K = 8 kernel holds 151 VGPRs, three waves per SIMD; more than 196608 lanes have not been measured.
constexpr int kFmU = 48;

// ---------------------------------------------------------------- FRAME_MAJOR
// One lane per thread, the rotating register window of stream_frame_major (lane_stream.h): frame f + U is requested right before
// frame f is consumed.  `ld(f)`: the thread's element of frame f in a 32-bit register; `run(v, f)` steps the lane and stores frame f.
// In place (y == x with one pitch) is safe: run(., f) comes after ld(f) and every later ld reads a later frame — a thread only
// overwrites elements it has already consumed.
template <int U, class Ld, class Run>
__device__ __forceinline__ void window_walk(const size_t frames, Ld ld, Run run)
{
    uint32_t ring[U];
#pragma unroll
    for (int u = 0; u < U; u++)
        if (size_t(u) < frames) ring[u] = ld(size_t(u));
    size_t f = 0;
    for (; f + 2 * U <= frames; f += U) {
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint32_t v = ring[u];
            ring[u] = ld(f + U + u);
            run(v, f + u);
        }
    }
    // drain: fewer than 2 U frames left, predicates are wave-uniform
#pragma unroll
    for (int u = 0; u < U; u++) {
        const size_t fr = f + u;
        if (fr < frames) {
            const uint32_t v = ring[u];
            if (fr + U < frames) ring[u] = ld(fr + U);
            run(v, fr);
        }
    }
    f += U;
#pragma unroll
    for (int u = 0; u < U; u++) {
        const size_t fr = f + u;
        if (fr < frames) run(ring[u], fr);
    }
}

// ----------------------------------------------------------------- LANE_MAJOR
// Adjacent lanes are a pitch apart, so a wave (one per workgroup) moves 64-lane x 64-dword tiles through a padded LDS tile, as
// stream_lane_major does: a load instruction takes 64 consecutive dwords of ONE lane, the owning thread walks its row conflict-free.

// the 64 lanes of a single-wave workgroup
struct WaveRows {
    int lid;             // the thread: column of a load instruction, row of the arithmetic
    size_t lane0, lane;  // first lane of the wave, the thread's own
    bool active;         // the thread's lane exists
    size_t nrows;        // lanes of the wave that exist: 64 but in the last wave
    __device__ __forceinline__ explicit WaveRows(size_t lanes)
        : lid(int(threadIdx.x)), lane0(size_t(blockIdx.x) * kWave), lane(lane0 + lid), active(lane < lanes),
          nrows(lanes - lane0 < size_t(kWave) ? lanes - lane0 : size_t(kWave))
    {
    }
};

// stage[r] = dword `lid` of the tile row of lane lane0 + r, which starts 4-byte aligned at x + (lane0 + r) * xl + t0; 0 where the lane
// does not exist or `col` (the thread's dword lies inside the row; a literal `true` for a whole tile folds away) is false.  One
// instruction per row: wave-uniform row base in SGPRs + the thread's 32-bit offset, no 64-bit address per row in VGPRs.
template <class T>
__device__ __forceinline__ void fetch_dwords(uint32_t (&stage)[kWave], const WaveRows &w, const T *x, size_t xl, size_t t0, bool col)
{
#pragma unroll
    for (int r = 0; r < kWave; r++)
        stage[r] = (size_t(r) < w.nrows && col) ? global_ld<uint32_t, true>(x + (w.lane0 + r) * xl + t0, uint32_t(w.lid) * 4u) : 0u;
}

// the staged column of every row into the padded tile
template <int W>
__device__ __forceinline__ void deposit(uint32_t (&tile)[kWave][W], const uint32_t (&stage)[kWave], int lid)
{
    static_assert(W == kWave + 1, "a load instruction covers one row of the tile, and the rows are padded by one word");
#pragma unroll
    for (int r = 0; r < kWave; r++) tile[r][lid] = stage[r];
}

// ----------------------------------------------------------------------- host
// bytes from the first to one past the last element of `rows` rows of `row` elements, `pitch` elements apart; saturating
inline size_t extent_bytes(size_t rows, size_t row, size_t pitch, size_t elem)
{
    const size_t lead = span_bytes(rows - 1, pitch, elem), last = span_bytes(row, 1, elem);
    return lead > SIZE_MAX - last ? SIZE_MAX : lead + last;
}

// what y == x means to an entry: `never` (x and y differ in element size) any overlap is an error; `same_rows` y == x with one pitch is
// the in-place call (the reference's inplace()), any other overlap an error
enum class InPlace { never, same_rows };

struct PitchedRows {
    size_t row, rows;  // elements per row, rows: FRAME_MAJOR rows are frames of `lanes` elements, LANE_MAJOR rows lanes of `frames`
    size_t xl, yl;     // elements between row starts, a pitch of 0 replaced by the dense one
};

// The row checks of an entry with x_pitch / y_pitch, after its own argument checks, in this order: a pitch shorter than a row; the
// EMPTY call (lanes or frames 0) returns IDSP_OK here with nothing below checked and xl, yl unset — the caller returns IDSP_OK too;
// x and y aligned to their element sizes xe, ye; extents inside size_t; overlap by `rule`.
inline int pitched_rows(PitchedRows &r, int layout, size_t lanes, size_t frames, const void *x, size_t x_pitch, size_t xe, const void *y, size_t y_pitch,
                        size_t ye, InPlace rule)
{
    const bool lm = layout == IDSP_LANE_MAJOR;
    r.row = lm ? frames : lanes, r.rows = lm ? lanes : frames;
    if ((x_pitch && x_pitch < r.row) || (y_pitch && y_pitch < r.row))
        return fail(IDSP_EINVAL, "pitch (%zu, %zu) shorter than a row of %zu elements", x_pitch, y_pitch, r.row);
    if (lanes == 0 || frames == 0) return IDSP_OK;
    if (reinterpret_cast<uintptr_t>(x) % xe || reinterpret_cast<uintptr_t>(y) % ye)  // (a one-byte y is never off its grid: the text names x alone)
        return ye == 1 ? fail(IDSP_EINVAL, "x must be %zu-byte aligned", xe) : fail(IDSP_EINVAL, "x and y must be %zu-byte aligned", xe);
    r.xl = x_pitch ? x_pitch : r.row, r.yl = y_pitch ? y_pitch : r.row;
    const size_t xn = extent_bytes(r.rows, r.row, r.xl, xe), yn = extent_bytes(r.rows, r.row, r.yl, ye);
    if (xn == SIZE_MAX || yn == SIZE_MAX) return fail(IDSP_EINVAL, "rows * pitch out of range");
    if (rule == InPlace::never) {
        if (ranges_overlap(x, xn, y, yn)) return fail(IDSP_EINVAL, "x and y overlap (there is no in-place form: the elements differ in size)");
    } else if (x == y) {
        if (r.xl != r.yl) return fail(IDSP_EINVAL, "in-place call with different x and y pitches (%zu, %zu)", r.xl, r.yl);
    } else if (ranges_overlap(x, xn, y, yn)) {
        return fail(IDSP_EINVAL, "x and y overlap without being the same rows (in place is y == x with one pitch)");
    }
    return IDSP_OK;
}

}  // namespace subword
}  // namespace idsp
