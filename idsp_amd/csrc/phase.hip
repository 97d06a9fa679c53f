// phase.hip — the phase consumers of the reference on the stream kernels (phase_procs.h): `PLL` (src/pll.rs:33-107),
// `Unwrapper<i64>` and `ClampWrap<W<i32>>` (src/unwrap.rs:107-194), plus the PLL coefficient builders (src/pll.rs:42-57, host code).
// All integer and bit-exact; both layouts, any lane count and in-place calls come from launch_stream (lane_stream.h).
#include <cmath>

#include "phase_procs.h"

namespace idsp {
namespace {

// `Q32::<32>::from_f32` (dsp-fixedpoint/src/num_traits_impl.rs:39-45): `(v * 2^32).round() as i32` — the product and `round()`
// (half away from zero) in f32, the cast saturating with NaN -> 0.
int32_t q32_from_f32(float v)
{
    const float r = roundf(v * 4294967296.0f);
    if (r != r) return 0;
    if (r >= 2147483648.0f) return INT32_MAX;
    if (r <= -2147483648.0f) return INT32_MIN;
    return int32_t(r);
}

// src/pll.rs:42-46
void pll_from_zpk_f32(float zero, float pole, float gain, int32_t ba[3])
{
    ba[0] = q32_from_f32(gain);
    ba[1] = q32_from_f32(-gain * zero);
    ba[2] = q32_from_f32(-(1.0f - pole));
}

int check_phase_args(const void *state, const void *x, const void *y, size_t lanes, size_t frames, int layout)
{
    if (int rc = check_stream_args(nullptr, 0, state, x, y, lanes, frames, layout)) return rc;
    if (!state || !x || !y) return fail(IDSP_EINVAL, "state, x or y is NULL");
    return IDSP_OK;
}

// the two-word output forms (i64 phase, {phase, frequency} pairs) store whole elements: y on the 8-byte grid
int check_pair_out(const void *y)
{
    if (reinterpret_cast<uintptr_t>(y) % 8) return fail(IDSP_EINVAL, "y holds 8-byte elements: it must be 8-byte aligned");
    return IDSP_OK;
}

}  // namespace
}  // namespace idsp

using namespace idsp;

extern "C" {

size_t idsp_pll_state_words(void) { return IDSP_PLL_STATE_WORDS; }

int idsp_pll_from_zpk(double zero, double pole, double gain, int32_t ba[3])
{
    if (!ba) return fail(IDSP_EINVAL, "ba is NULL");
    pll_from_zpk_f32(float(zero), float(pole), float(gain), ba);
    return IDSP_OK;
}

int idsp_pll_from_bandwidth(double bw_, double split_, int32_t ba[3])
{
    if (!ba) return fail(IDSP_EINVAL, "ba is NULL");
    const float bw = float(bw_), split = float(split_);
    // src/pll.rs:51-57, f32 throughout, the reference's order of operations
    const float a = bw * 2.0f * 3.14159265358979323846f;
    const float z = 1.0f - a / split;
    const float p = 1.0f - a * split;
    const float k = -a * a * split;
    pll_from_zpk_f32(z, p, k, ba);
    return IDSP_OK;
}

int idsp_pll_i32(const int32_t ba[3], void *state, const int32_t *x, int32_t *y, size_t lanes, size_t frames, int layout, int output,
                 void *stream)
{
    if (!ba) return fail(IDSP_EINVAL, "ba is NULL");
    if (output != IDSP_PLL_PHASE && output != IDSP_PLL_FREQUENCY && output != IDSP_PLL_BOTH)
        return fail(IDSP_EINVAL, "output %d is none of IDSP_PLL_PHASE, IDSP_PLL_FREQUENCY, IDSP_PLL_BOTH", output);
    if (int rc = check_phase_args(state, x, y, lanes, frames, layout)) return rc;
    if (output == IDSP_PLL_BOTH)
        if (int rc = check_pair_out(y)) return rc;
    if (lanes == 0 || frames == 0) return IDSP_OK;
    const PllParams p{{ba[0], ba[1], ba[2]}};
    if (output == IDSP_PLL_PHASE) return launch_stream<PllProc<0>>(p, state, x, y, lanes, frames, layout, as_stream(stream));
    if (output == IDSP_PLL_FREQUENCY) return launch_stream<PllProc<1>>(p, state, x, y, lanes, frames, layout, as_stream(stream));
    return launch_stream<PllProc<2>>(p, state, x, reinterpret_cast<PhaseFreq *>(y), lanes, frames, layout, as_stream(stream));
}

int idsp_unwrap_i32(void *state, const int32_t *x, int32_t *dx, size_t lanes, size_t frames, int layout, void *stream)
{
    if (int rc = check_phase_args(state, x, dx, lanes, frames, layout)) return rc;
    if (lanes == 0 || frames == 0) return IDSP_OK;
    return launch_stream<UnwrapProc<0>>(NoParams{0}, state, x, dx, lanes, frames, layout, as_stream(stream));
}

int idsp_unwrap_i32_phase(void *state, const int32_t *x, int64_t *y, size_t lanes, size_t frames, int layout, void *stream)
{
    if (int rc = check_phase_args(state, x, y, lanes, frames, layout)) return rc;
    if (int rc = check_pair_out(y)) return rc;
    if (lanes == 0 || frames == 0) return IDSP_OK;
    return launch_stream<UnwrapProc<1>>(NoParams{0}, state, x, y, lanes, frames, layout, as_stream(stream));
}

int idsp_clamp_wrap_i32(void *state, const int32_t *x, int32_t *y, size_t lanes, size_t frames, int layout, void *stream)
{
    if (int rc = check_phase_args(state, x, y, lanes, frames, layout)) return rc;
    if (lanes == 0 || frames == 0) return IDSP_OK;
    return launch_stream<ClampWrapProc>(NoParams{0}, state, x, y, lanes, frames, layout, as_stream(stream));
}

}  // extern "C"
