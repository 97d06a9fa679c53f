// sweep.hip — the exponential swept sine of the reference (src/sweptsine.rs): the generator `AccuOsc<Sweep>` on the stream kernels
// (sweep_procs.h; both layouts and any lane count come from launch_stream, lane_stream.h) and `Sweep`'s host functions — `fit`
// (:108-118), the descriptors (:43-81) and `inverse_filter` (:93-101) — with the reference's types and order of operations.
#include <cmath>

#include "sweep_procs.h"

namespace idsp {
namespace {

constexpr float kQf = 4294967296.0f;   // `const Q: f32 = (1i64 << 32) as f32` (:8)
constexpr double kQd = 4294967296.0;   // `Q as f64`

// Rust's float -> integer `as`: truncating, saturating, NaN -> 0
int32_t f32_as_i32(float v)
{
    if (v != v) return 0;
    if (v >= 2147483648.0f) return INT32_MAX;
    if (v <= -2147483648.0f) return INT32_MIN;
    return int32_t(v);
}
int64_t f32_as_i64(float v)
{
    if (v != v) return 0;
    if (v >= 9223372036854775808.0f) return INT64_MAX;
    if (v <= -9223372036854775808.0f) return INT64_MIN;
    return int64_t(v);
}

double sweep_rate(int32_t rate) { return log1p(double(rate) / kQd); }                             // :43-45
double sweep_cycles(int32_t rate, int64_t state) { return double(state) / (kQd * double(rate)); }  // :73-75

}  // namespace
}  // namespace idsp

using namespace idsp;

extern "C" {

size_t idsp_sweep_state_words(void) { return IDSP_SWEEP_STATE_WORDS; }

int idsp_sweep_i32(void *state, int32_t *out, size_t lanes, size_t frames, int layout, void *stream)
{
    if (layout != IDSP_FRAME_MAJOR && layout != IDSP_LANE_MAJOR) return fail(IDSP_EINVAL, "bad layout %d", layout);
    if (lanes && (!state || (frames && !out))) return fail(IDSP_EINVAL, "state or out is NULL");
    if (reinterpret_cast<uintptr_t>(out) % 8) return fail(IDSP_EINVAL, "out holds 8-byte [re, im] pairs: it must be 8-byte aligned");
    if (lanes == 0 || frames == 0) return IDSP_OK;
    return launch_stream<SweepProc>(SweepParams{0}, state, static_cast<const int32_t *>(nullptr), reinterpret_cast<Cplx *>(out), lanes, frames,
                                    layout, as_stream(stream));
}

int idsp_sweep_fit(double stop_, double harmonics_, double cycles_, int32_t *rate, int64_t *state)
{
    const float stop = float(stop_), harmonics = float(harmonics_), cycles = float(cycles_);
    if (!rate || !state) return fail(IDSP_EINVAL, "rate or state is NULL");
    if (!(stop >= 0.0f && stop <= 0.5f)) return fail(IDSP_EINVAL, "Stop out of bounds");  // :109-111, NaN included
    const int32_t r = f32_as_i32(roundf(kQf * expm1f(stop / (cycles * harmonics))));        // :112
    // :113 `(rate as i64 * cycles as i64) << 32`: the product wrapping (release build), the shift dropping bits
    const int64_t s = int64_t((uint64_t(int64_t(r)) * uint64_t(f32_as_i64(cycles))) << 32);
    if (s <= 0) return fail(IDSP_EINVAL, "Start out of bounds");  // :114-116
    *rate = r, *state = s;
    return IDSP_OK;
}

double idsp_sweep_rate(int32_t rate) { return sweep_rate(rate); }
double idsp_sweep_delay(int32_t rate, double harmonic) { return log(harmonic) / sweep_rate(rate); }  // :49-51
double idsp_sweep_octave(int32_t rate) { return M_LN2 / sweep_rate(rate); }                         // :55-57
double idsp_sweep_decade(int32_t rate) { return M_LN10 / sweep_rate(rate); }                        // :61-63
double idsp_sweep_cycles(int32_t rate, int64_t state) { return sweep_cycles(rate, state); }
double idsp_sweep_state(int32_t rate, int64_t state) { return sweep_cycles(rate, state) * sweep_rate(rate); }  // :67-69
double idsp_sweep_continuous(int32_t rate, int64_t state, double t)                                            // :79-81
{
    return sweep_cycles(rate, state) * exp(sweep_rate(rate) * t);
}

int idsp_sweep_inverse_filter(int32_t rate, int64_t state, double f_, float out[2])
{
    float f = float(f_);
    if (!out) return fail(IDSP_EINVAL, "out is NULL");
    // :93-101, f32 throughout
    const float r = log1pf(float(rate) / kQf);
    f /= r;
    const float amp = 2.0f * r * sqrtf(f);
    const float inv_cycles = kQf * float(rate) / float(state);
    const float turns = 0.125f - f * (1.0f - logf(f * inv_cycles));
    const float a = 6.28318530717958647692f * turns;
    out[0] = amp * cosf(a), out[1] = amp * sinf(a);
    return IDSP_OK;
}

}  // extern "C"
