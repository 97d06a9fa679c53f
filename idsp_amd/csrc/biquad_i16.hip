// biquad_i16.hip — `Biquad<Q16<F>>` / `BiquadClamp<Q16<F>, i16>` x `DirectForm1<i16>` (src/iir/biquad.rs:366-404): the host side of
// the shared-coefficient kernels of biquad_i16_kernels.h and the coefficient ingestion, of one section and of a by-lane bank (whose
// entries are in biquad_i16_bylane.hip).  The entries take row pitches and any 2-byte-aligned x and y:
// i16 rows with an odd row length are the normal case, and the pitch is how a caller keeps them on the 4-byte grid where the fast
// forms run (biquad_i16_plan.h).
#include <cmath>

#include "biquad_i16_kernels.h"
#include "biquad_pass_plan.h"

namespace idsp {
namespace {

using namespace bq16;

inline void pack(Sec &d, const int16_t (&ba)[5], int frac)
{
    d.b0lo = uint16_t(ba[0]), d.b0hi = uint32_t(uint16_t(ba[0])) << 16;
    d.b12 = uint32_t(uint16_t(ba[1])) | uint32_t(uint16_t(ba[2])) << 16;
    d.a12 = uint32_t(uint16_t(ba[3])) | uint32_t(uint16_t(ba[4])) << 16;
    d.frac = frac;
}
inline void fill(Sec &d, const idsp_biquad_i16 &c)
{
    pack(d, c.ba, c.frac);
    d.u = 0, d.mn = INT16_MIN, d.mx = INT16_MAX;
}
inline void fill(Sec &d, const idsp_biquad_clamp_i16 &c)
{
    pack(d, c.ba, c.frac);
    d.u = c.u, d.mn = c.min, d.mx = c.max;
}

// sections first .. first + N - 1 in one launch
template <int N, bool CLAMP, class Cfg>
int run_pass(const Cfg *cfg, size_t first, uint32_t *state, const int16_t *x, size_t xl, int16_t *y, size_t yl, size_t lanes, size_t frames, int layout,
             hipStream_t s)
{
    Params<N> prm;
    for (int k = 0; k < N; k++) fill(prm.sec[k], cfg[first + k]);
    uint32_t *st = state + first * 4 * lanes;
    const Plan pl = plan_biquad_i16(layout == IDSP_LANE_MAJOR, lanes, reinterpret_cast<uintptr_t>(x), reinterpret_cast<uintptr_t>(y), xl, yl, switches());
    note_kernel(pl.name);
    switch (pl.form) {
    case kFmPlain:
        hipLaunchKernelGGL((biquad_i16_frame_major<N, CLAMP, kFmU>), dim3(pl.grid), dim3(pl.block), 0, s, prm, st, x, y, lanes, frames, xl, yl);
        break;
    default:
        hipLaunchKernelGGL((biquad_i16_lane_major<N, CLAMP>), dim3(pl.grid), dim3(pl.block), 0, s, prm, st, x, y, lanes, frames, xl, yl,
                           int(pl.form == kLmDwordRuns));
        break;
    }
    return launch_status();
}

template <bool CLAMP, class Cfg>
int entry(const Cfg *cfg, size_t n, void *state, const int16_t *x, size_t x_pitch, int16_t *y, size_t y_pitch, size_t lanes, size_t frames, int layout,
          void *stream)
{
    if (int rc = check_stream_args(cfg, n, state, x, y, lanes, frames, layout)) return rc;
    for (size_t k = 0; k < n; k++)  // the shift of the i32 accumulator, the rule of idsp_biquad_i32 (biquad.rs:448-450)
        if (cfg[k].frac < 0 || cfg[k].frac > 31) return fail(IDSP_EINVAL, "section %zu: frac = %d not in 0..31", k, int(cfg[k].frac));
    // x and y on the 2-byte grid; y == x with one pitch is the reference's inplace() (biquad.rs:540-541)
    subword::PitchedRows r;
    if (int rc = subword::pitched_rows(r, layout, lanes, frames, x, x_pitch, 2, y, y_pitch, 2, subword::InPlace::same_rows)) return rc;
    if (lanes == 0 || frames == 0) return IDSP_OK;
    const size_t row = r.row, rows = r.rows, xl = r.xl, yl = r.yl;
    hipStream_t s = as_stream(stream);
    if (n == 0) {  // empty slice: y.copy_from_slice(x), compose.rs:63-65
        if (x != y) IDSP_HIP_TRY(hipMemcpy2DAsync(y, yl * 2, x, xl * 2, row * 2, rows, hipMemcpyDeviceToDevice, s));
        return IDSP_OK;
    }
    // the passes of biquad_pass_plan.h (never two waves): the first reads x, later ones run in place on y — literally the reference's slice composition
    uint32_t *st = static_cast<uint32_t *>(state);
    const int16_t *src = x;
    size_t sl = xl;
    for (size_t done = 0; done < n;) {
        const int m = next_pass(i16_rules(), n - done, lanes, layout, StreamSwitches{}).na;
        int rc;
        switch (m) {
        case 1: rc = run_pass<1, CLAMP>(cfg, done, st, src, sl, y, yl, lanes, frames, layout, s); break;
        case 2: rc = run_pass<2, CLAMP>(cfg, done, st, src, sl, y, yl, lanes, frames, layout, s); break;
        case 3: rc = run_pass<3, CLAMP>(cfg, done, st, src, sl, y, yl, lanes, frames, layout, s); break;
        default: rc = run_pass<4, CLAMP>(cfg, done, st, src, sl, y, yl, lanes, frames, layout, s); break;
        }
        if (rc) return rc;
        done += size_t(m);
        src = y, sl = yl;
    }
    return IDSP_OK;
}

// `(v * 2^F).round() as i16` (dsp-fixedpoint/src/num_traits_impl.rs:32-46): half away from zero, saturating, NaN -> 0
int16_t to_q16(double v, int frac)
{
    const double s = std::round(std::ldexp(v, frac));
    if (std::isnan(s)) return 0;
    if (s >= 32767.0) return INT16_MAX;
    if (s <= -32768.0) return INT16_MIN;
    return int16_t(s);
}

// [b0, b1, b2, a0, a1, a2] -> ba: biquad.rs:551-559, each value through to_q16
void ba_from_sos(const double *sos, int frac, int16_t *ba)
{
    const double a0 = 1.0 / sos[3];
    const double v[5] = {sos[0] * a0, sos[1] * a0, sos[2] * a0, -sos[4] * a0, -sos[5] * a0};
    for (int i = 0; i < 5; i++) ba[i] = to_q16(v[i], frac);
}

}  // namespace
}  // namespace idsp

using namespace idsp;

extern "C" {

int idsp_biquad_i16_from_sos(const double sos[6], int frac, idsp_biquad_i16 *out)
{
    if (!sos || !out) return fail(IDSP_EINVAL, "sos or out is NULL");
    if (frac < 0 || frac > 31) return fail(IDSP_EINVAL, "frac = %d not in 0..31", frac);
    ba_from_sos(sos, frac, out->ba);
    out->frac = int16_t(frac);
    return IDSP_OK;
}

int idsp_biquad_i16_bank_from_sos(const double *sos, size_t lanes, size_t n, int frac, size_t cv, int16_t *coef)
{
    if (frac < 0 || frac > 31) return fail(IDSP_EINVAL, "frac = %d not in 0..31", frac);
    if (cv != 5 && cv != 8) return fail(IDSP_EINVAL, "cv = %zu is neither 5 (ba) nor 8 (ba, u, min, max)", cv);
    if (n > IDSP_MAX_SECTIONS) return fail(IDSP_EINVAL, "n = %zu sections > IDSP_MAX_SECTIONS", n);
    if (lanes == 0 || n == 0) return IDSP_OK;
    if (!sos || !coef) return fail(IDSP_EINVAL, "sos or coef is NULL");
    for (size_t l = 0; l < lanes; l++)
        for (size_t k = 0; k < n; k++) {
            int16_t sec[8] = {0, 0, 0, 0, 0, 0, INT16_MIN, INT16_MAX};  // u, min, max: BiquadClamp::default (biquad.rs:159-171)
            ba_from_sos(sos + (l * n + k) * 6, frac, sec);
            for (size_t v = 0; v < cv; v++) coef[(k * cv + v) * lanes + l] = sec[v];
        }
    return IDSP_OK;
}

size_t idsp_biquad_i16_state_words(size_t n) { return 4 * n; }

int idsp_biquad_i16_df1(const idsp_biquad_i16 *cfg, size_t n, void *state, const int16_t *x, size_t x_pitch, int16_t *y, size_t y_pitch, size_t lanes,
                        size_t frames, int layout, void *stream)
{
    return entry<false>(cfg, n, state, x, x_pitch, y, y_pitch, lanes, frames, layout, stream);
}

int idsp_biquad_i16_df1_clamp(const idsp_biquad_clamp_i16 *cfg, size_t n, void *state, const int16_t *x, size_t x_pitch, int16_t *y, size_t y_pitch,
                              size_t lanes, size_t frames, int layout, void *stream)
{
    return entry<true>(cfg, n, state, x, x_pitch, y, y_pitch, lanes, frames, layout, stream);
}

}  // extern "C"
