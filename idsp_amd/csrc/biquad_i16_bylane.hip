// biquad_i16_bylane.hip — `ByLane<[Biquad<Q16<F>>; N]>` / `ByLane<[BiquadClamp<Q16<F>, i16>; N]>` x `DirectForm1<i16>`
// (dsp-process/src/compose.rs:363-390 over src/iir/biquad.rs:366-404): the entries of the by-lane kernels of biquad_i16_kernels.h.  The
// checks, the passes and the dispatch are those of biquad_i16.hip; a pass takes its planes from `coef` where that one takes its
// sections from `cfg`.  (A unit of its own: its 16 kernels compile beside the 16 of biquad_i16.hip under `make -j`.)
#include "biquad_i16_kernels.h"
#include "biquad_pass_plan.h"

namespace idsp {
namespace {

using namespace bq16;

// sections first .. first + N - 1 in one launch: their planes start at coef + first * CV * lanes
template <int N, bool CLAMP>
int run_pass(const int16_t *coef, int frac, size_t first, uint32_t *state, const int16_t *x, size_t xl, int16_t *y, size_t yl, size_t lanes, size_t frames,
             int layout, hipStream_t s)
{
    const int16_t *cf = coef + first * (CLAMP ? 8 : 5) * lanes;
    uint32_t *st = state + first * 4 * lanes;
    const Plan pl = plan_biquad_i16_bylane(layout == IDSP_LANE_MAJOR, lanes, reinterpret_cast<uintptr_t>(x), reinterpret_cast<uintptr_t>(y), xl, yl, switches());
    note_kernel(pl.name);
    switch (pl.form) {
    case kFmPlain:
        hipLaunchKernelGGL((biquad_i16_bylane_frame_major<N, CLAMP, kFmU>), dim3(pl.grid), dim3(pl.block), 0, s, cf, frac, st, x, y, lanes, frames, xl, yl);
        break;
    default:
        hipLaunchKernelGGL((biquad_i16_bylane_lane_major<N, CLAMP>), dim3(pl.grid), dim3(pl.block), 0, s, cf, frac, st, x, y, lanes, frames, xl, yl,
                           int(pl.form == kLmDwordRuns));
        break;
    }
    return launch_status();
}

template <bool CLAMP>
int entry(const int16_t *coef, int frac, size_t n, void *state, const int16_t *x, size_t x_pitch, int16_t *y, size_t y_pitch, size_t lanes, size_t frames,
          int layout, void *stream)
{
    // the planes of an empty bank (no lanes or no sections) hold nothing: any pointer will do for them, NULL too
    if (n && lanes && !coef) return fail(IDSP_EINVAL, "coef is NULL");
    if (reinterpret_cast<uintptr_t>(coef) % 2) return fail(IDSP_EINVAL, "coef is not 2-byte aligned");
    if (int rc = check_stream_args(&frac /* coef: checked above */, n, state, x, y, lanes, frames, layout)) return rc;
    if (frac < 0 || frac > 31) return fail(IDSP_EINVAL, "frac = %d not in 0..31", frac);  // the rule of the i32 by-lane entries
    subword::PitchedRows r;
    if (int rc = subword::pitched_rows(r, layout, lanes, frames, x, x_pitch, 2, y, y_pitch, 2, subword::InPlace::same_rows)) return rc;
    if (lanes == 0 || frames == 0) return IDSP_OK;
    const size_t row = r.row, rows = r.rows, xl = r.xl, yl = r.yl;
    hipStream_t s = as_stream(stream);
    if (n == 0) {  // empty slice: y.copy_from_slice(x), compose.rs:63-65
        if (x != y) IDSP_HIP_TRY(hipMemcpy2DAsync(y, yl * 2, x, xl * 2, row * 2, rows, hipMemcpyDeviceToDevice, s));
        return IDSP_OK;
    }
    // the passes of biquad_pass_plan.h (never two waves): the first reads x, later ones run in place on y — (biquad_i16.hip)
    uint32_t *st = static_cast<uint32_t *>(state);
    const int16_t *src = x;
    size_t sl = xl;
    for (size_t done = 0; done < n;) {
        const int m = next_pass(i16_rules(), n - done, lanes, layout, StreamSwitches{}).na;
        int rc;
        switch (m) {
        case 1: rc = run_pass<1, CLAMP>(coef, frac, done, st, src, sl, y, yl, lanes, frames, layout, s); break;
        case 2: rc = run_pass<2, CLAMP>(coef, frac, done, st, src, sl, y, yl, lanes, frames, layout, s); break;
        case 3: rc = run_pass<3, CLAMP>(coef, frac, done, st, src, sl, y, yl, lanes, frames, layout, s); break;
        default: rc = run_pass<4, CLAMP>(coef, frac, done, st, src, sl, y, yl, lanes, frames, layout, s); break;
        }
        if (rc) return rc;
        done += size_t(m);
        src = y, sl = yl;
    }
    return IDSP_OK;
}

}  // namespace
}  // namespace idsp

using namespace idsp;

extern "C" {

int idsp_biquad_i16_df1_bylane(const int16_t *coef, int frac, size_t n, void *state, const int16_t *x, size_t x_pitch, int16_t *y, size_t y_pitch,
                               size_t lanes, size_t frames, int layout, void *stream)
{
    return entry<false>(coef, frac, n, state, x, x_pitch, y, y_pitch, lanes, frames, layout, stream);
}

int idsp_biquad_i16_df1_clamp_bylane(const int16_t *coef, int frac, size_t n, void *state, const int16_t *x, size_t x_pitch, int16_t *y, size_t y_pitch,
                                     size_t lanes, size_t frames, int layout, void *stream)
{
    return entry<true>(coef, frac, n, state, x, x_pitch, y, y_pitch, lanes, frames, layout, stream);
}

}  // extern "C"
