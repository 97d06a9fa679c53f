// dsm.hip — `Dsm<K>` (src/dsm.rs), K = 0..8: the host side of the two kernels of dsm_kernels.h.  The one entry takes row pitches
// and any byte alignment of y: i8 rows with an odd row length are the normal case, and the pitch is how a caller keeps them aligned.
#include "dsm_kernels.h"

namespace idsp {
namespace {

template <int K>
int launch_dsm(uint32_t *st, const uint32_t *x, size_t xl, int8_t *y, size_t yl, size_t lanes, size_t frames, int layout, hipStream_t s)
{
    if (layout == IDSP_LANE_MAJOR) {
        // every 128-byte run of a lane starts on a 4-byte boundary: dword stores
        const int aligned = reinterpret_cast<uintptr_t>(y) % 4 == 0 && yl % 4 == 0;
        note_kernel(aligned ? "dsm_lane_major[dword runs]" : "dsm_lane_major[byte runs]");
        hipLaunchKernelGGL((dsm::dsm_lane_major<K, dsm::kLmOT>), dim3(unsigned((lanes + dsm::kWave - 1) / dsm::kWave)), dim3(dsm::kWave), 0, s, st, x, y, lanes,
                           frames, xl, yl, aligned);
        return launch_status();
    }
    note_kernel("dsm_frame_major[byte stores]");
    hipLaunchKernelGGL((dsm::dsm_frame_major<K, dsm::kFmU>), dim3(unsigned((lanes + dsm::kFmBlock - 1) / dsm::kFmBlock)), dim3(dsm::kFmBlock), 0, s, st, x, y,
                       lanes, frames, xl, yl);
    return launch_status();
}

}  // namespace
}  // namespace idsp

using namespace idsp;

extern "C" {

size_t idsp_dsm_state_words(int order) { return order < 0 || order > IDSP_DSM_MAX_ORDER ? 0 : size_t(2 * order); }

int idsp_dsm_u32(int order, void *state, const uint32_t *x, size_t x_pitch, int8_t *y, size_t y_pitch, size_t lanes, size_t frames, int layout,
                 void *stream)
{
    if (order < 0 || order > IDSP_DSM_MAX_ORDER) return fail(IDSP_EINVAL, "order = %d not in 0..%d", order, IDSP_DSM_MAX_ORDER);
    if (layout != IDSP_FRAME_MAJOR && layout != IDSP_LANE_MAJOR)
        return fail(IDSP_EINVAL, "layout %d is neither IDSP_FRAME_MAJOR nor IDSP_LANE_MAJOR", layout);
    if (!x || !y) return fail(IDSP_EINVAL, "x or y is NULL");
    if (order > 0 && !state) return fail(IDSP_EINVAL, "state is NULL");
    if (lanes > (size_t(1) << 31) || frames > (size_t(1) << 40)) return fail(IDSP_EINVAL, "lanes/frames out of range");
    subword::PitchedRows r;  // x on its 4-byte grid, any y, no overlap
    if (int rc = subword::pitched_rows(r, layout, lanes, frames, x, x_pitch, 4, y, y_pitch, 1, subword::InPlace::never)) return rc;
    if (lanes == 0 || frames == 0) return IDSP_OK;
    const size_t xl = r.xl, yl = r.yl;
    uint32_t *st = static_cast<uint32_t *>(state);
    hipStream_t s = as_stream(stream);
    switch (order) {
    case 0: return launch_dsm<0>(st, x, xl, y, yl, lanes, frames, layout, s);
    case 1: return launch_dsm<1>(st, x, xl, y, yl, lanes, frames, layout, s);
    case 2: return launch_dsm<2>(st, x, xl, y, yl, lanes, frames, layout, s);
    case 3: return launch_dsm<3>(st, x, xl, y, yl, lanes, frames, layout, s);
    case 4: return launch_dsm<4>(st, x, xl, y, yl, lanes, frames, layout, s);
    case 5: return launch_dsm<5>(st, x, xl, y, yl, lanes, frames, layout, s);
    case 6: return launch_dsm<6>(st, x, xl, y, yl, lanes, frames, layout, s);
    case 7: return launch_dsm<7>(st, x, xl, y, yl, lanes, frames, layout, s);
    default: return launch_dsm<8>(st, x, xl, y, yl, lanes, frames, layout, s);
    }
}

}  // extern "C"
