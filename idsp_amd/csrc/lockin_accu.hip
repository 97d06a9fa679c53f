// lockin_accu.hip — idsp_lockin_i32_accu_process: the external-LO lock-in with lowpass arms (src/lockin.rs:17-39) on the LO that
// idsp_accu_lo_i32 would write for the same `Accu` rows (src/accu.rs:34-54, src/complex.rs:237-240), evaluated inside the kernel
// (lockin_accu_procs.h) — the 8 bytes per sample of LO are neither written nor read.  A translation unit of its own: the sixteen
// launch_stream instantiations compile beside lockin_generic.hip and lockin_phase.hip, not inside them.
#include "lockin_accu_procs.h"

namespace idsp {
namespace {

template <template <int, int> class Proc, class OutT>
int dispatch_accu_nk(const idsp_lockin_i32 *cfg, const LpAccuParams &p, void *state, const int32_t *x, OutT *y, size_t lanes, size_t frames, int layout,
                     hipStream_t s)
{
    return for_nk(cfg, [&](auto n, auto k) { return launch_stream<Proc<decltype(n)::value, decltype(k)::value>>(p, state, x, y, lanes, frames, layout, s); });
}

}  // namespace
}  // namespace idsp

using namespace idsp;

extern "C" int idsp_lockin_i32_accu_process(const idsp_lockin_i32 *cfg, const idsp_accu_lo *lo_cfg, void *state, const int32_t *x, const int32_t *accu,
                                            int32_t *y, size_t lanes, size_t updates, int layout, void *stream)
{
    // the checks of idsp_lockin_i32_lo_process and of idsp_accu_lo_i32; an empty call (no lanes or no updates) touches no buffer and is IDSP_OK
    if (int rc = lockin_cfg_check(cfg)) return rc;
    if (!lo_cfg) return fail(IDSP_EINVAL, "lo_cfg is NULL");
    if (lo_cfg->batch_log2 < 0 || lo_cfg->batch_log2 > 24) return fail(IDSP_EINVAL, "batch_log2 = %d not in 0..24", lo_cfg->batch_log2);
    if (updates > ((size_t(1) << 40) >> lo_cfg->batch_log2)) return fail(IDSP_EINVAL, "updates << batch_log2 out of range");
    const size_t frames = updates << lo_cfg->batch_log2;
    if (int rc = check_stream_args(cfg, 1, state, x, y, lanes, frames, layout)) return rc;
    if (lanes == 0 || updates == 0) return IDSP_OK;
    if (!accu) return fail(IDSP_EINVAL, "accu is NULL");
    // accu and y hold pairs and are read / written 8 bytes at a time
    if ((reinterpret_cast<uintptr_t>(accu) | reinterpret_cast<uintptr_t>(y)) % 8) return fail(IDSP_EINVAL, "accu and y hold 8-byte pairs: both must be 8-byte aligned");
    // three separate buffers: x streams through the kernel, accu is walked by a side pointer, and x is 4 bytes where y is 8
    const size_t xb = span_bytes(lanes, frames, 4), ab = span_bytes(lanes, updates, 8), yb = span_bytes(lanes, frames, 8);
    if (ranges_overlap(x, xb, y, yb) || ranges_overlap(accu, ab, y, yb) || ranges_overlap(x, xb, accu, ab)) return fail(IDSP_EINVAL, "x, accu and y must not overlap");

    LpAccuParams p;
    p.lp = lp_params(cfg);
    p.xw = layout == IDSP_FRAME_MAJOR ? AccuWalk{accu, 1, lanes, updates} : AccuWalk{accu, updates, 1, updates};
    p.harmonic = uint32_t(lo_cfg->harmonic), p.offset = uint32_t(lo_cfg->offset);
    p.k = uint32_t(lo_cfg->batch_log2), p.jmask = (uint32_t(1) << lo_cfg->batch_log2) - 1u;
    // the I and Q arms on two threads up to the lane count where idsp_lockin_i32_process does so on its stream path
    if (lanes <= lockin_switches().split_max_lanes) return dispatch_accu_nk<LockinAccuSplitProc, int32_t>(cfg, p, state, x, y, 2 * lanes, frames, layout, as_stream(stream));
    return dispatch_accu_nk<LockinAccuProc, Cplx>(cfg, p, state, x, reinterpret_cast<Cplx *>(y), lanes, frames, layout, as_stream(stream));
}
