// rpll.hip — the reciprocal PLL of the reference (src/rpll.rs) on the stream kernels (rpll_procs.h; both layouts and any lane
// count come from launch_stream, lane_stream.h), and the local oscillator of a batch from the `Accu` it returns: the reference's
// own `Accu * T`, `Accu + Accu`, `next()` (src/accu.rs:34-54) and `Complex::from_angle` (src/complex.rs:237-240) in closed form,
// elementwise over the output.  All integer, bit-exact.
#include "dds_dev.h"
#include "rpll_procs.h"

namespace idsp {
namespace {

typedef int32_t i32x4 __attribute__((ext_vector_type(4)));

constexpr int kAccuLoRows = 16;  // output rows per workgroup trip (the 512-byte table fill of a workgroup is spread over 32 evaluations per thread)

// lo[t, l] = cossin(sample.state + (j + 1) * sample.step), t = u 2^k + j, sample = Accu(a.state, (u32)a.step >> k) * harmonic +
// Accu(offset, 0), a = accu[u, l] (include/idsp_hip.h).  The output is walked as a (row, column) grid with the contiguous axis as
// columns — lanes in FrameMajor (LM = false), samples in LaneMajor (LM = true) — so that no index is ever divided.
// One thread produces the two adjacent samples of a column pair and writes them with ONE 16-byte nontemporal store: a wave's
// store instruction covers 1 KiB of whole lines (cossin_kernel, dds.hip: four samples per thread split each line over two
// instructions and measured slower).  A row that does not start on the 16-byte grid (FrameMajor with an odd lane count, a base at
// 8 mod 16, LaneMajor with an odd frame count) takes two 8-byte stores per thread instead.
// An `accu` row is read once per 2^k output rows, through the caches: FrameMajor keeps the pair of a column across the rows of
// one update in registers, LaneMajor threads of one update read the same 8 bytes.
// cossin is `cossin_dev` on the 512-byte table.  `cossin_circle` on the 16 KiB full-circle table (dds_dev.h; the same bits) was
// built beside it as a template argument, measured and taken out.  At 65536, 32768 and 16384 lanes x 4096 frames with k = 0 / 3 / 8
// it took 0.99 to 1.04 times this form's time FrameMajor (1-4 % slower in the six shapes at 65536 and 32768 lanes, equal at 16384)
// and 0.97 to 1.03 times LaneMajor (0-3 % faster in seven of nine shapes), where two repeats of one form differ by up to 1 % at
// the large shapes and up to 7 % at 16384 lanes (profiles/NOTES.md, "RPLL").  Neither form wins in both layouts: the kernel is
// bound by its stores, not by cossin.  The small table stays: one form, and 32 times less LDS to fill per workgroup.
template <bool LM>
__global__ __launch_bounds__(256) void accu_lo_kernel(const int32_t *accu, int32_t *lo, const size_t rows, const size_t cols, const size_t updates,
                                                      const int k, const uint32_t harmonic, const uint32_t offset)
{
    __shared__ uint32_t tab[1 << kCossinDepth];
    fill_cossin(tab, threadIdx.x, 256);
    __syncthreads();
    const rpll_pair *ap = reinterpret_cast<const rpll_pair *>(accu);
    const size_t ncp = (cols + 1) / 2, nchunks = (rows + kAccuLoRows - 1) / kAccuLoRows;
    const size_t jmask = (size_t(1) << k) - 1;
    // phase of sample j of an update from its `Accu` (all wrapping)
    auto phase = [&](rpll_pair a, uint32_t j) {
        const uint32_t step = (uint32_t(a.y) >> k) * harmonic;  // `Accu::new(state, step >> k) * harmonic` (src/accu.rs:40-46)
        const uint32_t state = uint32_t(a.x) * harmonic + offset;  // `+ Accu::new(offset, 0)` (:48-54)
        return state + (j + 1u) * step;                          // j + 1 calls of the pre-incrementing `next()` (:34-37)
    };
    for (size_t cp = size_t(blockIdx.x) * 256 + threadIdx.x; cp < ncp; cp += size_t(gridDim.x) * 256) {
        const size_t c0 = 2 * cp;
        const bool two = c0 + 1 < cols;
        for (size_t chunk = blockIdx.y; chunk < nchunks; chunk += gridDim.y) {
            rpll_pair a0 = {0, 0}, a1 = {0, 0};
            size_t u_have = ~size_t(0);
            for (int i = 0; i < kAccuLoRows; i++) {
                const size_t r = chunk * kAccuLoRows + i;  // wave-uniform
                if (r >= rows) break;
                uint32_t ph0, ph1;
                if constexpr (LM) {
                    // row = lane, columns = samples t = c0, c0 + 1: the same update when k > 0 (c0 is even), adjacent updates when k == 0
                    const size_t u0 = c0 >> k, u1 = (c0 + 1) >> k;
                    a0 = ap[r * updates + u0];
                    a1 = (two && k == 0) ? ap[r * updates + u1] : a0;
                    ph0 = phase(a0, uint32_t(c0 & jmask));
                    ph1 = phase(a1, uint32_t((c0 + 1) & jmask));
                } else {
                    // row = sample t, columns = lanes c0, c0 + 1 of update t >> k: loaded when the row enters a new update
                    const size_t u = r >> k;
                    if (u != u_have) {
                        a0 = ap[u * cols + c0];
                        a1 = two ? ap[u * cols + c0 + 1] : a0;
                        u_have = u;
                    }
                    const uint32_t j = uint32_t(r & jmask);
                    ph0 = phase(a0, j);
                    ph1 = phase(a1, j);
                }
                const Cplx v0 = cossin_dev(int32_t(ph0), tab), v1 = cossin_dev(int32_t(ph1), tab);
                int32_t *row = lo + r * cols * 2;  // wave-uniform
                if (two && reinterpret_cast<uintptr_t>(row) % 16 == 0) {
                    __builtin_nontemporal_store(i32x4{v0.re, v0.im, v1.re, v1.im}, reinterpret_cast<i32x4 *>(row) + cp);
                } else {
                    __builtin_nontemporal_store(rpll_pair{v0.re, v0.im}, reinterpret_cast<rpll_pair *>(row) + c0);
                    if (two) __builtin_nontemporal_store(rpll_pair{v1.re, v1.im}, reinterpret_cast<rpll_pair *>(row) + c0 + 1);
                }
            }
        }
    }
}

template <bool LM>
int launch_accu_lo(const idsp_accu_lo *cfg, const int32_t *accu, int32_t *lo, size_t lanes, size_t updates, hipStream_t s)
{
    const size_t frames = updates << cfg->batch_log2;
    const size_t rows = LM ? lanes : frames, cols = LM ? frames : lanes;
    // column pairs in x, row chunks in y; both loops of the kernel stride by the grid, so the caps only bound the launch
    const size_t ncp = (cols + 1) / 2, nchunks = (rows + kAccuLoRows - 1) / kAccuLoRows;
    size_t gx = (ncp + 255) / 256, gy = nchunks;
    if (gx > 4096) gx = 4096;
    const size_t ymax = (size_t(1) << 20) / gx < 65535 ? (size_t(1) << 20) / gx : 65535;
    if (gy > ymax) gy = ymax;
    note_kernel(LM ? "accu_lo_kernel[LaneMajor]" : "accu_lo_kernel[FrameMajor]");
    hipLaunchKernelGGL((accu_lo_kernel<LM>), dim3(unsigned(gx), unsigned(gy)), dim3(256), 0, s, accu, lo, rows, cols, updates, int(cfg->batch_log2),
                       uint32_t(cfg->harmonic), uint32_t(cfg->offset));
    return launch_status();
}

}  // namespace
}  // namespace idsp

using namespace idsp;

extern "C" {

size_t idsp_rpll_state_words(void) { return IDSP_RPLL_STATE_WORDS; }

int idsp_rpll_i32(const idsp_rpll *cfg, void *state, const int32_t *ts, int32_t *accu, size_t lanes, size_t frames, int layout, void *stream)
{
    if (!cfg) return fail(IDSP_EINVAL, "cfg is NULL");
    // from the shifts of src/rpll.rs:58-74, not from its debug_asserts: `>> dt2` and `1 << dt2` as i32 (:68, :70), `1u32 << (sf - 1)`
    // and a u64 shift by sf (:60-61), `1u32 << (32 + dt2 - sf)` (:64: sf == dt2 would shift a u32 by 32), an i32 shift by sp - dt2 (:72)
    if (cfg->dt2 < 0 || cfg->dt2 > 30) return fail(IDSP_EINVAL, "dt2 = %d not in 0..30", cfg->dt2);
    if (cfg->shift_frequency <= cfg->dt2 || cfg->shift_frequency > 32)
        return fail(IDSP_EINVAL, "shift_frequency = %d not in dt2 + 1..32 (dt2 = %d; `1u32 << (32 + dt2 - shift_frequency)`, src/rpll.rs:64)", cfg->shift_frequency, cfg->dt2);
    if (cfg->shift_phase < cfg->dt2 || cfg->shift_phase > cfg->dt2 + 31)
        return fail(IDSP_EINVAL, "shift_phase = %d not in dt2..dt2 + 31 (dt2 = %d)", cfg->shift_phase, cfg->dt2);
    if (int rc = check_stream_args(nullptr, 0, state, ts, accu, lanes, frames, layout)) return rc;
    if (lanes == 0 || frames == 0) return IDSP_OK;
    if (!state) return fail(IDSP_EINVAL, "state is NULL");
    if ((reinterpret_cast<uintptr_t>(ts) | reinterpret_cast<uintptr_t>(accu)) % 8) return fail(IDSP_EINVAL, "ts and accu hold 8-byte pairs: they must be 8-byte aligned");
    if (ranges_overlap(ts, span_bytes(lanes, frames, 8), accu, span_bytes(lanes, frames, 8))) return fail(IDSP_EINVAL, "ts and accu overlap");
    RpllParams p;
    p.dt2 = cfg->dt2, p.sf = cfg->shift_frequency, p.sdy = cfg->shift_phase - cfg->dt2;
    p.half = uint32_t(1) << (cfg->shift_frequency - 1);
    p.p_ref = uint32_t(1) << (32 + cfg->dt2 - cfg->shift_frequency);
    p.dt_mask = (uint32_t(1) << cfg->dt2) - 1u;
    return launch_stream<RpllProc>(p, state, reinterpret_cast<const rpll_pair *>(ts), reinterpret_cast<rpll_pair *>(accu), lanes, frames, layout, as_stream(stream));
}

int idsp_accu_lo_i32(const idsp_accu_lo *cfg, const int32_t *accu, int32_t *lo, size_t lanes, size_t updates, int layout, void *stream)
{
    if (!cfg) return fail(IDSP_EINVAL, "cfg is NULL");
    if (cfg->batch_log2 < 0 || cfg->batch_log2 > 24) return fail(IDSP_EINVAL, "batch_log2 = %d not in 0..24", cfg->batch_log2);
    if (updates > ((size_t(1) << 40) >> cfg->batch_log2)) return fail(IDSP_EINVAL, "updates << batch_log2 out of range");
    const size_t frames = updates << cfg->batch_log2;
    if (int rc = check_stream_args(nullptr, 0, nullptr, accu, lo, lanes, frames, layout)) return rc;
    if (lanes == 0 || updates == 0) return IDSP_OK;
    if ((reinterpret_cast<uintptr_t>(accu) | reinterpret_cast<uintptr_t>(lo)) % 8) return fail(IDSP_EINVAL, "accu and lo hold 8-byte pairs: they must be 8-byte aligned");
    if (ranges_overlap(accu, span_bytes(lanes, updates, 8), lo, span_bytes(lanes, frames, 8))) return fail(IDSP_EINVAL, "accu and lo overlap");
    if (layout == IDSP_LANE_MAJOR) return launch_accu_lo<true>(cfg, accu, lo, lanes, updates, as_stream(stream));
    return launch_accu_lo<false>(cfg, accu, lo, lanes, updates, as_stream(stream));
}

}  // extern "C"
