// dds.hip — elementwise cossin() and atan2() and the Accu phase-accumulator DDS over many lanes (reference: src/cossin.rs,
// src/atan2.rs, src/accu.rs, src/complex.rs).  All integer, bit-exact.  (The lock-in phase entries and idsp_lowpass_i32 are in
// lockin_phase.hip, the FM discriminator in fm_disc.hip.)
//
// cossin's 128-entry LUT (512 B) is staged once per workgroup into LDS from
// the compile-time table; per-lane gathers then cost an LDS read instead of a
// divergent constant-memory fetch.  Everything after the gather is ~40 VALU
// ops in registers, fused in the lock-in kernels with the mixer and the
// lowpass cascade so a phase never touches memory.
#include "dds_dev.h"

namespace idsp {
namespace {

// ------------------------------------------------------------- processors
// Accu (src/accu.rs:34-41, pre-increment) -> Complex::from_angle (src/complex.rs:237-240)
// CIRCLE: cossin through the full-circle table (dds_dev.h cossin_circle: 9 VALU + 1 LDS instruction instead of ~28 + 1, 16 KiB of LDS
// per workgroup, filled at the start of every workgroup) — taken by FrameMajor calls of 256 frames or more (plan_dds, readout_plan.h); the 512-byte
// table otherwise (short calls, LaneMajor — its staged kernel needs the LDS for the 32 KiB tile slot of every wave — and the one-thread-per-lane form).
template <bool CIRCLE>
struct CosTab {
    static constexpr int WORDS = CIRCLE ? kCosCircleWords : (1 << kCossinDepth);
    static __device__ __forceinline__ void fill(uint32_t *sh, int tid, int n)
    {
        if constexpr (CIRCLE)
            fill_cossin_circle(sh, tid, n);
        else
            fill_cossin(sh, tid, n);
    }
    static __device__ __forceinline__ Cplx eval(uint32_t ph, const uint32_t *t)
    {
        if constexpr (CIRCLE)
            return cossin_circle(ph, t);
        else
            return cossin_dev(int32_t(ph), t);
    }
};

template <bool CIRCLE>
struct DdsProcT {
    using In = int32_t;  // unused
    using Out = Cplx;
    static constexpr bool HAS_IN = false;
    static constexpr int LDS_WORDS = CosTab<CIRCLE>::WORDS;
    static constexpr int IN_DIV = 1;
    static constexpr int COST = 100;
    struct Params {
        int32_t unused;
    };
    const uint32_t *lut;
    uint32_t acc, inc;
    static __device__ __forceinline__ void fill_shared(uint32_t *sh, int tid, int n) { CosTab<CIRCLE>::fill(sh, tid, n); }
    __device__ __forceinline__ void set_shared(const uint32_t *sh) { lut = sh; }
    __device__ __forceinline__ void load(const Params &, const uint32_t *st, size_t lanes, size_t lane)
    {
        acc = st[lane];
        inc = st[lanes + lane];
    }
    __device__ __forceinline__ void store(const Params &, uint32_t *st, size_t lanes, size_t lane) { st[lane] = acc; }
    __device__ __forceinline__ Out step(const Params &, In)
    {
        acc += inc;
        return CosTab<CIRCLE>::eval(acc, lut);
    }
};
using DdsProc = DdsProcT<false>;

template <bool CIRCLE>
struct DdsSplitProcT {
    using In = int32_t;  // unused
    using Out = int32_t;
    static constexpr bool HAS_IN = false;
    static constexpr int LDS_WORDS = CosTab<CIRCLE>::WORDS;
    static constexpr int IN_DIV = 2;
    static constexpr int COST = 100;
    struct Params {
        int32_t unused;
    };
    const uint32_t *lut;
    uint32_t acc, inc;
    bool q;
    static __device__ __forceinline__ void fill_shared(uint32_t *sh, int tid, int n) { CosTab<CIRCLE>::fill(sh, tid, n); }
    __device__ __forceinline__ void set_shared(const uint32_t *sh) { lut = sh; }
    __device__ __forceinline__ void load(const Params &, const uint32_t *st, size_t vlanes, size_t vlane)
    {
        q = vlane & 1;
        acc = st[vlane / 2];
        inc = st[vlanes / 2 + vlane / 2];
    }
    __device__ __forceinline__ void store(const Params &, uint32_t *st, size_t, size_t vlane)
    {
        if (!q) st[vlane / 2] = acc;
    }
    static constexpr int BATCH = 4;
    using Pre = int32_t;
    __device__ __forceinline__ Pre pre(const Params &)
    {
        acc += inc;
        const Cplx c = CosTab<CIRCLE>::eval(acc, lut);
        return q ? c.im : c.re;
    }
    __device__ __forceinline__ void pre_batch(const Params &, Pre (&out)[BATCH])
    {
#pragma unroll
        for (int j = 0; j < BATCH / 2; j++) {
            const uint32_t ph = acc + inc * uint32_t(2 * j + 1) + (q ? inc : 0u);
            const Cplx c = CosTab<CIRCLE>::eval(ph, lut);
            const int32_t mine = q ? c.im : c.re, other = q ? c.re : c.im;
            const int32_t recv = pair_swap(other);
            out[2 * j] = q ? recv : mine;
            out[2 * j + 1] = q ? mine : recv;
        }
        acc += inc * uint32_t(BATCH);
    }
    __device__ __forceinline__ Out step(const Params &, In, const Pre &v) { return v; }
};
using DdsSplitProc = DdsSplitProcT<false>;

typedef int32_t i32x2 __attribute__((ext_vector_type(2)));
typedef int32_t i32x4 __attribute__((ext_vector_type(4)));

// two phases per thread and trip: one dwordx2 load, one dwordx4 store, so that every store instruction
// of a wave writes 1 KiB of whole lines (four phases per thread would split each line over two
// instructions: measured slower).  `vec` needs 16-byte aligned buffers.
__global__ __launch_bounds__(256) void cossin_kernel(const int32_t *phase, Cplx *out, size_t n, bool vec)
{
    __shared__ uint32_t lut[1 << kCossinDepth];
    fill_cossin(lut, threadIdx.x, 256);
    __syncthreads();
    const size_t stride = size_t(gridDim.x) * 256, t = size_t(blockIdx.x) * 256 + threadIdx.x;
    const size_t nv = vec ? n / 2 : 0;
    for (size_t i = t; i < nv; i += stride) {
        const i32x2 p = __builtin_nontemporal_load(reinterpret_cast<const i32x2 *>(phase) + i);
        const Cplx a = cossin_dev(p.x, lut), b = cossin_dev(p.y, lut);
        __builtin_nontemporal_store(i32x4{a.re, a.im, b.re, b.im}, reinterpret_cast<i32x4 *>(out) + i);
    }
    for (size_t i = nv * 2 + t; i < n; i += stride) out[i] = cossin_dev(phase[i], lut);
}

__global__ __launch_bounds__(256) void atan2_kernel(const Cplx *xy, int32_t *out, size_t n, bool vec)
{
    __shared__ uint32_t tab[32];
    if (threadIdx.x < 32) tab[threadIdx.x] = d_atan2_table[threadIdx.x];
    __syncthreads();
    const size_t stride = size_t(gridDim.x) * 256, t = size_t(blockIdx.x) * 256 + threadIdx.x;
    const size_t nv = vec ? n / 4 : 0;
    for (size_t i = t; i < nv; i += stride) {  // rows are [x, y] = [re, im]
        const i32x4 a = __builtin_nontemporal_load(reinterpret_cast<const i32x4 *>(xy) + 2 * i);
        const i32x4 b = __builtin_nontemporal_load(reinterpret_cast<const i32x4 *>(xy) + 2 * i + 1);
        const i32x4 r = {atan2_dev(a.y, a.x, tab), atan2_dev(a.w, a.z, tab), atan2_dev(b.y, b.x, tab), atan2_dev(b.w, b.z, tab)};
        __builtin_nontemporal_store(r, reinterpret_cast<i32x4 *>(out) + i);
    }
    for (size_t i = nv * 4 + t; i < n; i += stride) {
        const Cplx v = xy[i];
        out[i] = atan2_dev(v.im, v.re, tab);
    }
}

}  // namespace
}  // namespace idsp

using namespace idsp;

extern "C" {

int idsp_cossin_i32(const int32_t *phase, int32_t *out, size_t n, void *stream)
{
    if (n && (!phase || !out)) return fail(IDSP_EINVAL, "phase or out is NULL");
    if (n == 0) return IDSP_OK;
    const bool vec = (reinterpret_cast<uintptr_t>(phase) | reinterpret_cast<uintptr_t>(out)) % 16 == 0;
    size_t blocks = (n / (vec ? 2 : 1) + 255) / 256 + 1;
    if (blocks > 8192) blocks = 8192;
    note_kernel("cossin_kernel");
    hipLaunchKernelGGL(cossin_kernel, dim3(unsigned(blocks)), dim3(256), 0, as_stream(stream), phase,
                       reinterpret_cast<Cplx *>(out), n, vec);
    return launch_status();
}

int idsp_atan2_i32(const int32_t *xy, int32_t *out, size_t n, void *stream)
{
    if (n && (!xy || !out)) return fail(IDSP_EINVAL, "xy or out is NULL");
    if (n == 0) return IDSP_OK;
    const bool vec = (reinterpret_cast<uintptr_t>(xy) | reinterpret_cast<uintptr_t>(out)) % 16 == 0;
    size_t blocks = (n / (vec ? 4 : 1) + 255) / 256 + 1;
    if (blocks > 8192) blocks = 8192;
    note_kernel("atan2_kernel");
    hipLaunchKernelGGL(atan2_kernel, dim3(unsigned(blocks)), dim3(256), 0, as_stream(stream),
                       reinterpret_cast<const Cplx *>(xy), out, n, vec);
    return launch_status();
}

// plan_dds (readout_plan.h) says which processor, this runs it
int idsp_dds_i32(void *state, int32_t *out, size_t lanes, size_t frames, int layout, void *stream)
{
    if (layout != IDSP_FRAME_MAJOR && layout != IDSP_LANE_MAJOR) return fail(IDSP_EINVAL, "bad layout %d", layout);
    if (lanes && (!state || (frames && !out))) return fail(IDSP_EINVAL, "state or out is NULL");
    if (lanes == 0) return IDSP_OK;
    DdsCall call;
    call.lanes = lanes, call.frames = frames, call.layout = layout;
    const DdsPlan plan = plan_dds(call, dds_switches());
    const int32_t *const no_x = nullptr;
    const hipStream_t s = as_stream(stream);
    if (plan.circle) return launch_stream<DdsSplitProcT<true>>(DdsSplitProcT<true>::Params{0}, state, no_x, out, 2 * lanes, frames, layout, s);
    if (plan.split) return launch_stream<DdsSplitProc>(DdsSplitProc::Params{0}, state, no_x, out, 2 * lanes, frames, layout, s);
    return launch_stream<DdsProc>(DdsProc::Params{0}, state, no_x, reinterpret_cast<Cplx *>(out), lanes, frames, layout, s);
}

}  // extern "C"
