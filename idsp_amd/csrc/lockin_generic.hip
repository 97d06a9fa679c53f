// lockin_generic.hip — `Lockin<C>` as the reference defines it (src/lockin.rs:11-39): arm filters other than `[Lowpass<N>; K]`
// and the external-LO form `(x, Complex<U>) -> Complex<X>` (:17-27), on the one-thread-per-lane stream kernels of
// lane_stream.h.  (The phase form with lowpass arms — the C4 configuration — has its own multi-wave kernels, lockin_waves.h.)
//
//   idsp_lockin_i32_biquad_process      phase form, arms `[Biquad<Q32<F>>; n]` x `[DirectForm1<i32>; n]`
//   idsp_lockin_i32_lo_process          external LO, arms `[Lowpass<N>; K]`
//   idsp_lockin_i32_biquad_lo_process   external LO, biquad arms (i32)
//   idsp_lockin_f32_biquad_lo_process   external LO, `[Biquad<f32>; n]` arms: the mix -> lowpass graph of examples/ddc_lockin.rs
//
// External LO: the stream kernel carries the LO samples (8 bytes, like the 8-byte output); the 4-byte x sample of the
// same (frame, lane) is read by the processor itself in its pre-stage (four frames ahead of the recurrence), through a
// pointer that walks the lane's x samples.  The kernels split lanes only for 4-byte-in / 4-byte-out processors, so the
// lane index a processor sees here is the caller's.
#include "biquad_sections.h"
#include "dds_dev.h"

namespace idsp {

// lockin_waves_biquad.hip, lockin_waves_lo.hip: the multi-wave lock-in kernel with these arms, in the plan's form (`plan.body` frames)
int lockin_waves_biquad_iq(const idsp_biquad_i32 *sec, size_t n, void *state, const int32_t *x, int32_t *y, size_t lanes, const LockinPlan &plan, hipStream_t s,
                           size_t pitch);
int lockin_waves_biquad_lo(const idsp_biquad_i32 *sec, size_t n, void *state, const int32_t *x, const int32_t *lo, int32_t *y, size_t lanes,
                           const LockinPlan &plan, hipStream_t s, size_t pitch);
int lockin_waves_lowpass_lo(const idsp_lockin_i32 *cfg, void *state, const int32_t *x, const int32_t *lo, int32_t *y, size_t lanes, const LockinPlan &plan,
                            hipStream_t s, size_t pitch);
int lockin_waves_biquad_lo_f32(const idsp_biquad_f32 *sec, size_t n, void *state, const float *x, const float *lo, float *y, size_t lanes,
                               const LockinPlan &plan, hipStream_t s, size_t pitch);

namespace {

typedef int32_t cplx_i32 __attribute__((ext_vector_type(2)));
typedef float cplx_f32 __attribute__((ext_vector_type(2)));

// n serial sections on one arm, state words at `word0` (section-major, {x0,x1,y0,y1} each)
template <class Sec, int NS>
struct Arm : bq::SectionState<NS, Sec::W> {
    template <class P>
    __device__ __forceinline__ typename Sec::T step(const P &p, typename Sec::T x)
    {
#pragma unroll
        for (int k = 0; k < NS; k++) x = Sec::step(p.sec[k], this->s[k], x);
        return x;
    }
};

// phase form, biquad arms (src/lockin.rs:30-39 -> :17-27)
template <int NS>
struct LockinBiquadProc {
    using In = int32_t;
    using Out = Cplx;
    static constexpr bool HAS_IN = true;
    static constexpr int LDS_WORDS = 1 << kCossinDepth;
    static constexpr int IN_DIV = 1;
    static constexpr int COST = 110 + 100 * NS;
    using Params = bq::ChainParams<bq::SecI32, NS>;
    const uint32_t *lut;
    uint32_t acc, inc;
    Arm<bq::Df1I32<false>, NS> bi, bqarm;
    static __device__ __forceinline__ void fill_shared(uint32_t *sh, int tid, int n) { fill_cossin(sh, tid, n); }
    __device__ __forceinline__ void set_shared(const uint32_t *sh) { lut = sh; }
    __device__ __forceinline__ void load(const Params &, const uint32_t *st, size_t lanes, size_t lane)
    {
        acc = st[lane];
        inc = st[lanes + lane];
        bi.load(st, lanes, lane, 2);
        bqarm.load(st, lanes, lane, 2 + 4 * NS);
    }
    __device__ __forceinline__ void store(const Params &, uint32_t *st, size_t lanes, size_t lane)
    {
        st[lane] = acc;
        bi.store(st, lanes, lane, 2);
        bqarm.store(st, lanes, lane, 2 + 4 * NS);
    }
    static constexpr int BATCH = 4;
    using Pre = Cplx;
    __device__ __forceinline__ Pre pre(const Params &)
    {
        acc += inc;
        return cossin_dev(int32_t(acc), lut);
    }
    __device__ __forceinline__ Out step(const Params &p, In x, const Pre &lo)
    {
        return Cplx{bi.step(p, __mulhi(lo.re, x)), bqarm.step(p, __mulhi(lo.im, x))};
    }
};

// where the x samples of the external-LO forms are, beside the kernel's own (LO) input stream
struct XWalk {
    const void *x;
    uint32_t frame_major;
    size_t frames;
};

// external LO, lowpass arms
struct LpLoParams {
    LpParams lp;
    XWalk xw;
};
template <int N, int K>
struct LockinLoProc {
    using In = cplx_i32;
    using Out = Cplx;
    static constexpr bool HAS_IN = true;
    static constexpr int LDS_WORDS = 0;
    static constexpr int IN_DIV = 1;
    static constexpr int COST = 20 + 80 * N * K;
    using Params = LpLoParams;
    const int32_t *xp;
    size_t xstride;
    LpBank<N, K> bi, bq_;
    __device__ __forceinline__ void load(const Params &p, const uint32_t *st, size_t lanes, size_t lane)
    {
        xp = static_cast<const int32_t *>(p.xw.x) + (p.xw.frame_major ? lane : lane * p.xw.frames);
        xstride = p.xw.frame_major ? lanes : 1;
        bi.load(st, lanes, lane, 0);
        bq_.load(st, lanes, lane, 2 * N * K);
    }
    __device__ __forceinline__ void store(const Params &, uint32_t *st, size_t lanes, size_t lane)
    {
        bi.store(st, lanes, lane, 0);
        bq_.store(st, lanes, lane, 2 * N * K);
    }
    static constexpr int BATCH = 4;
    using Pre = int32_t;  // the x sample of the frame
    __device__ __forceinline__ Pre pre(const Params &)
    {
        const int32_t v = *xp;
        xp += xstride;
        return v;
    }
    __device__ __forceinline__ Out step(const Params &p, In lo, const Pre &x)
    {
        return Cplx{bi.step(p.lp, __mulhi(lo.x, x)), bq_.step(p.lp, __mulhi(lo.y, x))};
    }
};

// external LO, biquad arms; T = int32_t (Q32<32> LO) or float
template <class Sec, int NS>
struct BqLoParams {
    typename Sec::Sec sec[NS];
    XWalk xw;
};
template <class Sec, int NS>
struct LockinBiquadLoProc {
    using T = typename Sec::T;
    typedef T In __attribute__((ext_vector_type(2)));
    typedef T Out __attribute__((ext_vector_type(2)));
    static constexpr bool HAS_IN = true;
    static constexpr int LDS_WORDS = 0;
    static constexpr int IN_DIV = 1;
    static constexpr int COST = 20 + 2 * NS * Sec::COST;
    // 2 x NS sections of state beside a deep register window or the staged kernel's staging registers spill (tools/check_scratch.py)
    static constexpr int MAX_U = NS >= 3 ? 8 : 24;
    static constexpr bool LM_STAGED = NS <= 2;
    using Params = BqLoParams<Sec, NS>;
    const T *xp;
    size_t xstride;
    Arm<Sec, NS> bi, bq_;
    __device__ __forceinline__ void load(const Params &p, const uint32_t *st, size_t lanes, size_t lane)
    {
        xp = static_cast<const T *>(p.xw.x) + (p.xw.frame_major ? lane : lane * p.xw.frames);
        xstride = p.xw.frame_major ? lanes : 1;
        bi.load(st, lanes, lane, 0);
        bq_.load(st, lanes, lane, 4 * NS);
    }
    __device__ __forceinline__ void store(const Params &, uint32_t *st, size_t lanes, size_t lane)
    {
        bi.store(st, lanes, lane, 0);
        bq_.store(st, lanes, lane, 4 * NS);
    }
    static constexpr int BATCH = 4;
    using Pre = T;
    __device__ __forceinline__ Pre pre(const Params &)
    {
        const T v = *xp;
        xp += xstride;
        return v;
    }
    static __device__ __forceinline__ int32_t mix(int32_t x, int32_t lo) { return __mulhi(lo, x); }
    static __device__ __forceinline__ float mix(float x, float lo) { return x * lo; }
    __device__ __forceinline__ Out step(const Params &p, In lo, const Pre &x)
    {
        return Out{bi.step(p, mix(x, lo.x)), bq_.step(p, mix(x, lo.y))};
    }
};

bool sections_ok(const void *sections, size_t n) { return sections && n >= 1 && n <= IDSP_LOCKIN_MAX_SECTIONS; }

int check_lo_args(const void *cfg, const void *state, const void *x, const void *lo, const void *y, size_t lanes, size_t frames, int layout)
{
    int rc = check_stream_args(cfg, 1, state, x, y, lanes, frames, layout);
    if (rc) return rc;
    if (lanes && frames && !lo) return fail(IDSP_EINVAL, "lo is NULL");
    // lo and y hold `Complex` pairs and are read / written 8 bytes at a time (i32x2 in lockin_waves.h, cplx_i32 / cplx_f32 in the stream
    // processors): an address that is only 4-byte aligned is legal by the C signature but would rely on the unaligned-access mode
    if (reinterpret_cast<uintptr_t>(lo) % 8 || reinterpret_cast<uintptr_t>(y) % 8)
        return fail(IDSP_EINVAL, "lo and y hold Complex pairs: both must be 8-byte aligned");
    // three separate buffers (include/idsp_hip.h): x is walked by a side pointer while lo streams through the kernel, no in-place form
    const size_t xb = span_bytes(lanes, frames, 4), cb = span_bytes(lanes, frames, 8);
    if (ranges_overlap(x, xb, y, cb) || ranges_overlap(lo, cb, y, cb) || ranges_overlap(x, xb, lo, cb)) return fail(IDSP_EINVAL, "x, lo and y must not overlap");
    return IDSP_OK;
}

inline XWalk x_walk(const void *x, int layout, size_t frames, size_t pitch) { return XWalk{x, layout == IDSP_FRAME_MAJOR ? 1u : 0u, pitch ? pitch : frames}; }

template <int NS>
int run_biquad_phase(const idsp_biquad_i32 *sec, void *state, const int32_t *x, int32_t *y, size_t lanes, size_t frames, int layout, hipStream_t s, size_t pitch)
{
    typename LockinBiquadProc<NS>::Params p;
    bq::fill_sections(bq::Fill{sec}, p.sec);
    return launch_stream<LockinBiquadProc<NS>>(p, state, x, reinterpret_cast<Cplx *>(y), lanes, frames, layout, s, Pitch{pitch, pitch});
}
// Sec = Df1I32<false> with Fill<idsp_biquad_i32> and T = int32_t, or Df1F32<false> with Fill<idsp_biquad_f32> and T = float
template <class Sec, int NS, class Fill, class T>
int run_biquad_lo(const Fill &fill, void *state, const T *x, const T *lo, T *y, size_t lanes, size_t frames, int layout, hipStream_t s, size_t pitch)
{
    using P = LockinBiquadLoProc<Sec, NS>;
    typename P::Params p;
    bq::fill_sections(fill, p.sec);
    p.xw = x_walk(x, layout, frames, pitch);
    return launch_stream<P>(p, state, reinterpret_cast<const typename P::In *>(lo), reinterpret_cast<typename P::Out *>(y), lanes, frames, layout, s,
                            Pitch{pitch, pitch});
}

// The three external-LO entries behind their checks.  `waves(plan, pitch)` runs the multi-wave kernel on `plan.body` frames,
// `stream(x, lo, y, frames, pitch)` the stream kernel — on the whole call, or on the last frames % 16 of every LaneMajor row at the
// call's row pitch (same stream; its launch leaves its own name in idsp_last_kernel()).
template <class T, class Waves, class Stream>
int lockin_lo(LockinArms arms, int order, int cascade, const T *x, const T *lo, T *y, size_t lanes, size_t frames, int layout, Waves waves, Stream stream)
{
    const LockinPlan plan = lockin_plan_for(arms, LockinLo::Buffer, MODE_IQ, order, cascade, x, y, lanes, frames, layout);
    size_t pitch = 0;
    if (plan.form != LockinForm::Stream) {
        const bool tail = plan.form == LockinForm::WavesTail;
        const int rc = waves(plan, tail ? frames : 0);
        if (rc || !tail) return rc;
        pitch = frames, x += plan.body, lo += 2 * plan.body, y += 2 * plan.body, frames -= plan.body;
    }
    return stream(x, lo, y, frames, pitch);
}

template <class Sec, class Fill, class S, class T, class Waves>
int lockin_biquad_lo(Waves waves, const S *sections, size_t n, void *state, const T *x, const T *lo, T *y, size_t lanes, size_t frames, int layout, void *stream)
{
    const hipStream_t s = as_stream(stream);
    return lockin_lo(
        LockinArms::Biquad, 0, 0, x, lo, y, lanes, frames, layout,
        [&](const LockinPlan &plan, size_t pitch) { return waves(sections, n, state, x, lo, y, lanes, plan, s, pitch); },
        [&](const T *xs, const T *los, T *ys, size_t fr, size_t pitch) {
            return for_sections(n, [&](auto ns) { return run_biquad_lo<Sec, decltype(ns)::value>(Fill{sections}, state, xs, los, ys, lanes, fr, layout, s, pitch); });
        });
}

}  // namespace
}  // namespace idsp

using namespace idsp;

extern "C" {

size_t idsp_lockin_biquad_state_words(size_t n, int with_accu)
{
    return n >= 1 && n <= IDSP_LOCKIN_MAX_SECTIONS ? size_t(with_accu ? 2 : 0) + 8 * n : 0;
}

int idsp_lockin_i32_biquad_process(const idsp_biquad_i32 *sections, size_t n, void *state, const int32_t *x, int32_t *y, size_t lanes,
                                   size_t frames, int layout, void *stream)
{
    if (!sections_ok(sections, n)) return fail(IDSP_EINVAL, "sections is NULL or n = %zu not in 1..%d", n, IDSP_LOCKIN_MAX_SECTIONS);
    int rc = check_stream_args(sections, 1, state, x, y, lanes, frames, layout);
    if (rc) return rc;
    for (size_t k = 0; k < n; k++)
        if (sections[k].frac < 0 || sections[k].frac > 31) return fail(IDSP_EINVAL, "section %zu: frac = %d not in 0..31", k, sections[k].frac);
    if (lanes == 0 || frames == 0) return IDSP_OK;
    const hipStream_t s = as_stream(stream);
    const auto on_stream = [&](const int32_t *xs, int32_t *ys, size_t fr, size_t pitch) {
        return for_sections(n, [&](auto ns) { return run_biquad_phase<decltype(ns)::value>(sections, state, xs, ys, lanes, fr, layout, s, pitch); });
    };
    const LockinPlan plan = lockin_plan_for(LockinArms::Biquad, LockinLo::Phase, MODE_IQ, 0, 0, x, y, lanes, frames, layout);
    if (plan.form == LockinForm::Stream) return on_stream(x, y, frames, 0);
    // WavesTail: the whole batches of every LaneMajor row on the multi-wave kernel at the call's row pitch, the last frames % 16 on the
    // stream kernel behind it (as for the lowpass arms, lockin_phase.hip)
    const bool tail = plan.form == LockinForm::WavesTail;
    rc = lockin_waves_biquad_iq(sections, n, state, x, y, lanes, plan, s, tail ? frames : 0);
    if (rc || !tail) return rc;
    rc = on_stream(x + plan.body, y + 2 * plan.body, frames - plan.body, frames);
    if (rc == IDSP_OK) note_kernel(lockin_plan_name(plan), "[Biquad; n]");
    return rc;
}

int idsp_lockin_i32_lo_process(const idsp_lockin_i32 *cfg, void *state, const int32_t *x, const int32_t *lo, int32_t *y, size_t lanes,
                               size_t frames, int layout, void *stream)
{
    int rc = lockin_cfg_check(cfg);
    if (rc) return rc;
    if ((rc = check_lo_args(cfg, state, x, lo, y, lanes, frames, layout))) return rc;
    if (lanes == 0 || frames == 0) return IDSP_OK;
    const hipStream_t s = as_stream(stream);
    return lockin_lo(
        LockinArms::Lowpass, cfg->order, cfg->cascade, x, lo, y, lanes, frames, layout,
        [&](const LockinPlan &plan, size_t pitch) { return lockin_waves_lowpass_lo(cfg, state, x, lo, y, lanes, plan, s, pitch); },
        [&](const int32_t *xs, const int32_t *los, int32_t *ys, size_t fr, size_t pitch) {
            const LpLoParams p{lp_params(cfg), x_walk(xs, layout, fr, pitch)};
            return for_nk(cfg, [&](auto nn, auto k) {
                return launch_stream<LockinLoProc<decltype(nn)::value, decltype(k)::value>>(p, state, reinterpret_cast<const cplx_i32 *>(los), reinterpret_cast<Cplx *>(ys),
                                                                                           lanes, fr, layout, s, Pitch{pitch, pitch});
            });
        });
}

int idsp_lockin_i32_biquad_lo_process(const idsp_biquad_i32 *sections, size_t n, void *state, const int32_t *x, const int32_t *lo, int32_t *y,
                                      size_t lanes, size_t frames, int layout, void *stream)
{
    if (!sections_ok(sections, n)) return fail(IDSP_EINVAL, "sections is NULL or n = %zu not in 1..%d", n, IDSP_LOCKIN_MAX_SECTIONS);
    int rc = check_lo_args(sections, state, x, lo, y, lanes, frames, layout);
    if (rc) return rc;
    for (size_t k = 0; k < n; k++)
        if (sections[k].frac < 0 || sections[k].frac > 31) return fail(IDSP_EINVAL, "section %zu: frac = %d not in 0..31", k, sections[k].frac);
    if (lanes == 0 || frames == 0) return IDSP_OK;
    return lockin_biquad_lo<bq::Df1I32<false>, bq::Fill<idsp_biquad_i32>>(lockin_waves_biquad_lo, sections, n, state, x, lo, y, lanes, frames, layout, stream);
}

int idsp_lockin_f32_biquad_lo_process(const idsp_biquad_f32 *sections, size_t n, void *state, const float *x, const float *lo, float *y,
                                      size_t lanes, size_t frames, int layout, void *stream)
{
    if (!sections_ok(sections, n)) return fail(IDSP_EINVAL, "sections is NULL or n = %zu not in 1..%d", n, IDSP_LOCKIN_MAX_SECTIONS);
    int rc = check_lo_args(sections, state, x, lo, y, lanes, frames, layout);
    if (rc) return rc;
    if (lanes == 0 || frames == 0) return IDSP_OK;
    return lockin_biquad_lo<bq::Df1F32<false>, bq::Fill<idsp_biquad_f32>>(lockin_waves_biquad_lo_f32, sections, n, state, x, lo, y, lanes, frames, layout, stream);
}

}  // extern "C"
