// biquad_host.h — the host side of the biquad entry points (biquad_*.hip, cascade*.hip, normal.hip): argument checks, the passes of
// a long chain and their launches.  Which sections go into which launch is biquad_pass_plan.h's `next_pass`; what stands here does
// what it says.  The device code — sections and processors — is biquad_sections.h.
#pragma once

#include "biquad_pass_plan.h"
#include "biquad_sections.h"

namespace idsp {
namespace bq {

// Row pitches of the `_pitch` entry points (include/idsp_hip.h): elements between the starts of consecutive lanes
// (LANE_MAJOR) or consecutive frames (FRAME_MAJOR); 0 = dense.  A pitch must cover a row, and an in-place call must
// use the same pitch on both sides.
inline int check_pitch(const void *x, const void *y, size_t lanes, size_t frames, int layout, Pitch pitch)
{
    const size_t row = layout == IDSP_LANE_MAJOR ? frames : lanes;
    if ((pitch.x && pitch.x < row) || (pitch.y && pitch.y < row))
        return fail(IDSP_EINVAL, "pitch (%zu, %zu) shorter than a row of %zu elements", pitch.x, pitch.y, row);
    if (x == y && (pitch.x ? pitch.x : row) != (pitch.y ? pitch.y : row))
        return fail(IDSP_EINVAL, "in-place call with different x and y pitches (%zu, %zu)", pitch.x, pitch.y);
    return IDSP_OK;
}

template <class T>
int copy_through(const T *x, T *y, size_t lanes, size_t frames, int layout, hipStream_t s, Pitch pitch)
{
    if (x == y) return IDSP_OK;
    const size_t row = layout == IDSP_LANE_MAJOR ? frames : lanes, rows = layout == IDSP_LANE_MAJOR ? lanes : frames;
    const size_t xp = pitch.x ? pitch.x : row, yp = pitch.y ? pitch.y : row;
    IDSP_HIP_TRY(hipMemcpy2DAsync(y, yp * sizeof(T), x, xp * sizeof(T), row * sizeof(T), rows, hipMemcpyDeviceToDevice, s));
    return IDSP_OK;
}

inline int check_frac(int frac, size_t k)
{
    // `const { assert!(F >= 0 && F < 32) }` biquad.rs:448-450,513-515
    if (frac < 0 || frac > 31) return fail(IDSP_EINVAL, "section %zu: frac = %d not in 0..31", k, frac);
    return IDSP_OK;
}

// n sections in the passes of `rules`: the first pass reads x, later passes run in place on y — literally the reference's slice
// composition.  `launch(first, pass, src, pitch)` runs sections first .. first + pass.na + pass.nb - 1 from src into y.
template <class T, class Launch>
int run_passes(const PassRules &rules, size_t n, const T *x, T *y, size_t lanes, size_t frames, int layout, hipStream_t s, Pitch pitch, Launch launch)
{
    if (lanes == 0 || frames == 0) return IDSP_OK;
    if (n == 0) return copy_through<T>(x, y, lanes, frames, layout, s, pitch);  // empty slice: y.copy_from_slice(x), compose.rs:63-65
    const T *src = x;
    for (size_t done = 0; done < n;) {
        const Pass p = next_pass(rules, n - done, lanes, layout, stream_switches());
        if (int rc = launch(done, p, src, pitch)) return rc;
        done += size_t(p.na + p.nb);
        src = y;
        pitch.x = pitch.y;
    }
    return IDSP_OK;
}

// ------------------------------------------------------------ Chain
// Sections first .. first + NA + NB - 1 in one launch.  NB != 0: on the two-wave kernel, wave 0 runs Chain<Sec, NA>, wave 1
// Chain<Sec, NB> one tile behind
template <class Sec, int NA, int NB, class CfgFill>
int launch_chain(CfgFill fill, size_t first, void *state, const typename Sec::T *x, typename Sec::T *y, size_t lanes, size_t frames, int layout,
                 hipStream_t s, Pitch pitch)
{
    typename Chain<Sec, NA>::Params pa;
    for (int k = 0; k < NA; k++) fill(pa.sec[k], first + k);
    uint32_t *st = static_cast<uint32_t *>(state) + first * Sec::W * lanes;
    if constexpr (NB == 0) {
        return launch_stream<Chain<Sec, NA>>(pa, st, x, y, lanes, frames, layout, s, pitch);
    } else {
        typename Chain<Sec, NB>::Params pb;
        for (int k = 0; k < NB; k++) fill(pb.sec[k], first + NA + k);
        return launch_duo<Chain<Sec, NA>, Chain<Sec, NB>>(pa, pb, st, st + size_t(NA) * Sec::W * lanes, x, y, lanes, frames, s, pitch);
    }
}

template <class Sec, class CfgFill>
int run_chain(CfgFill fill, size_t n, void *state, const typename Sec::T *x, typename Sec::T *y, size_t lanes, size_t frames, int layout, hipStream_t s,
              Pitch pitch = {})
{
    using T = typename Sec::T;
    static constexpr PassRules rules = chain_rules(sizeof(T), Sec::kClamp, Sec::W);
    return run_passes(rules, n, x, y, lanes, frames, layout, s, pitch, [&](size_t first, Pass p, const T *src, Pitch pt) {
#define IDSP_GO(NA, NB) return launch_chain<Sec, NA, NB>(fill, first, state, src, y, lanes, frames, layout, s, pt)
        if constexpr (rules.max_duo != 0)
            switch (p.nb ? p.na + p.nb : 0) {
                case 0: break;
                case 4: IDSP_GO(2, 2);
                case 5: IDSP_GO(3, 2);
                case 6: IDSP_GO(3, 3);
                case 7: IDSP_GO(4, 3);
                default: IDSP_GO(4, 4);
            }
        switch (p.na) {
            case 1: IDSP_GO(1, 0);
            case 2: IDSP_GO(2, 0);
            case 3: IDSP_GO(3, 0);
            default: IDSP_GO(4, 0);
        }
#undef IDSP_GO
    });
}

// `check_frac` exactly when the config type has a `frac`
template <class Sec, class Cfg, class CfgFill>
int entry_chain(const Cfg *cfg, size_t n, void *state, const typename Sec::T *x, typename Sec::T *y, size_t lanes, size_t frames, int layout, void *stream,
                Pitch pitch = {})
{
    int rc = check_stream_args(cfg, n, state, x, y, lanes, frames, layout);
    if (rc) return rc;
    if ((rc = check_pitch(x, y, lanes, frames, layout, pitch))) return rc;
    if constexpr (HasFrac<Cfg>::value)
        for (size_t k = 0; k < n; k++)
            if ((rc = check_frac(cfg[k].frac, k))) return rc;
    return run_chain<Sec>(CfgFill{cfg}, n, state, x, y, lanes, frames, layout, as_stream(stream), pitch);
}

// ------------------------------------------------------------ ChainByLane
// The same for per-lane sections: coefficient and state planes of section `first` (of the second wave: NA sections further into the records)
template <class Sec, int NA, int NB>
int launch_bylane(const void *coef, int frac, size_t first, void *state, const typename Sec::T *x, typename Sec::T *y, size_t lanes, size_t frames, int layout,
                  hipStream_t s, Pitch pitch)
{
    using T = typename Sec::T;
    constexpr int CV = ChainByLane<Sec, 1>::CV;
    const ByLaneParams pa{static_cast<const T *>(coef) + first * CV * lanes, frac};
    uint32_t *sa = static_cast<uint32_t *>(state) + first * Sec::W * lanes;
    if constexpr (NB == 0) {
        return launch_stream<ChainByLane<Sec, NA>>(pa, sa, x, y, lanes, frames, layout, s, pitch);
    } else {
        const ByLaneParams pb{static_cast<const T *>(coef) + (first + NA) * CV * lanes, frac};
        return launch_duo<ChainByLane<Sec, NA>, ChainByLane<Sec, NB>>(pa, pb, sa, sa + size_t(NA) * Sec::W * lanes, x, y, lanes, frames, s, pitch);
    }
}

template <class Sec>
int run_chain_bylane(const void *coef, int frac, size_t n, void *state, const typename Sec::T *x, typename Sec::T *y, size_t lanes, size_t frames, int layout,
                     hipStream_t s, Pitch pitch = {})
{
    using T = typename Sec::T;
    static constexpr PassRules rules = bylane_rules(sizeof(T));
    return run_passes(rules, n, x, y, lanes, frames, layout, s, pitch, [&](size_t first, Pass p, const T *src, Pitch pt) {
#define IDSP_GO(NA, NB) return launch_bylane<Sec, NA, NB>(coef, frac, first, state, src, y, lanes, frames, layout, s, pt)
        if constexpr (rules.max_duo != 0) {
            if (p.nb == 1) IDSP_GO(2, 1);
            if (p.nb == 2) IDSP_GO(2, 2);
        }
        if (p.na == 1) IDSP_GO(1, 0);
        IDSP_GO(2, 0);
#undef IDSP_GO
    });
}

template <class Sec>
int entry_bylane(const void *coef, int frac, size_t n, void *state, const typename Sec::T *x, typename Sec::T *y,
                 size_t lanes, size_t frames, int layout, void *stream, Pitch pitch = {})
{
    int rc = check_stream_args(coef, n, state, x, y, lanes, frames, layout);
    if (rc) return rc;
    if ((rc = check_pitch(x, y, lanes, frames, layout, pitch))) return rc;
    if (std::is_same<typename Sec::T, int32_t>::value && (rc = check_frac(frac, 0))) return rc;
    return run_chain_bylane<Sec>(coef, frac, n, state, x, y, lanes, frames, layout, as_stream(stream), pitch);
}

// ------------------------------------------------------------ CascadeDf1
// `Cascade` of NA + NB sections.  On the two-wave kernel section k's input history is section k - 1's output history, so wave 1 is
// the same processor type started 2 NA values into the state record: its "x history" is y[NA - 1]'s, which it keeps up to date
// from the samples wave 0 hands over (both waves write that pair back: the same values).
template <class T, int NA, int NB, class CfgFill>
int launch_cascade(CfgFill fill, void *state, const T *x, T *y, size_t lanes, size_t frames, int layout, hipStream_t s, Pitch pitch)
{
    typename CascadeDf1<T, NA>::Params pa;
    for (int k = 0; k < NA; k++) fill(pa.sec[k], size_t(k));
    if constexpr (NB == 0) {
        return launch_stream<CascadeDf1<T, NA>>(pa, state, x, y, lanes, frames, layout, s, pitch);
    } else {
        typename CascadeDf1<T, NB>::Params pb;
        for (int k = 0; k < NB; k++) fill(pb.sec[k], size_t(NA + k));
        uint32_t *st = static_cast<uint32_t *>(state);
        return launch_duo<CascadeDf1<T, NA>, CascadeDf1<T, NB>>(pa, pb, st, st + size_t(2 * NA) * (sizeof(T) / 4) * lanes, x, y, lanes, frames, s, pitch);
    }
}

// one launch whatever the length: a single "pass" of all n sections
template <class T, class CfgFill>
int run_cascade(CfgFill fill, size_t n, void *state, const T *x, T *y, size_t lanes, size_t frames, int layout, hipStream_t s, Pitch pitch = {})
{
    if (int rc = check_pitch(x, y, lanes, frames, layout, pitch)) return rc;
    if (n < 1 || n > size_t(kMaxCascade)) return fail(IDSP_EINVAL, "cascade sections n = %zu not in 1..%d", n, kMaxCascade);
    if (lanes == 0 || frames == 0) return IDSP_OK;
    static constexpr PassRules rules = cascade_rules(sizeof(T));
    const Pass p = next_pass(rules, n, lanes, layout, stream_switches());
#define IDSP_GO(NA, NB) return launch_cascade<T, NA, NB>(fill, state, x, y, lanes, frames, layout, s, pitch)
    if constexpr (rules.max_duo != 0)
        switch (p.nb ? p.na + p.nb : 0) {
            case 0: break;
            case 5: IDSP_GO(3, 2);
            case 6: IDSP_GO(3, 3);
            case 7: IDSP_GO(4, 3);
            default: IDSP_GO(4, 4);
        }
    switch (p.na) {
        case 1: IDSP_GO(1, 0);
        case 2: IDSP_GO(2, 0);
        case 3: IDSP_GO(3, 0);
        case 4: IDSP_GO(4, 0);
        case 5: IDSP_GO(5, 0);
        case 6: IDSP_GO(6, 0);
        case 7: IDSP_GO(7, 0);
        default: IDSP_GO(8, 0);
    }
#undef IDSP_GO
}

}  // namespace bq
}  // namespace idsp

// `<entry>_pitch` twin of a shared-coefficient entry point (include/idsp_hip.h): same call with explicit row pitches.
#define IDSP_PITCH_TWIN(name, Cfg, T, ENTRY, ...)                                                                      \
    int name##_pitch(const Cfg *cfg, size_t n, void *state, const T *x, size_t x_pitch, T *y, size_t y_pitch,          \
                     size_t lanes, size_t frames, int layout, void *stream)                                            \
    {                                                                                                                  \
        return ENTRY<__VA_ARGS__>(cfg, n, state, x, y, lanes, frames, layout, stream, ::idsp::Pitch{x_pitch, y_pitch}); \
    }
