// lockin_phase.hip — the three lock-in entries with lowpass arms on the internal phase accumulator (reference: src/lockin.rs,
// src/lowpass.rs, src/accu.rs), idsp_lockin_state_words and idsp_lowpass_i32.  plan_lockin (lockin_plan.h) says which kernels a call
// takes; the kernels themselves are in lockin_waves_{iq,arg,norm_sqr}.hip, lockin_stream_{iq,arg,norm_sqr}.hip and lowpass.hip.
// No kernel is compiled here: this unit is host code only.
#include "dds_dev.h"

namespace idsp {

// lockin_waves_{iq,arg,norm_sqr}.hip: one lane's work spread over several waves, in the plan's form (lockin_waves.h; `plan.body` frames)
using LockinWavesFn = int(const idsp_lockin_i32 *cfg, void *state, const int32_t *x, void *y, size_t lanes, const LockinPlan &plan, hipStream_t s, size_t pitch);
LockinWavesFn lockin_waves_iq, lockin_waves_arg, lockin_waves_norm_sqr;

// lockin_stream_{iq,arg,norm_sqr}.hip, lowpass.hip: the stream processors behind the multi-wave kernels (lockin_stream_procs.h)
int lockin_stream_iq(const idsp_lockin_i32 *cfg, void *state, const int32_t *x, int32_t *y, size_t lanes, size_t frames, int layout, bool split, hipStream_t s,
                     size_t pitch = 0);
int lockin_stream_arg(const idsp_lockin_i32 *cfg, void *state, const int32_t *x, int32_t *y, size_t lanes, size_t frames, int layout, hipStream_t s, size_t pitch = 0);
int lockin_stream_norm_sqr(const idsp_lockin_i32 *cfg, void *state, const int32_t *x, int64_t *y, size_t lanes, size_t frames, int layout, hipStream_t s,
                           size_t pitch = 0);
int lowpass_stream(const idsp_lockin_i32 *cfg, void *state, const int32_t *x, int32_t *y, size_t lanes, size_t frames, int layout, hipStream_t s);

namespace {

// What tells the three phase-form entries with lowpass arms apart: the waves launcher, the elements of y per frame and the stream
// launcher (only `Complex<i32>` has a two-thread split)
constexpr LockinWavesFn *kPhaseWaves[3] = {lockin_waves_iq, lockin_waves_arg, lockin_waves_norm_sqr};  // [MODE_*]
template <int MODE, class Y>
int lockin_phase_stream(const idsp_lockin_i32 *cfg, void *state, const int32_t *x, Y *y, size_t lanes, size_t frames, int layout, bool split, hipStream_t s, size_t pitch)
{
    if constexpr (MODE == MODE_IQ)
        return lockin_stream_iq(cfg, state, x, y, lanes, frames, layout, split, s, pitch);
    else if constexpr (MODE == MODE_ARG)
        return lockin_stream_arg(cfg, state, x, y, lanes, frames, layout, s, pitch);
    else
        return lockin_stream_norm_sqr(cfg, state, x, y, lanes, frames, layout, s, pitch);
}

// idsp_lockin_i32_process / _arg / _norm_sqr: plan_lockin (lockin_plan.h) says which kernels, this runs them
template <int MODE, class Y>
int lockin_phase(const idsp_lockin_i32 *cfg, void *state, const int32_t *x, Y *y, size_t lanes, size_t frames, int layout, void *stream)
{
    int rc = lockin_cfg_check(cfg);
    if (rc) return rc;
    if ((rc = check_stream_args(cfg, 1, state, x, y, lanes, frames, layout))) return rc;
    if (lanes == 0) return IDSP_OK;
    const hipStream_t s = as_stream(stream);
    const LockinPlan plan = lockin_plan_for(LockinArms::Lowpass, LockinLo::Phase, MODE, cfg->order, cfg->cascade, x, y, lanes, frames, layout);
    if (plan.form == LockinForm::Stream) return lockin_phase_stream<MODE>(cfg, state, x, y, lanes, frames, layout, plan.split, s, 0);
    // WavesTail: the multi-wave kernel takes the whole batches of every LaneMajor row at the call's row pitch and a stream kernel the last
    // frames % 16 behind it (same stream; the state carries over as between two calls)
    const bool tail = plan.form == LockinForm::WavesTail;
    rc = kPhaseWaves[MODE](cfg, state, x, y, lanes, plan, s, tail ? frames : 0);
    if (rc || !tail) return rc;
    rc = lockin_phase_stream<MODE>(cfg, state, x + plan.body, y + (MODE == MODE_IQ ? 2 : 1) * plan.body, lanes, frames - plan.body, layout, false, s, frames);
    if (rc == IDSP_OK) note_kernel(lockin_plan_name(plan));
    return rc;
}

}  // namespace
}  // namespace idsp

using namespace idsp;

extern "C" {

size_t idsp_lockin_state_words(const idsp_lockin_i32 *cfg)
{
    if (lockin_cfg_check(cfg)) return 0;
    return size_t(2 + 2 * cfg->cascade * cfg->order * 2);
}

int idsp_lockin_i32_process(const idsp_lockin_i32 *cfg, void *state, const int32_t *x, int32_t *y, size_t lanes,
                            size_t frames, int layout, void *stream)
{
    return lockin_phase<MODE_IQ>(cfg, state, x, y, lanes, frames, layout, stream);
}

int idsp_lockin_i32_arg(const idsp_lockin_i32 *cfg, void *state, const int32_t *x, int32_t *y, size_t lanes, size_t frames,
                        int layout, void *stream)
{
    return lockin_phase<MODE_ARG>(cfg, state, x, y, lanes, frames, layout, stream);
}

int idsp_lockin_i32_norm_sqr(const idsp_lockin_i32 *cfg, void *state, const int32_t *x, int64_t *y, size_t lanes,
                             size_t frames, int layout, void *stream)
{
    return lockin_phase<MODE_NORM_SQR>(cfg, state, x, y, lanes, frames, layout, stream);
}

int idsp_lowpass_i32(const idsp_lockin_i32 *cfg, void *state, const int32_t *x, int32_t *y, size_t lanes,
                     size_t frames, int layout, void *stream)
{
    int rc = lockin_cfg_check(cfg);
    if (rc) return rc;
    if ((rc = check_stream_args(cfg, 1, state, x, y, lanes, frames, layout))) return rc;
    if (lanes == 0) return IDSP_OK;
    return lowpass_stream(cfg, state, x, y, lanes, frames, layout, as_stream(stream));
}

}  // extern "C"
