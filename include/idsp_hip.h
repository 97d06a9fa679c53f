/*
 * idsp_hip.h — C ABI of libidsp_hip.so, the MI355X (gfx950) bulk engine for the
 * per-sample filter hot path of quartiq/idsp.
 *
 * This header is the drop-in boundary: every entry point replaces one
 * `dsp_process::{SplitProcess::block, SplitInplace::inplace,
 * SplitViewProcess::process_view}` call of the reference, executed for many
 * independent lanes at once.  Citations are `path:line` inside the reference
 * tree (idsp 0.22.0).  A Rust `extern "C"` block binding these symbols is shown
 * in INTEGRATION.md.
 *
 * Conventions common to all processing entry points
 * --------------------------------------------------
 *  - plain C types only; `x`, `y`, `state` are DEVICE pointers owned by the
 *    caller; `stream` is a `hipStream_t` passed as `void*` (NULL = default
 *    stream).  Calls are asynchronous on that stream.
 *  - the library never allocates hidden memory and keeps no mutable globals
 *    apart from the thread-local last-error string.
 *  - `lanes`  = number of independent channels (reference: const generic `N` of
 *    `Lanes<C>` / `[S; N]`, dsp-process/src/compose.rs:449-513).
 *    `frames` = samples per lane in this call (reference: slice length).
 *  - `layout` selects the two memory layouts of dsp-process/src/view.rs:10-17:
 *      IDSP_FRAME_MAJOR  `[[T; lanes]; frames]`  element (f, l) at `f*lanes + l`
 *      IDSP_LANE_MAJOR   `lanes` contiguous slices, element (f, l) at `l*frames + f`
 *    (view.rs:190-195 `lane(i) = flat[i*frames..]`).
 *  - `y == x` (in-place, reference `inplace()`) is allowed for all same-rate
 *    operators; partial overlap is not.
 *  - `state` is read at entry and written back at exit, so consecutive calls
 *    continue the stream exactly as consecutive `block()` calls do in the
 *    reference.  A zero-filled state is the reference's `Default::default()`.
 *    The reference state structs carry no `repr(C)` (src/iir/biquad.rs:258-269),
 *    so this ABI fixes its own record: a state is a sequence of 32-bit words per
 *    lane, stored WORD-PLANE-MAJOR on the device for coalescing:
 *        word w of lane l  ->  ((uint32_t*)state)[w * lanes + l]
 *    64-bit fields occupy two consecutive words (low word first).  The word
 *    lists are given with each operator below; idsp_*_state_words() return the
 *    counts.
 *  - return value: IDSP_OK (0) or a negative idsp_status.  Shape / parameter
 *    violations that are `debug_assert!`/`const assert!` in the reference
 *    (dsp-process/src/process.rs:42-45, src/iir/biquad.rs:448-450) are reported
 *    as IDSP_EINVAL; the library never aborts.  idsp_last_error() returns a
 *    thread-local description of the most recent failure.
 */
#ifndef IDSP_HIP_H
#define IDSP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 1: round-1 surface.  2: + the `_pitch` twins, idsp_multi_*, idsp_last_kernel, idsp_device_sync,
 * idsp_multi_last_block; dispatch switches honoured only with IDSP_DIAG=1.  3: + `Lockin<C>` with biquad arms and
 * the external-LO forms (idsp_lockin_*_biquad*, *_lo_*), the f64 half-band / FIR entries.  4: + idsp_device_copy.
 * Versions only ADD symbols:
 * a host binding refuses a library whose idsp_version() is LOWER than the version it was generated from and accepts
 * any higher one (the rule of idsp_amd/_lib.py, __graft_entry__.py and rust/idsp-hip). */
#define IDSP_ABI_VERSION 4

typedef enum idsp_status {
    IDSP_OK = 0,
    IDSP_EINVAL = -1,  /* bad shape / parameter (reference: debug_assert / const assert) */
    IDSP_EHIP = -2,    /* HIP runtime error, text in idsp_last_error() */
    IDSP_ENODEV = -3,  /* no usable gfx950 device */
    /* builder parameter validation, `iir::Error` (src/iir/error.rs:5-16); idsp_last_error()
     * holds the reference's Display text, e.g. "parameter `frequency` is out of range" */
    IDSP_ENONFINITE = -10,   /* Error::NonFinite     */
    IDSP_ENONPOSITIVE = -11, /* Error::NonPositive   */
    IDSP_EOUTOFRANGE = -12,  /* Error::OutOfRange    */
    IDSP_EINVERTED = -13,    /* Error::InvertedRange */
    IDSP_ESIGN = -14         /* Error::SignMismatch  */
} idsp_status;

typedef enum idsp_layout {
    IDSP_FRAME_MAJOR = 0, /* dsp-process/src/view.rs:10  */
    IDSP_LANE_MAJOR = 1   /* dsp-process/src/view.rs:17  */
} idsp_layout;

/* Maximum number of serial sections accepted per call (slice composition
 * `[C] x [S]`, dsp-process/src/compose.rs:43-77). */
#define IDSP_MAX_SECTIONS 64

/* ------------------------------------------------------------------------ */
/* library / device utilities                                               */
/* ------------------------------------------------------------------------ */

/* IDSP_ABI_VERSION the library was built with. */
int idsp_version(void);
/* Thread-local text of the last error returned on this thread ("" if none). */
const char *idsp_last_error(void);
/* Diagnostic: thread-local name of the kernel (and processor instantiation) the most recent processing call
 * of this thread dispatched to, e.g. "stream_frame_major_lds<idsp::bq::Chain<idsp::bq::Df1I32<false>, 1>>";
 * "" before the first launch.  Multi-pass calls report their last pass. */
const char *idsp_last_kernel(void);
/* Number of visible HIP devices, or a negative idsp_status. */
int idsp_device_count(void);
/* Select the device used by subsequent calls of this thread. */
int idsp_device_set(int device);
/* Plain device-memory helpers so a host language without a HIP binding (the
 * Rust shim, ctypes) can own buffers.  Not used on the hot path. */
int idsp_device_alloc(void **ptr, size_t bytes);
int idsp_device_free(void *ptr);
int idsp_device_memset(void *ptr, int value, size_t bytes, void *stream);
int idsp_device_h2d(void *dst_dev, const void *src_host, size_t bytes, void *stream);
int idsp_device_d2h(void *dst_host, const void *src_dev, size_t bytes, void *stream);
/* Device-to-device copy of non-overlapping buffers by a streaming kernel (16 bytes per thread, nontemporal, one contiguous
 * chunk per workgroup), asynchronous on `stream`: `copy_from_slice` for a host that owns device buffers, and the yardstick
 * bench.py prints beside the filter kernels (`copy_gbs`: what a plain copy of the same footprint reaches on this box in the
 * same run).  Any alignment and size; the bulk moves 16-byte aligned when dst and src are congruent mod 16. */
int idsp_device_copy(void *dst_dev, const void *src_dev, size_t bytes, void *stream);
int idsp_stream_sync(void *stream);
/* Wait for ALL work of the current device, whatever stream it was launched on (hipDeviceSynchronize) — what a
 * host must call before reading results back on another stream than the one it launched on: the idsp_multi
 * streams are non-blocking, so a NULL-stream copy does NOT wait for them. */
int idsp_device_sync(void);

/* ------------------------------------------------------------------------ */
/* iir::Biquad — fixed point (src/iir/biquad.rs)                            */
/* ------------------------------------------------------------------------ */

/* `Biquad<Q32<F>>` (src/iir/biquad.rs:96-116): ba = [b0,b1,b2,a1,a2] raw Q bits
 * with a1,a2 stored exactly as used in the recurrence; frac = F, 0 <= F < 32. */
typedef struct idsp_biquad_i32 {
    int32_t ba[5];
    int32_t frac;
} idsp_biquad_i32;

/* `BiquadClamp<Q32<F>, i32>` (src/iir/biquad.rs:121-157). */
typedef struct idsp_biquad_clamp_i32 {
    int32_t ba[5];
    int32_t frac;
    int32_t u;   /* summing junction offset */
    int32_t min; /* lower limit */
    int32_t max; /* upper limit */
} idsp_biquad_clamp_i32;

/* `Biquad<f32>`. */
typedef struct idsp_biquad_f32 {
    float ba[5];
} idsp_biquad_f32;

/* `BiquadClamp<f32, f32>`. */
typedef struct idsp_biquad_clamp_f32 {
    float ba[5];
    float u;
    float min;
    float max;
} idsp_biquad_clamp_f32;

/* `Biquad<f64>` / `BiquadClamp<f64, f64>` (the generic impl of src/iir/biquad.rs:366-440 with
 * C = T = A = f64). */
typedef struct idsp_biquad_f64 {
    double ba[5];
} idsp_biquad_f64;

typedef struct idsp_biquad_clamp_f64 {
    double ba[5];
    double u;
    double min;
    double max;
} idsp_biquad_clamp_f64;

/* Coefficient ingestion, host side, once per configuration.
 * `From<[[f64;3];2]> for Biquad<C>` (src/iir/biquad.rs:545-566) followed by the
 * float -> Q conversion `round(v * 2^F)` saturating, NaN -> 0
 * (dsp-fixedpoint/src/num_traits_impl.rs:32-46).  sos = [b0,b1,b2,a0,a1,a2]
 * with the literature sign of a1/a2 (this is also the row format of
 * `sos()` in src/py.rs:49-73). */
int idsp_biquad_i32_from_sos(const double sos[6], int frac, idsp_biquad_i32 *out);
/* Same normalisation evaluated in f32 (`From<[[f32;3];2]> for Biquad<f32>`). */
int idsp_biquad_f32_from_sos(const float sos[6], idsp_biquad_f32 *out);
/* Same normalisation evaluated in f64, then each coefficient cast `as f32`
 * (`From<[f64;5]> for Biquad<f32>`, src/iir/biquad.rs:570-576). */
int idsp_biquad_f32_from_sos_f64(const double sos[6], idsp_biquad_f32 *out);
/* `From<[[f64;3];2]> for Biquad<f64>`. */
int idsp_biquad_f64_from_sos(const double sos[6], idsp_biquad_f64 *out);

/* All idsp_biquad_* / idsp_cascade_* calls process `n` serial sections
 * (1 <= n <= IDSP_MAX_SECTIONS; `cfg` points at n host-side records; n == 0 is
 * the reference's empty-slice identity, compose.rs:63-65).  Section s owns the
 * state words [s*W, (s+1)*W).
 *
 * state words per section (W):
 *   DF1        `DirectForm1<T>`        W=4  { x0, x1, y0, y1 }        biquad.rs:260-269,319
 *   DF1 dither `DirectForm1Dither`     W=5  { x0, x1, y0, y1, e }     biquad.rs:484-491
 *   DF1 wide   `DirectForm1Wide`       W=6  { x0, x1, y0.lo, y0.hi, y1.lo, y1.hi }  biquad.rs:445-454
 *   DF2T       `DirectForm2Transposed` W=2  { s0, s1 }                biquad.rs:407
 *   Cascade    `DirectForm<T, n>`      2+2n words total { x0, x1, (y0, y1) x n }    biquad.rs:260-269,324
 */

/* `Biquad<Q32<F>>` x `DirectForm1<i32>` (src/iir/biquad.rs:366-383). */
int idsp_biquad_i32_df1(const idsp_biquad_i32 *cfg, size_t n, void *state,
                        const int32_t *x, int32_t *y, size_t lanes, size_t frames,
                        int layout, void *stream);
/* `BiquadClamp<Q32<F>, i32>` x `DirectForm1<i32>` (src/iir/biquad.rs:394-404). */
int idsp_biquad_i32_df1_clamp(const idsp_biquad_clamp_i32 *cfg, size_t n, void *state,
                              const int32_t *x, int32_t *y, size_t lanes, size_t frames,
                              int layout, void *stream);
/* `Biquad<Q32<F>>` x `DirectForm1Dither` (src/iir/biquad.rs:511-530). */
int idsp_biquad_i32_dither(const idsp_biquad_i32 *cfg, size_t n, void *state,
                           const int32_t *x, int32_t *y, size_t lanes, size_t frames,
                           int layout, void *stream);
/* `BiquadClamp<Q32<F>, i32>` x `DirectForm1Dither` (src/iir/biquad.rs:532-538). */
int idsp_biquad_i32_dither_clamp(const idsp_biquad_clamp_i32 *cfg, size_t n, void *state,
                                 const int32_t *x, int32_t *y, size_t lanes, size_t frames,
                                 int layout, void *stream);
/* `Biquad<Q32<F>>` x `DirectForm1Wide` (src/iir/biquad.rs:456-472). */
int idsp_biquad_i32_wide(const idsp_biquad_i32 *cfg, size_t n, void *state,
                         const int32_t *x, int32_t *y, size_t lanes, size_t frames,
                         int layout, void *stream);
/* `BiquadClamp<Q32<F>, i32>` x `DirectForm1Wide` (src/iir/biquad.rs:474-480);
 * this is the per-section operator of `sos_clamp_wide()` in src/py.rs:76-108. */
int idsp_biquad_i32_wide_clamp(const idsp_biquad_clamp_i32 *cfg, size_t n, void *state,
                               const int32_t *x, int32_t *y, size_t lanes, size_t frames,
                               int layout, void *stream);
/* `Cascade<[Biquad<Q32<F>>; n]>` x `DirectForm<i32, n>` — shared delay lines
 * (src/iir/biquad.rs:339-364).  1 <= n <= 8. */
int idsp_cascade_i32_df1(const idsp_biquad_i32 *cfg, size_t n, void *state,
                         const int32_t *x, int32_t *y, size_t lanes, size_t frames,
                         int layout, void *stream);

/* ------------------------------------------------------------------------ */
/* iir::Biquad — 16-bit fixed point, i16 rows (src/iir/biquad.rs)           */
/* ------------------------------------------------------------------------ */
/*
 * `Biquad<Q16<F>>` x `DirectForm1<i16>`: the generic impl of src/iir/biquad.rs:366-383 with C = Q<i16, i32, F>, T = i16,
 * A = Q<i32, i16, F> — the same per-lane recurrence as idsp_biquad_i32_df1 on half the bytes in and half the bytes out.  x and y
 * hold plain i16 rows, ONE ELEMENT per sample, in `layout`.  Computed as a RELEASE build of the reference computes it — every i32
 * and i16 operation wraps:
 *   acc: i32 = b0*x0 + b1*x[0] + b2*x[1] + a1*y[0] + a2*y[1]   each product i32(c) * i32(v) (dsp-fixedpoint/src/lib.rs:310-312,
 *                                                              ops.rs:91-97), the sum left to right in wrapping i32
 *                                                              (ops.rs:63-76).  Five products of up to 2^30 do leave i32: a
 *                                                              debug build panics there, here the sum wraps;
 *   y0 = (acc >> F) as i16                                     arithmetic shift of the i32, truncating cast
 *                                                              (num_traits_impl.rs:74-90, lib.rs:270-299);
 *   x = [x0, x[0]]; y = [y0, y[0]]                             (biquad.rs:379-380).
 * `BiquadClamp<Q16<F>, i16>` (biquad.rs:394-404): y0 = clamp(process(..) + u, min, max), the `+` in wrapping i16, `num_traits::clamp`
 * (a value below min yields min, else one above max yields max, also when min > max), then state.y[0] = y0.
 * frac = F, 0 <= F < 32, is the shift of the i32 accumulator: the rule of idsp_biquad_i32.
 */
typedef struct idsp_biquad_i16 {
    int16_t ba[5]; /* [b0,b1,b2,a1,a2] raw Q bits, a1,a2 exactly as used in the recurrence */
    int16_t frac;
} idsp_biquad_i16; /* 12 bytes */

typedef struct idsp_biquad_clamp_i16 {
    int16_t ba[5];
    int16_t frac;
    int16_t u;   /* summing junction offset */
    int16_t min; /* lower limit */
    int16_t max; /* upper limit */
} idsp_biquad_clamp_i16; /* 18 bytes */

/* `From<[[f64;3];2]> for Biquad<C>` (src/iir/biquad.rs:545-566) followed by `round(v * 2^F)`, half away from zero, saturating to
 * i16, NaN -> 0 (dsp-fixedpoint/src/num_traits_impl.rs:32-46).  Host code.  IDSP_EINVAL: NULL sos / out, frac outside 0..31. */
int idsp_biquad_i16_from_sos(const double sos[6], int frac, idsp_biquad_i16 *out);

/*
 * n serial sections, 0 <= n <= IDSP_MAX_SECTIONS, as for every idsp_biquad_* entry; n == 0 copies x to y and leaves the state
 * alone (compose.rs:63-65).  Up to four sections run in one launch; longer chains run as further passes in place on y (the
 * reference's slice composition, compose.rs:43-77).
 * State: W = 4 words per section and lane { x0, x1, y0, y1 } (biquad.rs:260-269,319), word-plane-major as everywhere, section s
 * owning words [4 s, 4 s + 4).  Each i16 sits in a 32-bit word that is read as its low half (`(int16_t)w`) and written back
 * sign-extended.  All zero is `Default::default()`.  Read at entry, written at exit; FRAME_MAJOR and LANE_MAJOR calls may be
 * mixed on one state.
 * x_pitch / y_pitch: ELEMENTS between the starts of consecutive rows (frames in FRAME_MAJOR, lanes in LANE_MAJOR), 0 = dense.
 * They belong to the one entry (there is no `_pitch` twin): i16 rows with an odd length are the normal case, and the pitch is how
 * a caller keeps them on the 4-byte grid.  x and y may start at any 2-BYTE-aligned address and any pitch >= a row is accepted;
 * elements of y in the gap of a pitched row are not written.  FRAME_MAJOR has one kernel form, a lane per thread on 16-bit accesses,
 * whatever the alignment.  LANE_MAJOR has a fast form that needs every row of x and y on the 4-byte grid — x and y 4-byte
 * aligned and both pitches (or dense row lengths) even; an odd frame count is fine —: then a thread moves a dword, two
 * consecutive frames of a lane.  Every other LANE_MAJOR call runs on 16-bit accesses, correct and slower (profiles/NOTES.md,
 * "Biquad i16").
 * In place: y == x with y_pitch == x_pitch is allowed (0 counting as the row length) — the reference's `inplace()`
 * (biquad.rs:540-541).  Any other overlap of the two extents, (rows-1) * pitch + row elements each, is IDSP_EINVAL.
 * Also IDSP_EINVAL, with nothing written: a bad layout, n > IDSP_MAX_SECTIONS, NULL cfg with n > 0, NULL state with n > 0 and
 * lanes > 0, NULL x or y with lanes, frames > 0, a frac outside 0..31, a pitch shorter than a row, an odd x or y address, an
 * extent past size_t.  lanes == 0 or frames == 0 is IDSP_OK and writes nothing.
 * Asynchronous on `stream`; no host synchronisation, no allocation.
 */
size_t idsp_biquad_i16_state_words(size_t n); /* 4 * n */
/* `Biquad<Q16<F>>` x `DirectForm1<i16>` (src/iir/biquad.rs:366-383). */
int idsp_biquad_i16_df1(const idsp_biquad_i16 *cfg, size_t n, void *state, const int16_t *x, size_t x_pitch,
                        int16_t *y, size_t y_pitch, size_t lanes, size_t frames, int layout, void *stream);
/* `BiquadClamp<Q16<F>, i16>` x `DirectForm1<i16>` (src/iir/biquad.rs:394-404). */
int idsp_biquad_i16_df1_clamp(const idsp_biquad_clamp_i16 *cfg, size_t n, void *state, const int16_t *x, size_t x_pitch,
                              int16_t *y, size_t y_pitch, size_t lanes, size_t frames, int layout, void *stream);

/*
 * Per-lane coefficient banks: `ByLane<[Biquad<Q16<F>>; N]>` / `ByLane<[BiquadClamp<Q16<F>, i16>; N]>` (dsp-process/src/compose.rs:363-390),
 * each configuration a slice of n sections (compose.rs:43-77).  Lane l is filtered by configuration l on state l; the arithmetic,
 * the state layout, the pitches, the alignment and in-place rules, n == 0, the passes of up to four sections and the kernel forms are
 * those of idsp_biquad_i16_df1 / _df1_clamp above.  Only the source of the coefficients changes.
 * coef: a DEVICE array of int16_t in lane-contiguous planes, the convention of idsp_biquad_i32_df1_bylane: value v of section k of
 * lane l is coef[(k*CV + v)*lanes + l], CV = 5 { b0, b1, b2, a1, a2 } (a1, a2 as used), CV = 8 { .., u, min, max } for the clamp
 * entry; n*CV*lanes elements.  Any 2-byte-aligned address: with an odd lane count every other plane is off the 4-byte grid anyway.
 * Read once per pass, before the first frame; read-only for the call.  Overlap of coef with y or state is NOT checked.
 * frac: the one F of `Q16<F>`, 0..31, shared by all lanes and sections (a const generic in the reference).
 * IDSP_EINVAL in addition, with nothing written: NULL coef with n > 0 and lanes > 0, an odd coef address.
 * idsp_last_kernel(): "biquad_i16_bylane_frame_major", "biquad_i16_bylane_lane_major[dword runs]" / "[half runs]".
 */
int idsp_biquad_i16_df1_bylane(const int16_t *coef, int frac, size_t n, void *state, const int16_t *x, size_t x_pitch,
                               int16_t *y, size_t y_pitch, size_t lanes, size_t frames, int layout, void *stream);
int idsp_biquad_i16_df1_clamp_bylane(const int16_t *coef, int frac, size_t n, void *state, const int16_t *x, size_t x_pitch,
                                     int16_t *y, size_t y_pitch, size_t lanes, size_t frames, int layout, void *stream);
/* sos[lanes][n][6] -> the planes above, on the HOST: each [b0,b1,b2,a0,a1,a2] quantised as idsp_biquad_i16_from_sos does; with
 * cv == 8 also u = 0, min = INT16_MIN, max = INT16_MAX (`BiquadClamp::default`, biquad.rs:159-171) for the caller to overwrite.
 * coef: n*cv*lanes elements of host memory.  IDSP_EINVAL: frac outside 0..31, cv neither 5 nor 8, n > IDSP_MAX_SECTIONS, NULL sos
 * or coef with lanes > 0 and n > 0. */
int idsp_biquad_i16_bank_from_sos(const double *sos, size_t lanes, size_t n, int frac, size_t cv, int16_t *coef);

/* ------------------------------------------------------------------------ */
/* iir::Biquad — f32                                                        */
/* ------------------------------------------------------------------------ */

/* `Biquad<f32>` x `DirectForm1<f32>` (src/iir/biquad.rs:366-383): every product
 * and sum individually rounded, evaluated left to right, no FMA. */
int idsp_biquad_f32_df1(const idsp_biquad_f32 *cfg, size_t n, void *state,
                        const float *x, float *y, size_t lanes, size_t frames,
                        int layout, void *stream);
/* `BiquadClamp<f32>` x `DirectForm1<f32>` (src/iir/biquad.rs:394-404). */
int idsp_biquad_f32_df1_clamp(const idsp_biquad_clamp_f32 *cfg, size_t n, void *state,
                              const float *x, float *y, size_t lanes, size_t frames,
                              int layout, void *stream);
/* `Biquad<f32>` x `DirectForm2Transposed<f32>` (src/iir/biquad.rs:418-428). */
int idsp_biquad_f32_df2t(const idsp_biquad_f32 *cfg, size_t n, void *state,
                         const float *x, float *y, size_t lanes, size_t frames,
                         int layout, void *stream);
/* `BiquadClamp<f32>` x `DirectForm2Transposed<f32>` (src/iir/biquad.rs:430-440). */
int idsp_biquad_f32_df2t_clamp(const idsp_biquad_clamp_f32 *cfg, size_t n, void *state,
                               const float *x, float *y, size_t lanes, size_t frames,
                               int layout, void *stream);
/* `Cascade<[Biquad<f32>; n]>` x `DirectForm<f32, n>` (src/iir/biquad.rs:339-364). */
int idsp_cascade_f32_df1(const idsp_biquad_f32 *cfg, size_t n, void *state,
                         const float *x, float *y, size_t lanes, size_t frames,
                         int layout, void *stream);

/* ------------------------------------------------------------------------ */
/* iir::Biquad — f64 (same generic impls; every value is two state words,   */
/* low word first: DF1 W=8 {x0,x1,y0,y1}, DF2T W=4 {s0,s1}, Cascade 4+4n)   */
/* ------------------------------------------------------------------------ */

int idsp_biquad_f64_df1(const idsp_biquad_f64 *cfg, size_t n, void *state,
                        const double *x, double *y, size_t lanes, size_t frames,
                        int layout, void *stream);
int idsp_biquad_f64_df1_clamp(const idsp_biquad_clamp_f64 *cfg, size_t n, void *state,
                              const double *x, double *y, size_t lanes, size_t frames,
                              int layout, void *stream);
int idsp_biquad_f64_df2t(const idsp_biquad_f64 *cfg, size_t n, void *state,
                         const double *x, double *y, size_t lanes, size_t frames,
                         int layout, void *stream);
int idsp_biquad_f64_df2t_clamp(const idsp_biquad_clamp_f64 *cfg, size_t n, void *state,
                               const double *x, double *y, size_t lanes, size_t frames,
                               int layout, void *stream);
int idsp_cascade_f64_df1(const idsp_biquad_f64 *cfg, size_t n, void *state,
                         const double *x, double *y, size_t lanes, size_t frames,
                         int layout, void *stream);

/*
 * Per-lane coefficients: `ByLane<[C; N]>` (dsp-process/src/compose.rs:363-390,
 * `process_view` :375-389: lane i is filtered by configuration i with state i)
 * for C = a slice of `n` Biquad/BiquadClamp sections (compose.rs:43-77).
 *
 * `coef` is a device array of lane-contiguous planes like the state: value v
 * of section k of lane l is coef[(k * CV + v) * lanes + l], with CV = 5
 * (`Biquad::ba`, biquad.rs:116) for the plain entries and CV = 8 (ba, u, min,
 * max; biquad.rs:121-157) for the `_clamp` entries.  The i32 variants share
 * one `frac` (the const generic F of `Q32<F>`) across lanes and sections.
 * State layout, x/y layout, in-place rule and status codes are those of the
 * shared-coefficient entries above.
 */
int idsp_biquad_i32_df1_bylane(const int32_t *coef, int frac, size_t n, void *state,
        const int32_t *x, int32_t *y, size_t lanes, size_t frames, int layout, void *stream);
int idsp_biquad_i32_df1_clamp_bylane(const int32_t *coef, int frac, size_t n, void *state,
        const int32_t *x, int32_t *y, size_t lanes, size_t frames, int layout, void *stream);
int idsp_biquad_i32_dither_bylane(const int32_t *coef, int frac, size_t n, void *state,
        const int32_t *x, int32_t *y, size_t lanes, size_t frames, int layout, void *stream);
int idsp_biquad_i32_dither_clamp_bylane(const int32_t *coef, int frac, size_t n, void *state,
        const int32_t *x, int32_t *y, size_t lanes, size_t frames, int layout, void *stream);
int idsp_biquad_i32_wide_bylane(const int32_t *coef, int frac, size_t n, void *state,
        const int32_t *x, int32_t *y, size_t lanes, size_t frames, int layout, void *stream);
int idsp_biquad_i32_wide_clamp_bylane(const int32_t *coef, int frac, size_t n, void *state,
        const int32_t *x, int32_t *y, size_t lanes, size_t frames, int layout, void *stream);
int idsp_biquad_f32_df1_bylane(const float *coef, size_t n, void *state,
        const float *x, float *y, size_t lanes, size_t frames, int layout, void *stream);
int idsp_biquad_f32_df1_clamp_bylane(const float *coef, size_t n, void *state,
        const float *x, float *y, size_t lanes, size_t frames, int layout, void *stream);
int idsp_biquad_f32_df2t_bylane(const float *coef, size_t n, void *state,
        const float *x, float *y, size_t lanes, size_t frames, int layout, void *stream);
int idsp_biquad_f32_df2t_clamp_bylane(const float *coef, size_t n, void *state,
        const float *x, float *y, size_t lanes, size_t frames, int layout, void *stream);
int idsp_biquad_f64_df1_bylane(const double *coef, size_t n, void *state,
        const double *x, double *y, size_t lanes, size_t frames, int layout, void *stream);
int idsp_biquad_f64_df1_clamp_bylane(const double *coef, size_t n, void *state,
        const double *x, double *y, size_t lanes, size_t frames, int layout, void *stream);
int idsp_biquad_f64_df2t_bylane(const double *coef, size_t n, void *state,
        const double *x, double *y, size_t lanes, size_t frames, int layout, void *stream);
int idsp_biquad_f64_df2t_clamp_bylane(const double *coef, size_t n, void *state,
        const double *x, double *y, size_t lanes, size_t frames, int layout, void *stream);

/* ------------------------------------------------------------------------ */
/* explicit row pitches: `<entry>_pitch`                                    */
/* ------------------------------------------------------------------------ */
/*
 * Every biquad / cascade / by-lane entry above has a `_pitch` twin that takes the distance between rows of x and
 * of y explicitly (like a BLAS leading dimension), in ELEMENTS:
 *   IDSP_LANE_MAJOR   pitch = elements between the starts of consecutive lanes  (dense: frames) — the reference's
 *                     `View::<_, LaneMajor>::lane(i) = flat[i * frames ..]` (dsp-process/src/view.rs:181-195) with the
 *                     lanes padded apart; element (f, l) at l * pitch + f;
 *   IDSP_FRAME_MAJOR  pitch = elements between the starts of consecutive frames (dense: lanes): a block of `lanes`
 *                     adjacent lanes of a wider `[[T; L]; frames]` tensor; element (f, l) at f * pitch + l.
 * 0 means dense.  A pitch shorter than a row is IDSP_EINVAL; an in-place call (y == x) needs x_pitch == y_pitch.
 * Why it exists: power-of-two LANE_MAJOR pitches (frames = 4096 -> 16 KiB) alias on the HBM channels and cost
 * 10-15 % (profiles/r01_lm_pitch_probe.jsonl); a caller that owns its buffers can pad each lane by a few cache
 * lines.  The FRAME_MAJOR form lets a caller process a lane block of a larger tensor without a re-layout pass
 * (this is also how a FRAME_MAJOR host tensor is split over several devices).  `pitch == dense` is bit-identical to
 * the plain entry.
 */
int idsp_biquad_i32_df1_pitch(const idsp_biquad_i32 *cfg, size_t n, void *state, const int32_t *x, size_t x_pitch, int32_t *y, size_t y_pitch,
        size_t lanes, size_t frames, int layout, void *stream);
int idsp_biquad_i32_df1_clamp_pitch(const idsp_biquad_clamp_i32 *cfg, size_t n, void *state, const int32_t *x, size_t x_pitch, int32_t *y, size_t y_pitch,
        size_t lanes, size_t frames, int layout, void *stream);
int idsp_biquad_i32_dither_pitch(const idsp_biquad_i32 *cfg, size_t n, void *state, const int32_t *x, size_t x_pitch, int32_t *y, size_t y_pitch,
        size_t lanes, size_t frames, int layout, void *stream);
int idsp_biquad_i32_dither_clamp_pitch(const idsp_biquad_clamp_i32 *cfg, size_t n, void *state, const int32_t *x, size_t x_pitch, int32_t *y, size_t y_pitch,
        size_t lanes, size_t frames, int layout, void *stream);
int idsp_biquad_i32_wide_pitch(const idsp_biquad_i32 *cfg, size_t n, void *state, const int32_t *x, size_t x_pitch, int32_t *y, size_t y_pitch,
        size_t lanes, size_t frames, int layout, void *stream);
int idsp_biquad_i32_wide_clamp_pitch(const idsp_biquad_clamp_i32 *cfg, size_t n, void *state, const int32_t *x, size_t x_pitch, int32_t *y, size_t y_pitch,
        size_t lanes, size_t frames, int layout, void *stream);
int idsp_cascade_i32_df1_pitch(const idsp_biquad_i32 *cfg, size_t n, void *state, const int32_t *x, size_t x_pitch, int32_t *y, size_t y_pitch,
        size_t lanes, size_t frames, int layout, void *stream);
int idsp_biquad_f32_df1_pitch(const idsp_biquad_f32 *cfg, size_t n, void *state, const float *x, size_t x_pitch, float *y, size_t y_pitch,
        size_t lanes, size_t frames, int layout, void *stream);
int idsp_biquad_f32_df1_clamp_pitch(const idsp_biquad_clamp_f32 *cfg, size_t n, void *state, const float *x, size_t x_pitch, float *y, size_t y_pitch,
        size_t lanes, size_t frames, int layout, void *stream);
int idsp_biquad_f32_df2t_pitch(const idsp_biquad_f32 *cfg, size_t n, void *state, const float *x, size_t x_pitch, float *y, size_t y_pitch,
        size_t lanes, size_t frames, int layout, void *stream);
int idsp_biquad_f32_df2t_clamp_pitch(const idsp_biquad_clamp_f32 *cfg, size_t n, void *state, const float *x, size_t x_pitch, float *y, size_t y_pitch,
        size_t lanes, size_t frames, int layout, void *stream);
int idsp_cascade_f32_df1_pitch(const idsp_biquad_f32 *cfg, size_t n, void *state, const float *x, size_t x_pitch, float *y, size_t y_pitch,
        size_t lanes, size_t frames, int layout, void *stream);
int idsp_biquad_f64_df1_pitch(const idsp_biquad_f64 *cfg, size_t n, void *state, const double *x, size_t x_pitch, double *y, size_t y_pitch,
        size_t lanes, size_t frames, int layout, void *stream);
int idsp_biquad_f64_df1_clamp_pitch(const idsp_biquad_clamp_f64 *cfg, size_t n, void *state, const double *x, size_t x_pitch, double *y, size_t y_pitch,
        size_t lanes, size_t frames, int layout, void *stream);
int idsp_biquad_f64_df2t_pitch(const idsp_biquad_f64 *cfg, size_t n, void *state, const double *x, size_t x_pitch, double *y, size_t y_pitch,
        size_t lanes, size_t frames, int layout, void *stream);
int idsp_biquad_f64_df2t_clamp_pitch(const idsp_biquad_clamp_f64 *cfg, size_t n, void *state, const double *x, size_t x_pitch, double *y, size_t y_pitch,
        size_t lanes, size_t frames, int layout, void *stream);
int idsp_cascade_f64_df1_pitch(const idsp_biquad_f64 *cfg, size_t n, void *state, const double *x, size_t x_pitch, double *y, size_t y_pitch,
        size_t lanes, size_t frames, int layout, void *stream);
int idsp_biquad_i32_df1_bylane_pitch(const int32_t *coef, int frac, size_t n, void *state, const int32_t *x, size_t x_pitch,
        int32_t *y, size_t y_pitch, size_t lanes, size_t frames, int layout, void *stream);
int idsp_biquad_i32_df1_clamp_bylane_pitch(const int32_t *coef, int frac, size_t n, void *state, const int32_t *x, size_t x_pitch,
        int32_t *y, size_t y_pitch, size_t lanes, size_t frames, int layout, void *stream);
int idsp_biquad_i32_dither_bylane_pitch(const int32_t *coef, int frac, size_t n, void *state, const int32_t *x, size_t x_pitch,
        int32_t *y, size_t y_pitch, size_t lanes, size_t frames, int layout, void *stream);
int idsp_biquad_i32_dither_clamp_bylane_pitch(const int32_t *coef, int frac, size_t n, void *state, const int32_t *x, size_t x_pitch,
        int32_t *y, size_t y_pitch, size_t lanes, size_t frames, int layout, void *stream);
int idsp_biquad_i32_wide_bylane_pitch(const int32_t *coef, int frac, size_t n, void *state, const int32_t *x, size_t x_pitch,
        int32_t *y, size_t y_pitch, size_t lanes, size_t frames, int layout, void *stream);
int idsp_biquad_i32_wide_clamp_bylane_pitch(const int32_t *coef, int frac, size_t n, void *state, const int32_t *x, size_t x_pitch,
        int32_t *y, size_t y_pitch, size_t lanes, size_t frames, int layout, void *stream);
int idsp_biquad_f32_df1_bylane_pitch(const float *coef, size_t n, void *state, const float *x, size_t x_pitch, float *y, size_t y_pitch,
        size_t lanes, size_t frames, int layout, void *stream);
int idsp_biquad_f32_df1_clamp_bylane_pitch(const float *coef, size_t n, void *state, const float *x, size_t x_pitch, float *y, size_t y_pitch,
        size_t lanes, size_t frames, int layout, void *stream);
int idsp_biquad_f32_df2t_bylane_pitch(const float *coef, size_t n, void *state, const float *x, size_t x_pitch, float *y, size_t y_pitch,
        size_t lanes, size_t frames, int layout, void *stream);
int idsp_biquad_f32_df2t_clamp_bylane_pitch(const float *coef, size_t n, void *state, const float *x, size_t x_pitch, float *y, size_t y_pitch,
        size_t lanes, size_t frames, int layout, void *stream);
int idsp_biquad_f64_df1_bylane_pitch(const double *coef, size_t n, void *state, const double *x, size_t x_pitch, double *y, size_t y_pitch,
        size_t lanes, size_t frames, int layout, void *stream);
int idsp_biquad_f64_df1_clamp_bylane_pitch(const double *coef, size_t n, void *state, const double *x, size_t x_pitch, double *y, size_t y_pitch,
        size_t lanes, size_t frames, int layout, void *stream);
int idsp_biquad_f64_df2t_bylane_pitch(const double *coef, size_t n, void *state, const double *x, size_t x_pitch, double *y, size_t y_pitch,
        size_t lanes, size_t frames, int layout, void *stream);
int idsp_biquad_f64_df2t_clamp_bylane_pitch(const double *coef, size_t n, void *state, const double *x, size_t x_pitch, double *y, size_t y_pitch,
        size_t lanes, size_t frames, int layout, void *stream);

/* ------------------------------------------------------------------------ */
/* iir::normal::Normal and iir::wdf::Wdf lanes                               */
/* ------------------------------------------------------------------------ */

/* `Normal<C>` x `DirectForm1<T>` (src/iir/normal.rs:28-58), the Rader-Gold / Chamberlin normal form:
 *   y1' = (b0*x0 + b1*x1 + b2*x2 + re*y1 + (-im)*y0).as_();  y0' = (im*y1 + re*y0).as_();  returns y0'
 * with state words {x0, x1, y0, y1} (y0 = in-phase, y1 = quadrature component, normal.rs:24-25).
 * The configuration reuses the biquad records: ba = [b0, b1, b2, p.re, p.im] (and frac for Q32<F>);
 * n sections run in series like the biquad entries. */
int idsp_normal_i32_df1(const idsp_biquad_i32 *cfg, size_t n, void *state, const int32_t *x, int32_t *y,
                        size_t lanes, size_t frames, int layout, void *stream);
int idsp_normal_f32_df1(const idsp_biquad_f32 *cfg, size_t n, void *state, const float *x, float *y,
                        size_t lanes, size_t frames, int layout, void *stream);
int idsp_normal_f64_df1(const idsp_biquad_f64 *cfg, size_t n, void *state, const double *x, double *y,
                        size_t lanes, size_t frames, int layout, void *stream);
/* `From<&[[f64; 3]; 2]> for Normal<C>` (src/iir/normal.rs:62-76): sos = [b0,b1,b2,a0,a1,a2] ->
 * out = [b0/a0, b1/a0, b2/a0, p.re, p.im]; IDSP_EINVAL when the poles are real (`assert!(pq >= 0.0)`). */
int idsp_normal_from_sos(const double sos[6], double out[5]);

/* `Wdf<N, M>` (src/iir/wdf.rs:103-171): N two-port adaptors, adaptor i of type nibble i of M
 * (`Tpa`, wdf.rs:14-32: 0xA A, 0xB B, 0xE B1, 0x1 X, 0xC C, 0xF C1, 0xD D, anything else Z), with
 * coefficients a[i] as raw `Q32<32>` bits.  State = `WdfState<N>::z` (N words per section). */
#define IDSP_WDF_MAX_ORDER 8
typedef struct idsp_wdf {
    int32_t n;   /* N: 1..8 */
    uint32_t m;  /* M: one nibble per adaptor, adaptor 0 in the low nibble */
    int32_t a[IDSP_WDF_MAX_ORDER];
} idsp_wdf;
/* `Wdf::<N, M>::quantize(&g)` (src/iir/wdf.rs:126-137, `Tpa::quantize` :50-62): fills out->a from the
 * allpass poles g[0..n) for the architecture nibbles m; IDSP_EOUTOFRANGE when a pole does not fit its
 * adaptor type (the reference returns None). */
int idsp_wdf_quantize(int n, uint32_t m, const double *g, idsp_wdf *out);
/* Per-lane state words of a chain of n_sections sections (sum of their n). */
size_t idsp_wdf_state_words(const idsp_wdf *cfg, size_t n_sections);
/* Serial chain of n_sections `Wdf` sections (array / tuple composition, dsp-process/src/compose.rs:43-113),
 * `SplitProcess<i32, i32, WdfState<N>>` (wdf.rs:153-169); in place allowed. */
int idsp_wdf_i32(const idsp_wdf *cfg, size_t n_sections, void *state, const int32_t *x, int32_t *y,
                 size_t lanes, size_t frames, int layout, void *stream);

/* ------------------------------------------------------------------------ */
/* Cic — cascaded integrator-comb rate changer (src/cic.rs)                 */
/* ------------------------------------------------------------------------ */

#define IDSP_CIC_MAX_ORDER 6
#define IDSP_CIC_MAX_DELAY 4

/* `Cic<T, N, M>::new(rate)` (src/cic.rs:13-28,39-47): order N (1..6), comb delay M
 * (1..4), rate = fast/slow - 1.  T = i32 or i64 is chosen by the entry point. */
typedef struct idsp_cic {
    int32_t order;
    int32_t comb_delay;
    uint32_t rate;
} idsp_cic;

/* `Cic::gain()` as i64 (wrapping), `gain_log2()`, `response_length()` (src/cic.rs:103-118);
 * gain_log2 / response_length return a negative idsp_status / 0 for an invalid cfg. */
int64_t idsp_cic_gain(const idsp_cic *cfg);
int idsp_cic_gain_log2(const idsp_cic *cfg);
size_t idsp_cic_response_length(const idsp_cic *cfg);
/* 32-bit state words per lane for T of `bits` (32 or 64) width; 0 for an invalid cfg.
 * Values in order: zoh, combs[N][M] (row n = comb n, oldest first), integrators[N];
 * a 64-bit value is two words, low first; planes are lane-contiguous like every state.
 * `index` is not part of the record: the chunked entries below start and end every call
 * at index == 0 (`tick()`), the only phase `Decimator` / `Interpolator` accept. */
size_t idsp_cic_state_words(const idsp_cic *cfg, int bits);

/* `Split::stateful(Cic::<T, N, M>::new(R - 1)).decimate()` (src/cic.rs:338-341; `Process<T, Option<T>>`
 * :186-207 under `Decimator`, dsp-process/src/adapters.rs:158-167): x holds `frames` chunks `[T; R]`
 * per lane (R = rate + 1; FRAME_MAJOR x[(f*lanes + l)*R + r], LANE_MAJOR x[(l*frames + f)*R + r]),
 * y one sample per chunk.  Integrators and combs wrap (cic.rs:191,199). */
int idsp_cic_dec_i32(const idsp_cic *cfg, void *state, const int32_t *x, int32_t *y,
                     size_t lanes, size_t frames, int layout, void *stream);
int idsp_cic_dec_i64(const idsp_cic *cfg, void *state, const int64_t *x, int64_t *y,
                     size_t lanes, size_t frames, int layout, void *stream);
/* `...interpolate()` (src/cic.rs:343-346; `Process<Option<T>, T>` :160-182 under `Interpolator`,
 * adapters.rs:27-35): one input sample per frame, y holds chunks `[T; R]`.  Release-mode
 * (wrapping) arithmetic; the reference's debug build would panic on overflow (cic.rs:177). */
int idsp_cic_int_i32(const idsp_cic *cfg, void *state, const int32_t *x, int32_t *y,
                     size_t lanes, size_t frames, int layout, void *stream);
int idsp_cic_int_i64(const idsp_cic *cfg, void *state, const int64_t *x, int64_t *y,
                     size_t lanes, size_t frames, int layout, void *stream);

/* ------------------------------------------------------------------------ */
/* coefficient front-end (host side, no device work)                        */
/* ------------------------------------------------------------------------ */
/*
 * `iir::coefficients::Filter<T>`, `iir::pid::{Builder, Pid, Units}` and
 * `iir::config::BiquadConfig::{build, try_build}`: pure host functions that
 * produce the idsp_biquad_* records above (or rows of the per-lane coefficient
 * planes).  Parameters travel as f64; `f32 != 0` selects T = f32, i.e. every
 * field is first rounded to f32 and all arithmetic is carried out in f32 like
 * the reference's generic code instantiated with T = f32.  `validate != 0`
 * runs the reference's `validate()` first (the `try_build*` methods) and
 * returns IDSP_ENONFINITE .. IDSP_ESIGN; `validate == 0` is the unchecked
 * `build*` which, like the reference, may produce NaN/inf coefficients.
 * The `_i32` outputs are C = `Q32<frac>`, Y = i32; `_f32`: C = Y = f32;
 * `_f64`: C = Y = f64.
 */

/* `coefficients::Type` (src/iir/coefficients.rs:43-66) */
typedef enum idsp_filter_type {
    IDSP_LOWPASS = 0, IDSP_HIGHPASS, IDSP_BANDPASS, IDSP_ALLPASS, IDSP_NOTCH,
    IDSP_PEAKING, IDSP_LOWSHELF, IDSP_HIGHSHELF, IDSP_IHO
} idsp_filter_type;

/* `coefficients::Shape` (src/iir/coefficients.rs:6-16) */
typedef enum idsp_shape_kind { IDSP_SHAPE_Q = 0, IDSP_SHAPE_BANDWIDTH = 1, IDSP_SHAPE_SLOPE = 2 } idsp_shape_kind;

/* `coefficients::Filter<T>` (src/iir/coefficients.rs:27-40); Default (:88-97) is
 * frequency 0, gain 1, shelf 1, Shape::Q(1/sqrt 2). */
typedef struct idsp_filter {
    double frequency; /* angular critical frequency w0, pi = Nyquist */
    double gain;      /* linear passband gain */
    double shelf;     /* linear shelf gain (peaking / shelves / iho) */
    double shape;     /* Q, bandwidth in octaves, or shelf slope */
    int32_t shape_kind;
    int32_t f32;
} idsp_filter;

/* `Filter::build(typ)` / `try_build(typ)` (coefficients.rs:483-501): cookbook
 * `[[b0,b1,b2],[a0,a1,a2]]` flattened to ba[6] = the `sos` row format of
 * idsp_biquad_*_from_sos.  With f32 set the six values are exact f32 values. */
int idsp_filter_build(const idsp_filter *f, int type, int validate, double ba[6]);

/* `pid::Order` (src/iir/pid.rs:14-24) and `pid::Action` (:61-75) index values */
#define IDSP_PID_ORDER_P 2
#define IDSP_PID_ORDER_I 1
#define IDSP_PID_ORDER_I2 0

/* `pid::Builder<T>` (src/iir/pid.rs:40-45); gain/limit index = Action: I2, I, P, D, D2.
 * Default (:47-55): order I, gains 0, limits +inf. */
typedef struct idsp_pid_builder {
    int32_t order;
    int32_t f32;
    double gain[5];
    double limit[5];
} idsp_pid_builder;

/* `Build<[C; 5]> for Builder<T>` (src/iir/pid.rs:256-313) with context `period`;
 * validate = `Builder::validate` (:195-222).  ba = [b0, b1, b2, a1, a2]. */
int idsp_pid_build_i32(const idsp_pid_builder *b, double period, int validate, int frac, int32_t ba[5]);
int idsp_pid_build_f32(const idsp_pid_builder *b, double period, int validate, float ba[5]);
int idsp_pid_build_f64(const idsp_pid_builder *b, double period, int validate, double ba[5]);

/* `pid::Units<T>` (src/iir/pid.rs:350-369), Default 1, 1, 1 */
typedef struct idsp_units {
    double t, x, y;
} idsp_units;

/* `pid::Pid<T>` (src/iir/pid.rs:384-417); Default: builder default, setpoint 0, min -inf, max +inf */
typedef struct idsp_pid {
    idsp_pid_builder builder;
    double setpoint, min, max;
} idsp_pid;

/* `Build<BiquadClamp<C, Y>> for Pid<T>` (src/iir/pid.rs:533-567) = `BiquadConfig::Pid`
 * (config.rs:371,408); validate = `Pid::validate` (pid.rs:497-518). */
int idsp_pid_build_clamp_i32(const idsp_pid *p, const idsp_units *units, int validate, int frac,
                             idsp_biquad_clamp_i32 *out);
int idsp_pid_build_clamp_f32(const idsp_pid *p, const idsp_units *units, int validate, idsp_biquad_clamp_f32 *out);
int idsp_pid_build_clamp_f64(const idsp_pid *p, const idsp_units *units, int validate, idsp_biquad_clamp_f64 *out);

/* `config::BaConfig<T>` (src/iir/config.rs:19-31): SI-unit `[[b],[a]]`, offset, limits */
typedef struct idsp_ba_config {
    double ba[6];
    double offset, min, max;
    int32_t f32;
} idsp_ba_config;

/* `BiquadConfig::Ba(..).build(units)` (config.rs:359-367) / `.try_build` (:389-407) */
int idsp_config_ba_build_i32(const idsp_ba_config *c, const idsp_units *units, int validate, int frac,
                             idsp_biquad_clamp_i32 *out);
int idsp_config_ba_build_f32(const idsp_ba_config *c, const idsp_units *units, int validate, idsp_biquad_clamp_f32 *out);
int idsp_config_ba_build_f64(const idsp_ba_config *c, const idsp_units *units, int validate, idsp_biquad_clamp_f64 *out);

/* `config::FilterConfig<T>` (src/iir/config.rs:46-67): frequency relative to 1/units.t, gains in dB */
typedef struct idsp_filter_config {
    int32_t typ; /* idsp_filter_type */
    int32_t shape_kind;
    double frequency, gain_db, shelf_db, shape;
    double offset, min, max;
    int32_t f32;
} idsp_filter_config;

/* `BiquadConfig::Filter(..).build(units)` (config.rs:372-385) / `.try_build` (:409-427) */
int idsp_config_filter_build_i32(const idsp_filter_config *c, const idsp_units *units, int validate, int frac,
                                 idsp_biquad_clamp_i32 *out);
int idsp_config_filter_build_f32(const idsp_filter_config *c, const idsp_units *units, int validate,
                                 idsp_biquad_clamp_f32 *out);
int idsp_config_filter_build_f64(const idsp_filter_config *c, const idsp_units *units, int validate,
                                 idsp_biquad_clamp_f64 *out);

/* ------------------------------------------------------------------------ */
/* hbf — symmetric FIR and half-band decimator / interpolator cascades      */
/* ------------------------------------------------------------------------ */

#define IDSP_HBF_MAX_STAGES 5
#define IDSP_HBF_MAX_TAPS 32

/* A cascade of `EvenSymmetric<[f32; M]>` half-band stages (src/hbf.rs:70-138)
 * in PROCESSING order.  taps[s][0..m[s]) are ordered outermost (small) to
 * centre (large) exactly like HBF_TAPS (src/hbf.rs:308-349). */
typedef struct idsp_hbf_cascade_f32 {
    int32_t stages;                 /* 1..IDSP_HBF_MAX_STAGES */
    int32_t m[IDSP_HBF_MAX_STAGES]; /* one-sided tap count per stage, 1..IDSP_HBF_MAX_TAPS */
    float taps[IDSP_HBF_MAX_STAGES][IDSP_HBF_MAX_TAPS];
} idsp_hbf_cascade_f32;

/* Built-in tap sets: set 0 = HBF_TAPS (140 dB, src/hbf.rs:308-349),
 * set 1 = HBF_TAPS_98 (src/hbf.rs:258-292). */
/* Fill `out` like `HBF_DEC_CASCADE` restricted to a 2^stages rate change
 * (src/hbf.rs:385-421: highest-rate/fewest-tap stage first, i.e. tuple index
 * stages-1 down to 0). */
int idsp_hbf_dec_cascade(int tap_set, int stages, idsp_hbf_cascade_f32 *out);
/* Fill `out` like `HBF_INT_CASCADE` (src/hbf.rs:476-512: tuple index 0 first). */
int idsp_hbf_int_cascade(int tap_set, int stages, idsp_hbf_cascade_f32 *out);
/* `hbf_dec_response_length` / `hbf_int_response_length` (src/hbf.rs:424-448,515-539)
 * generalised to an arbitrary cascade. */
int idsp_hbf_dec_response_length(const idsp_hbf_cascade_f32 *cfg);
int idsp_hbf_int_response_length(const idsp_hbf_cascade_f32 *cfg);

/* State words per lane: for each stage s in processing order
 *   decimator   `HbfDec`  (src/hbf.rs:142-145): even[m-1] then odd[2m-1], oldest first
 *   interpolator `HbfInt` (src/hbf.rs:196-198): x[2m-1], oldest first
 * i.e. exactly the samples `copy_within` keeps (src/hbf.rs:182-183,224). */
size_t idsp_hbf_dec_state_words(const idsp_hbf_cascade_f32 *cfg);
size_t idsp_hbf_int_state_words(const idsp_hbf_cascade_f32 *cfg);

/* Half-band decimator cascade, rate change R = 2^stages
 * (`SplitProcess<[f32; R], f32, _>` for the `Major`/`ChunkIn` nest,
 * src/hbf.rs:156-192,385-421).  `frames` counts OUTPUT samples per lane; each
 * input element is a chunk `[f32; R]` of R consecutive high-rate samples:
 *   FRAME_MAJOR  x[(f*lanes + l)*R + k]   y[f*lanes + l]
 *   LANE_MAJOR   x[(l*frames + f)*R + k]  y[l*frames + f]   (lane = contiguous stream)
 */
int idsp_hbf_dec_f32(const idsp_hbf_cascade_f32 *cfg, void *state, const float *x, float *y,
                     size_t lanes, size_t frames, int layout, void *stream);
/* Half-band interpolator cascade (src/hbf.rs:200-236,476-512).  `frames`
 * counts INPUT samples per lane; each output element is a chunk `[f32; R]`:
 *   FRAME_MAJOR  x[f*lanes + l]   y[(f*lanes + l)*R + k]
 *   LANE_MAJOR   x[l*frames + f]  y[(l*frames + f)*R + k]
 */
int idsp_hbf_int_f32(const idsp_hbf_cascade_f32 *cfg, void *state, const float *x, float *y,
                     size_t lanes, size_t frames, int layout, void *stream);

/* Same-rate linear-phase FIR, `SplitProcess<f32, f32, [f32; N]>` for the four
 * symmetry types of `type_fir!` (src/hbf.rs:70-138, `get()` :46-68):
 *   window w of 2M + odd samples ending at the current input,
 *   y = sum_k (w[2M-1+odd-k] +/- w[k]) * tap[k]  (+ w[M] for ODD_SYMMETRIC: unity centre tap)
 * State words per lane: the last LEN = 2M - 1 + odd inputs, oldest first
 * (what `copy_within` keeps, src/hbf.rs:103,121). */
typedef enum idsp_fir_kind {
    IDSP_FIR_ODD_SYMMETRIC = 0,     /* Type I,   `OddSymmetric`      src/hbf.rs:129 */
    IDSP_FIR_EVEN_SYMMETRIC = 1,    /* Type II,  `EvenSymmetric`     src/hbf.rs:131 */
    IDSP_FIR_ODD_ANTISYMMETRIC = 2, /* Type III, `OddAntiSymmetric`  src/hbf.rs:134 */
    IDSP_FIR_EVEN_ANTISYMMETRIC = 3 /* Type IV,  `EvenAntiSymmetric` src/hbf.rs:136 */
} idsp_fir_kind;

typedef struct idsp_fir_sym_f32 {
    int32_t kind; /* idsp_fir_kind */
    int32_t m;    /* one-sided tap count, 1..IDSP_HBF_MAX_TAPS */
    float taps[IDSP_HBF_MAX_TAPS];
} idsp_fir_sym_f32;

size_t idsp_fir_sym_state_words(const idsp_fir_sym_f32 *cfg);
int idsp_fir_sym_f32_process(const idsp_fir_sym_f32 *cfg, void *state, const float *x, float *y,
                             size_t lanes, size_t frames, int layout, void *stream);

/* The same three processors on f64 samples with f64 taps: `EvenSymmetric<[C; M]>` and the `type_fir!` types are generic in
 * the sample type (src/hbf.rs:70-138, `T: Mul<C, Output = T>`), so `HbfDec<[f64; N]>` / `HbfInt<[f64; N]>` cascades run
 * with `[f64; M]` taps.  Same definitions as the f32 entries above; every f64 state value takes two state words
 * (value v -> words 2v: low half, 2v + 1: high half), so the `_f64` word counts are twice the f32 ones.  The cascade
 * builders widen the built-in f32 tap sets exactly (an f32 is an f64). */
typedef struct idsp_hbf_cascade_f64 {
    int32_t stages;
    int32_t m[IDSP_HBF_MAX_STAGES];
    double taps[IDSP_HBF_MAX_STAGES][IDSP_HBF_MAX_TAPS];
} idsp_hbf_cascade_f64;
typedef struct idsp_fir_sym_f64 {
    int32_t kind; /* idsp_fir_kind */
    int32_t m;
    double taps[IDSP_HBF_MAX_TAPS];
} idsp_fir_sym_f64;
int idsp_hbf_dec_cascade_f64(int tap_set, int stages, idsp_hbf_cascade_f64 *out);
int idsp_hbf_int_cascade_f64(int tap_set, int stages, idsp_hbf_cascade_f64 *out);
size_t idsp_hbf_dec_state_words_f64(const idsp_hbf_cascade_f64 *cfg);
size_t idsp_hbf_int_state_words_f64(const idsp_hbf_cascade_f64 *cfg);
size_t idsp_fir_sym_state_words_f64(const idsp_fir_sym_f64 *cfg);
int idsp_hbf_dec_f64(const idsp_hbf_cascade_f64 *cfg, void *state, const double *x, double *y,
                     size_t lanes, size_t frames, int layout, void *stream);
int idsp_hbf_int_f64(const idsp_hbf_cascade_f64 *cfg, void *state, const double *x, double *y,
                     size_t lanes, size_t frames, int layout, void *stream);
int idsp_fir_sym_f64_process(const idsp_fir_sym_f64 *cfg, void *state, const double *x, double *y,
                             size_t lanes, size_t frames, int layout, void *stream);

/* ------------------------------------------------------------------------ */
/* cossin / Accu DDS / Lockin                                               */
/* ------------------------------------------------------------------------ */

/* `cossin(phase)` (src/cossin.rs:14-67) elementwise: out[2*i] = cos, out[2*i+1]
 * = sin — the `cossin(p) -> i32[N,2]` function of src/py.rs:10-28. */
int idsp_cossin_i32(const int32_t *phase, int32_t *out, size_t n, void *stream);

/* `atan2(y, x)` (src/atan2.rs:66-82) elementwise over rows [x, y] — the
 * `atan2(xy: i32[N,2]) -> i32[N]` function of src/py.rs:30-47 and `Complex::<i32>::arg`
 * (src/complex.rs:254-256) for `Complex<i32>` = [re, im] rows such as the lock-in output.
 * Result: i32::MIN = -pi ... i32::MAX = one count below +pi. */
int idsp_atan2_i32(const int32_t *xy, int32_t *out, size_t n, void *stream);

/* DDS: per lane `Accu<Wrapping<i32>>` (src/accu.rs:34-41, pre-increment) feeding
 * `Complex::<i32>::from_angle` (src/complex.rs:237-240).  State words per lane:
 * { accu.state, accu.step }.  Output element = Complex<i32> = [re, im] adjacent
 * (src/complex.rs:15-20): out[(index(f,l))*2 + {0,1}]. */
int idsp_dds_i32(void *state, int32_t *out, size_t lanes, size_t frames, int layout,
                 void *stream);

#define IDSP_LOCKIN_MAX_CASCADE 4

/* `Lockin<[Lowpass<N>; K]>` (src/lockin.rs:11-39, src/lowpass.rs:13-80).
 * order = N (1 or 2), cascade = K (1..IDSP_LOCKIN_MAX_CASCADE),
 * k[c][0..N) = `Lowpass<N>.0` of cascade element c. */
typedef struct idsp_lockin_i32 {
    int32_t order;
    int32_t cascade;
    int32_t k[IDSP_LOCKIN_MAX_CASCADE][2];
} idsp_lockin_i32;

/* State words per lane: { accu.state, accu.step } followed by
 * `[[LowpassState<N>; K]; 2]` (index 0 = I/re, 1 = Q/im), each i64 as lo,hi:
 *   word 2 + ((iq*K + c)*N + j)*2 + {0: lo, 1: hi}. */
size_t idsp_lockin_state_words(const idsp_lockin_i32 *cfg);

/* Phase-accumulator lock-in: per frame `phase = accu.next()`, then
 * `Lockin::process(state, (x, Wrapping(phase)))` (src/lockin.rs:30-39):
 * cossin -> `x * Q32<32>` mix (dsp-fixedpoint/src/lib.rs:449-456) -> the lowpass
 * cascade on I and Q.  Output Complex<i32>: y[index(f,l)*2 + {0: re, 1: im}]. */
int idsp_lockin_i32_process(const idsp_lockin_i32 *cfg, void *state, const int32_t *x,
                            int32_t *y, size_t lanes, size_t frames, int layout,
                            void *stream);

/* The lock-in above with the polar read-out of its `Complex<i32>` output fused in (SURVEY 8f rank 2:
 * cossin -> mix -> lowpass -> atan2 in one pass, no Complex<i32> round trip through memory):
 *   _arg:      y[index(f,l)] = `Lockin::process(..).arg()`       (src/complex.rs:254-256 -> src/atan2.rs:66-82), i32
 *   _norm_sqr: y[index(f,l)] = `Lockin::process(..).norm_sqr()`  (src/complex.rs:214-217), i64; the sum wraps
 *              for (i32::MIN, i32::MIN) as in a release build.
 * Same cfg and state as idsp_lockin_i32_process; the three entries may be mixed on one state. */
int idsp_lockin_i32_arg(const idsp_lockin_i32 *cfg, void *state, const int32_t *x, int32_t *y,
                        size_t lanes, size_t frames, int layout, void *stream);
int idsp_lockin_i32_norm_sqr(const idsp_lockin_i32 *cfg, void *state, const int32_t *x,
                             int64_t *y, size_t lanes, size_t frames, int layout, void *stream);

/* ---- `Lockin<C>` as the reference defines it (src/lockin.rs:11-39): any arm filter `C: SplitProcess<X, X, S>`, the LO
 * either from a phase (:30-39, the entries above and idsp_lockin_i32_biquad_process) or given per sample (:17-27, the `_lo`
 * entries).  Arm filters here: `[Lowpass<N>; K]` (idsp_lockin_i32 above) and `[Biquad<C>; n]` x `[DirectForm1<T>; n]`
 * (src/iir/biquad.rs:366-383 under the array composition of dsp-process/src/compose.rs:80-113; n = 1 is a plain
 * `Biquad<C>`), 1 <= n <= IDSP_LOCKIN_MAX_SECTIONS; the same sections run on I (`state[0]`) and on Q (`state[1]`).
 * External LO: lo[index(f,l)*2 + {0: re, 1: im}] holds `Complex<Q32<32>>` bits (i32) or `Complex<f32>`; the mixer is
 * `x * lo.re`, `x * lo.im` — for i32 `((q as i64 * x as i64) >> 32) as i32` (dsp-fixedpoint/src/lib.rs:449-456), for f32 one
 * rounded multiply — and the output `Complex<X>` = [re, im] adjacent as above.  x, lo and y are three separate buffers
 * (overlap is IDSP_EINVAL), lo and y 8-byte aligned (they hold pairs).
 * The f32 entry with lo = (cos, -sin) is the `mix * lowpass.lanes()` graph of examples/ddc_lockin.rs:35-42.
 * State words per lane: phase form { accu.state, accu.step, I: n x {x0,x1,y0,y1}, Q: n x {x0,x1,y0,y1} };
 * `_lo` forms: the two arms only — biquad arms { I: n x {x0,x1,y0,y1}, Q: ... }, lowpass arms the words of
 * idsp_lockin_state_words() without its first two (idsp_lockin_state_words(cfg) - 2). */
#define IDSP_LOCKIN_MAX_SECTIONS 4
size_t idsp_lockin_biquad_state_words(size_t n, int with_accu);
int idsp_lockin_i32_biquad_process(const idsp_biquad_i32 *sections, size_t n, void *state, const int32_t *x, int32_t *y,
                                   size_t lanes, size_t frames, int layout, void *stream);
int idsp_lockin_i32_lo_process(const idsp_lockin_i32 *cfg, void *state, const int32_t *x, const int32_t *lo, int32_t *y,
                               size_t lanes, size_t frames, int layout, void *stream);
int idsp_lockin_i32_biquad_lo_process(const idsp_biquad_i32 *sections, size_t n, void *state, const int32_t *x,
                                      const int32_t *lo, int32_t *y, size_t lanes, size_t frames, int layout, void *stream);
int idsp_lockin_f32_biquad_lo_process(const idsp_biquad_f32 *sections, size_t n, void *state, const float *x,
                                      const float *lo, float *y, size_t lanes, size_t frames, int layout, void *stream);

/* `Lowpass<N>` cascade alone on a real stream (src/lowpass.rs:47-78; array
 * composition dsp-process/src/compose.rs:80-113).  State: `[LowpassState<N>; K]`
 * words ((c*N + j)*2 + {lo,hi}). */
int idsp_lowpass_i32(const idsp_lockin_i32 *cfg, void *state, const int32_t *x, int32_t *y,
                     size_t lanes, size_t frames, int layout, void *stream);

/* FM discriminator receiver core of examples/fm_disc.rs:25-50, `(disc * deemph).minor()`:
 *   z = x * conj(prev.into_bits())   (`Complex<Q32<32>> * Complex<i32>`, src/complex.rs:117-134:
 *        re = (x.re*p.re - x.im*(-p.im)) >> 32, im = (x.re*(-p.im) + x.im*p.re) >> 32, i64 wrapping)
 *   d = z.arg() - carrier            (src/complex.rs:254-256 -> atan2, wrapping; 0 while prev is None)
 *   y = deemph(d)                    (`Biquad<Q32<F>>` x `DirectForm1`, src/iir/biquad.rs:366-383)
 * x holds `Complex<Q32<32>>` bits [re, im] per sample (8 bytes), y one i32 per sample.
 * State words per lane: {has_prev, prev.re, prev.im, x0, x1, y0, y1}; zero = (None, DirectForm1::default()). */
typedef struct idsp_fm_disc {
    int32_t carrier;
    idsp_biquad_i32 deemph;
} idsp_fm_disc;
#define IDSP_FM_DISC_STATE_WORDS 7
int idsp_fm_disc_i32(const idsp_fm_disc *cfg, void *state, const int32_t *x, int32_t *y,
                     size_t lanes, size_t frames, int layout, void *stream);

/* ---- phase consumers: what follows `arg()`, the discriminator or a DDS phase in a demodulation chain.  Wrapping i32 phase
 * in (2^32 = one turn), one independent recurrence per lane, all integer and bit-exact; x and y in either layout, y == x
 * allowed where the output element is 4 bytes.  The all-zero state is the reference's `Default::default()`.
 *
 * `ClampWrap<W<i32>>` (src/unwrap.rs:166-194, `overflowing_sub` :73-80): maps wraps of the input to saturation.
 * State words per lane: { x0, clamp as -1 / 0 / 1 (`Wrap`, src/unwrap.rs:18-27) }. */
int idsp_clamp_wrap_i32(void *state, const int32_t *x, int32_t *y, size_t lanes, size_t frames, int layout, void *stream);

/* `Unwrapper<i64>` fed i32 (src/unwrap.rs:109-156).  State words per lane: { y lo, y hi }.
 *   idsp_unwrap_i32:       dx[index(f,l)] = `process(x)`, the wrapped difference to the previous sample (i32)
 *   idsp_unwrap_i32_phase: y[index(f,l)]  = `phase::<i64>()` after the sample, the unwrapped running phase (i64)
 * The two may be mixed on one state; `wraps::<i32, S>()` (:119-127) is host arithmetic on the state.
 * idsp_unwrap_i32_phase: y must be 8-byte aligned (IDSP_EINVAL otherwise, nothing is written). */
int idsp_unwrap_i32(void *state, const int32_t *x, int32_t *dx, size_t lanes, size_t frames, int layout, void *stream);
int idsp_unwrap_i32_phase(void *state, const int32_t *x, int64_t *y, size_t lanes, size_t frames, int layout, void *stream);

/* `PLL` (src/pll.rs:33-107): type-2, order-3 phase-locked loop on a sampled phase.  ba = `PLL::ba` as `Q32<32>` bits.
 * State words per lane (`PLLState`, :62-75): { clamp.x0, clamp.clamp as -1 / 0 / 1, z0, y0, f0 lo, f0 hi, f lo, f hi, y }.
 * output: IDSP_PLL_PHASE      y[index(f,l)] = `process(x)`, the output phase (:106)
 *         IDSP_PLL_FREQUENCY  y[index(f,l)] = `state.frequency()` after the sample (:84-86)
 *         IDSP_PLL_BOTH       y[index(f,l)*2 + {0: phase, 1: frequency}] (y holds 2*lanes*frames words, 8-byte aligned — IDSP_EINVAL
 *                             otherwise, nothing is written; no in-place form)
 * `state.phase()` / `state.frequency()` after a call are state word 8 / state word 7. */
#define IDSP_PLL_STATE_WORDS 9
#define IDSP_PLL_PHASE 0
#define IDSP_PLL_FREQUENCY 1
#define IDSP_PLL_BOTH 2
size_t idsp_pll_state_words(void);
int idsp_pll_i32(const int32_t ba[3], void *state, const int32_t *x, int32_t *y, size_t lanes, size_t frames, int layout,
                 int output, void *stream);
/* `PLL::from_zpk(zero, pole, gain)` (src/pll.rs:42-46) and `PLL::from_bandwidth(bw, split)` (:51-57): host code, no GPU needed.
 * The arguments are narrowed to f32 first and the arithmetic runs in f32 in the reference's order; each coefficient is
 * `Q32::<32>::from_f32`: times 2^32, rounded half away from zero, saturating (NaN -> 0). */
int idsp_pll_from_zpk(double zero, double pole, double gain, int32_t ba[3]);
int idsp_pll_from_bandwidth(double bw, double split, int32_t ba[3]);

/* ------------------------------------------------------------------------ */
/* four-channel polyphase channelizer (examples/polyphase_channelizer.rs)   */
/* ------------------------------------------------------------------------ */
/*
 * A maximally decimated polyphase FIR bank on complex f32 frames, optionally followed by a 4-point DFT.  One lane is one
 * independent input stream with its own `BankState` (:46-50).  The element of x and of y is a `Frame` = `[[f32; 2]; 4]` (:22-25),
 * 8 floats `[m][re, im]`, under the convention of the `[f32; R]` elements of idsp_hbf_dec_f32:
 *   FRAME_MAJOR x[(f*lanes + l)*8 + k],  LANE_MAJOR x[(l*frames + f)*8 + k];  `frames` counts frames (4 input samples each).
 * Per frame, `PolyphaseBank::process` (:57-75): head = (head + taps - 1) % taps; hist[head] = x; y = +0.0; then for tap = 0 .. taps
 * in that order, for each m and each of re / im: y[m][c] = y[m][c] + hist[(head + tap) % taps][m][c] * coeff[tap][m] — one IEEE
 * multiply, then one IEEE add, never fused.  dft = 1 hands y to `Dft4::process` (:80-100, the eight sums as written, left to
 * right): the `.minor()` tuple of :107.  M stays 4, the only size `Dft4` defines an order of additions for.
 * State: 8*taps + 1 words per lane, state[w*lanes + lane]: word (slot*4 + m)*2 + c is `hist[slot][m][c]` in the reference's
 * physical slot order, word 8*taps is `head`; all zero is `Default`.  Read at entry and written at exit: chunked calls equal
 * one long call bit for bit, in y and in every state word.  A head >= taps is a caller error; it is taken modulo taps.
 * y == x is allowed (same-rate operator); any other overlap of x and y is IDSP_EINVAL, as are taps outside
 * 1..IDSP_PFB_MAX_TAPS, a dft other than 0 / 1, a bad layout, NULL pointers with work to do and an x or y that is not 16-byte
 * aligned.  lanes == 0 or frames == 0 launches nothing, as for idsp_fir_sym_f32_process.
 */
#define IDSP_PFB_MAX_TAPS 16
typedef struct idsp_pfb_f32 {
    int32_t taps;                        /* 1..IDSP_PFB_MAX_TAPS (`TAPS`, :20: 8) */
    int32_t dft;                         /* 0: `PolyphaseBank` alone (:57-75), 1: `PolyphaseBank` -> `Dft4` (:80-100, :107-109) */
    float coeff[IDSP_PFB_MAX_TAPS][4];   /* coeff[tap][m] = prototype[tap*4 + m] (`bytemuck::cast`, :104) */
} idsp_pfb_f32;
/* 8*taps + 1 (`BankState`, :46-50); 0 for an invalid configuration. */
size_t idsp_pfb_state_words(const idsp_pfb_f32 *cfg);
/* `prototype()` (:29-44) for 4*taps coefficients: a Hamming-windowed sinc at 0.9 of the channel spacing, normalised to a sum of
 * one; f32 throughout in the reference's order of operations.  Sets taps and dft = 1.  Host code, no GPU needed. */
int idsp_pfb_prototype_f32(int taps, idsp_pfb_f32 *out);
/* `PolyphaseBank::process` (:57-75), then `Dft4::process` (:80-100) when cfg->dft, over `frames` frames of every lane. */
int idsp_pfb_f32_process(const idsp_pfb_f32 *cfg, void *state, const float *x, float *y, size_t lanes, size_t frames, int layout,
                         void *stream);

/* ------------------------------------------------------------------------ */
/* CORDIC family (src/cordic.rs)                                            */
/* ------------------------------------------------------------------------ */
/*
 * `cordic::<VECTORING, COORD>(x, y, z, None)` (src/cordic.rs:13-77) elementwise: 30 table entries, every +, - and negation of x, y
 * and z wrapping (release build), `>>` arithmetic.  Pre-rotation (:25-34): vectoring flips when x < 0, rotating when
 * z.wrapping_sub(i32::MIN >> 1) < 0; a flip negates x and y and subtracts i32::MIN from z.  Sigma (:55): vectoring y <= 0,
 * rotating z >= 0.  Hyperbolic mode shifts by i = j + 1 for table entry j and runs the micro-rotation twice at i = 4 and at
 * i = 13 (:43-52); linear mode computes its angle as (0x80000000u32 >> j) as i32 and leaves x alone (:39-41).
 * xy: n rows [x, y] (`Complex<i32>`, 8-byte aligned); z: n words, or NULL for z = 0 in every element.  The pair functions
 * write n rows [first, second] of the reference's tuple, mul and div write n words:
 *   cos_sin     (:80-82)    [F*(x cos(pi z) - y sin(pi z)), F*(x sin(pi z) + y cos(pi z))]
 *   sqrt_atan2  (:85-87)    [F*sqrt(x^2 + y^2), z + atan2(y, x)/pi]
 *   cosh_sinh   (:100-102)  [G*(x cosh z + y sinh z), G*(x sinh z + y cosh z)]
 *   sqrt_atanh2 (:105-107)  [G*sqrt(x^2 - y^2), z + atanh2(y, x)]
 *   mul         (:90-92)    y + x*z          div (:95-97)  z + y/x
 * with F = idsp_cordic_circular_gain(), G = idsp_cordic_hyperbolic_gain() (build.rs:80, :92-104), angles of the circular
 * functions in turns (2^31 = pi) and of the hyperbolic ones in units of 2^-31.  The functions are elementwise: one call serves
 * FRAME_MAJOR and LANE_MAJOR buffers alike, such as the `Complex<i32>` output of idsp_lockin_i32_process or idsp_dds_i32.
 * In place: out == xy for the four pair functions, out == z for mul and div; any other overlap of out with an input is
 * IDSP_EINVAL, as are a NULL xy or out with n > 0 and an xy or pair out that is not 8-byte aligned.  n == 0 returns IDSP_OK
 * before any pointer check, as idsp_atan2_i32.
 */
int idsp_cordic_cos_sin_i32(const int32_t *xy, const int32_t *z, int32_t *out, size_t n, void *stream);
int idsp_cordic_sqrt_atan2_i32(const int32_t *xy, const int32_t *z, int32_t *out, size_t n, void *stream);
int idsp_cordic_cosh_sinh_i32(const int32_t *xy, const int32_t *z, int32_t *out, size_t n, void *stream);
int idsp_cordic_sqrt_atanh2_i32(const int32_t *xy, const int32_t *z, int32_t *out, size_t n, void *stream);
int idsp_cordic_mul_i32(const int32_t *xy, const int32_t *z, int32_t *out, size_t n, void *stream);
int idsp_cordic_div_i32(const int32_t *xy, const int32_t *z, int32_t *out, size_t n, void *stream);
/* `CORDIC_CIRCULAR_GAIN` (build.rs:80) and `CORDIC_HYPERBOLIC_GAIN` (build.rs:92-104).  Host code, no GPU needed. */
double idsp_cordic_circular_gain(void);
double idsp_cordic_hyperbolic_gain(void);

/* ------------------------------------------------------------------------ */
/* exponential swept sine: `Sweep`, `AccuOsc` (src/sweptsine.rs)            */
/* ------------------------------------------------------------------------ */
/*
 * Per lane `AccuOsc<Sweep>` with `Osc` for `W<i32>` (src/sweptsine.rs:22-32, :180-188): an exponentially growing phase increment
 * `state: i64` with a first-order delta-sigma modulator in its low word, integrated by `Integrator<Wrapping<i64>>`
 * (dsp-process/src/basic.rs:461-466) into `accu`, whose high word is the argument of cossin.  One frame:
 *     s  = state
 *     t  = wrapping_i64(s + 2^31) >> 32           arithmetic shift; t fits an i32
 *     ns = s + rate * t                           exact; rate * t fits an i64
 *     if ns is outside i64:                       the reference's `checked_add` -> None
 *         out = (0, 0); nothing changes           the lane has ENDED and stays ended
 *     else:
 *         state = ns; accu = wrapping_i64(accu + s); emitted += 1
 *         out = cossin((accu >> 32) as i32)       (re, im) = (cos, sin)
 * `s + BIAS` is a plain `+` in the reference: it wraps in a release build and panics in a debug build; this is the wrapping form.
 * The reference's iterator stops at the end, a block call has a fixed frame count: an ended lane writes (0, 0) — a pair cossin
 * never returns — and its state does not move.  "Ended" is a pure function of (state, rate); no flag is stored.
 * State words per lane: { state lo, state hi, accu lo, accu hi, rate, emitted lo, emitted hi }.  `emitted` counts the samples
 * produced since the state was created (it wraps): the caller sets it to 0 and reads where each lane stopped from it.
 * Output element = Complex<i32> = [re, im] adjacent, laid out as in idsp_dds_i32; both layouts, any lane and frame count.
 * `out` must be 8-byte aligned (IDSP_EINVAL otherwise, nothing is written).
 */
#define IDSP_SWEEP_STATE_WORDS 7
size_t idsp_sweep_state_words(void);
int idsp_sweep_i32(void *state, int32_t *out, size_t lanes, size_t frames, int layout, void *stream);

/* `Sweep`'s host functions with the reference's types and order of operations.  Host code, no GPU needed.
 * idsp_sweep_fit: `Sweep::fit(stop, harmonics, cycles)` (:108-118) in f32 — stop: the highest frequency in units of the sample
 * rate (0 ..= 0.5), harmonics: how many harmonics the sweep covers, cycles: phase wraps per harmonic (>= 1).  `cycles as i64`
 * truncates, the `<< 32` drops bits.  IDSP_EINVAL with idsp_last_error() = "Stop out of bounds" (a NaN stop included) or
 * "Start out of bounds" (state <= 0), the reference's `SweepError` texts; rate and state are written on success only.
 * The descriptors (:43-81) are f64: rate() = ln_1p(rate / 2^32), delay(h) = ln(h) / rate(), octave() = LN_2 / rate(),
 * decade() = LN_10 / rate(), cycles() = state / (2^32 rate), state() = cycles() rate(), continuous(t) = cycles() exp(rate() t).
 * idsp_sweep_inverse_filter: `Sweep::inverse_filter(f)` (:93-101) in f32, out = [re, im].
 * The f32 arguments travel as double and are narrowed to f32 on entry, as in idsp_pll_from_zpk (every f32 is a double).
 * `Osc` for f32 and f64 (libm `sin_cos` of radians) has no entry: it cannot be held to bit equality on the device. */
int idsp_sweep_fit(double stop, double harmonics, double cycles, int32_t *rate, int64_t *state);
double idsp_sweep_rate(int32_t rate);
double idsp_sweep_delay(int32_t rate, double harmonic);
double idsp_sweep_octave(int32_t rate);
double idsp_sweep_decade(int32_t rate);
double idsp_sweep_cycles(int32_t rate, int64_t state);
double idsp_sweep_state(int32_t rate, int64_t state);
double idsp_sweep_continuous(int32_t rate, int64_t state, double t);
int idsp_sweep_inverse_filter(int32_t rate, int64_t state, double f, float out[2]);

/* ------------------------------------------------------------------------ */
/* reciprocal PLL: `RPLLConfig`, `RPLL` (src/rpll.rs) and the batch LO       */
/* ------------------------------------------------------------------------ */
/*
 * Per lane `RPLLConfig::process` on `RPLL` (src/rpll.rs:13-78): quantised edge timestamps of a reference signal, at most one per
 * `update()`, in; the phase and frequency of the `update()` calls relative to that reference (2^32 = one turn, one turn per
 * update) out, as the `Accu<W<i32>>` the reference returns.  One independent recurrence per lane, all integer and bit-exact.
 *   ts   one `Option<W<i32>>` per lane and frame as two adjacent words: ts[index(f,l)*2 + {0: some, 1: x}].  some == 0 is `None`
 *        and x is then ignored; any other value is `Some(x)`.
 *   accu the returned `Accu` as two adjacent words: accu[index(f,l)*2 + {0: state = y, 1: step = f as i32}] (:76).
 * index(f,l) as everywhere: FRAME_MAJOR f*lanes + l, LANE_MAJOR l*frames + f; any lane count.  ts and accu are separate buffers
 * (any overlap is IDSP_EINVAL, there is no in-place form) and 8-byte aligned.
 * One sample, with the wrapping semantics of a release build (:47-77):
 *     y += (i32)f                                              :51
 *     if some:
 *         dx    = x - x0 (wrapping i32);  x0 = x               :54-56
 *         p64   = (u64)ff * (u64)(i64)dx                       :58   `dx.0 as u64` SIGN-extends; the product wraps mod 2^64
 *         p_sig = (u32)((p64 + (1 << (sf-1))) >> sf)           :60-62 u64 wrapping add, logical shift, truncation
 *         p_ref = 1u32 << (32 + dt2 - sf)                      :64
 *         ff   += p_ref - p_sig            (wrapping u32)      :66
 *         dt    = (u32)((-x) & ((1 << dt2) - 1))               :68
 *         y_ref = (i32)((f >> dt2) * dt)                       :70   the OLD f, logical shift, wrapping u32 product
 *         dy    = (y_ref - y) >> (sp - dt2)                    :72   y already advanced; wrapping sub, ARITHMETIC shift
 *         f     = ff + (u32)dy                                 :74   the NEW ff
 *     return { y, (i32)f }
 * with sf = shift_frequency, sp = shift_phase.  State words per lane (`RPLL`, :13-18), state[w*lanes + lane]: { x, ff, f, y }; all
 * zero is `RPLL::default()`.  Read at entry and written at exit: consecutive calls on one state equal one long call bit for bit.
 * `phase()` / `frequency()` (:80-90) after a call are state word 3 / state word 2.
 * IDSP_EINVAL unless 0 <= dt2 <= 30, dt2 < shift_frequency <= 32 and dt2 <= shift_phase <= dt2 + 31: the ranges in which every
 * shift above is defined.  They come from the shifts, not from the reference's `debug_assert`s (:48-49):
 * shift_frequency == dt2 passes the assert, but `1u32 << 32` at :64 then overflows (a panic in a debug build, a shift by 0 in
 * a release build), so it is rejected.
 */
typedef struct idsp_rpll {
    int32_t dt2;              /* 1 << dt2: counter rate to update() rate ratio (:24-25) */
    int32_t shift_frequency;  /* 1 << shift_frequency: frequency lock settling time in counter periods (:26-31) */
    int32_t shift_phase;      /* phase lock settling time, usually shift_frequency - 1 (:32-35) */
} idsp_rpll;                  /* RPLLConfig, src/rpll.rs:23-36 */
#define IDSP_RPLL_STATE_WORDS 4
size_t idsp_rpll_state_words(void);
int idsp_rpll_i32(const idsp_rpll *cfg, void *state, const int32_t *ts, int32_t *accu, size_t lanes, size_t frames, int layout,
                  void *stream);

/* The local oscillator of a batch from the `Accu` the RPLL returned.  `update()` runs once per batch of 2^k samples
 * (k = batch_log2), and the sample phases of the batch are iterated from the returned `Accu` with the reference's own operators:
 * `Accu * T` (src/accu.rs:40-46), `Accu + Accu` (:48-54), the pre-incrementing `next()` (:34-37) and
 * `Complex::<i32>::from_angle` (src/complex.rs:237-240, i.e. cossin).  accu: `updates` rows of { state, step } pairs in the layout
 * of idsp_rpll_i32's output with frames = updates.  lo: `Complex<i32>` [re, im] for frames = updates << k samples per lane in the
 * same layout — exactly the `lo` argument of idsp_lockin_i32_lo_process.  For sample t = u*2^k + j, 0 <= j < 2^k, of lane l, with
 * a = accu[u, l]:
 *     sample = Accu::new(a.state, ((u32)a.step >> k) as i32) * harmonic + Accu::new(offset, 0)     all wrapping
 *     phase  = sample.state + (j + 1) * sample.step                                                j + 1 calls of next()
 *     lo[t, l] = cossin(phase)                                                                      re = cos, im = sin
 * The LOGICAL shift of the step by k is the one operation here that is not in the reference: the RPLL's f is phase per
 * update(), and a batch holds 2^k samples per update.
 * No state: a call on rows [u0, u1) equals those rows of a longer call.  IDSP_EINVAL unless 0 <= batch_log2 <= 24 and
 * updates << batch_log2 is a frame count every stream entry accepts (<= 2^40); accu and lo are 8-byte aligned and must not overlap.
 */
typedef struct idsp_accu_lo {
    int32_t batch_log2;  /* k: 2^k samples per update() */
    int32_t harmonic;    /* `Accu * harmonic` */
    int32_t offset;      /* `+ Accu::new(offset, 0)`: phase offset of the LO */
} idsp_accu_lo;
int idsp_accu_lo_i32(const idsp_accu_lo *cfg, const int32_t *accu, int32_t *lo, size_t lanes, size_t updates, int layout,
                     void *stream);

/* idsp_accu_lo_i32 followed by idsp_lockin_i32_lo_process, with the LO never stored: the lock-in with `[Lowpass<N>; K]` arms
 * (src/lockin.rs:17-39) whose LO is iterated inside the kernel from the `Accu` rows (src/accu.rs:34-54, `Complex::from_angle`
 * src/complex.rs:237-240).  y and the state are bit for bit those of
 *     idsp_accu_lo_i32(lo_cfg, accu, lo, lanes, updates, layout, stream);
 *     idsp_lockin_i32_lo_process(cfg, state, x, lo, y, lanes, updates << lo_cfg->batch_log2, layout, stream);
 * without the 8 bytes per sample of `lo` being written and read again (nor allocated: 2 GiB at 65536 lanes x 4096 frames).
 *   x     frames = updates << batch_log2 i32 samples per lane
 *   accu  `updates` rows of { state, step } pairs per lane, as idsp_rpll_i32 writes them
 *   y     frames `Complex<i32>` [re, im] per lane
 * all three in `layout`, as the two entries above define it.  State: the two arms only, idsp_lockin_state_words(cfg) - 2 words
 * per lane — the state of idsp_lockin_i32_lo_process, and the two entries may be mixed on one state mid-stream.  Read at entry,
 * written at exit: consecutive calls on update ranges equal one long call.
 * IDSP_EINVAL (and nothing written) unless cfg has order 1..2 and cascade 1..IDSP_LOCKIN_MAX_CASCADE, 0 <= batch_log2 <= 24,
 * updates << batch_log2 <= 2^40, accu and y are 8-byte aligned and x, accu and y are pairwise disjoint (no in-place form: x is 4
 * bytes per sample and y 8).  lanes == 0 or updates == 0 is IDSP_OK.
 * When to prefer it (MI355X, 4096 output frames, k = 3, three low-pass shapes; profiles/NOTES.md, "Lock-in on Accu rows"): at 65536
 * lanes it takes 0.46-0.52 of the chain's time FrameMajor and 0.64-0.69 LaneMajor, at 32768 lanes 0.77-0.85 and 0.95-0.97.  At 16384
 * lanes the CHAIN is the faster route: this entry takes 1.08-1.22 x its time FrameMajor and 1.22-1.32 x LaneMajor.  The chain's
 * lock-in runs the multi-wave kernels and this entry has no multi-wave form; at that lane count the bytes it saves no longer pay
 * for the difference.  Where between 16384 and 32768 lanes the two cross was not measured.  What it always saves is the LO buffer. */
int idsp_lockin_i32_accu_process(const idsp_lockin_i32 *cfg, const idsp_accu_lo *lo_cfg, void *state, const int32_t *x,
                                 const int32_t *accu, int32_t *y, size_t lanes, size_t updates, int layout, void *stream);

/* ------------------------------------------------------------------------ */
/* Dsm<K> — MASH-(1)^K delta-sigma modulator, u32 -> i8 (src/dsm.rs)        */
/* ------------------------------------------------------------------------ */
/*
 * `Dsm::<K>::process(x: u32) -> i8` (src/dsm.rs:44-57) per lane, K = `order` = 0..IDSP_DSM_MAX_ORDER: the output stage of the
 * reference, a 32-bit word in, the small integer a DAC, PWM or fractional-N divider consumes out.  The only entry whose output
 * element is smaller than a 32-bit word: y holds plain i8 rows, ONE BYTE per sample, in `layout`.
 * Computed as a RELEASE build of the reference computes it — every u32 and i8 operation wraps:
 *   stage fold (:47-51)          a[i], carry[i] = a[i].overflowing_add(v); v = x for stage 0, the new a[i-1] after it
 *   recombination fold (:52-56)  y = carry[K-1]; for j = 0..K-2: (y, c[j]) = (carry[K-2-j] + y - c[j], y), wrapping i8
 * What the reference leaves open and this ABI fixes:
 *   - from `Dsm::default()` no i8 operation overflows and the output stays inside 1 - 2^(K-1) ..= 2^(K-1); from arbitrary c
 *     words the second fold overflows i8 already at K = 3, where a debug build of the reference panics.  Here it wraps;
 *   - K = 1: the output is the carry.  K = 0: the output is the constant 0 (what the release build yields and the doc comment
 *     promises), there is no state and `state` may be NULL;
 *   - c[K-1] is a field of the struct that `process` never reads or writes (`take(K - 1)`).
 * State: 2 K words per lane, word-plane-major as everywhere: words 0..K-1 = a[0..K-1], words K..2K-1 = c[0..K-1].  A c word is
 * read as its low byte (`(int8_t)w`) and written back sign-extended; word 2K-1 is never written.  All zero is `Dsm::default()`.
 * Read at entry, written at exit; FRAME_MAJOR and LANE_MAJOR calls may be mixed on one state.
 * x_pitch / y_pitch: ELEMENTS between the starts of consecutive rows (frames in FRAME_MAJOR, lanes in LANE_MAJOR) of x and of
 * y, as the `_pitch` twins above define them; 0 = dense.  They belong to the one entry: i8 rows with an odd row length are the
 * normal case, and the pitch is how a caller keeps them aligned.  x must be 4-byte aligned; y may start at ANY byte and
 * y_pitch may be any value >= a row.  Bytes of y outside the `lanes` x `frames` elements (the gap of a pitched row) are not
 * written.  LANE_MAJOR rows aligned to 4 bytes (y and y_pitch multiples of 4) leave through dword stores, in about half the time of
 * unaligned ones (profiles/NOTES.md, "Dsm"); FRAME_MAJOR stores bytes whatever the alignment.
 * There is no in-place form (the elements differ in size): any overlap of the two extents, (rows-1) * pitch + row elements
 * each, is IDSP_EINVAL.  Also IDSP_EINVAL, with nothing written: an order outside 0..8, a bad layout, NULL x or y, NULL state
 * with order > 0, a pitch shorter than a row.  lanes == 0 or frames == 0 is IDSP_OK and writes nothing.
 * Asynchronous on `stream`; no host synchronisation, no allocation.
 */
#define IDSP_DSM_MAX_ORDER 8
size_t idsp_dsm_state_words(int order); /* 2 * order; 0 for an order outside 0..IDSP_DSM_MAX_ORDER */
int idsp_dsm_u32(int order, void *state, const uint32_t *x, size_t x_pitch, int8_t *y, size_t y_pitch,
                 size_t lanes, size_t frames, int layout, void *stream);

/* ------------------------------------------------------------------------ */
/* lane split over several devices in ONE process: idsp_multi_*             */
/* ------------------------------------------------------------------------ */
/*
 * Lanes never interact (`Lanes::process` indexes state[i], x[i] only, dsp-process/src/compose.rs:468-476), so G
 * devices take G contiguous lane blocks — device g gets lanes [g*L/G, (g+1)*L/G) — and there is NO data-path
 * exchange between them.  An idsp_multi holds a device list and one non-blocking stream per device; it is host-side
 * bookkeeping for hosts that drive all GPUs from one process (the Rust shim, a C program).  One process per GPU
 * (torch.distributed / MPI, each calling the plain entry points on its own lane block) is equivalent and is what
 * bench.py uses.  Per-device buffers hold that device's lane block only: LANE_MAJOR shards are contiguous pieces of
 * the host tensor, FRAME_MAJOR shards are `[[T; L/G]; frames]` tensors of their own (or lane blocks of a wider
 * tensor through the `_pitch` entries).
 */
typedef struct idsp_multi idsp_multi;

/* `devices` = n_devices device ordinals (a device may appear more than once: its lane blocks then share the
 * device); devices == NULL and n_devices <= 0 = every visible device. */
int idsp_multi_create(const int *devices, int n_devices, idsp_multi **out);
int idsp_multi_destroy(idsp_multi *m);
/* Number of lane blocks G; device ordinal and stream (hipStream_t) of block `index`. */
int idsp_multi_size(const idsp_multi *m);
int idsp_multi_device(const idsp_multi *m, int index);
void *idsp_multi_stream(const idsp_multi *m, int index);
/* Lane block [*lane_lo, *lane_hi) of block `index` for a job of `lanes` lanes. */
int idsp_multi_shard(const idsp_multi *m, size_t lanes, int index, size_t *lane_lo, size_t *lane_hi);

/* Generic driver: for every block, make its device current and call fn(user, index, lane_lo, lane_hi, stream) —
 * fn issues whatever entry points it likes on that stream for that lane block.  ANY non-zero return stops the
 * loop and is returned as it is (negative: an idsp_status; positive: the callback's own stop code).  Blocks before
 * the stopping one have been handed to fn already and their work is in flight: after a stop the per-block state is
 * indeterminate until the caller has synchronised and reloaded it; idsp_multi_last_block() names the block.
 * The caller's current device is restored. */
typedef int (*idsp_shard_fn)(void *user, int index, size_t lane_lo, size_t lane_hi, void *stream);
int idsp_multi_for_each(idsp_multi *m, size_t lanes, idsp_shard_fn fn, void *user);
/* Index of the lane block at which the most recent idsp_multi_for_each / idsp_multi_biquad_* call of this thread
 * stopped with a non-zero status; -1 if it ran through. */
int idsp_multi_last_block(void);
/* Wait for every block's stream (the "barrier" of a single-process run). */
int idsp_multi_sync(idsp_multi *m);

/* Per-block device buffers of (block lanes) * bytes_per_lane bytes, zero-filled: ptrs[G] out. */
int idsp_multi_alloc(idsp_multi *m, size_t lanes, size_t bytes_per_lane, void **ptrs);
int idsp_multi_free(idsp_multi *m, void **ptrs);
/* Scatter (to_device != 0) / gather a host array of `lanes` records of bytes_per_lane bytes, lane-contiguous (a
 * LANE_MAJOR tensor, or one state / coefficient plane), to / from the per-block buffers; asynchronous on the
 * block streams (pinned host memory overlaps). */
int idsp_multi_copy(idsp_multi *m, size_t lanes, size_t bytes_per_lane, void *const *dev_ptrs, void *host, int to_device);

/* The two headline operators over the split: state[g], x[g], y[g] are block g's device buffers; `lanes` is the
 * TOTAL lane count.  Every block's arguments are validated BEFORE any block is launched (a bad block is reported
 * with nothing in flight); a failure after that leaves earlier blocks running and the state indeterminate, see
 * idsp_multi_last_block().  Asynchronous; idsp_multi_sync() waits. */
int idsp_multi_biquad_i32_df1(idsp_multi *m, const idsp_biquad_i32 *cfg, size_t n, void *const *state,
                              const int32_t *const *x, int32_t *const *y, size_t lanes, size_t frames, int layout);
int idsp_multi_biquad_f32_df2t(idsp_multi *m, const idsp_biquad_f32 *cfg, size_t n, void *const *state,
                               const float *const *x, float *const *y, size_t lanes, size_t frames, int layout);

#ifdef __cplusplus
}
#endif
#endif /* IDSP_HIP_H */
