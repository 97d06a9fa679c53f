// pfb.hip — the reference's four-channel polyphase analysis bank (examples/polyphase_channelizer.rs): `PolyphaseBank::process`
// (:57-75), a maximally decimated polyphase FIR on complex f32 frames `[[f32; 2]; 4]`, optionally followed by `Dft4::process`
// (:80-100); plus the prototype low-pass of :29-44 (host code).  One lane is one input stream with its own `BankState` (:46-50).
//
// Both kernels are bound by HBM (32 B in, 32 B out, at taps = 8 152 f32 operations per frame and lane — several times below the
// issue roof of DESIGN §3), so each is built to read every frame once and write it once, plus halos:
//   FRAME_MAJOR  one thread per lane, the window of `taps` frames in registers (rotation fully unrolled: TAPS is a template
//                argument), the time axis cut into segments of kPfbFmSegFrames frames across waves — a call with few lanes and many
//                frames has no other parallelism, and at 16384 lanes one wave per 64 lanes alone would leave a CU with one wave.
//   LANE_MAJOR   one workgroup per (lane, tile of kPfbLmTileFrames frames): the tile goes through LDS behind `taps` frames of
//                history (as fir_sym_kernel, hbf.hip), thread i produces frame i.  A frame is kept as two 16-byte halves in two
//                planes, so the `taps` window reads of a wave are stride-1 ds_read_b128.  That is taps x 32 B of LDS reads per
//                frame: 256 + 32 B written = 288 B at taps = 8, 2.25 LDS clocks per frame and CU at 128 B/clk, against about
//                6.4 clocks the 64 B of HBM traffic take at 10 B/clk/CU (derived from the guide's rates, not measured) — so the
//                plain one-frame-per-thread form was chosen over register blocking of neighbouring frames.
// State is touched by ONE workgroup per lane (group): the one that owns the call's first frames reads it and writes it back,
// taking the call's last `taps` frames from x again when other workgroups computed them (x is unchanged then: a call with
// y == x runs unsegmented, since a segment's halo would be another segment's output).
#include <cmath>

#include "pfb.h"

namespace idsp {
namespace {

using f4 = float __attribute__((ext_vector_type(4)));

// `Frame` = [[f32; 2]; 4] (:22-25): a = {m0.re, m0.im, m1.re, m1.im}, b = {m2.re, m2.im, m3.re, m3.im}
struct Frame {
    f4 a, b;
};

struct PfbArgs {
    int32_t dft;
    float coeff[IDSP_PFB_MAX_TAPS][4];
};

// :69-70 for the four phases of one tap: one multiply, then one add (never fused: -ffp-contract=off)
__device__ __forceinline__ void bank_tap(Frame &y, const Frame h, const float c0, const float c1, const float c2, const float c3)
{
    y.a.x = y.a.x + h.a.x * c0;
    y.a.y = y.a.y + h.a.y * c0;
    y.a.z = y.a.z + h.a.z * c1;
    y.a.w = y.a.w + h.a.w * c1;
    y.b.x = y.b.x + h.b.x * c2;
    y.b.y = y.b.y + h.b.y * c2;
    y.b.z = y.b.z + h.b.z * c3;
    y.b.w = y.b.w + h.b.w * c3;
}

// `Dft4::process` (:80-100): the eight sums as written, left to right
__device__ __forceinline__ Frame dft4(const Frame v)
{
    const float x0r = v.a.x, x0i = v.a.y, x1r = v.a.z, x1i = v.a.w, x2r = v.b.x, x2i = v.b.y, x3r = v.b.z, x3i = v.b.w;
    Frame o;
    o.a.x = x0r + x1r + x2r + x3r;
    o.a.y = x0i + x1i + x2i + x3i;
    o.a.z = x0r + x1i - x2r - x3i;
    o.a.w = x0i - x1r - x2i + x3r;
    o.b.x = x0r - x1r + x2r - x3r;
    o.b.y = x0i - x1i + x2i - x3i;
    o.b.z = x0r - x1i - x2r + x3i;
    o.b.w = x0i + x1r - x2i - x3r;
    return o;
}

__device__ __forceinline__ float elem(const Frame &v, const int e)  // e is a constant after unrolling
{
    return e < 4 ? v.a[e] : v.b[e - 4];
}

// ------------------------------------------------------------------------------------------------------------ FRAME_MAJOR
// grid (64-lane groups, min(segments, 65535)), 64 threads.  Register slot r of `hist` is the physical slot of a circular bank whose
// head starts at 0 with every segment: step j of the unrolled batch writes slot TAPS - 1 - j % TAPS (:59-60), so every register
// index is a constant.  The reference's own head differs per lane and is applied where state is read and written (memory
// addresses), never to a register index.  `nxt` is a rolling prefetch B frames ahead of the frame being computed.
template <int TAPS>
__global__ __launch_bounds__(64) void pfb_frame_major(const PfbArgs a, uint32_t *st, const float *x, float *y, const size_t lanes,
                                                      const size_t frames, const size_t seg)
{
    constexpr int B = TAPS * ((8 + TAPS - 1) / TAPS);  // frames per unrolled batch: a multiple of TAPS, at least 8
    const size_t lane0 = size_t(blockIdx.x) * 64;
    const size_t lane = lane0 + threadIdx.x;
    if (lane >= lanes) return;  // no barrier in this kernel
    const uint32_t voff = threadIdx.x * 32u;
    const size_t nseg = (frames + seg - 1) / seg;
    auto load = [&](const size_t f) {
        const float *row = x + (f * lanes + lane0) * 8;
        return Frame{global_ld<f4, false>(row, voff), global_ld<f4, false>(row, voff + 16u)};
    };

    Frame hist[TAPS];
    uint32_t head0 = 0;
    size_t done = 0;  // frames of the segment computed last
    for (size_t s = blockIdx.y; s < nseg; s += gridDim.y) {
        const size_t f0 = s * seg, f1 = f0 + seg < frames ? f0 + seg : frames;
        if (s == 0) {
            // `hist[(head + k) % TAPS]` is the frame k + 1 steps back; a head >= TAPS (caller error) is reduced, so no thread leaves its lane's words
            head0 = st[size_t(8 * TAPS) * lanes + lane] % uint32_t(TAPS);
#pragma unroll
            for (int r = 0; r < TAPS; r++) {
                const size_t slot = (head0 + uint32_t(r)) % uint32_t(TAPS);
                float v[8];
#pragma unroll
                for (int e = 0; e < 8; e++) v[e] = __uint_as_float(st[(slot * 8 + e) * lanes + lane]);
                hist[r] = Frame{{v[0], v[1], v[2], v[3]}, {v[4], v[5], v[6], v[7]}};
            }
        } else {
#pragma unroll
            for (int r = 0; r < TAPS; r++) hist[r] = r < TAPS - 1 ? load(f0 - 1 - size_t(r)) : Frame{{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
        }
        Frame nxt[B];
#pragma unroll
        for (int j = 0; j < B; j++)
            if (f0 + j < f1) nxt[j] = load(f0 + j);
        for (size_t f = f0; f < f1; f += B) {
#pragma unroll
            for (int j = 0; j < B; j++) {
                if (f + j < f1) {
                    const int p = TAPS - 1 - j % TAPS;
                    hist[p] = nxt[j];
                    if (f + B + j < f1) nxt[j] = load(f + B + j);
                    Frame acc{{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};  // `Frame::default()` (:62)
#pragma unroll
                    for (int tap = 0; tap < TAPS; tap++)
                        bank_tap(acc, hist[(p + tap) % TAPS], a.coeff[tap][0], a.coeff[tap][1], a.coeff[tap][2], a.coeff[tap][3]);
                    if (a.dft) acc = dft4(acc);
                    float *row = y + ((f + j) * lanes + lane0) * 8;
                    global_st<f4, false>(row, voff, acc.a);
                    global_st<f4, false>(row, voff + 16u, acc.b);
                }
            }
        }
        done = f1 - f0;
    }
    if (blockIdx.y != 0) return;
    // register slot r holds the frame k + 1 steps back, k = (r - hr) mod TAPS, hr the register bank's head after `done` frames
    uint32_t hr = uint32_t((size_t(TAPS) - done % TAPS) % TAPS);
    if (nseg > 1) {  // other waves computed the call's end: its last TAPS frames come from x (out of place, unchanged)
#pragma unroll
        for (int r = 0; r < TAPS; r++) hist[r] = load(frames - 1 - size_t(r));
        hr = 0;
    }
    const uint32_t head = uint32_t((head0 + size_t(TAPS) - frames % TAPS) % TAPS);
#pragma unroll
    for (int r = 0; r < TAPS; r++) {
        const uint32_t k = (uint32_t(r) + uint32_t(TAPS) - hr) % uint32_t(TAPS);
        const size_t slot = (head + k) % uint32_t(TAPS);
#pragma unroll
        for (int e = 0; e < 8; e++) st[(slot * 8 + e) * lanes + lane] = __float_as_uint(elem(hist[r], e));
    }
    st[size_t(8 * TAPS) * lanes + lane] = head;
}

// ------------------------------------------------------------------------------------------------------------- LANE_MAJOR
// grid (lanes, workgroups per lane), 256 threads; a workgroup takes `cpb` consecutive tiles of its lane (1 out of place; all of
// them in place).  LDS index i of a plane: 0 .. TAPS - 1 the history (the frame TAPS - i steps in front of the tile), TAPS + i frame i.
template <int TAPS>
__global__ __launch_bounds__(256) void pfb_lane_major(const PfbArgs a, uint32_t *st, const float *x, float *y, const size_t lanes,
                                                      const size_t frames, const size_t cpb)
{
    constexpr int T = kPfbLmTileFrames;
    static_assert(T == 256, "one output frame per thread");
    __shared__ f4 pa[TAPS + T], pb[TAPS + T];
    const int tid = threadIdx.x;
    const size_t lane = blockIdx.x;
    const f4 *xl = reinterpret_cast<const f4 *>(x) + lane * frames * 2;
    f4 *yl = reinterpret_cast<f4 *>(y) + lane * frames * 2;
    const size_t ntiles = (frames + T - 1) / T;
    const size_t c0 = size_t(blockIdx.y) * cpb, c1 = c0 + cpb < ntiles ? c0 + cpb : ntiles;
    if (c0 >= c1) return;  // whole workgroup

    uint32_t head0 = 0;
    if (c0 == 0) {
        head0 = st[size_t(8 * TAPS) * lanes + lane] % uint32_t(TAPS);
        if (tid < TAPS * 8) {  // word `tid` of the history in LDS order: frame i = tid / 8 is k + 1 = TAPS - i steps back
            const int i = tid / 8, e = tid % 8;
            const size_t slot = (head0 + uint32_t(TAPS - 1 - i)) % uint32_t(TAPS);
            const float v = __uint_as_float(st[(slot * 8 + e) * lanes + lane]);
            (e < 4 ? reinterpret_cast<float *>(&pa[i]) : reinterpret_cast<float *>(&pb[i]))[e & 3] = v;
        }
    } else if (tid < TAPS * 2) {
        const size_t q = (c0 * T - TAPS) * 2 + tid;  // 16-byte piece of x
        (tid & 1 ? pb : pa)[tid / 2] = xl[q];
    }
    // tile c as 2 * T pieces of 16 bytes, thread t takes pieces t and t + 256 (coalesced); piece q is half q & 1 of frame q / 2
    f4 p0 = {0.f, 0.f, 0.f, 0.f}, p1 = p0;
    auto fetch = [&](const size_t c) {
        const size_t q = c * T * 2 + tid;
        if (q < frames * 2) p0 = xl[q];
        if (q + T < frames * 2) p1 = xl[q + T];
    };
    fetch(c0);
    int n = 0;
    for (size_t c = c0; c < c1; c++) {
        n = int(frames - c * T < size_t(T) ? frames - c * T : size_t(T));
        (tid & 1 ? pb : pa)[TAPS + tid / 2] = p0;
        (tid & 1 ? pb : pa)[TAPS + T / 2 + tid / 2] = p1;
        if (c + 1 < c1) fetch(c + 1);
        lds_barrier();
        Frame acc{{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};  // `Frame::default()` (:62)
        if (tid < n) {
#pragma unroll
            for (int tap = 0; tap < TAPS; tap++)
                bank_tap(acc, Frame{pa[TAPS + tid - tap], pb[TAPS + tid - tap]}, a.coeff[tap][0], a.coeff[tap][1], a.coeff[tap][2], a.coeff[tap][3]);
            if (a.dft) acc = dft4(acc);
        }
        f4 ka = {0.f, 0.f, 0.f, 0.f}, kb = ka;
        if (tid < TAPS) ka = pa[n + tid], kb = pb[n + tid];
        lds_barrier();
        if (tid < TAPS) pa[tid] = ka, pb[tid] = kb;
        if (tid < n) {
            yl[(c * T + tid) * 2] = acc.a;
            yl[(c * T + tid) * 2 + 1] = acc.b;
        }
    }
    if (c0 != 0) return;  // whole workgroup
    lds_barrier();
    const uint32_t head = uint32_t((head0 + size_t(TAPS) - frames % TAPS) % TAPS);
    if (tid < TAPS * 8) {  // state word `tid`: physical slot tid / 8 holds the frame k + 1 steps back
        const int slot = tid / 8, e = tid % 8;
        const uint32_t k = (uint32_t(slot) + uint32_t(TAPS) - head) % uint32_t(TAPS);
        float v;
        if (c1 == ntiles) {
            const int i = TAPS - 1 - int(k);
            v = (e < 4 ? reinterpret_cast<const float *>(&pa[i]) : reinterpret_cast<const float *>(&pb[i]))[e & 3];
        } else {  // other workgroups computed the call's end: its last TAPS frames come from x (out of place, unchanged)
            // (the address space is named: selected against the LDS pointer above, a plain `x[...]` becomes a flat load)
            v = reinterpret_cast<const __attribute__((address_space(1))) float *>(reinterpret_cast<uintptr_t>(x))[(lane * frames + (frames - 1 - k)) * 8 + e];
        }
        st[size_t(tid) * lanes + lane] = __float_as_uint(v);
    }
    if (tid == 0) st[size_t(8 * TAPS) * lanes + lane] = head;
}

template <int TAPS>
int launch_pfb(const PfbArgs &a, uint32_t *st, const float *x, float *y, size_t lanes, size_t frames, int layout, bool inplace, hipStream_t s)
{
    if (layout == IDSP_FRAME_MAJOR) {
        const size_t seg = inplace ? frames : size_t(kPfbFmSegFrames), nseg = (frames + seg - 1) / seg;
        hipLaunchKernelGGL(pfb_frame_major<TAPS>, dim3(unsigned((lanes + 63) / 64), unsigned(nseg < 65535 ? nseg : 65535)), dim3(64), 0, s, a, st, x, y,
                           lanes, frames, seg);
    } else {
        const size_t ntiles = (frames + kPfbLmTileFrames - 1) / kPfbLmTileFrames;
        const size_t cpb = inplace ? ntiles : (ntiles + 65534) / 65535, per_lane = (ntiles + cpb - 1) / cpb;
        hipLaunchKernelGGL(pfb_lane_major<TAPS>, dim3(unsigned(lanes), unsigned(per_lane)), dim3(256), 0, s, a, st, x, y, lanes, frames, cpb);
    }
    return launch_status();
}

// `sinc` (:29-31)
float sinc(float v) { return v == 0.0f ? 1.0f : sinf(v) / v; }

}  // namespace
}  // namespace idsp

using namespace idsp;

extern "C" {

size_t idsp_pfb_state_words(const idsp_pfb_f32 *cfg)
{
    if (!cfg || cfg->taps < 1 || cfg->taps > IDSP_PFB_MAX_TAPS) return 0;
    return size_t(8 * cfg->taps + 1);
}

int idsp_pfb_prototype_f32(int taps, idsp_pfb_f32 *out)
{
    if (!out) return fail(IDSP_EINVAL, "out is NULL");
    if (taps < 1 || taps > IDSP_PFB_MAX_TAPS) return fail(IDSP_EINVAL, "taps = %d outside 1..%d", taps, IDSP_PFB_MAX_TAPS);
    // `prototype()` (:33-44) for M * TAPS = 4 * taps coefficients, f32 throughout, the reference's order of operations
    constexpr float kTau = 6.28318530717958647692f;  // std::f32::consts::TAU
    const int n_taps = 4 * taps;
    const float fc = 0.5f / 4.0f * 0.9f;
    const float mid = float(n_taps - 1) * 0.5f;
    float h[4 * IDSP_PFB_MAX_TAPS];
    for (int i = 0; i < n_taps; i++) {
        const float n = float(i) - mid;
        const float w = 0.54f - 0.46f * cosf(kTau * float(i) / float(n_taps - 1));
        h[i] = 2.0f * fc * sinc(kTau * fc * n) * w;
    }
    float sum = -0.0f;  // f32::sum
    for (int i = 0; i < n_taps; i++) sum = sum + h[i];
    std::memset(out, 0, sizeof(*out));
    out->taps = taps;
    out->dft = 1;
    for (int i = 0; i < n_taps; i++) out->coeff[i / 4][i % 4] = h[i] / sum;  // `bytemuck::cast` (:104)
    return IDSP_OK;
}

int idsp_pfb_f32_process(const idsp_pfb_f32 *cfg, void *state, const float *x, float *y, size_t lanes, size_t frames, int layout,
                         void *stream)
{
    if (!cfg) return fail(IDSP_EINVAL, "cfg is NULL");
    if (cfg->taps < 1 || cfg->taps > IDSP_PFB_MAX_TAPS) return fail(IDSP_EINVAL, "taps = %d outside 1..%d", cfg->taps, IDSP_PFB_MAX_TAPS);
    if (cfg->dft != 0 && cfg->dft != 1) return fail(IDSP_EINVAL, "dft = %d is neither 0 nor 1", cfg->dft);
    if (layout != IDSP_FRAME_MAJOR && layout != IDSP_LANE_MAJOR) return fail(IDSP_EINVAL, "bad layout %d", layout);
    if (lanes && (!state || (frames && (!x || !y)))) return fail(IDSP_EINVAL, "state, x or y is NULL");
    if (lanes > (size_t(1) << 31) - 1 || frames > (size_t(1) << 40)) return fail(IDSP_EINVAL, "lanes/frames out of range");
    const uintptr_t xb = reinterpret_cast<uintptr_t>(x), yb = reinterpret_cast<uintptr_t>(y);
    if (xb % 16 || yb % 16) return fail(IDSP_EINVAL, "x and y hold 32-byte frames read 16 bytes at a time: both must be 16-byte aligned");
    if (lanes == 0 || frames == 0) return IDSP_OK;
    const uintptr_t bytes = uintptr_t(lanes) * frames * 32;
    if (xb != yb && xb < yb + bytes && yb < xb + bytes) return fail(IDSP_EINVAL, "x and y overlap without being equal");
    PfbArgs a;
    a.dft = cfg->dft;
    for (int t = 0; t < IDSP_PFB_MAX_TAPS; t++)
        for (int m = 0; m < 4; m++) a.coeff[t][m] = t < cfg->taps ? cfg->coeff[t][m] : 0.f;
    const bool inplace = xb == yb, fm = layout == IDSP_FRAME_MAJOR;
    uint32_t *st = static_cast<uint32_t *>(state);
    switch (cfg->taps) {
#define IDSP_PFB_CASE(N)                                                                                                              \
    case N:                                                                                                                           \
        note_kernel(fm ? (inplace ? "pfb_frame_major[unsegmented, in place]<taps " #N ">"                                             \
                                  : "pfb_frame_major[segment " IDSP_PFB_FM_SEG_STR " frames]<taps " #N ">")                           \
                       : (inplace ? "pfb_lane_major[tile " IDSP_PFB_LM_TILE_STR " frames, one workgroup per lane, in place]<taps " #N ">" \
                                  : "pfb_lane_major[tile " IDSP_PFB_LM_TILE_STR " frames]<taps " #N ">"));                            \
        return launch_pfb<N>(a, st, x, y, lanes, frames, layout, inplace, as_stream(stream));
        IDSP_PFB_CASE(1)
        IDSP_PFB_CASE(2)
        IDSP_PFB_CASE(3)
        IDSP_PFB_CASE(4)
        IDSP_PFB_CASE(5)
        IDSP_PFB_CASE(6)
        IDSP_PFB_CASE(7)
        IDSP_PFB_CASE(8)
        IDSP_PFB_CASE(9)
        IDSP_PFB_CASE(10)
        IDSP_PFB_CASE(11)
        IDSP_PFB_CASE(12)
        IDSP_PFB_CASE(13)
        IDSP_PFB_CASE(14)
        IDSP_PFB_CASE(15)
        IDSP_PFB_CASE(16)
#undef IDSP_PFB_CASE
    }
    return fail(IDSP_EINVAL, "taps = %d", cfg->taps);
}

}  // extern "C"
