// cordic.hip — the generic CORDIC of the reference (src/cordic.rs:13-77) and its six entry points (:80-107), elementwise over
// rows [x, y] and words z.  All integer, wrapping (release-build semantics), bit-exact.
//
// The kernel is bound by VALU issue, not by memory (measured: 1.5 to 2.9 times a copy of the same bytes, profiles/NOTES.md):
// 30 (circular, linear) or 32 (hyperbolic) dependent micro-rotations per element.  So the micro-rotations are unrolled by
// template recursion — every angle and shift count is an immediate, there is no table in LDS or in memory and no per-thread
// array — sigma is a select instead of a branch, and a thread carries four independent elements whose chains the compiler
// interleaves and whose loads and stores are 16 bytes wide.
#include <utility>

#include "common.h"
#include "cordic_table.h"

namespace idsp {
namespace {

constexpr int kCircular = 0, kHyperbolic = 1, kLinear = 2;  // `COORD` (:7-9)
constexpr bool kRotate = false, kDerotate = true;            // `VECTORING` (:5-6)

// Grid cap of the launcher: 256 CUs x 8 workgroups of four waves = eight waves per SIMD.  The four-element loops need 72 to 77
// VGPRs, so six waves per SIMD are resident and the capped grid runs as one generation and a third.  More elements than
// kCordicMaxBlocks * 256 threads * 4 take further trips of the grid-stride loop.
constexpr unsigned kCordicMaxBlocks = 2048;

typedef int32_t i32x2 __attribute__((ext_vector_type(2)));
typedef int32_t i32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint32_t asr(uint32_t v, int i) { return uint32_t(int32_t(v) >> i); }

// Micro-rotation J of the table (:37-74).  x, y, z are kept as u32 so that every +, - and negation wraps.
template <bool VECTORING, int COORD, int J>
__device__ __forceinline__ void cordic_step(uint32_t &x, uint32_t &y, uint32_t &z)
{
    constexpr int I = COORD == kHyperbolic ? J + 1 : J;  // hyperbolic starts at i = 1 (:43-45)
    // linear: computed, entry 0 is i32::MIN (:39-41)
    constexpr uint32_t A = COORD == kLinear ? 0x80000000u >> J : uint32_t(COORD == kCircular ? kCordicCircular[J] : kCordicHyperbolic[J]);
    constexpr int REPEAT = COORD == kHyperbolic && (I == 4 || I == 13) ? 2 : 1;  // k = 4, then 3 k + 1 = 13, then 40 (:36, :47-52)
#pragma unroll
    for (int r = 0; r < REPEAT; r++) {
        // sigma (:55) as a select between the two candidates of each update (v_cmp + v_cndmask), no branch.  The sign-mask form
        // v + ((d ^ m) - m) has as many instructions, but the select form measured 11-37 % faster in the rotating kernels (profiles/NOTES.md).
        const bool lower = VECTORING ? int32_t(y) <= 0 : int32_t(z) >= 0;
        const uint32_t dx = asr(y, I), dy = asr(x, I);                    // (:56)
        if constexpr (COORD == kCircular) x = lower ? x - dx : x + dx;    // (:58-59, :66-67)
        if constexpr (COORD == kHyperbolic) x = lower ? x + dx : x - dx;  // (:60-61, :68-69)
        y = lower ? y + dy : y - dy;                                      // (:63, :71)
        z = lower ? z - A : z + A;                                        // (:64, :72)
    }
}

template <bool VECTORING, int COORD, int... J>
__device__ __forceinline__ void cordic_steps(uint32_t &x, uint32_t &y, uint32_t &z, std::integer_sequence<int, J...>)
{
    (cordic_step<VECTORING, COORD, J>(x, y, z), ...);
}

// `cordic::<VECTORING, COORD>(x, y, z, None)` (:13-77); leaves the results in x, y and z
template <bool VECTORING, int COORD>
__device__ __forceinline__ void cordic_dev(uint32_t &x, uint32_t &y, uint32_t &z)
{
    // `left` (:25-29) as a mask: vectoring x < 0, rotating z - (i32::MIN >> 1) < 0
    const uint32_t s = VECTORING ? asr(x, 31) : asr(z - 0xC0000000u, 31);
    x = (x ^ s) - s;        // (:31)
    y = (y ^ s) - s;        // (:32)
    z ^= s & 0x80000000u;   // `z.wrapping_sub(i32::MIN)` (:33)
    cordic_steps<VECTORING, COORD>(x, y, z, std::make_integer_sequence<int, kCordicDepth>{});
}

// Four elements per thread and trip on 16-byte aligned buffers (`vec`): two dwordx4 loads of rows, one of z, two (pair) or one
// (word) dwordx4 store.  Everything else — buffers only 8- or 4-byte aligned, the last n % 4 elements — goes one element per
// thread.  Every thread writes exactly the elements it has read, so out may be xy (pair) or z (word).
// z == nullptr: every z is 0 and nothing is loaded for it (a uniform branch).
template <bool VECTORING, int COORD, bool PAIR_OUT>
__global__ __launch_bounds__(256) void cordic_kernel(const int32_t *xy, const int32_t *z, int32_t *out, size_t n, bool vec)
{
    const size_t stride = size_t(gridDim.x) * 256, t = size_t(blockIdx.x) * 256 + threadIdx.x;
    const size_t nv = vec ? n / 4 : 0;
    for (size_t i = t; i < nv; i += stride) {
        const i32x4 a = __builtin_nontemporal_load(reinterpret_cast<const i32x4 *>(xy) + 2 * i);
        const i32x4 b = __builtin_nontemporal_load(reinterpret_cast<const i32x4 *>(xy) + 2 * i + 1);
        i32x4 c = {0, 0, 0, 0};
        if (z) c = __builtin_nontemporal_load(reinterpret_cast<const i32x4 *>(z) + i);
        uint32_t x0 = a.x, y0 = a.y, z0 = c.x, x1 = a.z, y1 = a.w, z1 = c.y, x2 = b.x, y2 = b.y, z2 = c.z, x3 = b.z, y3 = b.w, z3 = c.w;
        cordic_dev<VECTORING, COORD>(x0, y0, z0);
        cordic_dev<VECTORING, COORD>(x1, y1, z1);
        cordic_dev<VECTORING, COORD>(x2, y2, z2);
        cordic_dev<VECTORING, COORD>(x3, y3, z3);
        // (x, z) when vectoring, (x, y) when rotating (:76); mul / div keep the second (:91, :96)
        const i32x4 second = VECTORING ? i32x4{int32_t(z0), int32_t(z1), int32_t(z2), int32_t(z3)} : i32x4{int32_t(y0), int32_t(y1), int32_t(y2), int32_t(y3)};
        if constexpr (PAIR_OUT) {
            __builtin_nontemporal_store(i32x4{int32_t(x0), second.x, int32_t(x1), second.y}, reinterpret_cast<i32x4 *>(out) + 2 * i);
            __builtin_nontemporal_store(i32x4{int32_t(x2), second.z, int32_t(x3), second.w}, reinterpret_cast<i32x4 *>(out) + 2 * i + 1);
        } else {
            __builtin_nontemporal_store(second, reinterpret_cast<i32x4 *>(out) + i);
        }
    }
    for (size_t i = nv * 4 + t; i < n; i += stride) {
        const i32x2 a = __builtin_nontemporal_load(reinterpret_cast<const i32x2 *>(xy) + i);
        uint32_t x0 = a.x, y0 = a.y, z0 = 0;
        if (z) z0 = uint32_t(__builtin_nontemporal_load(z + i));
        cordic_dev<VECTORING, COORD>(x0, y0, z0);
        const int32_t second = int32_t(VECTORING ? z0 : y0);
        if constexpr (PAIR_OUT)
            __builtin_nontemporal_store(i32x2{int32_t(x0), second}, reinterpret_cast<i32x2 *>(out) + i);
        else
            __builtin_nontemporal_store(second, out + i);
    }
}

template <bool VECTORING, int COORD, bool PAIR_OUT>
int launch_cordic(const char *vec_name, const char *scalar_name, const int32_t *xy, const int32_t *z, int32_t *out, size_t n, void *stream)
{
    if (n == 0) return IDSP_OK;
    if (!xy || !out) return fail(IDSP_EINVAL, "xy or out is NULL");
    if (n > (size_t(1) << 58)) return fail(IDSP_EINVAL, "n out of range");
    const uintptr_t xb = reinterpret_cast<uintptr_t>(xy), zb = reinterpret_cast<uintptr_t>(z), ob = reinterpret_cast<uintptr_t>(out);
    const uintptr_t xn = uintptr_t(n) * 8, zn = uintptr_t(n) * 4, on = uintptr_t(n) * (PAIR_OUT ? 8 : 4);
    if (xb % 8) return fail(IDSP_EINVAL, "xy holds 8-byte rows [x, y]: it must be 8-byte aligned");
    if (ob % (PAIR_OUT ? 8 : 4)) return fail(IDSP_EINVAL, "out must be %d-byte aligned", PAIR_OUT ? 8 : 4);
    if (zb % 4) return fail(IDSP_EINVAL, "z must be 4-byte aligned");
    // in place: out == xy (pair results) or out == z (word results); every other overlap of out with an input is an error
    if (!(PAIR_OUT && ob == xb) && ob < xb + xn && xb < ob + on) return fail(IDSP_EINVAL, "out overlaps xy%s", PAIR_OUT ? " without being equal" : "");
    if (z && !(!PAIR_OUT && ob == zb) && ob < zb + zn && zb < ob + on) return fail(IDSP_EINVAL, "out overlaps z%s", PAIR_OUT ? "" : " without being equal");
    const bool vec = (xb | zb | ob) % 16 == 0;
    size_t blocks = (n / (vec ? 4 : 1) + 255) / 256 + 1;
    if (blocks > kCordicMaxBlocks) blocks = kCordicMaxBlocks;
    note_kernel(vec ? vec_name : scalar_name);
    hipLaunchKernelGGL((cordic_kernel<VECTORING, COORD, PAIR_OUT>), dim3(unsigned(blocks)), dim3(256), 0, as_stream(stream), xy, z, out, n, vec);
    return launch_status();
}

}  // namespace
}  // namespace idsp

using namespace idsp;

#define IDSP_CORDIC_ENTRY(NAME, VECTORING, COORD, PAIR)                                                                            \
    int idsp_cordic_##NAME##_i32(const int32_t *xy, const int32_t *z, int32_t *out, size_t n, void *stream)                         \
    {                                                                                                                              \
        return launch_cordic<VECTORING, COORD, PAIR>("cordic_kernel<" #NAME ">[four elements per thread]",                         \
                                                     "cordic_kernel<" #NAME ">[one element per thread]", xy, z, out, n, stream);   \
    }

extern "C" {

IDSP_CORDIC_ENTRY(cos_sin, kRotate, kCircular, true)          // (:80-82)
IDSP_CORDIC_ENTRY(sqrt_atan2, kDerotate, kCircular, true)     // (:85-87)
IDSP_CORDIC_ENTRY(mul, kRotate, kLinear, false)               // (:90-92)
IDSP_CORDIC_ENTRY(div, kDerotate, kLinear, false)             // (:95-97)
IDSP_CORDIC_ENTRY(cosh_sinh, kRotate, kHyperbolic, true)      // (:100-102)
IDSP_CORDIC_ENTRY(sqrt_atanh2, kDerotate, kHyperbolic, true)  // (:105-107)

double idsp_cordic_circular_gain(void) { return kCordicCircularGain; }
double idsp_cordic_hyperbolic_gain(void) { return kCordicHyperbolicGain; }

}  // extern "C"
