// Argument validation of the six CORDIC entries (include/idsp_hip.h) and the empty calls of their C++ mirrors
// (include/idsp_hip.hpp: idsp_hip::cordic).  Every call here returns before anything is launched, so the program runs without a
// GPU: the pointers are host addresses that are only compared, never followed.
#include <cstdio>
#include <cstring>

#include "idsp_hip.hpp"

using namespace idsp_hip;

typedef int (*Entry)(const int32_t *, const int32_t *, int32_t *, size_t, void *);
struct Fn {
    const char *name;
    Entry f;
    bool pair;
};
static const Fn kFns[] = {
    {"cos_sin", idsp_cordic_cos_sin_i32, true},     {"sqrt_atan2", idsp_cordic_sqrt_atan2_i32, true},   {"cosh_sinh", idsp_cordic_cosh_sinh_i32, true},
    {"sqrt_atanh2", idsp_cordic_sqrt_atanh2_i32, true}, {"mul", idsp_cordic_mul_i32, false},             {"div", idsp_cordic_div_i32, false},
};

static int einval(const Fn &fn, const char *what, const int32_t *xy, const int32_t *z, int32_t *out, size_t n)
{
    const int rc = fn.f(xy, z, out, n, nullptr);
    if (rc != IDSP_EINVAL || !idsp_last_error() || !std::strlen(idsp_last_error())) {
        std::printf("%s, %s: status %d, message '%s'\n", fn.name, what, rc, idsp_last_error() ? idsp_last_error() : "(null)");
        return 1;
    }
    return 0;
}

int main()
{
    alignas(16) static int32_t a[64], b[64], c[64];  // three disjoint regions
    const size_t n = 8;
    int bad = 0;
    for (const Fn &fn : kFns) {
        // n == 0 succeeds before any pointer check
        if (fn.f(nullptr, nullptr, nullptr, 0, nullptr) != IDSP_OK || fn.f(a + 1, a + 1, a + 1, 0, nullptr) != IDSP_OK) {
            std::printf("%s: n == 0 refused\n", fn.name);
            bad++;
        }
        bad += einval(fn, "xy NULL", nullptr, b, c, n);
        bad += einval(fn, "out NULL", a, b, nullptr, n);
        bad += einval(fn, "xy NULL, z NULL", nullptr, nullptr, c, n);
        bad += einval(fn, "xy 4 bytes off the 8-byte grid", a + 1, b, c, n);
        bad += einval(fn, "out behind xy by one row", a, b, a + 2, n);
        bad += einval(fn, "out in front of xy by one row", a + 2, b, a, n);
        bad += einval(fn, "out overlaps the end of xy", a, b, a + 2 * n - 2, n);
        bad += einval(fn, "out overlaps z by one word", a, b, b + 2, n);
        bad += einval(fn, "out in front of z", a, b + 2, b, n);
        if (fn.pair) {
            bad += einval(fn, "pair out 4 bytes off the 8-byte grid", a, b, c + 1, n);
            bad += einval(fn, "pair out == z", a, b, b, n);
        } else {
            bad += einval(fn, "word out == xy", a, b, a, n);
            bad += einval(fn, "word out inside xy", a, nullptr, a + 4, n);
        }
    }
    try {
        DeviceBuffer<int32_t> none, out;
        cordic::cos_sin(none, out);  // without z: z = 0
        cordic::sqrt_atan2(none, none, out);
        cordic::cosh_sinh(none, out);
        cordic::sqrt_atanh2(none, none, out);
        cordic::mul(none, out);
        cordic::div(none, none, out);
    } catch (const std::exception &e) {
        std::printf("empty mirror call threw: %s\n", e.what());
        bad++;
    }
    if (!(cordic::circular_gain() > 1.6467602581 && cordic::circular_gain() < 1.6467602582) ||
        !(cordic::hyperbolic_gain() > 0.8281593609 && cordic::hyperbolic_gain() < 0.8281593610)) {
        std::printf("gains %.17g %.17g\n", cordic::circular_gain(), cordic::hyperbolic_gain());
        bad++;
    }
    if (bad) return std::printf("%d failures\n", bad), 1;
    std::printf("cordic argument-validation tests passed\n");
    return 0;
}
