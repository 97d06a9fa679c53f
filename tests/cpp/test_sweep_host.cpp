// The swept sine's host side (include/idsp_hip.h, idsp_sweep_*) through the C++ mirrors of include/idsp_hip.hpp: `Sweep::fit`
// with the reference test's figures (src/sweptsine.rs:197-220) and its two errors, the descriptors, and the argument errors and
// empty calls of idsp_sweep_i32.  Every call here returns before anything is launched, so the program runs without a
// GPU: the pointers are host addresses that are only compared, never followed.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>

#include "idsp_hip.hpp"

using namespace idsp_hip;

static int bad = 0;
#define EXPECT(cond)                                           \
    do {                                                       \
        if (!(cond)) {                                         \
            std::printf("line %d: %s\n", __LINE__, #cond);     \
            bad++;                                             \
        }                                                      \
    } while (0)

static bool close(double a, double b, double atol) { return std::fabs(a - b) <= atol; }

static bool fit_fails(float stop, float harmonics, float cycles, const char *text)
{
    try {
        Sweep::fit(stop, harmonics, cycles);
    } catch (const Error &e) {
        return e.code == IDSP_EINVAL && std::strstr(e.what(), text) && !std::strcmp(idsp_last_error(), text);
    }
    return false;
}

static bool einval(int rc) { return rc == IDSP_EINVAL && idsp_last_error() && std::strlen(idsp_last_error()); }

int main()
{
    const Sweep s = Sweep::fit(0.3f, 3000.0f, 3.0f);
    EXPECT(s.rate == 0x22f40);
    EXPECT(s.state == (int64_t(0x22f40) * 3) << 32);
    EXPECT(close(s.delay(3000.0), 240190.96, 1e-2));
    EXPECT(close(s.cycles(), 3.0, 1e-2));
    EXPECT(s.state_f() == s.continuous(0.0) * s.rate_f());
    EXPECT(float(s.state_f()) * 3000.0f >= 0.3f * 0.99f && float(s.state_f()) * 3000.0f <= 1.01f * 0.3f);
    for (int h = 0; h < 3000; h++) EXPECT(close(s.continuous(s.delay(double(h))), h * 3.0, 1e-10));  // 0 included: delay(0) = -inf
    EXPECT(close(s.octave() * std::log2(10.0), s.decade(), 1e-6));
    const auto inv = s.inverse_filter(0.01f);
    EXPECT(close(std::hypot(inv[0], inv[1]), 2.0 * s.rate_f() * std::sqrt(0.01 / s.rate_f()), 1e-6));

    const float nan = std::numeric_limits<float>::quiet_NaN();
    EXPECT(fit_fails(0.6f, 1.0f, 1.0f, "Stop out of bounds"));
    EXPECT(fit_fails(-1e-9f, 1.0f, 1.0f, "Stop out of bounds"));
    EXPECT(fit_fails(nan, 1.0f, 1.0f, "Stop out of bounds"));
    EXPECT(fit_fails(0.1f, 1.0f, 0.5f, "Start out of bounds"));  // `cycles as i64` truncates to 0
    EXPECT(fit_fails(0.0f, 1.0f, 1.0f, "Start out of bounds"));  // rate 0
    int32_t rate = -7;
    int64_t state = -7;
    EXPECT(einval(idsp_sweep_fit(0.6f, 1.0f, 1.0f, &rate, &state)) && rate == -7 && state == -7);
    EXPECT(einval(idsp_sweep_fit(0.3f, 3000.0f, 3.0f, nullptr, &state)));
    EXPECT(einval(idsp_sweep_inverse_filter(1, 1, 0.1f, nullptr)));

    EXPECT(idsp_sweep_state_words() == IDSP_SWEEP_STATE_WORDS && IDSP_SWEEP_STATE_WORDS == 7);
    alignas(16) static int32_t a[64], c[128];
    EXPECT(idsp_sweep_i32(nullptr, nullptr, 0, 5, IDSP_FRAME_MAJOR, nullptr) == IDSP_OK);
    EXPECT(idsp_sweep_i32(a, nullptr, 4, 0, IDSP_LANE_MAJOR, nullptr) == IDSP_OK);
    EXPECT(einval(idsp_sweep_i32(a, c, 4, 2, 2, nullptr)));
    EXPECT(einval(idsp_sweep_i32(nullptr, c, 4, 2, IDSP_FRAME_MAJOR, nullptr)));
    EXPECT(einval(idsp_sweep_i32(a, nullptr, 4, 2, IDSP_FRAME_MAJOR, nullptr)));

    try {  // no lanes: nothing is allocated, nothing launched
        SweepOsc osc({});
        DeviceBuffer<int32_t> none;
        osc.generate(ViewMut<int32_t, FrameMajor>{none.data(), 3, 0});
        EXPECT(osc.emitted().empty());
    } catch (const std::exception &e) {
        std::printf("empty mirror call threw: %s\n", e.what());
        bad++;
    }
    if (bad) return std::printf("%d failures\n", bad), 1;
    std::printf("sweep host tests passed\n");
    return 0;
}
