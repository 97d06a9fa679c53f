// The RPLL's host side through the C++ mirrors of include/idsp_hip.hpp: `RPLLConfig` and `AccuLo` validate as idsp_rpll_i32 and
// idsp_accu_lo_i32 do (every bound just inside and just outside), the state helpers of a mirror without lanes, and the argument
// errors and empty calls of the two entries.  Every call here returns before anything is launched, so the program runs without a
// GPU: the pointers are host addresses that are only compared, never followed.
#include <cstdio>
#include <cstring>

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

static bool einval(int rc) { return rc == IDSP_EINVAL && idsp_last_error() && std::strlen(idsp_last_error()); }

// the mirror and the entry agree on a configuration
static bool both(int dt2, int sf, int sp, bool ok)
{
    bool threw = false;
    try {
        RPLLConfig c(dt2, sf, sp);
        (void)c;
    } catch (const Error &e) {
        threw = e.code == IDSP_EINVAL;
    }
    const idsp_rpll c{dt2, sf, sp};
    const int rc = idsp_rpll_i32(&c, nullptr, nullptr, nullptr, 0, 0, IDSP_FRAME_MAJOR, nullptr);
    return ok ? (!threw && rc == IDSP_OK) : (threw && einval(rc));
}

static bool both_lo(int k, bool ok)
{
    bool threw = false;
    try {
        AccuLo a(k, 3, -5);
        (void)a;
    } catch (const Error &e) {
        threw = e.code == IDSP_EINVAL;
    }
    const idsp_accu_lo c{k, 3, -5};
    const int rc = idsp_accu_lo_i32(&c, nullptr, nullptr, 0, 0, IDSP_LANE_MAJOR, nullptr);
    return ok ? (!threw && rc == IDSP_OK) : (threw && einval(rc));
}

int main()
{
    EXPECT(idsp_rpll_state_words() == IDSP_RPLL_STATE_WORDS && IDSP_RPLL_STATE_WORDS == 4);
    const int good[][3] = {{0, 1, 0}, {0, 32, 31}, {8, 9, 8}, {8, 23, 22}, {11, 23, 23}, {30, 31, 30}, {30, 32, 61}, {8, 9, 39}, {0, 1, 31}};
    const int wrong[][3] = {{-1, 9, 8}, {31, 32, 31}, {8, 8, 8}, {8, 33, 8}, {0, 0, 0}, {8, 9, 7}, {8, 9, 40}, {30, 32, 62}, {0, 1, 32}};
    for (const auto &c : good) EXPECT(both(c[0], c[1], c[2], true));
    for (const auto &c : wrong) EXPECT(both(c[0], c[1], c[2], false));
    EXPECT(both_lo(0, true) && both_lo(24, true) && both_lo(-1, false) && both_lo(25, false));

    alignas(16) static int32_t a[256], b[256];
    static uint32_t st[16];
    const idsp_rpll cfg{8, 9, 8};
    EXPECT(einval(idsp_rpll_i32(nullptr, st, a, b, 4, 4, IDSP_FRAME_MAJOR, nullptr)));
    EXPECT(einval(idsp_rpll_i32(&cfg, st, a, b, 4, 4, 2, nullptr)));
    EXPECT(einval(idsp_rpll_i32(&cfg, nullptr, a, b, 4, 4, IDSP_FRAME_MAJOR, nullptr)));
    EXPECT(einval(idsp_rpll_i32(&cfg, st, nullptr, b, 4, 4, IDSP_FRAME_MAJOR, nullptr)));
    EXPECT(einval(idsp_rpll_i32(&cfg, st, a, a, 4, 4, IDSP_FRAME_MAJOR, nullptr)));           // ts == accu
    EXPECT(einval(idsp_rpll_i32(&cfg, st, a, a + 30, 4, 4, IDSP_LANE_MAJOR, nullptr)));       // the last pair of ts
    EXPECT(einval(idsp_rpll_i32(&cfg, st, a + 1, b, 4, 4, IDSP_FRAME_MAJOR, nullptr)));       // 4 mod 8
    EXPECT(einval(idsp_rpll_i32(&cfg, st, a, b + 1, 4, 4, IDSP_FRAME_MAJOR, nullptr)));
    EXPECT(idsp_rpll_i32(&cfg, st, a, b, 0, 4, IDSP_FRAME_MAJOR, nullptr) == IDSP_OK);
    EXPECT(idsp_rpll_i32(&cfg, st, a, b, 4, 0, IDSP_LANE_MAJOR, nullptr) == IDSP_OK);

    const idsp_accu_lo lo{3, 1, 0};
    EXPECT(einval(idsp_accu_lo_i32(nullptr, a, b, 2, 2, IDSP_FRAME_MAJOR, nullptr)));
    EXPECT(einval(idsp_accu_lo_i32(&lo, a, b, 2, 2, 2, nullptr)));
    EXPECT(einval(idsp_accu_lo_i32(&lo, nullptr, b, 2, 2, IDSP_FRAME_MAJOR, nullptr)));
    EXPECT(einval(idsp_accu_lo_i32(&lo, a, nullptr, 2, 2, IDSP_FRAME_MAJOR, nullptr)));
    EXPECT(einval(idsp_accu_lo_i32(&lo, a, a, 2, 2, IDSP_FRAME_MAJOR, nullptr)));
    EXPECT(einval(idsp_accu_lo_i32(&lo, a + 1, b, 2, 2, IDSP_FRAME_MAJOR, nullptr)));
    EXPECT(einval(idsp_accu_lo_i32(&lo, a, b + 1, 2, 2, IDSP_LANE_MAJOR, nullptr)));
    EXPECT(einval(idsp_accu_lo_i32(&lo, a, b, 2, ((size_t(1) << 40) >> 3) + 1, IDSP_FRAME_MAJOR, nullptr)));
    EXPECT(idsp_accu_lo_i32(&lo, a, b, 0, 2, IDSP_FRAME_MAJOR, nullptr) == IDSP_OK);
    EXPECT(idsp_accu_lo_i32(&lo, a, b, 2, 0, IDSP_LANE_MAJOR, nullptr) == IDSP_OK);

    try {  // no lanes: nothing is allocated, nothing launched
        RPLLLanes r = RPLLConfig(8, 9, 8).lanes(0);
        DeviceBuffer<int32_t> none;
        r.process_view(View<int32_t, FrameMajor>{none.data(), 3, 0}, ViewMut<int32_t, FrameMajor>{none.data(), 3, 0});
        EXPECT(r.phase().empty() && r.frequency().empty() && r.state().len() == 0);
        AccuLo(3).process_view(View<int32_t, LaneMajor>{none.data(), 2, 0}, ViewMut<int32_t, LaneMajor>{none.data(), 16, 0});
        bool threw = false;
        try {
            AccuLo(3).process_view(View<int32_t, LaneMajor>{none.data(), 2, 0}, ViewMut<int32_t, LaneMajor>{none.data(), 15, 0});
        } catch (const Error &) {
            threw = true;
        }
        EXPECT(threw);
    } catch (const std::exception &e) {
        std::printf("empty mirror call threw: %s\n", e.what());
        bad++;
    }
    if (bad) return std::printf("%d failures\n", bad), 1;
    std::printf("rpll host tests passed\n");
    return 0;
}
