// The modulator's host side through the C++ mirrors of include/idsp_hip.hpp: `Dsm` validates its order as idsp_dsm_u32 does,
// `DsmLanes::process_view` refuses mismatched views and short pitches, and the argument errors and empty calls of the entry.
// Every call here returns before anything is launched, so the program runs without a GPU: the pointers are host addresses that
// are only compared, never followed.
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

alignas(16) static uint32_t x[256];
alignas(16) static int8_t y[1024];
static uint32_t st[64];

// the mirror and the entry agree on an order
static bool both(int order, bool ok)
{
    bool threw = false;
    try {
        Dsm d(order);
        (void)d;
    } catch (const Error &e) {
        threw = e.code == IDSP_EINVAL;
    }
    const int rc = idsp_dsm_u32(order, st, x, 0, y, 0, 0, 0, IDSP_FRAME_MAJOR, nullptr);
    return ok ? (!threw && rc == IDSP_OK && idsp_dsm_state_words(order) == size_t(2 * order)) : (threw && einval(rc) && idsp_dsm_state_words(order) == 0);
}

template <class F>
static bool throws(F f)
{
    try {
        f();
    } catch (const Error &e) {
        return e.code == IDSP_EINVAL;
    }
    return false;
}

int main()
{
    EXPECT(IDSP_DSM_MAX_ORDER == 8);
    for (int k = 0; k <= 8; k++) EXPECT(both(k, true));
    EXPECT(both(-1, false) && both(9, false) && both(1 << 30, false));

    EXPECT(einval(idsp_dsm_u32(3, st, x, 0, y, 0, 4, 4, 2, nullptr)));                       // layout
    EXPECT(einval(idsp_dsm_u32(3, st, nullptr, 0, y, 0, 4, 4, IDSP_FRAME_MAJOR, nullptr)));
    EXPECT(einval(idsp_dsm_u32(3, st, x, 0, nullptr, 0, 4, 4, IDSP_LANE_MAJOR, nullptr)));
    EXPECT(einval(idsp_dsm_u32(3, nullptr, x, 0, y, 0, 4, 4, IDSP_FRAME_MAJOR, nullptr)));   // NULL state, order > 0
    EXPECT(einval(idsp_dsm_u32(3, st, x, 3, y, 0, 4, 4, IDSP_FRAME_MAJOR, nullptr)));        // pitch < row
    EXPECT(einval(idsp_dsm_u32(3, st, x, 0, y, 3, 4, 4, IDSP_LANE_MAJOR, nullptr)));
    EXPECT(einval(idsp_dsm_u32(3, st, x, 0, y, 4, 5, 4, IDSP_FRAME_MAJOR, nullptr)));        // row = lanes in FrameMajor
    EXPECT(einval(idsp_dsm_u32(3, st, x, 4, y, 0, 4, 5, IDSP_LANE_MAJOR, nullptr)));         // row = frames in LaneMajor
    EXPECT(einval(idsp_dsm_u32(3, st, reinterpret_cast<const uint32_t *>(reinterpret_cast<const char *>(x) + 2), 0, y, 0, 4, 4, IDSP_FRAME_MAJOR, nullptr)));
    // overlap, both orders: y inside x, y on the last byte of x, x starting on the last byte of y, y in the gap of a pitched x
    int8_t *xb = reinterpret_cast<int8_t *>(x);
    EXPECT(einval(idsp_dsm_u32(3, st, x, 0, xb, 0, 4, 4, IDSP_FRAME_MAJOR, nullptr)));
    EXPECT(einval(idsp_dsm_u32(3, st, x, 0, xb + 63, 0, 4, 4, IDSP_FRAME_MAJOR, nullptr)));
    EXPECT(einval(idsp_dsm_u32(3, st, x + 4, 0, xb + 1, 0, 4, 4, IDSP_LANE_MAJOR, nullptr)));   // y = bytes 1..16, x starts at byte 16
    EXPECT(einval(idsp_dsm_u32(3, st, x, 8, xb + 16, 32, 4, 4, IDSP_FRAME_MAJOR, nullptr)));    // y rows of 4 bytes in the gaps of x
    EXPECT(einval(idsp_dsm_u32(3, st, x, size_t(1) << 62, y, 0, 4, 4, IDSP_FRAME_MAJOR, nullptr)));  // an extent past size_t
    // the empty calls; K = 0 takes no state
    EXPECT(idsp_dsm_u32(3, st, x, 0, y, 0, 0, 4, IDSP_FRAME_MAJOR, nullptr) == IDSP_OK);
    EXPECT(idsp_dsm_u32(3, st, x, 0, y, 0, 4, 0, IDSP_LANE_MAJOR, nullptr) == IDSP_OK);
    EXPECT(idsp_dsm_u32(0, nullptr, x, 0, y, 0, 0, 4, IDSP_FRAME_MAJOR, nullptr) == IDSP_OK);
    // y just behind x, byte-exact: not an overlap (checked with no lanes left to launch: shapes only)
    EXPECT(idsp_dsm_u32(3, st, x, 0, xb + 64, 0, 0, 0, IDSP_FRAME_MAJOR, nullptr) == IDSP_OK);

    try {  // no lanes: nothing is allocated, nothing launched
        DsmLanes d = Dsm(3).lanes(0);
        EXPECT(d.order() == 3 && d.state().len() == 0);
        d.reset();
        d.process_view(View<uint32_t, LaneMajor>{x, 3, 0}, ViewMut<int8_t, LaneMajor>{y, 3, 0});
        d.block(View<uint32_t, FrameMajor>{x, 3, 0}, ViewMut<int8_t, FrameMajor>{y, 3, 0});
        EXPECT(throws([&] { d.process_view(View<uint32_t, LaneMajor>{x, 3, 0}, ViewMut<int8_t, LaneMajor>{y, 4, 0}); }));   // frames differ
        EXPECT(throws([&] { d.process_view(View<uint32_t, LaneMajor>{x, 3, 1}, ViewMut<int8_t, LaneMajor>{y, 3, 1}); }));   // lanes differ
        EXPECT(throws([&] { d.process_view(View<uint32_t, LaneMajor>{x, 3, 0}, ViewMut<int8_t, LaneMajor>{y, 3, 0}, 2, 0); }));  // x_pitch < frames
        EXPECT(throws([&] { d.process_view(View<uint32_t, LaneMajor>{x, 3, 0}, ViewMut<int8_t, LaneMajor>{y, 3, 0}, 0, 2); }));
        EXPECT(throws([] { Dsm(9); }) && throws([] { Dsm(-1); }));
        DsmLanes z = Dsm(0).lanes(0);
        EXPECT(z.state().len() == 0);
    } catch (const std::exception &e) {
        std::printf("empty mirror call threw: %s\n", e.what());
        bad++;
    }
    if (bad) return std::printf("%d failures\n", bad), 1;
    std::printf("dsm host tests passed\n");
    return 0;
}
