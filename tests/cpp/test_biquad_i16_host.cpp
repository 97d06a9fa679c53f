// The 16-bit biquad's host side through the C ABI and the C++ mirror of include/idsp_hip.hpp: struct sizes, coefficient ingestion, the
// argument errors (the odd address and the in-place rule among them) and the empty calls of idsp_biquad_i16_df1 / _df1_clamp, and what
// `BiquadI16Lanes` refuses.  Every call here returns before anything is launched, so the program runs without a GPU: the pointers are
// host addresses that are only compared, never followed.
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

static bool einval(int rc) { return rc == IDSP_EINVAL && idsp_last_error() && std::strlen(idsp_last_error()); }

alignas(16) static int16_t x[512];
alignas(16) static int16_t y[512];
static uint32_t st[256];

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

static char *odd(int16_t *p) { return reinterpret_cast<char *>(p) + 1; }

int main()
{
    static_assert(sizeof(idsp_biquad_i16) == 12 && sizeof(idsp_biquad_clamp_i16) == 18, "ABI struct sizes");
    EXPECT(idsp_version() == 4);
    EXPECT(idsp_biquad_i16_state_words(0) == 0 && idsp_biquad_i16_state_words(1) == 4 && idsp_biquad_i16_state_words(9) == 36);

    // from_sos: the known low-pass, half away from zero, saturation, NaN -> 0
    const double lp[6] = {0.06745527388907189, 0.13491054777814377, 0.06745527388907189, 1.0, -1.1429805025399011, 0.4128015980961886};
    idsp_biquad_i16 q = biquad_i16_from_sos(lp, 13);
    EXPECT(q.ba[0] == 553 && q.ba[1] == 1105 && q.ba[2] == 553 && q.ba[3] == 9363 && q.ba[4] == -3382 && q.frac == 13);
    const double ties[6] = {0.5 / 8192, -0.5 / 8192, 1.5 / 8192, 1.0, 2.5 / 8192, -2.5 / 8192};
    q = biquad_i16_from_sos(ties, 13);
    EXPECT(q.ba[0] == 1 && q.ba[1] == -1 && q.ba[2] == 2 && q.ba[3] == -3 && q.ba[4] == 3);
    const double wild[6] = {4.0, -4.0 - 1.0 / 8192, std::numeric_limits<double>::quiet_NaN(), 1.0, std::numeric_limits<double>::infinity(), 3.9998779296875};
    q = biquad_i16_from_sos(wild, 13);
    EXPECT(q.ba[0] == 32767 && q.ba[1] == -32768 && q.ba[2] == 0 && q.ba[3] == -32768 && q.ba[4] == -32767);
    EXPECT(einval(idsp_biquad_i16_from_sos(nullptr, 13, &q)) && einval(idsp_biquad_i16_from_sos(lp, 13, nullptr)));
    EXPECT(einval(idsp_biquad_i16_from_sos(lp, -1, &q)) && einval(idsp_biquad_i16_from_sos(lp, 32, &q)));
    EXPECT(throws([&] { biquad_i16_from_sos(lp, 32); }));

    idsp_biquad_i16 c[2] = {{{553, 1105, 553, 9363, -3382}, 13}, {{1, 2, 3, 4, 5}, 31}};
    idsp_biquad_clamp_i16 cc[1] = {{{553, 1105, 553, 9363, -3382}, 0, 7, 100, -100}};  // min > max is the caller's business
    const int FMj = IDSP_FRAME_MAJOR, LMj = IDSP_LANE_MAJOR;
    EXPECT(einval(idsp_biquad_i16_df1(c, 2, st, x, 0, y, 0, 4, 4, 2, nullptr)));                 // layout
    EXPECT(einval(idsp_biquad_i16_df1(c, IDSP_MAX_SECTIONS + 1, st, x, 0, y, 0, 4, 4, FMj, nullptr)));
    EXPECT(einval(idsp_biquad_i16_df1(nullptr, 2, st, x, 0, y, 0, 4, 4, FMj, nullptr)));         // NULL cfg with n > 0
    EXPECT(einval(idsp_biquad_i16_df1(c, 2, nullptr, x, 0, y, 0, 4, 4, FMj, nullptr)));          // NULL state
    EXPECT(einval(idsp_biquad_i16_df1(c, 2, st, nullptr, 0, y, 0, 4, 4, FMj, nullptr)));
    EXPECT(einval(idsp_biquad_i16_df1_clamp(cc, 1, st, x, 0, nullptr, 0, 4, 4, LMj, nullptr)));
    c[1].frac = 32;
    EXPECT(einval(idsp_biquad_i16_df1(c, 2, st, x, 0, y, 0, 4, 4, FMj, nullptr)));               // frac
    c[1].frac = -1;
    EXPECT(einval(idsp_biquad_i16_df1(c, 2, st, x, 0, y, 0, 4, 4, FMj, nullptr)));
    EXPECT(!einval(idsp_biquad_i16_df1(c, 1, st, x, 0, y, 0, 0, 4, FMj, nullptr)));              // ... of a section that does not run
    c[1].frac = 31;
    cc[0].frac = 32;
    EXPECT(einval(idsp_biquad_i16_df1_clamp(cc, 1, st, x, 0, y, 0, 4, 4, FMj, nullptr)));
    cc[0].frac = 0;
    EXPECT(einval(idsp_biquad_i16_df1(c, 2, st, x, 3, y, 0, 4, 9, FMj, nullptr)));               // pitch < row (FrameMajor: row = lanes)
    EXPECT(einval(idsp_biquad_i16_df1(c, 2, st, x, 0, y, 3, 4, 9, FMj, nullptr)));
    EXPECT(einval(idsp_biquad_i16_df1(c, 2, st, x, 8, y, 0, 4, 9, LMj, nullptr)));               // (LaneMajor: row = frames)
    EXPECT(einval(idsp_biquad_i16_df1(c, 2, st, x, 0, y, 8, 4, 9, LMj, nullptr)));
    EXPECT(einval(idsp_biquad_i16_df1(c, 2, st, reinterpret_cast<int16_t *>(odd(x)), 0, y, 0, 4, 4, FMj, nullptr)));  // odd addresses
    EXPECT(einval(idsp_biquad_i16_df1(c, 2, st, x, 0, reinterpret_cast<int16_t *>(odd(y)), 0, 4, 4, LMj, nullptr)));
    // the in-place rule: y == x needs one pitch, 0 counting as the row; every other overlap of the extents is refused
    EXPECT(einval(idsp_biquad_i16_df1(c, 2, st, x, 0, x, 5, 4, 4, FMj, nullptr)));
    EXPECT(einval(idsp_biquad_i16_df1(c, 2, st, x, 6, x, 0, 4, 4, LMj, nullptr)));
    EXPECT(einval(idsp_biquad_i16_df1(c, 2, st, x, 0, x + 15, 0, 4, 4, FMj, nullptr)));          // y on the last element of x
    EXPECT(einval(idsp_biquad_i16_df1(c, 2, st, x + 15, 0, x, 0, 4, 4, LMj, nullptr)));          // x on the last element of y
    EXPECT(einval(idsp_biquad_i16_df1(c, 2, st, x, 8, x + 4, 8, 4, 4, FMj, nullptr)));           // y rows in the gaps of a pitched x
    EXPECT(einval(idsp_biquad_i16_df1(c, 2, st, x, size_t(1) << 62, y, 0, 4, 4, FMj, nullptr))); // an extent past size_t
    // the empty calls
    EXPECT(idsp_biquad_i16_df1(c, 2, st, x, 0, y, 0, 0, 4, FMj, nullptr) == IDSP_OK);
    EXPECT(idsp_biquad_i16_df1_clamp(cc, 1, st, x, 0, y, 0, 4, 0, LMj, nullptr) == IDSP_OK);
    EXPECT(idsp_biquad_i16_df1(nullptr, 0, nullptr, nullptr, 0, nullptr, 0, 0, 0, FMj, nullptr) == IDSP_OK);
    EXPECT(idsp_biquad_i16_df1(c, 2, st, x, 7, y, 1, 0, 5, FMj, nullptr) == IDSP_OK);            // FrameMajor row = lanes = 0: any pitch covers it
    EXPECT(idsp_biquad_i16_df1(c, 2, st, x, 0, x + 16, 0, 0, 0, FMj, nullptr) == IDSP_OK);

    try {  // no lanes: nothing is allocated, nothing launched
        BiquadI16Lanes<idsp_biquad_i16> d({c[0], c[1]}, 0);
        EXPECT(d.sections() == 2 && d.state().len() == 0);
        d.reset();
        d.process_view(View<int16_t, LaneMajor>{x, 3, 0}, ViewMut<int16_t, LaneMajor>{y, 3, 0});
        d.block(View<int16_t, FrameMajor>{x, 3, 0}, ViewMut<int16_t, FrameMajor>{y, 3, 0});
        d.inplace_view(ViewMut<int16_t, LaneMajor>{y, 3, 0});
        EXPECT(throws([&] { d.process_view(View<int16_t, LaneMajor>{x, 3, 0}, ViewMut<int16_t, LaneMajor>{y, 4, 0}); }));        // frames differ
        EXPECT(throws([&] { d.process_view(View<int16_t, LaneMajor>{x, 3, 1}, ViewMut<int16_t, LaneMajor>{y, 3, 1}); }));        // lanes differ
        EXPECT(throws([&] { d.process_view(View<int16_t, LaneMajor>{x, 3, 0}, ViewMut<int16_t, LaneMajor>{y, 3, 0}, 2, 0); }));  // x_pitch < frames
        EXPECT(throws([&] { d.process_view(View<int16_t, LaneMajor>{x, 3, 0}, ViewMut<int16_t, LaneMajor>{y, 3, 0}, 0, 2); }));
        idsp_biquad_i16 wrong = c[0];
        wrong.frac = 32;
        EXPECT(throws([&] { BiquadI16Lanes<idsp_biquad_i16> e({wrong}, 0); }));
        EXPECT(throws([&] { BiquadI16Lanes<idsp_biquad_i16> e(std::vector<idsp_biquad_i16>(IDSP_MAX_SECTIONS + 1, c[0]), 0); }));
        BiquadI16Lanes<idsp_biquad_clamp_i16> k({cc[0]}, 0);
        EXPECT(k.sections() == 1);
    } catch (const std::exception &e) {
        std::printf("empty mirror call threw: %s\n", e.what());
        bad++;
    }
    if (bad) return std::printf("%d failures\n", bad), 1;
    std::printf("biquad i16 host tests passed\n");
    return 0;
}
