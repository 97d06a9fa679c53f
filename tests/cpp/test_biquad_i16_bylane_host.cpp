// The by-lane 16-bit biquad's host side through the C ABI and the C++ mirror of include/idsp_hip.hpp: the bank ingestion
// (idsp_biquad_i16_bank_from_sos), the argument errors of idsp_biquad_i16_df1_bylane / _df1_clamp_bylane (NULL and odd `coef` among
// them), their empty calls, and what `BiquadI16ByLane` refuses and how it lays its planes out.  Every call here returns before anything
// is launched or allocated, so the program runs without a GPU: the pointers are host addresses that are only compared, never followed.
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
alignas(16) static int16_t cf[512];
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

template <class T>
static T *odd(T *p) { return reinterpret_cast<T *>(reinterpret_cast<char *>(p) + 1); }

int main()
{
    const int FMj = IDSP_FRAME_MAJOR, LMj = IDSP_LANE_MAJOR;
    EXPECT(idsp_version() == 4);

    // bank_from_sos: three lanes of two sections into planes, each section as idsp_biquad_i16_from_sos quantises it
    const double lp[6] = {0.06745527388907189, 0.13491054777814377, 0.06745527388907189, 1.0, -1.1429805025399011, 0.4128015980961886};
    const double ties[6] = {0.5 / 8192, -0.5 / 8192, 1.5 / 8192, 1.0, 2.5 / 8192, -2.5 / 8192};
    const double wild[6] = {4.0, -4.0 - 1.0 / 8192, std::numeric_limits<double>::quiet_NaN(), 1.0, std::numeric_limits<double>::infinity(), 3.9998779296875};
    const double *rows[3][2] = {{lp, ties}, {wild, lp}, {ties, wild}};
    std::vector<double> sos;
    for (auto &lane : rows)
        for (const double *r : lane) sos.insert(sos.end(), r, r + 6);
    for (size_t cv : {size_t(5), size_t(8)}) {
        const std::vector<int16_t> coef = biquad_i16_bank_from_sos(sos, 3, 2, 13, cv);
        EXPECT(coef.size() == 2 * cv * 3);
        for (size_t l = 0; l < 3; l++)
            for (size_t k = 0; k < 2; k++) {
                idsp_biquad_i16 q{};
                EXPECT(idsp_biquad_i16_from_sos(rows[l][k], 13, &q) == IDSP_OK);
                for (size_t v = 0; v < 5; v++) EXPECT(coef[(k * cv + v) * 3 + l] == q.ba[v]);
                if (cv == 8) EXPECT(coef[(k * cv + 5) * 3 + l] == 0 && coef[(k * cv + 6) * 3 + l] == INT16_MIN && coef[(k * cv + 7) * 3 + l] == INT16_MAX);
            }
    }
    EXPECT(einval(idsp_biquad_i16_bank_from_sos(nullptr, 3, 2, 13, 5, cf)) && einval(idsp_biquad_i16_bank_from_sos(sos.data(), 3, 2, 13, 5, nullptr)));
    EXPECT(einval(idsp_biquad_i16_bank_from_sos(sos.data(), 3, 2, -1, 5, cf)) && einval(idsp_biquad_i16_bank_from_sos(sos.data(), 3, 2, 32, 5, cf)));
    EXPECT(einval(idsp_biquad_i16_bank_from_sos(sos.data(), 3, 2, 13, 6, cf)) && einval(idsp_biquad_i16_bank_from_sos(sos.data(), 3, 2, 13, 0, cf)));
    EXPECT(einval(idsp_biquad_i16_bank_from_sos(sos.data(), 1, IDSP_MAX_SECTIONS + 1, 13, 5, cf)));
    EXPECT(idsp_biquad_i16_bank_from_sos(nullptr, 0, 2, 13, 5, nullptr) == IDSP_OK && idsp_biquad_i16_bank_from_sos(nullptr, 3, 0, 13, 8, nullptr) == IDSP_OK);
    EXPECT(throws([&] { biquad_i16_bank_from_sos(sos, 3, 2, 32); }) && throws([&] { biquad_i16_bank_from_sos(sos, 2, 2, 13); }));

    // the entries: what idsp_biquad_i16_df1 refuses, and coef
    EXPECT(einval(idsp_biquad_i16_df1_bylane(nullptr, 13, 2, st, x, 0, y, 0, 4, 4, FMj, nullptr)));        // NULL coef with n > 0 and lanes > 0
    EXPECT(einval(idsp_biquad_i16_df1_clamp_bylane(nullptr, 13, 1, st, x, 0, y, 0, 4, 4, LMj, nullptr)));
    EXPECT(einval(idsp_biquad_i16_df1_bylane(odd(cf), 13, 2, st, x, 0, y, 0, 4, 4, FMj, nullptr)));        // an odd coef address
    EXPECT(einval(idsp_biquad_i16_df1_clamp_bylane(odd(cf), 13, 2, st, x, 0, y, 0, 4, 4, LMj, nullptr)));
    EXPECT(einval(idsp_biquad_i16_df1_bylane(cf, 13, 2, st, x, 0, y, 0, 4, 4, 2, nullptr)));                // layout
    EXPECT(einval(idsp_biquad_i16_df1_bylane(cf, 13, IDSP_MAX_SECTIONS + 1, st, x, 0, y, 0, 4, 4, FMj, nullptr)));
    EXPECT(einval(idsp_biquad_i16_df1_bylane(cf, 13, 2, nullptr, x, 0, y, 0, 4, 4, FMj, nullptr)));         // NULL state
    EXPECT(einval(idsp_biquad_i16_df1_bylane(cf, 13, 2, st, nullptr, 0, y, 0, 4, 4, FMj, nullptr)));
    EXPECT(einval(idsp_biquad_i16_df1_clamp_bylane(cf, 13, 1, st, x, 0, nullptr, 0, 4, 4, LMj, nullptr)));
    EXPECT(einval(idsp_biquad_i16_df1_bylane(cf, 32, 2, st, x, 0, y, 0, 4, 4, FMj, nullptr)));              // frac
    EXPECT(einval(idsp_biquad_i16_df1_clamp_bylane(cf, -1, 2, st, x, 0, y, 0, 4, 4, FMj, nullptr)));
    EXPECT(einval(idsp_biquad_i16_df1_bylane(cf, 13, 2, st, x, 3, y, 0, 4, 9, FMj, nullptr)));              // pitch < row
    EXPECT(einval(idsp_biquad_i16_df1_bylane(cf, 13, 2, st, x, 0, y, 8, 4, 9, LMj, nullptr)));
    EXPECT(einval(idsp_biquad_i16_df1_bylane(cf, 13, 2, st, odd(x), 0, y, 0, 4, 4, FMj, nullptr)));         // odd x / y
    EXPECT(einval(idsp_biquad_i16_df1_bylane(cf, 13, 2, st, x, 0, odd(y), 0, 4, 4, LMj, nullptr)));
    EXPECT(einval(idsp_biquad_i16_df1_bylane(cf, 13, 2, st, x, 0, x, 5, 4, 4, FMj, nullptr)));              // y == x with two pitches
    EXPECT(einval(idsp_biquad_i16_df1_bylane(cf, 13, 2, st, x, 0, x + 15, 0, 4, 4, FMj, nullptr)));         // partial overlap
    EXPECT(einval(idsp_biquad_i16_df1_bylane(cf, 13, 0, st, x, 0, x + 2, 0, 4, 4, FMj, nullptr)));          // ... also for the copy of n == 0
    EXPECT(einval(idsp_biquad_i16_df1_bylane(cf, 13, 2, st, x, size_t(1) << 62, y, 0, 4, 4, FMj, nullptr)));
    // the empty calls
    EXPECT(idsp_biquad_i16_df1_bylane(cf, 13, 2, st, x, 0, y, 0, 0, 4, FMj, nullptr) == IDSP_OK);
    EXPECT(idsp_biquad_i16_df1_clamp_bylane(cf, 0, 1, st, x, 0, y, 0, 4, 0, LMj, nullptr) == IDSP_OK);
    EXPECT(idsp_biquad_i16_df1_bylane(nullptr, 31, 0, nullptr, nullptr, 0, nullptr, 0, 0, 0, FMj, nullptr) == IDSP_OK);
    EXPECT(idsp_biquad_i16_df1_bylane(nullptr, 13, 2, nullptr, x, 0, y, 0, 0, 5, FMj, nullptr) == IDSP_OK);  // no lanes: no planes, no state
    EXPECT(idsp_biquad_i16_df1_bylane(cf, 13, 2, st, x, 0, x, 0, 4, 0, LMj, nullptr) == IDSP_OK);            // in place, one pitch

    // the mirror: the planes it would upload, and what it refuses before it allocates anything
    const idsp_biquad_i16 a{{1, 2, 3, 4, 5}, 13}, b{{-1, -2, -3, -4, -5}, 13}, c{{6, 7, 8, 9, 10}, 13};
    const std::vector<int16_t> pl = BiquadI16ByLane<idsp_biquad_i16>::planes({{a, b}, {b, c}, {c, a}});
    EXPECT(pl.size() == 2 * 5 * 3);
    const idsp_biquad_i16 *want[3][2] = {{&a, &b}, {&b, &c}, {&c, &a}};
    for (size_t l = 0; l < 3; l++)
        for (size_t k = 0; k < 2; k++)
            for (size_t v = 0; v < 5; v++) EXPECT(pl[(k * 5 + v) * 3 + l] == want[l][k]->ba[v]);
    const idsp_biquad_clamp_i16 ka{{1, 2, 3, 4, 5}, 0, 7, 100, -100}, kb{{5, 4, 3, 2, 1}, 0, -7, -32768, 32767};
    const std::vector<int16_t> kp = BiquadI16ByLane<idsp_biquad_clamp_i16>::planes({{ka}, {kb}});
    EXPECT(kp.size() == 8 * 2 && kp[0] == 1 && kp[1] == 5 && kp[5 * 2] == 7 && kp[5 * 2 + 1] == -7 && kp[6 * 2] == 100 && kp[6 * 2 + 1] == -32768 &&
           kp[7 * 2] == -100 && kp[7 * 2 + 1] == 32767);
    using Bank = BiquadI16ByLane<idsp_biquad_i16>;
    idsp_biquad_i16 f14 = a, f32 = a;
    f14.frac = 14, f32.frac = 32;
    EXPECT(throws([&] { Bank e(std::vector<std::vector<idsp_biquad_i16>>{}); }));                        // no lane
    EXPECT(throws([&] { Bank e(std::vector<std::vector<idsp_biquad_i16>>{{}, {}}); }));                  // no section
    EXPECT(throws([&] { Bank e({{a, b}, {c}}); }));                                                      // section counts differ
    EXPECT(throws([&] { Bank e({{a, b}, {c, f14}}); }));                                                 // two fracs
    EXPECT(throws([&] { Bank e({{f32}}); }));                                                            // frac outside 0..31
    EXPECT(throws([&] { Bank e({std::vector<idsp_biquad_i16>(IDSP_MAX_SECTIONS + 1, a)}); }));
    if (bad) return std::printf("%d failures\n", bad), 1;
    std::printf("biquad i16 by-lane host tests passed\n");
    return 0;
}
