// `idsp_hip::RPLLLanes` and `idsp_hip::AccuLo` (include/idsp_hip.hpp) against direct calls of the C ABI on one small shape, `phase()` / `frequency()` included.  Needs a GPU; tests/test_gpu_rpll_host_mirror.py builds and runs it.
#include <cstdio>
#include <vector>

#include "idsp_hip.hpp"

using namespace idsp_hip;

int main()
{
    const size_t lanes = 65, updates = 17;
    const int k = 3;
    int bad = 0;
    try {
        // a reference of period 333 + lane counter cycles per lane, one update per 256: the harness of src/rpll.rs:134-151 without noise
        std::vector<int32_t> ts(updates * lanes * 2, 0);
        for (size_t l = 0; l < lanes; l++) {
            int32_t next = int32_t(l), time = 0;
            for (size_t u = 0; u < updates; u++, time += 256)
                if (time - next >= 0) ts[(l * updates + u) * 2] = 1, ts[(l * updates + u) * 2 + 1] = next, next += 333 + int32_t(l);
        }
        DeviceBuffer<int32_t> tsd(ts), want_a(updates * lanes * 2), got_a(updates * lanes * 2);
        DeviceBuffer<int32_t> want_lo((updates << k) * lanes * 2), got_lo((updates << k) * lanes * 2);
        DeviceBuffer<uint32_t> raw(IDSP_RPLL_STATE_WORDS * lanes);
        const idsp_rpll cfg{8, 9, 8};
        const idsp_accu_lo lo{k, 2, 1000};
        check(idsp_rpll_i32(&cfg, raw.data(), tsd.data(), want_a.data(), lanes, updates, IDSP_LANE_MAJOR, nullptr));
        check(idsp_accu_lo_i32(&lo, want_a.data(), want_lo.data(), lanes, updates, IDSP_LANE_MAJOR, nullptr));
        RPLLLanes r = RPLLConfig(8, 9, 8).lanes(lanes);
        r.process_view(View<int32_t, LaneMajor>::from_flat(tsd, lanes, 2), ViewMut<int32_t, LaneMajor>::from_flat(got_a, lanes, 2));
        AccuLo(k, 2, 1000).process_view(View<int32_t, LaneMajor>::from_flat(got_a, lanes, 2), ViewMut<int32_t, LaneMajor>::from_flat(got_lo, lanes, 2));
        check(idsp_stream_sync(nullptr));
        const std::vector<uint32_t> st = raw.to_host();
        if (got_a.to_host() != want_a.to_host() || r.state().to_host() != st) std::printf("RPLLLanes differs from idsp_rpll_i32\n"), bad++;
        if (got_lo.to_host() != want_lo.to_host()) std::printf("AccuLo differs from idsp_accu_lo_i32\n"), bad++;
        const std::vector<int32_t> y = r.phase();
        const std::vector<uint32_t> f = r.frequency();
        const std::vector<int32_t> a = want_a.to_host();
        for (size_t l = 0; l < lanes; l++) {
            // the last `Accu` of a lane is { phase(), frequency() as i32 } (src/rpll.rs:76)
            if (y[l] != int32_t(st[3 * lanes + l]) || f[l] != st[2 * lanes + l] || y[l] != a[(l * updates + updates - 1) * 2] ||
                int32_t(f[l]) != a[(l * updates + updates - 1) * 2 + 1]) {
                std::printf("lane %zu: phase / frequency differ from the state words\n", l);
                bad++;
                break;
            }
        }
        if (f[0] == 0) std::printf("lane 0 saw no timestamp\n"), bad++;
    } catch (const std::exception &ex) {
        std::printf("threw: %s\n", ex.what());
        bad++;
    }
    if (bad) return std::printf("%d failures\n", bad), 1;
    std::printf("rpll host-mirror tests passed\n");
    return 0;
}
