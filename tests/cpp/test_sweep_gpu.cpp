// `idsp_hip::SweepOsc` (include/idsp_hip.hpp) against direct calls of the C ABI on one small shape, `emitted()` included.  Needs a GPU; tests/test_gpu_sweep_host_mirror.py builds and runs it.
#include <cstdio>
#include <vector>

#include "idsp_hip.hpp"

using namespace idsp_hip;

int main()
{
    const size_t lanes = 65, frames = 17;
    const Sweep fit = Sweep::fit(0.3f, 3000.0f, 3.0f);
    std::vector<Sweep> sweeps(lanes, fit);
    sweeps[1] = Sweep(1 << 30, int64_t(1) << 62);           // emits 3, then ends
    sweeps[2] = Sweep((1u << 31) - 1, (int64_t(1) << 62) + 12345);  // emits 1
    sweeps[64] = Sweep(1, INT64_MIN);                        // has ended
    int bad = 0;
    try {
        // the state the mirrors must build: state lo, hi, accu = 0, rate, emitted = 0
        std::vector<uint32_t> st(IDSP_SWEEP_STATE_WORDS * lanes, 0u);
        for (size_t l = 0; l < lanes; l++) {
            st[l] = uint32_t(uint64_t(sweeps[l].state)), st[lanes + l] = uint32_t(uint64_t(sweeps[l].state) >> 32);
            st[4 * lanes + l] = uint32_t(sweeps[l].rate);
        }
        DeviceBuffer<uint32_t> raw(st);
        DeviceBuffer<int32_t> want(lanes * frames * 2), got(lanes * frames * 2);
        check(idsp_sweep_i32(raw.data(), want.data(), lanes, frames, IDSP_LANE_MAJOR, nullptr));
        SweepOsc osc(sweeps);
        osc.generate(ViewMut<int32_t, LaneMajor>::from_flat(got, lanes, 2));
        check(idsp_stream_sync(nullptr));
        if (got.to_host() != want.to_host() || osc.state().to_host() != raw.to_host()) std::printf("SweepOsc differs from idsp_sweep_i32\n"), bad++;
        const std::vector<uint64_t> e = osc.emitted();
        if (e.size() != lanes || e[0] != frames || e[1] != 3 || e[2] != 1 || e[64] != 0) {
            std::printf("emitted: %llu %llu %llu %llu\n", (unsigned long long)e[0], (unsigned long long)e[1], (unsigned long long)e[2], (unsigned long long)e[64]);
            bad++;
        }

    } catch (const std::exception &ex) {
        std::printf("threw: %s\n", ex.what());
        bad++;
    }
    if (bad) return std::printf("%d failures\n", bad), 1;
    std::printf("sweep host-mirror tests passed\n");
    return 0;
}
