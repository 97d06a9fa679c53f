// `idsp_hip::Dsm` / `DsmLanes` (include/idsp_hip.hpp) against direct calls of the C ABI on one small shape: dense in both layouts on one state, a pitched y, `reset()`.  Needs a GPU; tests/test_gpu_dsm_host_mirror.py builds and runs it.
#include <cstdio>
#include <vector>

#include "idsp_hip.hpp"

using namespace idsp_hip;

int main()
{
    const size_t lanes = 65, frames = 37, yp = 68;  // FrameMajor y rows of 65 bytes, 68 apart
    const int order = 3;
    int bad = 0;
    try {
        std::vector<uint32_t> x(frames * lanes);
        uint32_t s = 12345u;
        for (auto &v : x) v = (s = s * 1664525u + 1013904223u);
        for (size_t f = 0; f < frames; f++) x[f * lanes + 1] = 0x87654321u;
        DeviceBuffer<uint32_t> xd(x), raw(idsp_dsm_state_words(order) * lanes);
        DeviceBuffer<int8_t> want(frames * lanes), got(frames * lanes), want2(frames * lanes), got2(frames * lanes);
        // FrameMajor, then the same buffer read as LaneMajor (other samples per lane, the state goes on): C ABI
        check(idsp_dsm_u32(order, raw.data(), xd.data(), 0, want.data(), 0, lanes, frames, IDSP_FRAME_MAJOR, nullptr));
        check(idsp_dsm_u32(order, raw.data(), xd.data(), 0, want2.data(), 0, lanes, frames, IDSP_LANE_MAJOR, nullptr));
        // the mirror
        DsmLanes d = Dsm(order).lanes(lanes);
        if (d.order() != order || d.state().len() != 6 * lanes) std::printf("DsmLanes: order / state size\n"), bad++;
        d.block(View<uint32_t, FrameMajor>::from_flat(xd, lanes), ViewMut<int8_t, FrameMajor>::from_flat(got, lanes));
        d.process_view(View<uint32_t, LaneMajor>::from_flat(xd, lanes), ViewMut<int8_t, LaneMajor>::from_flat(got2, lanes));
        check(idsp_stream_sync(nullptr));
        const std::vector<int8_t> w = want.to_host();
        if (got.to_host() != w || got2.to_host() != want2.to_host() || d.state().to_host() != raw.to_host()) std::printf("DsmLanes differs from idsp_dsm_u32\n"), bad++;
        bool any = false;
        for (int8_t v : w) any = any || v != 0;
        if (!any) std::printf("all outputs are zero\n"), bad++;
        // reset() is `Dsm::default()` again, and the pitches reach the entry: rows land yp apart, the gaps keep their content
        d.reset();
        DeviceBuffer<uint32_t> zero(6 * lanes);
        DeviceBuffer<int8_t> dense(frames * lanes), pitched(std::vector<int8_t>((frames - 1) * yp + lanes, int8_t(-77)));
        check(idsp_dsm_u32(order, zero.data(), xd.data(), 0, dense.data(), 0, lanes, frames, IDSP_FRAME_MAJOR, nullptr));
        d.process_view(View<uint32_t, FrameMajor>{xd.data(), frames, lanes}, ViewMut<int8_t, FrameMajor>{pitched.data(), frames, lanes}, 0, yp);
        check(idsp_stream_sync(nullptr));
        const std::vector<int8_t> a = dense.to_host(), b = pitched.to_host();
        for (size_t f = 0; f < frames && !bad; f++)
            for (size_t c = 0; c < yp && f * yp + c < b.size(); c++)
                if (b[f * yp + c] != (c < lanes ? a[f * lanes + c] : int8_t(-77))) {
                    std::printf("pitched y differs at frame %zu column %zu\n", f, c);
                    bad++;
                    break;
                }
        if (d.state().to_host() != zero.to_host()) std::printf("state after reset() and one call differs\n"), bad++;
        bool threw = false;
        try {
            d.process_view(View<uint32_t, FrameMajor>{xd.data(), frames, lanes}, ViewMut<int8_t, FrameMajor>{pitched.data(), frames, lanes}, 0, lanes - 1);
        } catch (const Error &e) {
            threw = e.code == IDSP_EINVAL;
        }
        if (!threw) std::printf("a short pitch was accepted\n"), bad++;
    } catch (const std::exception &ex) {
        std::printf("threw: %s\n", ex.what());
        bad++;
    }
    if (bad) return std::printf("%d failures\n", bad), 1;
    std::printf("dsm host-mirror tests passed\n");
    return 0;
}
