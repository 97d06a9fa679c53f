// The C++ mirror of the polyphase channelizer (include/idsp_hip.hpp: PolyphaseBank) against direct calls of the C ABI: the same
// bytes in y and in every state word, both layouts, dft 0 / 1, out of place, continued on the same state, and in place.
#include <cstdio>
#include <cstring>
#include <vector>

#include "idsp_hip.hpp"

using namespace idsp_hip;

static uint32_t lcg(uint32_t &s) { return s = s * 1664525u + 1013904223u; }

template <class Layout>
static int run(int taps, bool dft, size_t lanes, size_t frames)
{
    uint32_t seed = uint32_t(taps * 131 + int(dft) + int(lanes));
    std::vector<float> x(lanes * frames * 8);
    for (float &v : x) v = float(int32_t(lcg(seed)) >> 8) * (1.0f / 8388608.0f);
    PolyphaseBank bank = PolyphaseBank::prototype(taps, dft, lanes);
    const idsp_pfb_f32 cfg = bank.config();
    const size_t words = idsp_pfb_state_words(&cfg);
    if (words != size_t(8 * taps + 1) || bank.state().len() != words * lanes) return 1;
    DeviceBuffer<float> xd(x), y1(x.size()), y2(x.size());
    DeviceBuffer<uint32_t> st(words * lanes);
    for (int round = 0; round < 2; round++) {  // the second round continues the state
        bank.process_view(View<float, Layout>::from_flat(xd, lanes, 8), ViewMut<float, Layout>::from_flat(y1, lanes, 8));
        check(idsp_pfb_f32_process(&cfg, st.data(), xd.data(), y2.data(), lanes, frames, Layout::value, nullptr));
        check(idsp_stream_sync(nullptr));
        const std::vector<float> a = y1.to_host(), b = y2.to_host();
        const std::vector<uint32_t> sa = bank.state().to_host(), sb = st.to_host();
        if (std::memcmp(a.data(), b.data(), a.size() * 4) || std::memcmp(sa.data(), sb.data(), sa.size() * 4)) return 2;
    }
    DeviceBuffer<float> xy(x);
    bank.inplace_view(ViewMut<float, Layout>::from_flat(xy, lanes, 8));
    check(idsp_pfb_f32_process(&cfg, st.data(), xd.data(), xd.data(), lanes, frames, Layout::value, nullptr));
    check(idsp_stream_sync(nullptr));
    const std::vector<float> a = xy.to_host(), b = xd.to_host();
    const std::vector<uint32_t> sa = bank.state().to_host(), sb = st.to_host();
    if (std::memcmp(a.data(), b.data(), a.size() * 4) || std::memcmp(sa.data(), sb.data(), sa.size() * 4)) return 3;
    return 0;
}

int main()
{
    try {
        for (int taps : {1, 3, 8, 16})
            for (bool dft : {false, true})
                for (size_t lanes : {size_t(1), size_t(65)}) {
                    const size_t frames = 256 + 9;
                    if (int rc = run<FrameMajor>(taps, dft, lanes, frames)) return std::printf("FrameMajor taps %d dft %d lanes %zu: %d\n", taps, int(dft), lanes, rc), 1;
                    if (int rc = run<LaneMajor>(taps, dft, lanes, frames)) return std::printf("LaneMajor taps %d dft %d lanes %zu: %d\n", taps, int(dft), lanes, rc), 1;
                }
        bool threw = false;
        try {
            PolyphaseBank::prototype(17, true, 4);
        } catch (const Error &) {
            threw = true;
        }
        if (!threw) return std::printf("taps 17 accepted\n"), 1;
    } catch (const std::exception &e) {
        return std::printf("exception: %s\n", e.what()), 1;
    }
    std::printf("polyphase host-mirror tests passed\n");
    return 0;
}
