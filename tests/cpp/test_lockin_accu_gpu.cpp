// `idsp_hip::AccuLo::lockin_view` (include/idsp_hip.hpp, idsp_lockin_i32_accu_process) against the chain it fuses — `AccuLo::process_view` into an LO buffer, then
// idsp_lockin_i32_lo_process — on one small shape per layout, from the same non-zero arm state.  Needs a GPU; tests/test_gpu_lockin_accu_host_mirror.py builds and runs it.
#include <cstdio>
#include <vector>

#include "idsp_hip.hpp"

using namespace idsp_hip;

template <class Layout>
static int run(const char *name)
{
    const size_t lanes = 65, updates = 9;
    const int k = 3;
    const size_t frames = updates << k;
    idsp_lockin_i32 arms{};
    arms.order = 2, arms.cascade = 2;
    for (int c = 0; c < 2; c++) arms.k[c][0] = 1 << (20 + c), arms.k[c][1] = -(1 << (27 - c));
    const size_t words = idsp_lockin_state_words(&arms) - 2;
    uint32_t r = 12345u;
    auto next = [&r]() { return r = r * 1664525u + 1013904223u; };
    std::vector<int32_t> x(frames * lanes), accu(updates * lanes * 2);
    std::vector<uint32_t> st(words * lanes);
    for (auto &v : x) v = int32_t(next());
    for (auto &v : accu) v = int32_t(next());
    for (auto &v : st) v = next();
    DeviceBuffer<int32_t> xd(x), ad(accu), lo(frames * lanes * 2), want(frames * lanes * 2), got(frames * lanes * 2);
    DeviceBuffer<uint32_t> s_chain(st), s_fused(st);
    const AccuLo a(k, 3, -99);
    a.process_view(View<int32_t, Layout>::from_flat(ad, lanes, 2), ViewMut<int32_t, Layout>::from_flat(lo, lanes, 2));
    check(idsp_lockin_i32_lo_process(&arms, s_chain.data(), xd.data(), lo.data(), want.data(), lanes, frames, Layout::value, nullptr));
    a.lockin_view(arms, s_fused, View<int32_t, Layout>::from_flat(xd, lanes), View<int32_t, Layout>::from_flat(ad, lanes, 2),
                  ViewMut<int32_t, Layout>::from_flat(got, lanes, 2));
    check(idsp_stream_sync(nullptr));
    int bad = 0;
    if (got.to_host() != want.to_host()) std::printf("%s: y differs from the chain\n", name), bad++;
    if (s_fused.to_host() != s_chain.to_host()) std::printf("%s: state differs from the chain\n", name), bad++;
    if (s_fused.to_host() == st) std::printf("%s: the state did not move\n", name), bad++;
    bool threw = false;
    try {
        DeviceBuffer<uint32_t> small(words * lanes - 1);
        a.lockin_view(arms, small, View<int32_t, Layout>::from_flat(xd, lanes), View<int32_t, Layout>::from_flat(ad, lanes, 2),
                      ViewMut<int32_t, Layout>::from_flat(got, lanes, 2));
    } catch (const std::exception &) {
        threw = true;
    }
    if (!threw) std::printf("%s: a short state was accepted\n", name), bad++;
    return bad;
}

int main()
{
    int bad = 0;
    try {
        bad += run<FrameMajor>("FrameMajor");
        bad += run<LaneMajor>("LaneMajor");
    } catch (const std::exception &ex) {
        std::printf("threw: %s\n", ex.what());
        bad++;
    }
    if (bad) return std::printf("%d failures\n", bad), 1;
    std::printf("lockin_accu host-mirror tests passed\n");
    return 0;
}
