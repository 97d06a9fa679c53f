// cic_ring_host.h — host-side coefficient helpers of the wave-per-lane Cic kernels (cic_ring.h).
#pragma once

#include "cic_ring.h"

namespace idsp {
namespace cicr_host {

// g_d(n) = (A^n)[d][0], d = 0 .. N-1, for n = R 2^k: Toeplitz triangles multiply like polynomials truncated to N terms;
// A itself is all ones.  u64 wrapping arithmetic — the low 32 bits are the i32 coefficients.
struct Poly {
    uint64_t c[IDSP_CIC_MAX_ORDER];
};
inline Poly mul(const Poly &a, const Poly &b, int n)
{
    Poly r{};
    for (int i = 0; i < n; i++)
        for (int j = 0; i + j < n; j++) r.c[i + j] += a.c[i] * b.c[j];
    return r;
}
inline Poly power(uint64_t e, int n)
{
    Poly base{}, r{};
    for (int i = 0; i < n; i++) base.c[i] = 1;
    r.c[0] = 1;
    while (e) {
        if (e & 1) r = mul(r, base, n);
        base = mul(base, base, n);
        e >>= 1;
    }
    return r;
}

// scan coefficients g_d(R 2^k), k = 0 .. 5
template <class T, int N>
inline cicr::ScanCoef<T, N> scan_coef(size_t R)
{
    cicr::ScanCoef<T, N> coef{};
    Poly g = power(R, N);
    for (int k = 0; k < cicr::kSteps; k++) {
        for (int d = 1; d < N; d++) coef.g[k][d - 1] = static_cast<typename std::make_unsigned<T>::type>(g.c[d]);
        g = mul(g, g, N);
    }
    return coef;
}

// f(N, PPT) with the order (1..6) and the pieces per chunk (1, 2, 4, 8: CicPlan::ppt) as compile-time constants: both ring launchers' ladder
template <class F>
inline int for_order_pieces(int order, int ppt, F &&f)
{
    const auto pieces = [&](auto n) {
        switch (ppt) {
            case 1: return f(n, int_c<1>{});
            case 2: return f(n, int_c<2>{});
            case 4: return f(n, int_c<4>{});
            case 8: return f(n, int_c<8>{});
            default: return fail(IDSP_EINVAL, "no Cic ring kernel for %d pieces per chunk", ppt);
        }
    };
    switch (order) {
        case 1: return pieces(int_c<1>{});
        case 2: return pieces(int_c<2>{});
        case 3: return pieces(int_c<3>{});
        case 4: return pieces(int_c<4>{});
        case 5: return pieces(int_c<5>{});
        case 6: return pieces(int_c<6>{});
        default: return fail(IDSP_EINVAL, "Cic order N = %d not in 1..%d", order, IDSP_CIC_MAX_ORDER);
    }
}

static_assert(cicr::kW == thr::kCicRingMinFrames && cicr::kFmLanes == thr::kCicRingFmLanes, "plan_cic: one whole block of chunks, groups of 16 lanes");

}  // namespace cicr_host
}  // namespace idsp
