// idsp_hip.hpp — header-only C++17 host layer above the C ABI (idsp_hip.h).
//
// The reference is compiled code (Rust) and no Rust toolchain exists in the
// build image, so the host side that mirrors its operator interface is C++:
// the same names, argument meaning and error behaviour as `dsp_process` /
// `idsp`, resolved statically like the reference's traits.  Needs only the C
// ABI (no HIP headers): buffers are owned through idsp_device_alloc.
//
//   reference                                                   here
//   ----------------------------------------------------------  --------------------------------
//   Biquad<Q32<F>> / Biquad<f32>        (src/iir/biquad.rs:96)  Biquad<Q32<F>> / Biquad<float>
//   BiquadClamp<C, T>                   (src/iir/biquad.rs:121) BiquadClamp<C>
//   DirectForm1<T> / DirectForm2Transposed<T> / DirectForm1Wide / DirectForm1Dither   (state tags)
//   Split::new(cfg, S::default()).lanes::<N>()  (split.rs:272)  Split(cfg, S{}).lanes(n)
//   Process::block / Inplace::inplace           (process.rs:34) .block(x, y) / .inplace(xy)   FrameMajor
//   ViewProcess::process_view(View<LaneMajor>)  (view.rs:245)   .process_view(View, ViewMut)
//   HBF_DEC_CASCADE + HbfDec2..32 / HBF_INT_CASCADE (hbf.rs)    HbfDecCascade / HbfIntCascade
//   Lockin<[Lowpass<N>; K]> + Accu      (lockin.rs, accu.rs)    Lockin<N, K>
//   ByLane<[C; N]>                      (compose.rs:363)        ByLane<Cfg, S>(configs)
//   coefficients::Filter, pid::Builder, Pid, Units (iir/coefficients.rs, iir/pid.rs)  Filter, pid::Builder, Pid, Units
//   Split::stateful(Cic::new(rate)).decimate()/.interpolate() (cic.rs:338-346)  CicDecimator<T> / CicInterpolator<T>
//   cossin(phase)                       (cossin.rs:14)          cossin(phases, out)
//   atan2(y, x) / Complex::arg          (atan2.rs:66)           atan2(xy, out)
//   cordic::{cos_sin, sqrt_atan2, ...}  (cordic.rs:80-107)      cordic::cos_sin(xy, z, out), cordic::sqrt_atan2(xy, z, out), ...
//   PLL / PLLState                      (pll.rs:33-107)         PLL::from_bandwidth(bw, split).lanes(n)
//   Unwrapper<i64> / ClampWrap<W<i32>>  (unwrap.rs:109-194)     Unwrapper(n) / ClampWrap(n)
//   overflowing_sub / saturating_scale  (unwrap.rs:73-101)      overflowing_sub(y, x) / saturating_scale(lo, hi, shift)
//
// Misuse that is a `debug_assert!`/panic in the reference throws idsp_hip::Error.
#pragma once

#include <array>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "idsp_hip.h"

namespace idsp_hip {

struct Error : std::runtime_error {
    int code;
    Error(int c, const std::string &what) : std::runtime_error(what), code(c) {}
};

inline void check(int rc)
{
    if (rc < 0) throw Error(rc, std::string("idsp status ") + std::to_string(rc) + ": " + idsp_last_error());
}
inline void require(bool ok, const char *what)
{
    if (!ok) throw Error(IDSP_EINVAL, what);
}

// ------------------------------------------------------------------ memory
/// Device-resident slice `[T]` (the engine never allocates behind the caller's back).
template <class T>
class DeviceBuffer {
public:
    DeviceBuffer() = default;
    explicit DeviceBuffer(size_t n, bool zero = true) : n_(n)
    {
        if (n) {
            check(idsp_device_alloc(reinterpret_cast<void **>(&p_), n * sizeof(T)));
            if (zero) check(idsp_device_memset(p_, 0, n * sizeof(T), nullptr));
        }
    }
    explicit DeviceBuffer(const std::vector<T> &host) : DeviceBuffer(host.size(), false) { upload(host); }
    DeviceBuffer(const DeviceBuffer &) = delete;
    DeviceBuffer &operator=(const DeviceBuffer &) = delete;
    DeviceBuffer(DeviceBuffer &&o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr, o.n_ = 0; }
    DeviceBuffer &operator=(DeviceBuffer &&o) noexcept
    {
        std::swap(p_, o.p_);
        std::swap(n_, o.n_);
        return *this;
    }
    ~DeviceBuffer()
    {
        if (p_) idsp_device_free(p_);
    }
    T *data() { return p_; }
    const T *data() const { return p_; }
    size_t len() const { return n_; }
    void upload(const std::vector<T> &host)
    {
        require(host.size() == n_, "upload: length mismatch");
        if (n_) {
            check(idsp_device_h2d(p_, host.data(), n_ * sizeof(T), nullptr));
            check(idsp_stream_sync(nullptr));
        }
    }
    std::vector<T> to_host() const
    {
        std::vector<T> h(n_);
        if (n_) {
            check(idsp_device_d2h(h.data(), p_, n_ * sizeof(T), nullptr));
            check(idsp_stream_sync(nullptr));
        }
        return h;
    }

private:
    T *p_ = nullptr;
    size_t n_ = 0;
};

// ------------------------------------------------------------------- views
struct FrameMajor {  // dsp-process/src/view.rs:10
    static constexpr int value = IDSP_FRAME_MAJOR;
};
struct LaneMajor {  // dsp-process/src/view.rs:17
    static constexpr int value = IDSP_LANE_MAJOR;
};

/// `View<'_, T, Layout, L>` with a runtime lane count (dsp-process/src/view.rs:24-28).
template <class T, class Layout>
struct View {
    const T *flat;
    size_t frames, lanes;
    /// `from_flat`: `assert_eq!(flat.len(), frames * L)` (view.rs:182)
    static View from_flat(const DeviceBuffer<T> &b, size_t lanes, size_t width = 1)
    {
        require(lanes && b.len() % (lanes * width) == 0, "flat.len() is not frames * L");
        return View{b.data(), b.len() / (lanes * width), lanes};
    }
};
template <class T, class Layout>
struct ViewMut {
    T *flat;
    size_t frames, lanes;
    static ViewMut from_flat(DeviceBuffer<T> &b, size_t lanes, size_t width = 1)
    {
        require(lanes && b.len() % (lanes * width) == 0, "flat.len() is not frames * L");
        return ViewMut{b.data(), b.len() / (lanes * width), lanes};
    }
    operator View<T, Layout>() const { return View<T, Layout>{flat, frames, lanes}; }
};

// ---------------------------------------------------------- configurations
/// Coefficient type tag `Q32<F>` = `Q<i32, i64, F>` (dsp-fixedpoint/src/lib.rs:474-492).
template <int F>
struct Q32 {
    static_assert(F >= 0 && F < 32, "0 <= F < 32");
    static constexpr int frac = F;
};

template <class C>
struct Biquad;  // src/iir/biquad.rs:96-116: ba = [b0, b1, b2, a1, a2], a1/a2 as used

template <int F>
struct Biquad<Q32<F>> {
    using Sample = int32_t;
    std::array<int32_t, 5> ba{};  // raw Q bits
    /// `Biquad::from([[b0,b1,b2],[a0,a1,a2]])` (biquad.rs:545-566) + f64 -> Q32<F> (num_traits_impl.rs:32-46)
    static Biquad from_sos(const std::array<double, 6> &sos)
    {
        idsp_biquad_i32 q;
        check(idsp_biquad_i32_from_sos(sos.data(), F, &q));
        Biquad b;
        std::memcpy(b.ba.data(), q.ba, sizeof(q.ba));
        return b;
    }
    static Biquad proportional(int32_t k) { return Biquad{{k, 0, 0, 0, 0}}; }          // biquad.rs:196-200
    static Biquad identity() { return proportional(int32_t(1) << F); }                   // biquad.rs:184
    static Biquad hold() { return Biquad{{0, 0, 0, int32_t(1) << F, 0}}; }               // biquad.rs:212-214
    int32_t forward_gain() const { return int32_t(uint32_t(ba[0]) + uint32_t(ba[1]) + uint32_t(ba[2])); }
    idsp_biquad_i32 abi() const
    {
        idsp_biquad_i32 q;
        std::memcpy(q.ba, ba.data(), sizeof(q.ba));
        q.frac = F;
        return q;
    }
};

template <>
struct Biquad<float> {
    using Sample = float;
    std::array<float, 5> ba{};
    static Biquad from_sos(const std::array<float, 6> &sos)
    {
        idsp_biquad_f32 q;
        check(idsp_biquad_f32_from_sos(sos.data(), &q));
        Biquad b;
        std::memcpy(b.ba.data(), q.ba, sizeof(q.ba));
        return b;
    }
    static Biquad from_sos(const std::array<double, 6> &sos)
    {
        idsp_biquad_f32 q;
        check(idsp_biquad_f32_from_sos_f64(sos.data(), &q));
        Biquad b;
        std::memcpy(b.ba.data(), q.ba, sizeof(q.ba));
        return b;
    }
    static Biquad proportional(float k) { return Biquad{{k, 0, 0, 0, 0}}; }
    static Biquad identity() { return proportional(1.0f); }
    static Biquad hold() { return Biquad{{0, 0, 0, 1.0f, 0}}; }
    float forward_gain() const { return ba[0] + ba[1] + ba[2]; }
    idsp_biquad_f32 abi() const
    {
        idsp_biquad_f32 q;
        std::memcpy(q.ba, ba.data(), sizeof(q.ba));
        return q;
    }
};

template <>
struct Biquad<double> {
    using Sample = double;
    std::array<double, 5> ba{};
    static Biquad from_sos(const std::array<double, 6> &sos)
    {
        idsp_biquad_f64 q;
        check(idsp_biquad_f64_from_sos(sos.data(), &q));
        Biquad b;
        std::memcpy(b.ba.data(), q.ba, sizeof(q.ba));
        return b;
    }
    static Biquad proportional(double k) { return Biquad{{k, 0, 0, 0, 0}}; }
    static Biquad identity() { return proportional(1.0); }
    static Biquad hold() { return Biquad{{0, 0, 0, 1.0, 0}}; }
    double forward_gain() const { return ba[0] + ba[1] + ba[2]; }
    idsp_biquad_f64 abi() const
    {
        idsp_biquad_f64 q;
        std::memcpy(q.ba, ba.data(), sizeof(q.ba));
        return q;
    }
};

/// `BiquadClamp<C, T>` (biquad.rs:121-171); defaults u = 0, min = T::MIN, max = T::MAX
/// (+-inf for floats, src/num.rs:33-52).
template <class C>
struct BiquadClamp {
    using Sample = typename Biquad<C>::Sample;
    Biquad<C> coeff{};
    Sample u = Sample(0);
    Sample min = std::numeric_limits<Sample>::has_infinity ? -std::numeric_limits<Sample>::infinity()
                                                           : std::numeric_limits<Sample>::lowest();
    Sample max = std::numeric_limits<Sample>::has_infinity ? std::numeric_limits<Sample>::infinity()
                                                           : std::numeric_limits<Sample>::max();
    BiquadClamp() = default;
    BiquadClamp(const Biquad<C> &c) : coeff(c) {}  // `From<F: Into<Biquad<C>>>` (biquad.rs:578-588)
};

// state kinds (tags): words per lane and section
// words are per 32-bit value; f64 states take twice as many (Lanes multiplies by sizeof(Sample)/4)
struct DirectForm1 { static constexpr int words = 4; };            // biquad.rs:319
struct DirectForm2Transposed { static constexpr int words = 2; };  // biquad.rs:407
struct DirectForm1Wide { static constexpr int words = 6; };        // biquad.rs:445-454
struct DirectForm1Dither { static constexpr int words = 5; };      // biquad.rs:484-491

namespace detail {
using StreamI32 = int (*)(const idsp_biquad_i32 *, size_t, void *, const int32_t *, int32_t *, size_t, size_t, int, void *);
using StreamClampI32 = int (*)(const idsp_biquad_clamp_i32 *, size_t, void *, const int32_t *, int32_t *, size_t, size_t, int, void *);
using StreamF32 = int (*)(const idsp_biquad_f32 *, size_t, void *, const float *, float *, size_t, size_t, int, void *);
using StreamClampF32 = int (*)(const idsp_biquad_clamp_f32 *, size_t, void *, const float *, float *, size_t, size_t, int, void *);
using StreamF64 = int (*)(const idsp_biquad_f64 *, size_t, void *, const double *, double *, size_t, size_t, int, void *);
using StreamClampF64 = int (*)(const idsp_biquad_clamp_f64 *, size_t, void *, const double *, double *, size_t, size_t, int, void *);

// (configuration, state) -> C entry point; a missing specialisation is the reference's
// "trait not implemented" compile error.
template <class Cfg, class S>
struct Entry;
template <int F> struct Entry<Biquad<Q32<F>>, DirectForm1> { static constexpr StreamI32 fn = idsp_biquad_i32_df1; };
template <int F> struct Entry<Biquad<Q32<F>>, DirectForm1Dither> { static constexpr StreamI32 fn = idsp_biquad_i32_dither; };
template <int F> struct Entry<Biquad<Q32<F>>, DirectForm1Wide> { static constexpr StreamI32 fn = idsp_biquad_i32_wide; };
template <int F> struct Entry<BiquadClamp<Q32<F>>, DirectForm1> { static constexpr StreamClampI32 fn = idsp_biquad_i32_df1_clamp; };
template <int F> struct Entry<BiquadClamp<Q32<F>>, DirectForm1Dither> { static constexpr StreamClampI32 fn = idsp_biquad_i32_dither_clamp; };
template <int F> struct Entry<BiquadClamp<Q32<F>>, DirectForm1Wide> { static constexpr StreamClampI32 fn = idsp_biquad_i32_wide_clamp; };
template <> struct Entry<Biquad<float>, DirectForm1> { static constexpr StreamF32 fn = idsp_biquad_f32_df1; };
template <> struct Entry<Biquad<float>, DirectForm2Transposed> { static constexpr StreamF32 fn = idsp_biquad_f32_df2t; };
template <> struct Entry<BiquadClamp<float>, DirectForm1> { static constexpr StreamClampF32 fn = idsp_biquad_f32_df1_clamp; };
template <> struct Entry<BiquadClamp<float>, DirectForm2Transposed> { static constexpr StreamClampF32 fn = idsp_biquad_f32_df2t_clamp; };

template <> struct Entry<Biquad<double>, DirectForm1> { static constexpr StreamF64 fn = idsp_biquad_f64_df1; };
template <> struct Entry<Biquad<double>, DirectForm2Transposed> { static constexpr StreamF64 fn = idsp_biquad_f64_df2t; };
template <> struct Entry<BiquadClamp<double>, DirectForm1> { static constexpr StreamClampF64 fn = idsp_biquad_f64_df1_clamp; };
template <> struct Entry<BiquadClamp<double>, DirectForm2Transposed> { static constexpr StreamClampF64 fn = idsp_biquad_f64_df2t_clamp; };

inline idsp_biquad_f64 to_abi(const Biquad<double> &b) { return b.abi(); }
inline idsp_biquad_clamp_f64 to_abi(const BiquadClamp<double> &c)
{
    idsp_biquad_clamp_f64 q;
    std::memcpy(q.ba, c.coeff.ba.data(), sizeof(q.ba));
    q.u = c.u, q.min = c.min, q.max = c.max;
    return q;
}
template <int F> idsp_biquad_i32 to_abi(const Biquad<Q32<F>> &b) { return b.abi(); }
inline idsp_biquad_f32 to_abi(const Biquad<float> &b) { return b.abi(); }
template <int F>
idsp_biquad_clamp_i32 to_abi(const BiquadClamp<Q32<F>> &c)
{
    idsp_biquad_clamp_i32 q;
    std::memcpy(q.ba, c.coeff.ba.data(), sizeof(q.ba));
    q.frac = F, q.u = c.u, q.min = c.min, q.max = c.max;
    return q;
}
inline idsp_biquad_clamp_f32 to_abi(const BiquadClamp<float> &c)
{
    idsp_biquad_clamp_f32 q;
    std::memcpy(q.ba, c.coeff.ba.data(), sizeof(q.ba));
    q.u = c.u, q.min = c.min, q.max = c.max;
    return q;
}
}  // namespace detail

/// `Split<Lanes<C>, [S; lanes]>` resident on the GPU: one shared configuration (or a serial
/// slice of sections, `[C] x [S]`, dsp-process/src/compose.rs:43-77), `lanes` independent states.
template <class Cfg, class S>
class Lanes {
public:
    using Sample = typename Cfg::Sample;
    using Abi = decltype(detail::to_abi(std::declval<Cfg>()));

    Lanes(const std::vector<Cfg> &sections, size_t lanes, void *stream = nullptr)
        : lanes_(lanes), stream_(stream),
          state_(size_t(S::words) * (sizeof(Sample) / 4) * (sections.empty() ? 1 : sections.size()) * lanes)
    {
        for (const auto &c : sections) abi_.push_back(detail::to_abi(c));
    }
    size_t lanes() const { return lanes_; }
    /// per-lane state words, word-plane-major; zero == `Default::default()`
    DeviceBuffer<uint32_t> &state() { return state_; }

    /// `Process::block(&mut self, x: &[[X; N]], y: &mut [[Y; N]])` — FrameMajor (process.rs:44-49)
    void block(const DeviceBuffer<Sample> &x, DeviceBuffer<Sample> &y)
    {
        require(x.len() == y.len(), "x.len() != y.len()");  // process.rs:45 debug_assert_eq!
        require(lanes_ && x.len() % lanes_ == 0, "slice is not a whole number of frames");
        run(x.data(), y.data(), x.len() / lanes_, IDSP_FRAME_MAJOR);
    }
    /// `Inplace::inplace(&mut self, xy: &mut [[X; N]])` (process.rs:61-65)
    void inplace(DeviceBuffer<Sample> &xy)
    {
        require(lanes_ && xy.len() % lanes_ == 0, "slice is not a whole number of frames");
        run(xy.data(), xy.data(), xy.len() / lanes_, IDSP_FRAME_MAJOR);
    }
    /// `ViewProcess::process_view` (view.rs:245-248; `Lanes` lane-slice path compose.rs:478-494)
    template <class Layout>
    void process_view(View<Sample, Layout> x, ViewMut<Sample, Layout> y)
    {
        require(x.frames == y.frames, "x.frames() != y.frames()");  // compose.rs:488
        require(x.lanes == lanes_ && y.lanes == lanes_, "view lane count != Lanes lane count");
        run(x.flat, y.flat, x.frames, Layout::value);
    }
    template <class Layout>
    void inplace_view(ViewMut<Sample, Layout> xy)
    {
        require(xy.lanes == lanes_, "view lane count != Lanes lane count");
        run(xy.flat, xy.flat, xy.frames, Layout::value);
    }

private:
    void run(const Sample *x, Sample *y, size_t frames, int layout)
    {
        check(detail::Entry<Cfg, S>::fn(abi_.data(), abi_.size(), state_.data(), x, y, lanes_, frames, layout, stream_));
    }
    size_t lanes_;
    void *stream_;
    std::vector<Abi> abi_;
    DeviceBuffer<uint32_t> state_;
};

/// `Split<C, S>` (dsp-process/src/split.rs:29-34).
template <class Cfg, class S>
struct SplitT {
    std::vector<Cfg> sections;
    /// `.lanes::<N>()` (split.rs:272-277)
    Lanes<Cfg, S> lanes(size_t n, void *stream = nullptr) const { return Lanes<Cfg, S>(sections, n, stream); }
};
template <class Cfg, class S>
SplitT<Cfg, S> Split(const Cfg &cfg, S)
{
    return SplitT<Cfg, S>{{cfg}};
}
template <class Cfg, class S>
SplitT<Cfg, S> Split(const std::vector<Cfg> &sections, S)
{
    return SplitT<Cfg, S>{sections};
}

namespace detail {
using ByLaneI32 = int (*)(const int32_t *, int, size_t, void *, const int32_t *, int32_t *, size_t, size_t, int, void *);
using ByLaneF32 = int (*)(const float *, size_t, void *, const float *, float *, size_t, size_t, int, void *);
using ByLaneF64 = int (*)(const double *, size_t, void *, const double *, double *, size_t, size_t, int, void *);
template <class Cfg, class S>
struct EntryByLane;
template <int F> struct EntryByLane<Biquad<Q32<F>>, DirectForm1> { static constexpr ByLaneI32 fn = idsp_biquad_i32_df1_bylane; };
template <int F> struct EntryByLane<Biquad<Q32<F>>, DirectForm1Dither> { static constexpr ByLaneI32 fn = idsp_biquad_i32_dither_bylane; };
template <int F> struct EntryByLane<Biquad<Q32<F>>, DirectForm1Wide> { static constexpr ByLaneI32 fn = idsp_biquad_i32_wide_bylane; };
template <int F> struct EntryByLane<BiquadClamp<Q32<F>>, DirectForm1> { static constexpr ByLaneI32 fn = idsp_biquad_i32_df1_clamp_bylane; };
template <int F> struct EntryByLane<BiquadClamp<Q32<F>>, DirectForm1Dither> { static constexpr ByLaneI32 fn = idsp_biquad_i32_dither_clamp_bylane; };
template <int F> struct EntryByLane<BiquadClamp<Q32<F>>, DirectForm1Wide> { static constexpr ByLaneI32 fn = idsp_biquad_i32_wide_clamp_bylane; };
template <> struct EntryByLane<Biquad<float>, DirectForm1> { static constexpr ByLaneF32 fn = idsp_biquad_f32_df1_bylane; };
template <> struct EntryByLane<Biquad<float>, DirectForm2Transposed> { static constexpr ByLaneF32 fn = idsp_biquad_f32_df2t_bylane; };
template <> struct EntryByLane<BiquadClamp<float>, DirectForm1> { static constexpr ByLaneF32 fn = idsp_biquad_f32_df1_clamp_bylane; };
template <> struct EntryByLane<BiquadClamp<float>, DirectForm2Transposed> { static constexpr ByLaneF32 fn = idsp_biquad_f32_df2t_clamp_bylane; };
template <> struct EntryByLane<Biquad<double>, DirectForm1> { static constexpr ByLaneF64 fn = idsp_biquad_f64_df1_bylane; };
template <> struct EntryByLane<Biquad<double>, DirectForm2Transposed> { static constexpr ByLaneF64 fn = idsp_biquad_f64_df2t_bylane; };
template <> struct EntryByLane<BiquadClamp<double>, DirectForm1> { static constexpr ByLaneF64 fn = idsp_biquad_f64_df1_clamp_bylane; };
template <> struct EntryByLane<BiquadClamp<double>, DirectForm2Transposed> { static constexpr ByLaneF64 fn = idsp_biquad_f64_df2t_clamp_bylane; };

template <class C> struct FracOf { static constexpr int value = -1; };
template <int F> struct FracOf<Biquad<Q32<F>>> { static constexpr int value = F; };
template <int F> struct FracOf<BiquadClamp<Q32<F>>> { static constexpr int value = F; };
// one lane's section as the 5 (ba) or 8 (ba, u, min, max) plane values
template <class C> std::vector<typename Biquad<C>::Sample> plane_values(const Biquad<C> &b)
{
    return {b.ba.begin(), b.ba.end()};
}
template <class C> std::vector<typename Biquad<C>::Sample> plane_values(const BiquadClamp<C> &c)
{
    std::vector<typename Biquad<C>::Sample> v(c.coeff.ba.begin(), c.coeff.ba.end());
    v.push_back(c.u), v.push_back(c.min), v.push_back(c.max);
    return v;
}
}  // namespace detail

/// `Split<ByLane<[C; lanes]>, [S; lanes]>` (dsp-process/src/compose.rs:363-390): lane i is filtered by
/// configuration i with state i.  `configs[i]` is the serial slice of sections of lane i; every lane
/// has the same number of sections.  The coefficients are kept on the GPU as lane-contiguous planes.
template <class Cfg, class S>
class ByLane {
public:
    using Sample = typename Cfg::Sample;
    explicit ByLane(const std::vector<std::vector<Cfg>> &configs, void *stream = nullptr)
        : lanes_(configs.size()), sections_(configs.empty() ? 0 : configs[0].size()), stream_(stream),
          state_(size_t(S::words) * (sizeof(Sample) / 4) * (sections_ ? sections_ : 1) * lanes_)
    {
        require(lanes_ && sections_, "ByLane needs at least one lane and one section");
        const size_t cv = detail::plane_values(configs[0][0]).size();
        std::vector<Sample> host(sections_ * cv * lanes_);
        for (size_t l = 0; l < lanes_; l++) {
            require(configs[l].size() == sections_, "every lane needs the same number of sections");
            for (size_t k = 0; k < sections_; k++) {
                const auto v = detail::plane_values(configs[l][k]);
                for (size_t i = 0; i < cv; i++) host[(k * cv + i) * lanes_ + l] = v[i];
            }
        }
        coef_ = DeviceBuffer<Sample>(host);
    }
    /// one section per lane
    explicit ByLane(const std::vector<Cfg> &configs, void *stream = nullptr) : ByLane(wrap(configs), stream) {}
    size_t lanes() const { return lanes_; }
    DeviceBuffer<uint32_t> &state() { return state_; }
    DeviceBuffer<Sample> &coefficients() { return coef_; }

    /// `Process::block` over `&[[X; N]]` — FrameMajor (compose.rs:363-372 per frame)
    void block(const DeviceBuffer<Sample> &x, DeviceBuffer<Sample> &y)
    {
        require(x.len() == y.len(), "x.len() != y.len()");
        require(x.len() % lanes_ == 0, "slice is not a whole number of frames");
        run(x.data(), y.data(), x.len() / lanes_, IDSP_FRAME_MAJOR);
    }
    void inplace(DeviceBuffer<Sample> &xy)
    {
        require(xy.len() % lanes_ == 0, "slice is not a whole number of frames");
        run(xy.data(), xy.data(), xy.len() / lanes_, IDSP_FRAME_MAJOR);
    }
    /// `SplitViewProcess::process_view` (compose.rs:375-389)
    template <class Layout>
    void process_view(View<Sample, Layout> x, ViewMut<Sample, Layout> y)
    {
        require(x.frames == y.frames, "x.frames() != y.frames()");  // compose.rs:386
        require(x.lanes == lanes_ && y.lanes == lanes_, "view lane count != ByLane lane count");
        run(x.flat, y.flat, x.frames, Layout::value);
    }

private:
    static std::vector<std::vector<Cfg>> wrap(const std::vector<Cfg> &c)
    {
        std::vector<std::vector<Cfg>> r;
        for (const auto &v : c) r.push_back({v});
        return r;
    }
    void run(const Sample *x, Sample *y, size_t frames, int layout)
    {
        if constexpr (detail::FracOf<Cfg>::value >= 0)
            check(detail::EntryByLane<Cfg, S>::fn(coef_.data(), detail::FracOf<Cfg>::value, sections_, state_.data(), x, y,
                                                  lanes_, frames, layout, stream_));
        else
            check(detail::EntryByLane<Cfg, S>::fn(coef_.data(), sections_, state_.data(), x, y, lanes_, frames, layout, stream_));
    }
    size_t lanes_, sections_;
    void *stream_;
    DeviceBuffer<uint32_t> state_;
    DeviceBuffer<Sample> coef_;
};

// ------------------------------------------------------- coefficient front-end
namespace detail {
template <class C> struct OutOf;
template <int F> struct OutOf<Q32<F>> {
    using Rec = idsp_biquad_clamp_i32;
    static int pid(const idsp_pid_builder *b, double t, int v, int32_t *ba) { return idsp_pid_build_i32(b, t, v, F, ba); }
    static int pid_clamp(const idsp_pid *p, const idsp_units *u, int v, Rec *o) { return idsp_pid_build_clamp_i32(p, u, v, F, o); }
    static int ba(const idsp_ba_config *c, const idsp_units *u, int v, Rec *o) { return idsp_config_ba_build_i32(c, u, v, F, o); }
    static int filter(const idsp_filter_config *c, const idsp_units *u, int v, Rec *o) { return idsp_config_filter_build_i32(c, u, v, F, o); }
};
template <> struct OutOf<float> {
    using Rec = idsp_biquad_clamp_f32;
    static int pid(const idsp_pid_builder *b, double t, int v, float *ba) { return idsp_pid_build_f32(b, t, v, ba); }
    static int pid_clamp(const idsp_pid *p, const idsp_units *u, int v, Rec *o) { return idsp_pid_build_clamp_f32(p, u, v, o); }
    static int ba(const idsp_ba_config *c, const idsp_units *u, int v, Rec *o) { return idsp_config_ba_build_f32(c, u, v, o); }
    static int filter(const idsp_filter_config *c, const idsp_units *u, int v, Rec *o) { return idsp_config_filter_build_f32(c, u, v, o); }
};
template <> struct OutOf<double> {
    using Rec = idsp_biquad_clamp_f64;
    static int pid(const idsp_pid_builder *b, double t, int v, double *ba) { return idsp_pid_build_f64(b, t, v, ba); }
    static int pid_clamp(const idsp_pid *p, const idsp_units *u, int v, Rec *o) { return idsp_pid_build_clamp_f64(p, u, v, o); }
    static int ba(const idsp_ba_config *c, const idsp_units *u, int v, Rec *o) { return idsp_config_ba_build_f64(c, u, v, o); }
    static int filter(const idsp_filter_config *c, const idsp_units *u, int v, Rec *o) { return idsp_config_filter_build_f64(c, u, v, o); }
};
template <class C, class Rec>
BiquadClamp<C> clamp_from(const Rec &r)
{
    BiquadClamp<C> c;
    for (int i = 0; i < 5; i++) c.coeff.ba[i] = r.ba[i];
    c.u = r.u, c.min = r.min, c.max = r.max;
    return c;
}
}  // namespace detail

/// `pid::Units<T>` (src/iir/pid.rs:350-375)
struct Units : idsp_units {
    Units(double t_ = 1.0, double x_ = 1.0, double y_ = 1.0) : idsp_units{t_, x_, y_} {}
};

/// `coefficients::Filter<T>` (src/iir/coefficients.rs:27-40) with T = f64 (f32 = true: T = f32);
/// setters as in the reference (:110-238).  `build*` is unchecked, `try_build*` validates and throws.
class Filter {
public:
    explicit Filter(bool f32 = false) : f_{0.0, 1.0, 1.0, f32 ? double(1.0f / std::sqrt(2.0f)) : 1.0 / std::sqrt(2.0), IDSP_SHAPE_Q, f32} {}
    Filter &frequency(double critical, double sample) { return critical_frequency(t(t(critical) / t(sample))); }
    Filter &critical_frequency(double f0) { return angular_critical_frequency(t(t(6.283185307179586476925286766559) * t(f0))); }
    Filter &angular_critical_frequency(double w0) { f_.frequency = t(w0); return *this; }
    Filter &gain(double k) { f_.gain = t(k); return *this; }
    Filter &gain_db(double k_db) { return gain(pow10(k_db)); }
    Filter &shelf(double a) { f_.shelf = t(a); return *this; }
    Filter &shelf_db(double a_db) { return shelf(pow10(a_db)); }
    Filter &inverse_q(double qi) { return q(t(1.0 / t(qi))); }
    Filter &q(double v) { return set_shape(IDSP_SHAPE_Q, v); }
    Filter &bandwidth(double bw) { return set_shape(IDSP_SHAPE_BANDWIDTH, bw); }
    Filter &shelf_slope(double s) { return set_shape(IDSP_SHAPE_SLOPE, s); }
    Filter &set_shape(idsp_shape_kind kind, double v) { f_.shape_kind = kind, f_.shape = t(v); return *this; }
    /// `Filter::build(typ)` (:483-495) -> [b0, b1, b2, a0, a1, a2]
    std::array<double, 6> build(idsp_filter_type typ) const { return go(typ, 0); }
    /// `Filter::try_build(typ)` (:498-501)
    std::array<double, 6> try_build(idsp_filter_type typ) const { return go(typ, 1); }
    void validate() const { go(IDSP_LOWPASS, 1); }
    std::array<double, 6> lowpass() const { return build(IDSP_LOWPASS); }
    std::array<double, 6> highpass() const { return build(IDSP_HIGHPASS); }
    std::array<double, 6> bandpass() const { return build(IDSP_BANDPASS); }
    std::array<double, 6> allpass() const { return build(IDSP_ALLPASS); }
    std::array<double, 6> notch() const { return build(IDSP_NOTCH); }
    std::array<double, 6> peaking() const { return build(IDSP_PEAKING); }
    std::array<double, 6> lowshelf() const { return build(IDSP_LOWSHELF); }
    std::array<double, 6> highshelf() const { return build(IDSP_HIGHSHELF); }
    std::array<double, 6> iho() const { return build(IDSP_IHO); }
    /// `build_biquad::<C>` / `try_build_biquad::<C>` (:504-517): `From<[[T; 3]; 2]>` evaluated in T
    template <class C> Biquad<C> build_biquad(idsp_filter_type typ) const { return to_biquad<C>(build(typ)); }
    template <class C> Biquad<C> try_build_biquad(idsp_filter_type typ) const { return to_biquad<C>(try_build(typ)); }
    template <class C> BiquadClamp<C> build_clamped(idsp_filter_type typ) const { return BiquadClamp<C>(build_biquad<C>(typ)); }

private:
    double t(double v) const { return f_.f32 ? double(float(v)) : v; }
    double pow10(double db) const { return f_.f32 ? double(std::pow(10.0f, float(db) / 20.0f)) : std::pow(10.0, db / 20.0); }
    std::array<double, 6> go(idsp_filter_type typ, int validate) const
    {
        std::array<double, 6> ba{};
        check(idsp_filter_build(&f_, typ, validate, ba.data()));
        return ba;
    }
    template <class C>
    Biquad<C> to_biquad(const std::array<double, 6> &ba) const
    {
        idsp_ba_config c{};
        for (int i = 0; i < 6; i++) c.ba[i] = ba[i];
        c.min = -std::numeric_limits<double>::infinity(), c.max = std::numeric_limits<double>::infinity(), c.f32 = f_.f32;
        const Units one;
        typename detail::OutOf<C>::Rec r;
        check(detail::OutOf<C>::ba(&c, &one, 0, &r));
        return detail::clamp_from<C>(r).coeff;
    }
    idsp_filter f_;
};

namespace pid {
enum Action { I2 = 0, I = 1, P = 2, D = 3, D2 = 4 };                  // src/iir/pid.rs:61-75
enum Order { OrderP = 2, OrderI = 1, OrderI2 = 0 };                  // src/iir/pid.rs:14-24

/// `pid::Builder<T>` (src/iir/pid.rs:40-55)
class Builder {
public:
    explicit Builder(bool f32 = false)
    {
        b_.order = OrderI, b_.f32 = f32;
        for (int i = 0; i < 5; i++) b_.gain[i] = 0.0, b_.limit[i] = std::numeric_limits<double>::infinity();
    }
    Builder &order(Order o) { b_.order = o; return *this; }
    Builder &gain(Action a, double g) { b_.gain[a] = g; return *this; }
    Builder &limit(Action a, double l) { b_.limit[a] = l; return *this; }
    Builder &kp(double g) { return gain(P, g); }
    Builder &ki(double g) { return gain(I, g); }
    Builder &ki2(double g) { return gain(I2, g); }
    Builder &kd(double g) { return gain(D, g); }
    Builder &kd2(double g) { return gain(D2, g); }
    Builder &limit_i(double l) { return limit(I, l); }
    Builder &limit_i2(double l) { return limit(I2, l); }
    Builder &limit_d(double l) { return limit(D, l); }
    Builder &limit_d2(double l) { return limit(D2, l); }
    /// `Build<Biquad<C>>::build(&period)` (pid.rs:256-328) / `try_build` (:225-232)
    template <class C> Biquad<C> build(double period) const { return go<C>(period, 0); }
    template <class C> Biquad<C> try_build(double period) const { return go<C>(period, 1); }
    const idsp_pid_builder &abi() const { return b_; }

private:
    template <class C>
    Biquad<C> go(double period, int validate) const
    {
        Biquad<C> out;
        check(detail::OutOf<C>::pid(&b_, period, validate, out.ba.data()));
        return out;
    }
    idsp_pid_builder b_{};
};
}  // namespace pid

/// `pid::Pid<T>` (src/iir/pid.rs:384-431) == `config::PidConfig<T>`
class Pid {
public:
    explicit Pid(bool f32 = false) : b_(f32) {}
    Pid &order(pid::Order o) { b_.order(o); return *this; }
    Pid &kp(double g) { b_.kp(g); return *this; }
    Pid &ki(double g) { b_.ki(g); return *this; }
    Pid &ki2(double g) { b_.ki2(g); return *this; }
    Pid &kd(double g) { b_.kd(g); return *this; }
    Pid &kd2(double g) { b_.kd2(g); return *this; }
    Pid &limit_i(double l) { b_.limit_i(l); return *this; }
    Pid &limit_i2(double l) { b_.limit_i2(l); return *this; }
    Pid &limit_d(double l) { b_.limit_d(l); return *this; }
    Pid &limit_d2(double l) { b_.limit_d2(l); return *this; }
    Pid &setpoint(double s) { setpoint_ = s; return *this; }
    Pid &output_limits(double mn, double mx) { min_ = mn, max_ = mx; return *this; }
    /// `Build<BiquadClamp<C, Y>> for Pid<T>` (pid.rs:533-567) / `try_build` (:521-528)
    template <class C> BiquadClamp<C> build(const Units &u) const { return go<C>(u, 0); }
    template <class C> BiquadClamp<C> try_build(const Units &u) const { return go<C>(u, 1); }

private:
    template <class C>
    BiquadClamp<C> go(const Units &u, int validate) const
    {
        const idsp_pid p{b_.abi(), setpoint_, min_, max_};
        typename detail::OutOf<C>::Rec r;
        check(detail::OutOf<C>::pid_clamp(&p, &u, validate, &r));
        return detail::clamp_from<C>(r);
    }
    pid::Builder b_;
    double setpoint_ = 0.0, min_ = -std::numeric_limits<double>::infinity(), max_ = std::numeric_limits<double>::infinity();
};

/// `BiquadConfig::Ba(BaConfig)` and `BiquadConfig::Filter(FilterConfig)` arms of
/// `BiquadConfig::{build, try_build}` (src/iir/config.rs:355-430); the Pid arm is `Pid` above,
/// the Raw arm is the `BiquadClamp` itself.
template <class C>
BiquadClamp<C> build_config(const idsp_ba_config &c, const Units &u, bool validate = false)
{
    typename detail::OutOf<C>::Rec r;
    check(detail::OutOf<C>::ba(&c, &u, validate, &r));
    return detail::clamp_from<C>(r);
}
template <class C>
BiquadClamp<C> build_config(const idsp_filter_config &c, const Units &u, bool validate = false)
{
    typename detail::OutOf<C>::Rec r;
    check(detail::OutOf<C>::filter(&c, &u, validate, &r));
    return detail::clamp_from<C>(r);
}

/// Same-rate linear-phase FIR `type_fir!` (src/hbf.rs:70-138): OddSymmetric / EvenSymmetric /
/// OddAntiSymmetric / EvenAntiSymmetric `<[f32; M]>` as `SplitProcess<f32, f32, [f32; N]>`.
class FirSym {
public:
    FirSym(idsp_fir_kind kind, const std::vector<float> &taps, size_t lanes, void *stream = nullptr)
        : lanes_(lanes), stream_(stream)
    {
        require(!taps.empty() && taps.size() <= IDSP_HBF_MAX_TAPS, "1..32 taps");
        cfg_.kind = kind, cfg_.m = int32_t(taps.size());
        for (size_t k = 0; k < taps.size(); k++) cfg_.taps[k] = taps[k];
        state_ = DeviceBuffer<uint32_t>(idsp_fir_sym_state_words(&cfg_) * lanes);
    }
    DeviceBuffer<uint32_t> &state() { return state_; }
    template <class Layout>
    void process_view(View<float, Layout> x, ViewMut<float, Layout> y)
    {
        require(x.frames == y.frames && x.lanes == lanes_ && y.lanes == lanes_, "view shape mismatch");
        check(idsp_fir_sym_f32_process(&cfg_, state_.data(), x.flat, y.flat, lanes_, x.frames, Layout::value, stream_));
    }

private:
    idsp_fir_sym_f32 cfg_{};
    size_t lanes_;
    void *stream_;
    DeviceBuffer<uint32_t> state_;
};

// ----------------------------------------------------------------- half-band
enum class HbfTaps { Taps140 = 0 /* HBF_TAPS, hbf.rs:308-349 */, Taps98 = 1 /* HBF_TAPS_98, hbf.rs:258-292 */ };

template <bool DEC>
class HbfCascade {
public:
    /// `HBF_DEC_CASCADE` / `HBF_INT_CASCADE` restricted to a 2^stages rate change with
    /// `HbfDec2..32` / `HbfInt2..32` state for `lanes` streams (hbf.rs:363-421,454-512).
    HbfCascade(int stages, size_t lanes, HbfTaps taps = HbfTaps::Taps140, void *stream = nullptr)
        : lanes_(lanes), stream_(stream)
    {
        check(DEC ? idsp_hbf_dec_cascade(int(taps), stages, &cfg_) : idsp_hbf_int_cascade(int(taps), stages, &cfg_));
        state_ = DeviceBuffer<uint32_t>((DEC ? idsp_hbf_dec_state_words(&cfg_) : idsp_hbf_int_state_words(&cfg_)) * lanes);
    }
    size_t rate() const { return size_t(1) << cfg_.stages; }
    /// `hbf_dec_response_length` / `hbf_int_response_length` (hbf.rs:424-448,515-539)
    int response_length() const { return DEC ? idsp_hbf_dec_response_length(&cfg_) : idsp_hbf_int_response_length(&cfg_); }
    DeviceBuffer<uint32_t> &state() { return state_; }
    /// decimator: x = `[[f32; R]]` chunks, y = `[f32]`; interpolator: the reverse
    template <class Layout>
    void process_view(View<float, Layout> x, ViewMut<float, Layout> y)
    {
        require(x.frames == y.frames && x.lanes == lanes_ && y.lanes == lanes_, "view shape mismatch");
        check(DEC ? idsp_hbf_dec_f32(&cfg_, state_.data(), x.flat, y.flat, lanes_, x.frames, Layout::value, stream_)
                  : idsp_hbf_int_f32(&cfg_, state_.data(), x.flat, y.flat, lanes_, x.frames, Layout::value, stream_));
    }

private:
    idsp_hbf_cascade_f32 cfg_{};
    size_t lanes_;
    void *stream_;
    DeviceBuffer<uint32_t> state_;
};
using HbfDecCascade = HbfCascade<true>;
using HbfIntCascade = HbfCascade<false>;

/// `iir::normal::Normal<C>` (src/iir/normal.rs:28-35) x `DirectForm1`: the record is `Biquad<C>` with
/// ba = [b0, b1, b2, p.re, p.im]; `Split(normal, DirectForm1{})`-style lanes.
template <class C>
class NormalLanes {
public:
    using Sample = typename Biquad<C>::Sample;
    NormalLanes(const std::vector<Biquad<C>> &sections, size_t lanes, void *stream = nullptr)
        : lanes_(lanes), stream_(stream), state_(size_t(4) * (sizeof(Sample) / 4) * (sections.empty() ? 1 : sections.size()) * lanes)
    {
        for (const auto &c : sections) abi_.push_back(detail::to_abi(c));
    }
    /// `Normal::<f64>::from(&[[b0,b1,b2],[a0,a1,a2]])` (normal.rs:62-76) as the ba record; throws for real poles
    static Biquad<double> from_ba(const std::array<double, 6> &sos)
    {
        Biquad<double> b;
        check(idsp_normal_from_sos(sos.data(), b.ba.data()));
        return b;
    }
    DeviceBuffer<uint32_t> &state() { return state_; }
    template <class Layout>
    void process_view(View<Sample, Layout> x, ViewMut<Sample, Layout> y)
    {
        require(x.frames == y.frames && x.lanes == lanes_ && y.lanes == lanes_, "view shape mismatch");
        if constexpr (std::is_same<Sample, int32_t>::value)
            check(idsp_normal_i32_df1(abi_.data(), abi_.size(), state_.data(), x.flat, y.flat, lanes_, x.frames, Layout::value, stream_));
        else if constexpr (std::is_same<Sample, float>::value)
            check(idsp_normal_f32_df1(abi_.data(), abi_.size(), state_.data(), x.flat, y.flat, lanes_, x.frames, Layout::value, stream_));
        else
            check(idsp_normal_f64_df1(abi_.data(), abi_.size(), state_.data(), x.flat, y.flat, lanes_, x.frames, Layout::value, stream_));
    }

private:
    size_t lanes_;
    void *stream_;
    std::vector<decltype(detail::to_abi(std::declval<Biquad<C>>()))> abi_;
    DeviceBuffer<uint32_t> state_;
};

/// Serial chain of `iir::wdf::Wdf<N, M>` sections (src/iir/wdf.rs:103-171) over `lanes` lanes.
class WdfLanes {
public:
    /// `Wdf::<N, M>::quantize(&g)` (wdf.rs:126-137); throws Error(IDSP_EOUTOFRANGE) where the reference returns None
    static idsp_wdf quantize(uint32_t m, const std::vector<double> &g)
    {
        idsp_wdf w;
        check(idsp_wdf_quantize(int(g.size()), m, g.data(), &w));
        return w;
    }
    WdfLanes(const std::vector<idsp_wdf> &sections, size_t lanes, void *stream = nullptr)
        : sec_(sections), lanes_(lanes), stream_(stream), state_(idsp_wdf_state_words(sections.data(), sections.size()) * lanes)
    {
    }
    DeviceBuffer<uint32_t> &state() { return state_; }
    template <class Layout>
    void process_view(View<int32_t, Layout> x, ViewMut<int32_t, Layout> y)
    {
        require(x.frames == y.frames && x.lanes == lanes_ && y.lanes == lanes_, "view shape mismatch");
        check(idsp_wdf_i32(sec_.data(), sec_.size(), state_.data(), x.flat, y.flat, lanes_, x.frames, Layout::value, stream_));
    }

private:
    std::vector<idsp_wdf> sec_;
    size_t lanes_;
    void *stream_;
    DeviceBuffer<uint32_t> state_;
};

/// `Cic<T, N, M>::new(rate)` (src/cic.rs:13-47), T = int32_t or int64_t, chunked as
/// `Split::stateful(cic).decimate()` / `.interpolate()` (src/cic.rs:338-346) over `lanes` lanes.
template <class T, bool DEC>
class CicLanes {
    static_assert(std::is_same<T, int32_t>::value || std::is_same<T, int64_t>::value, "Cic<T>: T is i32 or i64");

public:
    CicLanes(int order, uint32_t rate, size_t lanes, int comb_delay = 1, void *stream = nullptr)
        : cfg_{order, comb_delay, rate}, lanes_(lanes), stream_(stream)
    {
        const size_t words = idsp_cic_state_words(&cfg_, int(sizeof(T) * 8));
        require(words > 0, "Cic: order 1..6, comb delay 1..4");
        state_ = DeviceBuffer<uint32_t>(words * lanes);
    }
    int64_t gain() const { return std::is_same<T, int64_t>::value ? idsp_cic_gain(&cfg_) : int64_t(int32_t(idsp_cic_gain(&cfg_))); }
    int gain_log2() const { return idsp_cic_gain_log2(&cfg_); }                 // cic.rs:111-113
    size_t response_length() const { return idsp_cic_response_length(&cfg_); }  // cic.rs:116-118
    size_t chunk() const { return size_t(cfg_.rate) + 1; }                      // R
    DeviceBuffer<uint32_t> &state() { return state_; }
    /// x: chunks `[T; R]` (decimator) or samples (interpolator); y the other
    template <class Layout>
    void process_view(View<T, Layout> x, ViewMut<T, Layout> y)
    {
        require(x.frames == y.frames && x.lanes == lanes_ && y.lanes == lanes_, "view shape mismatch");
        if constexpr (std::is_same<T, int64_t>::value)
            check((DEC ? idsp_cic_dec_i64 : idsp_cic_int_i64)(&cfg_, state_.data(), x.flat, y.flat, lanes_, x.frames, Layout::value, stream_));
        else
            check((DEC ? idsp_cic_dec_i32 : idsp_cic_int_i32)(&cfg_, state_.data(), x.flat, y.flat, lanes_, x.frames, Layout::value, stream_));
    }

private:
    idsp_cic cfg_;
    size_t lanes_;
    void *stream_;
    DeviceBuffer<uint32_t> state_;
};
template <class T> using CicDecimator = CicLanes<T, true>;
template <class T> using CicInterpolator = CicLanes<T, false>;

// ------------------------------------------------------------ DDS / lock-in
/// `cossin(p: i32[N]) -> i32[N, 2]` (src/py.rs:10-28)
inline void cossin(const DeviceBuffer<int32_t> &phase, DeviceBuffer<int32_t> &out, void *stream = nullptr)
{
    require(out.len() == 2 * phase.len(), "out.len() != 2 * phase.len()");
    check(idsp_cossin_i32(phase.data(), out.data(), phase.len(), stream));
}

/// `atan2(xy: i32[N, 2]) -> i32[N]` (src/py.rs:30-47); on `[re, im]` rows = `Complex<i32>::arg` (src/complex.rs:254-256)
inline void atan2(const DeviceBuffer<int32_t> &xy, DeviceBuffer<int32_t> &out, void *stream = nullptr)
{
    require(xy.len() == 2 * out.len(), "xy.len() != 2 * out.len()");
    check(idsp_atan2_i32(xy.data(), out.data(), out.len(), stream));
}

/// The CORDIC family (src/cordic.rs:80-107): xy holds rows `[x, y]`, z one word per row; the overloads without z take z = 0 for
/// every row (the C entry's NULL).  The pair functions write rows `[first, second]` of the reference's tuple (out may be xy), mul
/// and div one word per row (out may be z).
namespace cordic {
namespace detail {
using Entry = int (*)(const int32_t *, const int32_t *, int32_t *, size_t, void *);
inline void run(Entry f, bool pair, const DeviceBuffer<int32_t> &xy, const DeviceBuffer<int32_t> *z, DeviceBuffer<int32_t> &out, void *stream)
{
    require(xy.len() % 2 == 0, "xy.len() is odd");
    const size_t n = xy.len() / 2;
    require(!z || z->len() == n, "z.len() != xy.len() / 2");
    require(out.len() == (pair ? 2 * n : n), pair ? "out.len() != xy.len()" : "out.len() != xy.len() / 2");
    check(f(xy.data(), z ? z->data() : nullptr, out.data(), n, stream));
}
}  // namespace detail
/// `cos_sin(x, y, z)` (src/cordic.rs:80-82)
inline void cos_sin(const DeviceBuffer<int32_t> &xy, const DeviceBuffer<int32_t> &z, DeviceBuffer<int32_t> &out, void *stream = nullptr)
{
    detail::run(idsp_cordic_cos_sin_i32, true, xy, &z, out, stream);
}
/// `cos_sin(x, y, 0)`
inline void cos_sin(const DeviceBuffer<int32_t> &xy, DeviceBuffer<int32_t> &out, void *stream = nullptr)
{
    detail::run(idsp_cordic_cos_sin_i32, true, xy, nullptr, out, stream);
}
/// `sqrt_atan2(x, y, z)` (src/cordic.rs:85-87)
inline void sqrt_atan2(const DeviceBuffer<int32_t> &xy, const DeviceBuffer<int32_t> &z, DeviceBuffer<int32_t> &out, void *stream = nullptr)
{
    detail::run(idsp_cordic_sqrt_atan2_i32, true, xy, &z, out, stream);
}
/// `sqrt_atan2(x, y, 0)`
inline void sqrt_atan2(const DeviceBuffer<int32_t> &xy, DeviceBuffer<int32_t> &out, void *stream = nullptr)
{
    detail::run(idsp_cordic_sqrt_atan2_i32, true, xy, nullptr, out, stream);
}
/// `mul(x, y, z)` (src/cordic.rs:90-92)
inline void mul(const DeviceBuffer<int32_t> &xy, const DeviceBuffer<int32_t> &z, DeviceBuffer<int32_t> &out, void *stream = nullptr)
{
    detail::run(idsp_cordic_mul_i32, false, xy, &z, out, stream);
}
/// `mul(x, y, 0)`
inline void mul(const DeviceBuffer<int32_t> &xy, DeviceBuffer<int32_t> &out, void *stream = nullptr)
{
    detail::run(idsp_cordic_mul_i32, false, xy, nullptr, out, stream);
}
/// `div(x, y, z)` (src/cordic.rs:95-97)
inline void div(const DeviceBuffer<int32_t> &xy, const DeviceBuffer<int32_t> &z, DeviceBuffer<int32_t> &out, void *stream = nullptr)
{
    detail::run(idsp_cordic_div_i32, false, xy, &z, out, stream);
}
/// `div(x, y, 0)`
inline void div(const DeviceBuffer<int32_t> &xy, DeviceBuffer<int32_t> &out, void *stream = nullptr)
{
    detail::run(idsp_cordic_div_i32, false, xy, nullptr, out, stream);
}
/// `cosh_sinh(x, y, z)` (src/cordic.rs:100-102)
inline void cosh_sinh(const DeviceBuffer<int32_t> &xy, const DeviceBuffer<int32_t> &z, DeviceBuffer<int32_t> &out, void *stream = nullptr)
{
    detail::run(idsp_cordic_cosh_sinh_i32, true, xy, &z, out, stream);
}
/// `cosh_sinh(x, y, 0)`
inline void cosh_sinh(const DeviceBuffer<int32_t> &xy, DeviceBuffer<int32_t> &out, void *stream = nullptr)
{
    detail::run(idsp_cordic_cosh_sinh_i32, true, xy, nullptr, out, stream);
}
/// `sqrt_atanh2(x, y, z)` (src/cordic.rs:105-107)
inline void sqrt_atanh2(const DeviceBuffer<int32_t> &xy, const DeviceBuffer<int32_t> &z, DeviceBuffer<int32_t> &out, void *stream = nullptr)
{
    detail::run(idsp_cordic_sqrt_atanh2_i32, true, xy, &z, out, stream);
}
/// `sqrt_atanh2(x, y, 0)`
inline void sqrt_atanh2(const DeviceBuffer<int32_t> &xy, DeviceBuffer<int32_t> &out, void *stream = nullptr)
{
    detail::run(idsp_cordic_sqrt_atanh2_i32, true, xy, nullptr, out, stream);
}
/// `CORDIC_CIRCULAR_GAIN`, `CORDIC_HYPERBOLIC_GAIN` (build.rs:80, :92-104)
inline double circular_gain() { return idsp_cordic_circular_gain(); }
inline double hyperbolic_gain() { return idsp_cordic_hyperbolic_gain(); }
}  // namespace cordic

/// `Lockin<[Lowpass<N>; K]>` fed by a per-lane `Accu<Wrapping<i32>>` (src/lockin.rs:30-39).
template <int N, int K>
class Lockin {
    static_assert(N == 1 || N == 2, "Lowpass order must be 1 or 2 (src/lowpass.rs:75)");
    static_assert(K >= 1 && K <= IDSP_LOCKIN_MAX_CASCADE, "1..4 cascaded lowpasses");

public:
    Lockin(const std::array<std::array<int32_t, N>, K> &k, const std::vector<int32_t> &accu_state,
           const std::vector<int32_t> &accu_step, void *stream = nullptr)
        : lanes_(accu_step.size()), stream_(stream)
    {
        require(accu_state.size() == lanes_, "one Accu per lane");
        cfg_.order = N, cfg_.cascade = K;
        for (int c = 0; c < K; c++)
            for (int j = 0; j < N; j++) cfg_.k[c][j] = k[c][j];
        std::vector<uint32_t> st(idsp_lockin_state_words(&cfg_) * lanes_, 0u);
        for (size_t l = 0; l < lanes_; l++) st[l] = uint32_t(accu_state[l]), st[lanes_ + l] = uint32_t(accu_step[l]);
        state_ = DeviceBuffer<uint32_t>(st);
    }
    DeviceBuffer<uint32_t> &state() { return state_; }
    /// x: real samples, y: `Complex<i32>` = [re, im] per sample
    template <class Layout>
    void process_view(View<int32_t, Layout> x, ViewMut<int32_t, Layout> y)
    {
        require(x.frames == y.frames && x.lanes == lanes_ && y.lanes == lanes_, "view shape mismatch");
        check(idsp_lockin_i32_process(&cfg_, state_.data(), x.flat, y.flat, lanes_, x.frames, Layout::value, stream_));
    }
    /// Same pass with `Complex::arg()` fused in (src/complex.rs:254-256): y = one i32 phase per sample
    template <class Layout>
    void process_view_arg(View<int32_t, Layout> x, ViewMut<int32_t, Layout> y)
    {
        require(x.frames == y.frames && x.lanes == lanes_ && y.lanes == lanes_, "view shape mismatch");
        check(idsp_lockin_i32_arg(&cfg_, state_.data(), x.flat, y.flat, lanes_, x.frames, Layout::value, stream_));
    }
    /// Same pass with `Complex::norm_sqr()` fused in (src/complex.rs:214-217): y = one i64 per sample
    template <class Layout>
    void process_view_norm_sqr(View<int32_t, Layout> x, ViewMut<int64_t, Layout> y)
    {
        require(x.frames == y.frames && x.lanes == lanes_ && y.lanes == lanes_, "view shape mismatch");
        check(idsp_lockin_i32_norm_sqr(&cfg_, state_.data(), x.flat, y.flat, lanes_, x.frames, Layout::value, stream_));
    }

private:
    idsp_lockin_i32 cfg_{};
    size_t lanes_;
    void *stream_;
    DeviceBuffer<uint32_t> state_;
};

// ------------------------------------------------------- exponential swept sine
/// `Sweep { rate, state }` (src/sweptsine.rs:12-119).  `fit` and the descriptors are host calls into the library (f32 / f64 with
/// the reference's order of operations); no GPU needed.
struct Sweep {
    int32_t rate = 0;
    int64_t state = 0;
    Sweep() = default;
    Sweep(int32_t rate_, int64_t state_) : rate(rate_), state(state_) {}
    /// `Sweep::fit(stop, harmonics, cycles)` (:108-118); `SweepError` -> Error(IDSP_EINVAL, "... Stop / Start out of bounds")
    static Sweep fit(float stop, float harmonics, float cycles)
    {
        Sweep s;
        check(idsp_sweep_fit(stop, harmonics, cycles, &s.rate, &s.state));
        return s;
    }
    double rate_f() const { return idsp_sweep_rate(rate); }                       ///< `rate()` (:43-45)
    double delay(double harmonic) const { return idsp_sweep_delay(rate, harmonic); }
    double octave() const { return idsp_sweep_octave(rate); }
    double decade() const { return idsp_sweep_decade(rate); }
    double cycles() const { return idsp_sweep_cycles(rate, state); }
    double state_f() const { return idsp_sweep_state(rate, state); }              ///< `state()` (:67-69)
    double continuous(double t) const { return idsp_sweep_continuous(rate, state, t); }
    std::array<float, 2> inverse_filter(float f) const                            ///< [re, im] (:93-101)
    {
        std::array<float, 2> out{};
        check(idsp_sweep_inverse_filter(rate, state, f, out.data()));
        return out;
    }
};

/// Per-lane `AccuOsc<Sweep>` (src/sweptsine.rs:160-188) with `Osc` for `W<i32>`.  A lane whose sweep has ended writes (0, 0).
class SweepOsc {
public:
    explicit SweepOsc(const std::vector<Sweep> &sweeps, void *stream = nullptr) : lanes_(sweeps.size()), stream_(stream)
    {
        std::vector<uint32_t> st(IDSP_SWEEP_STATE_WORDS * lanes_, 0u);  // accu = 0, emitted = 0
        for (size_t l = 0; l < lanes_; l++) {
            st[l] = uint32_t(uint64_t(sweeps[l].state)), st[lanes_ + l] = uint32_t(uint64_t(sweeps[l].state) >> 32);
            st[4 * lanes_ + l] = uint32_t(sweeps[l].rate);
        }
        state_ = DeviceBuffer<uint32_t>(st);
    }
    DeviceBuffer<uint32_t> &state() { return state_; }
    /// out: `Complex<i32>` = [re, im] per sample (build the view with width 2)
    template <class Layout>
    void generate(ViewMut<int32_t, Layout> out)
    {
        require(out.lanes == lanes_, "view shape mismatch");
        check(idsp_sweep_i32(state_.data(), out.flat, lanes_, out.frames, Layout::value, stream_));
    }
    /// samples each lane has produced (where a lane that ended stopped); synchronises
    std::vector<uint64_t> emitted() const
    {
        const std::vector<uint32_t> st = state_.to_host();
        std::vector<uint64_t> e(lanes_);
        for (size_t l = 0; l < lanes_; l++) e[l] = uint64_t(st[5 * lanes_ + l]) | (uint64_t(st[6 * lanes_ + l]) << 32);
        return e;
    }

private:
    size_t lanes_;
    void *stream_;
    DeviceBuffer<uint32_t> state_;
};

// ------------------------------------------------------- phase consumers
/// `Wrap` (src/unwrap.rs:15-27)
enum class Wrap : int8_t { Negative = -1, None = 0, Positive = 1 };

/// `overflowing_sub(y, x)` on i32 (src/unwrap.rs:73-80): the wrapped difference and the signum of the overflow.  Host arithmetic.
inline std::pair<int32_t, Wrap> overflowing_sub(int32_t y, int32_t x)
{
    const int32_t delta = int32_t(uint32_t(y) - uint32_t(x));
    return {delta, Wrap(int(delta >= 0) - int(y >= x))};
}

/// `saturating_scale(lo, hi, shift)` (src/unwrap.rs:90-101), 1 <= shift <= 32.  Host arithmetic.
inline int32_t saturating_scale(int32_t lo, int32_t hi, uint32_t shift)
{
    require(shift >= 1 && shift <= 32, "shift must be in 1..=32");
    const int64_t hi_range = -(int64_t(1) << (shift - 1)), min = std::numeric_limits<int32_t>::min();
    if (hi <= hi_range) return int32_t(min - hi_range);
    if (-int64_t(hi) <= hi_range) return int32_t(hi_range - min);
    return int32_t(uint32_t(int64_t(lo) >> shift) + uint32_t(uint64_t(int64_t(hi)) << (32 - shift)));
}

// ------------------------------------------------------ polyphase channelizer
/// `PolyphaseBank` (examples/polyphase_channelizer.rs:52-75), followed by `Dft4` (:77-101) when `dft` (the `.minor()` tuple of
/// :107-109), over `lanes` independent streams, each with its own `BankState` (zero words = `Default`).  The element of both
/// views is a `Frame` = `[[f32; 2]; 4]`: build them with width 8.
class PolyphaseBank {
public:
    /// `coeff[tap][m]` = `prototype[tap*4 + m]` (`bytemuck::cast`, :104), 1..16 taps
    PolyphaseBank(const std::vector<std::array<float, 4>> &coeff, bool dft, size_t lanes, void *stream = nullptr)
        : lanes_(lanes), stream_(stream)
    {
        require(!coeff.empty() && coeff.size() <= IDSP_PFB_MAX_TAPS, "1..16 taps");
        cfg_.taps = int32_t(coeff.size()), cfg_.dft = dft ? 1 : 0;
        for (size_t t = 0; t < coeff.size(); t++)
            for (size_t m = 0; m < 4; m++) cfg_.coeff[t][m] = coeff[t][m];
        state_ = DeviceBuffer<uint32_t>(idsp_pfb_state_words(&cfg_) * lanes);
    }
    /// the reference's own bank: `prototype()` (:33-44) for 4 * taps coefficients
    static PolyphaseBank prototype(int taps, bool dft, size_t lanes, void *stream = nullptr)
    {
        idsp_pfb_f32 c{};
        check(idsp_pfb_prototype_f32(taps, &c));
        std::vector<std::array<float, 4>> coeff(size_t(c.taps));
        for (size_t t = 0; t < coeff.size(); t++)
            for (size_t m = 0; m < 4; m++) coeff[t][m] = c.coeff[t][m];
        return PolyphaseBank(coeff, dft, lanes, stream);
    }
    const idsp_pfb_f32 &config() const { return cfg_; }
    DeviceBuffer<uint32_t> &state() { return state_; }
    /// y may be x (`Inplace`)
    template <class Layout>
    void process_view(View<float, Layout> x, ViewMut<float, Layout> y)
    {
        require(x.frames == y.frames && x.lanes == lanes_ && y.lanes == lanes_, "view shape mismatch");
        check(idsp_pfb_f32_process(&cfg_, state_.data(), x.flat, y.flat, lanes_, x.frames, Layout::value, stream_));
    }
    template <class Layout>
    void inplace_view(ViewMut<float, Layout> xy)
    {
        process_view(View<float, Layout>{xy.flat, xy.frames, xy.lanes}, xy);
    }

private:
    idsp_pfb_f32 cfg_{};
    size_t lanes_;
    void *stream_;
    DeviceBuffer<uint32_t> state_;
};

class PLLLanes;
/// `PLL { ba: [Q32<32>; 3] }` (src/pll.rs:33-58); the builders run in f32 inside the library, in the reference's order.
struct PLL {
    std::array<int32_t, 3> ba{};
    static PLL from_zpk(float zero, float pole, float gain)
    {
        PLL p;
        check(idsp_pll_from_zpk(zero, pole, gain, p.ba.data()));
        return p;
    }
    static PLL from_bandwidth(float bw, float split)
    {
        PLL p;
        check(idsp_pll_from_bandwidth(bw, split, p.ba.data()));
        return p;
    }
    inline PLLLanes lanes(size_t n, void *stream = nullptr) const;
};

/// `Split<Lanes<PLL>, [PLLState; n]>` (src/pll.rs:60-107): zero state = `PLLState::default()`.
class PLLLanes {
public:
    PLLLanes(const PLL &pll, size_t lanes, void *stream = nullptr)
        : pll_(pll), lanes_(lanes), stream_(stream), state_(idsp_pll_state_words() * lanes)
    {
    }
    DeviceBuffer<uint32_t> &state() { return state_; }
    /// y = `process(x)`, the output phase (src/pll.rs:106); y may be x
    template <class Layout>
    void process_view(View<int32_t, Layout> x, ViewMut<int32_t, Layout> y)
    {
        run(x, y, IDSP_PLL_PHASE);
    }
    /// y = `state.frequency()` after each sample (src/pll.rs:84-86); y may be x
    template <class Layout>
    void process_view_frequency(View<int32_t, Layout> x, ViewMut<int32_t, Layout> y)
    {
        run(x, y, IDSP_PLL_FREQUENCY);
    }
    /// y = `{phase, frequency}` pairs: build the view with width 2
    template <class Layout>
    void process_view_both(View<int32_t, Layout> x, ViewMut<int32_t, Layout> y)
    {
        run(x, y, IDSP_PLL_BOTH);
    }
    /// `PLLState::phase()` / `PLLState::frequency()` of every lane (src/pll.rs:79-86)
    std::vector<int32_t> phase() const { return word(8); }
    std::vector<int32_t> frequency() const { return word(7); }

private:
    template <class Layout>
    void run(View<int32_t, Layout> x, ViewMut<int32_t, Layout> y, int output)
    {
        require(x.frames == y.frames && x.lanes == lanes_ && y.lanes == lanes_, "view shape mismatch");
        check(idsp_pll_i32(pll_.ba.data(), state_.data(), x.flat, y.flat, lanes_, x.frames, Layout::value, output, stream_));
    }
    std::vector<int32_t> word(size_t w) const
    {
        check(idsp_stream_sync(stream_));
        const std::vector<uint32_t> st = state_.to_host();
        std::vector<int32_t> out(lanes_);
        for (size_t l = 0; l < lanes_; l++) out[l] = int32_t(st[w * lanes_ + l]);
        return out;
    }
    PLL pll_;
    size_t lanes_;
    void *stream_;
    DeviceBuffer<uint32_t> state_;
};
inline PLLLanes PLL::lanes(size_t n, void *stream) const { return PLLLanes(*this, n, stream); }

/// `Unwrapper<i64>` fed i32, one per lane (src/unwrap.rs:109-156).
class Unwrapper {
public:
    explicit Unwrapper(size_t lanes, void *stream = nullptr) : lanes_(lanes), stream_(stream), state_(2 * lanes) {}
    DeviceBuffer<uint32_t> &state() { return state_; }
    /// dx = `process(x)`, the wrapped difference to the previous sample; dx may be x
    template <class Layout>
    void process_view(View<int32_t, Layout> x, ViewMut<int32_t, Layout> dx)
    {
        require(x.frames == dx.frames && x.lanes == lanes_ && dx.lanes == lanes_, "view shape mismatch");
        check(idsp_unwrap_i32(state_.data(), x.flat, dx.flat, lanes_, x.frames, Layout::value, stream_));
    }
    /// y = `phase::<i64>()` after each sample
    template <class Layout>
    void process_view_phase(View<int32_t, Layout> x, ViewMut<int64_t, Layout> y)
    {
        require(x.frames == y.frames && x.lanes == lanes_ && y.lanes == lanes_, "view shape mismatch");
        check(idsp_unwrap_i32_phase(state_.data(), x.flat, y.flat, lanes_, x.frames, Layout::value, stream_));
    }
    /// `phase::<i64>()` of every lane (src/unwrap.rs:130-136)
    std::vector<int64_t> phase() const
    {
        check(idsp_stream_sync(stream_));
        const std::vector<uint32_t> st = state_.to_host();
        std::vector<int64_t> y(lanes_);
        for (size_t l = 0; l < lanes_; l++) y[l] = int64_t(uint64_t(st[l]) | (uint64_t(st[lanes_ + l]) << 32));
        return y;
    }
    /// `wraps::<i32, S>()` of every lane (src/unwrap.rs:119-127), 1 <= shift <= 63
    std::vector<int32_t> wraps(uint32_t shift) const
    {
        require(shift >= 1 && shift <= 63, "shift must be in 1..=63");
        const std::vector<int64_t> y = phase();
        std::vector<int32_t> w(lanes_);
        for (size_t l = 0; l < lanes_; l++) w[l] = int32_t(uint32_t(y[l] >> shift) + (uint32_t(y[l] >> (shift - 1)) & 1u));
        return w;
    }

private:
    size_t lanes_;
    void *stream_;
    DeviceBuffer<uint32_t> state_;
};

/// `ClampWrap<W<i32>>`, one per lane (src/unwrap.rs:166-194).
class ClampWrap {
public:
    explicit ClampWrap(size_t lanes, void *stream = nullptr) : lanes_(lanes), stream_(stream), state_(2 * lanes) {}
    DeviceBuffer<uint32_t> &state() { return state_; }
    template <class Layout>
    void process_view(View<int32_t, Layout> x, ViewMut<int32_t, Layout> y)  // y may be x
    {
        require(x.frames == y.frames && x.lanes == lanes_ && y.lanes == lanes_, "view shape mismatch");
        check(idsp_clamp_wrap_i32(state_.data(), x.flat, y.flat, lanes_, x.frames, Layout::value, stream_));
    }

private:
    size_t lanes_;
    void *stream_;
    DeviceBuffer<uint32_t> state_;
};

// ------------------------------------------------------- reciprocal PLL
class RPLLLanes;
/// `RPLLConfig { dt2, shift_frequency, shift_phase }` (src/rpll.rs:23-36), validated as idsp_rpll_i32 validates it: the ranges in
/// which every shift of `process` (:58-74) is defined (shift_frequency == dt2 would be `1u32 << 32` at :64).
struct RPLLConfig {
    int32_t dt2, shift_frequency, shift_phase;
    RPLLConfig(int32_t dt2_, int32_t shift_frequency_, int32_t shift_phase_) : dt2(dt2_), shift_frequency(shift_frequency_), shift_phase(shift_phase_)
    {
        require(dt2 >= 0 && dt2 <= 30, "dt2 must be in 0..=30");
        require(shift_frequency > dt2 && shift_frequency <= 32, "shift_frequency must be in dt2 + 1..=32");
        require(shift_phase >= dt2 && shift_phase <= dt2 + 31, "shift_phase must be in dt2..=dt2 + 31");
    }
    inline RPLLLanes lanes(size_t n, void *stream = nullptr) const;
};

/// `RPLLConfig::process` per lane (src/rpll.rs:47-77): zero state = `RPLL::default()`.
class RPLLLanes {
public:
    RPLLLanes(const RPLLConfig &cfg, size_t lanes, void *stream = nullptr)
        : cfg_{cfg.dt2, cfg.shift_frequency, cfg.shift_phase}, lanes_(lanes), stream_(stream), state_(idsp_rpll_state_words() * lanes)
    {
    }
    DeviceBuffer<uint32_t> &state() { return state_; }
    /// ts: `Option<W<i32>>` = {some, x} per sample, accu: the returned `Accu` = {state, step} (build both views with width 2); separate buffers
    template <class Layout>
    void process_view(View<int32_t, Layout> ts, ViewMut<int32_t, Layout> accu)
    {
        require(ts.frames == accu.frames && ts.lanes == lanes_ && accu.lanes == lanes_, "view shape mismatch");
        check(idsp_rpll_i32(&cfg_, state_.data(), ts.flat, accu.flat, lanes_, ts.frames, Layout::value, stream_));
    }
    /// `RPLL::phase()` / `RPLL::frequency()` of every lane (src/rpll.rs:80-90); synchronises
    std::vector<int32_t> phase() const
    {
        const std::vector<uint32_t> w = word(3);
        return std::vector<int32_t>(w.begin(), w.end());
    }
    std::vector<uint32_t> frequency() const { return word(2); }

private:
    std::vector<uint32_t> word(size_t w) const
    {
        if (lanes_) check(idsp_stream_sync(stream_));  // no lanes: nothing was launched, and no device is needed
        const std::vector<uint32_t> st = state_.to_host();
        return std::vector<uint32_t>(st.begin() + w * lanes_, st.begin() + (w + 1) * lanes_);
    }
    idsp_rpll cfg_;
    size_t lanes_;
    void *stream_;
    DeviceBuffer<uint32_t> state_;
};
inline RPLLLanes RPLLConfig::lanes(size_t n, void *stream) const { return RPLLLanes(*this, n, stream); }

/// The LO of a batch from the `Accu`s an RPLL returned (idsp_accu_lo_i32): `Accu::new(state, step >> batch_log2) * harmonic +
/// Accu::new(offset, 0)` iterated by `next()` into `Complex::from_angle`.  accu: `updates` rows of {state, step}, lo:
/// `updates << batch_log2` rows of [re, im] (both views with width 2) — the `lo` of LockinLo.
struct AccuLo {
    int32_t batch_log2, harmonic, offset;
    explicit AccuLo(int32_t batch_log2_, int32_t harmonic_ = 1, int32_t offset_ = 0) : batch_log2(batch_log2_), harmonic(harmonic_), offset(offset_)
    {
        require(batch_log2 >= 0 && batch_log2 <= 24, "batch_log2 must be in 0..=24");
    }
    template <class Layout>
    void process_view(View<int32_t, Layout> accu, ViewMut<int32_t, Layout> lo, void *stream = nullptr) const
    {
        require(lo.lanes == accu.lanes && lo.frames == accu.frames << batch_log2, "view shape mismatch");
        const idsp_accu_lo cfg{batch_log2, harmonic, offset};
        check(idsp_accu_lo_i32(&cfg, accu.flat, lo.flat, accu.lanes, accu.frames, Layout::value, stream));
    }
    /// `process_view` followed by the external-LO lock-in with `[Lowpass<N>; K]` arms (idsp_lockin_i32_lo_process) in one kernel,
    /// the LO never stored (idsp_lockin_i32_accu_process).  arms: order, cascade and gains; state: the two arms,
    /// `idsp_lockin_state_words(&arms) - 2` words per lane, shared with idsp_lockin_i32_lo_process; x: `updates << batch_log2`
    /// samples per lane; y: [re, im] per sample (accu and y with width 2).
    template <class Layout>
    void lockin_view(const idsp_lockin_i32 &arms, DeviceBuffer<uint32_t> &state, View<int32_t, Layout> x, View<int32_t, Layout> accu,
                     ViewMut<int32_t, Layout> y, void *stream = nullptr) const
    {
        require(x.lanes == accu.lanes && y.lanes == accu.lanes && x.frames == accu.frames << batch_log2 && y.frames == x.frames, "view shape mismatch");
        require(idsp_lockin_state_words(&arms) >= 2 && state.len() == (idsp_lockin_state_words(&arms) - 2) * accu.lanes, "state: the two arms per lane");
        const idsp_accu_lo cfg{batch_log2, harmonic, offset};
        check(idsp_lockin_i32_accu_process(&arms, &cfg, state.data(), x.flat, accu.flat, y.flat, accu.lanes, accu.frames, Layout::value, stream));
    }
};

// ------------------------------------------------ delta-sigma modulator
class DsmLanes;
/// `Dsm<K>` (src/dsm.rs:22-26), the MASH-(1)^K delta-sigma modulator with a runtime `order` = K in 0..=IDSP_DSM_MAX_ORDER.
struct Dsm {
    int order;
    explicit Dsm(int order_) : order(order_) { require(order >= 0 && order <= IDSP_DSM_MAX_ORDER, "order must be in 0..=8"); }
    inline DsmLanes lanes(size_t n, void *stream = nullptr) const;
};

/// `Dsm::<K>::process` per lane (src/dsm.rs:44-57, release-build wrapping; idsp_dsm_u32): u32 in, i8 out, one byte per sample.
/// Zero state = `Dsm::default()`; state words 0..K-1 are `a`, K..2K-1 are `c`.  No in-place form: x and y differ in element size.
class DsmLanes {
public:
    DsmLanes(const Dsm &dsm, size_t lanes, void *stream = nullptr)
        : order_(dsm.order), lanes_(lanes), stream_(stream), state_(idsp_dsm_state_words(dsm.order) * lanes)
    {
    }
    DeviceBuffer<uint32_t> &state() { return state_; }
    int order() const { return order_; }
    /// back to `Dsm::default()` in every lane
    void reset()
    {
        if (state_.len()) check(idsp_device_memset(state_.data(), 0, state_.len() * sizeof(uint32_t), stream_));
    }
    /// x_pitch / y_pitch: elements between the starts of consecutive rows of x / y (frames in FrameMajor, lanes in LaneMajor), 0 =
    /// dense; a view of pitched rows is built by hand (`View{ptr, frames, lanes}`), `from_flat` describes dense ones.  y may start at
    /// any byte; LaneMajor rows of y aligned to 4 bytes (y and y_pitch multiples of 4) are the fast case.
    template <class Layout>
    void process_view(View<uint32_t, Layout> x, ViewMut<int8_t, Layout> y, size_t x_pitch = 0, size_t y_pitch = 0)
    {
        require(x.frames == y.frames && x.lanes == lanes_ && y.lanes == lanes_, "view shape mismatch");
        const size_t row = Layout::value == IDSP_LANE_MAJOR ? x.frames : lanes_;
        require((!x_pitch || x_pitch >= row) && (!y_pitch || y_pitch >= row), "pitch shorter than a row");
        if (lanes_ == 0 || x.frames == 0) return;
        check(idsp_dsm_u32(order_, state_.data(), x.flat, x_pitch, y.flat, y_pitch, lanes_, x.frames, Layout::value, stream_));
    }
    /// `Process::block` over `&[[u32; N]]`: FrameMajor
    void block(View<uint32_t, FrameMajor> x, ViewMut<int8_t, FrameMajor> y, size_t x_pitch = 0, size_t y_pitch = 0) { process_view(x, y, x_pitch, y_pitch); }

private:
    int order_;
    size_t lanes_;
    void *stream_;
    DeviceBuffer<uint32_t> state_;
};
inline DsmLanes Dsm::lanes(size_t n, void *stream) const { return DsmLanes(*this, n, stream); }

// ------------------------------------------------ 16-bit fixed-point biquad
/// `Biquad<Q16<F>>` from `[[b0,b1,b2],[a0,a1,a2]]` (src/iir/biquad.rs:545-566, idsp_biquad_i16_from_sos)
inline idsp_biquad_i16 biquad_i16_from_sos(const double (&sos)[6], int frac)
{
    idsp_biquad_i16 out{};
    check(idsp_biquad_i16_from_sos(sos, frac, &out));
    return out;
}

/// `Biquad<Q16<F>>` (Cfg = idsp_biquad_i16) or `BiquadClamp<Q16<F>, i16>` (Cfg = idsp_biquad_clamp_i16) x `DirectForm1<i16>` per lane
/// (src/iir/biquad.rs:366-404, release-build wrapping; idsp_biquad_i16_df1 / _df1_clamp): i16 rows in and out, `sections` in series.
/// Zero state = `Default::default()`; state words {x0, x1, y0, y1} per section, each read as its low half.
template <class Cfg>
class BiquadI16Lanes {
    static_assert(std::is_same<Cfg, idsp_biquad_i16>::value || std::is_same<Cfg, idsp_biquad_clamp_i16>::value, "Cfg: idsp_biquad_i16 or idsp_biquad_clamp_i16");

public:
    BiquadI16Lanes(std::vector<Cfg> sections, size_t lanes, void *stream = nullptr)
        : cfg_(std::move(sections)), lanes_(lanes), stream_(stream), state_(idsp_biquad_i16_state_words(checked(cfg_)) * lanes)
    {
    }
    DeviceBuffer<uint32_t> &state() { return state_; }
    size_t sections() const { return cfg_.size(); }
    /// back to `Default::default()` in every lane
    void reset()
    {
        if (state_.len()) check(idsp_device_memset(state_.data(), 0, state_.len() * sizeof(uint32_t), stream_));
    }
    /// x_pitch / y_pitch: elements between the starts of consecutive rows of x / y (frames in FrameMajor, lanes in LaneMajor), 0 =
    /// dense; a view of pitched rows is built by hand (`View{ptr, frames, lanes}`).  x and y may start at any 2-byte-aligned address;
    /// LaneMajor rows on the 4-byte grid are the fast case.  y.flat == x.flat with one pitch is in place.
    template <class Layout>
    void process_view(View<int16_t, Layout> x, ViewMut<int16_t, Layout> y, size_t x_pitch = 0, size_t y_pitch = 0)
    {
        require(x.frames == y.frames && x.lanes == lanes_ && y.lanes == lanes_, "view shape mismatch");
        const size_t row = Layout::value == IDSP_LANE_MAJOR ? x.frames : lanes_;
        require((!x_pitch || x_pitch >= row) && (!y_pitch || y_pitch >= row), "pitch shorter than a row");
        if (lanes_ == 0 || x.frames == 0) return;
        if constexpr (std::is_same<Cfg, idsp_biquad_i16>::value)
            check(idsp_biquad_i16_df1(cfg_.data(), cfg_.size(), state_.data(), x.flat, x_pitch, y.flat, y_pitch, lanes_, x.frames, Layout::value, stream_));
        else
            check(idsp_biquad_i16_df1_clamp(cfg_.data(), cfg_.size(), state_.data(), x.flat, x_pitch, y.flat, y_pitch, lanes_, x.frames, Layout::value, stream_));
    }
    /// `Process::block` over `&[[i16; N]]`: FrameMajor
    void block(View<int16_t, FrameMajor> x, ViewMut<int16_t, FrameMajor> y, size_t x_pitch = 0, size_t y_pitch = 0) { process_view(x, y, x_pitch, y_pitch); }
    /// `Inplace::inplace` / `ViewInplace::inplace_view` (biquad.rs:540-541)
    template <class Layout>
    void inplace_view(ViewMut<int16_t, Layout> xy, size_t pitch = 0)
    {
        process_view(View<int16_t, Layout>{xy.flat, xy.frames, xy.lanes}, xy, pitch, pitch);
    }

private:
    static size_t checked(const std::vector<Cfg> &c)
    {
        require(c.size() <= IDSP_MAX_SECTIONS, "at most IDSP_MAX_SECTIONS sections");
        for (const Cfg &s : c) require(s.frac >= 0 && s.frac <= 31, "frac must be in 0..=31");
        return c.size();
    }
    std::vector<Cfg> cfg_;
    size_t lanes_;
    void *stream_;
    DeviceBuffer<uint32_t> state_;
};

/// `Split<ByLane<[C; lanes]>, [S; lanes]>` (dsp-process/src/compose.rs:363-390) with C = `Biquad<Q16<F>>` (Cfg = idsp_biquad_i16) or
/// `BiquadClamp<Q16<F>, i16>` (Cfg = idsp_biquad_clamp_i16) and S = `DirectForm1<i16>`: lane i is filtered by configuration i on
/// state i (idsp_biquad_i16_df1_bylane / _df1_clamp_bylane).  `configs[i]` is the serial slice of sections of lane i; every lane has
/// the same number of sections and every section the same frac (the one F of the bank).  The coefficients are kept on the GPU as
/// lane-contiguous i16 planes.
template <class Cfg>
class BiquadI16ByLane {
    static_assert(std::is_same<Cfg, idsp_biquad_i16>::value || std::is_same<Cfg, idsp_biquad_clamp_i16>::value, "Cfg: idsp_biquad_i16 or idsp_biquad_clamp_i16");

public:
    static constexpr size_t cv = std::is_same<Cfg, idsp_biquad_i16>::value ? 5 : 8;  ///< values per section and lane
    /// the planes of `configs` on the host, value v of section k of lane l at [(k * cv + v) * lanes + l]; checks what the class requires
    static std::vector<int16_t> planes(const std::vector<std::vector<Cfg>> &configs)
    {
        const size_t lanes = configs.size(), n = lanes ? configs[0].size() : 0;
        require(lanes && n, "BiquadI16ByLane needs at least one lane and one section");
        require(n <= IDSP_MAX_SECTIONS, "at most IDSP_MAX_SECTIONS sections");
        const int frac = configs[0][0].frac;
        require(frac >= 0 && frac <= 31, "frac must be in 0..=31");
        std::vector<int16_t> host(n * cv * lanes);
        for (size_t l = 0; l < lanes; l++) {
            require(configs[l].size() == n, "every lane needs the same number of sections");
            for (size_t k = 0; k < n; k++) {
                const Cfg &c = configs[l][k];
                require(c.frac == frac, "all lanes and sections of a bank share one frac");
                for (size_t v = 0; v < 5; v++) host[(k * cv + v) * lanes + l] = c.ba[v];
                if constexpr (cv == 8) {
                    host[(k * cv + 5) * lanes + l] = c.u;
                    host[(k * cv + 6) * lanes + l] = c.min;
                    host[(k * cv + 7) * lanes + l] = c.max;
                }
            }
        }
        return host;
    }
    explicit BiquadI16ByLane(const std::vector<std::vector<Cfg>> &configs, void *stream = nullptr)
        : host_(planes(configs)), lanes_(configs.size()), sections_(configs[0].size()), frac_(configs[0][0].frac), stream_(stream),
          state_(idsp_biquad_i16_state_words(sections_) * lanes_), coef_(host_)
    {
    }
    size_t lanes() const { return lanes_; }
    size_t sections() const { return sections_; }
    int frac() const { return frac_; }
    DeviceBuffer<uint32_t> &state() { return state_; }
    DeviceBuffer<int16_t> &coefficients() { return coef_; }
    /// back to `Default::default()` in every lane
    void reset() { check(idsp_device_memset(state_.data(), 0, state_.len() * sizeof(uint32_t), stream_)); }
    /// replace the configuration of one lane; its state is kept (assigning `by_lane.0[lane]`)
    void set_lane(size_t lane, const std::vector<Cfg> &config)
    {
        require(lane < lanes_, "lane out of range");
        require(config.size() == sections_, "every lane needs the same number of sections");
        for (const Cfg &c : config) require(c.frac == frac_, "all lanes and sections of a bank share one frac");
        const std::vector<int16_t> one = planes({config});
        for (size_t i = 0; i < sections_ * cv; i++) host_[i * lanes_ + lane] = one[i];
        coef_.upload(host_);
    }
    /// pitches, alignment and in place: as `BiquadI16Lanes::process_view`
    template <class Layout>
    void process_view(View<int16_t, Layout> x, ViewMut<int16_t, Layout> y, size_t x_pitch = 0, size_t y_pitch = 0)
    {
        require(x.frames == y.frames && x.lanes == lanes_ && y.lanes == lanes_, "view shape mismatch");
        const size_t row = Layout::value == IDSP_LANE_MAJOR ? x.frames : lanes_;
        require((!x_pitch || x_pitch >= row) && (!y_pitch || y_pitch >= row), "pitch shorter than a row");
        if (x.frames == 0) return;
        if constexpr (cv == 5)
            check(idsp_biquad_i16_df1_bylane(coef_.data(), frac_, sections_, state_.data(), x.flat, x_pitch, y.flat, y_pitch, lanes_, x.frames, Layout::value, stream_));
        else
            check(idsp_biquad_i16_df1_clamp_bylane(coef_.data(), frac_, sections_, state_.data(), x.flat, x_pitch, y.flat, y_pitch, lanes_, x.frames, Layout::value, stream_));
    }
    /// `Process::block` over `&[[i16; N]]`: FrameMajor
    void block(View<int16_t, FrameMajor> x, ViewMut<int16_t, FrameMajor> y, size_t x_pitch = 0, size_t y_pitch = 0) { process_view(x, y, x_pitch, y_pitch); }
    template <class Layout>
    void inplace_view(ViewMut<int16_t, Layout> xy, size_t pitch = 0)
    {
        process_view(View<int16_t, Layout>{xy.flat, xy.frames, xy.lanes}, xy, pitch, pitch);
    }

private:
    std::vector<int16_t> host_;  // the planes as uploaded: set_lane edits and uploads again
    size_t lanes_, sections_;
    int frac_;
    void *stream_;
    DeviceBuffer<uint32_t> state_;
    DeviceBuffer<int16_t> coef_;
};

/// sos[lanes][n][6] -> the host planes of a bank (idsp_biquad_i16_bank_from_sos); cv = 8 adds `BiquadClamp::default`'s u, min, max
inline std::vector<int16_t> biquad_i16_bank_from_sos(const std::vector<double> &sos, size_t lanes, size_t n, int frac, size_t cv = 5)
{
    require(sos.size() == lanes * n * 6, "sos is [lanes][n][6]");
    std::vector<int16_t> coef(n * (cv == 8 ? 8 : 5) * lanes);
    check(idsp_biquad_i16_bank_from_sos(sos.data(), lanes, n, frac, cv, coef.data()));
    return coef;
}

}  // namespace idsp_hip
