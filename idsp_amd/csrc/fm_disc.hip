// fm_disc.hip — the FM discriminator with deemphasis over many lanes (reference: examples/fm_disc.rs:25-50): its stream processor, the two
// role-wave kernels and idsp_fm_disc_i32.  All integer, bit-exact.  Which kernel a call takes: plan_fm_disc (readout_plan.h).
// (cossin(), atan2() and their tables: dds_dev.h; the elementwise entries and the DDS: dds.hip.)
#include "dds_dev.h"

namespace idsp {
namespace {

// FM discriminator + deemphasis (examples/fm_disc.rs:25-50).  In = Complex<Q32<32>> bits as a 2-vector.
typedef int32_t cplx_bits __attribute__((ext_vector_type(2)));

// The discriminator of one sample: z = x * conj(prev) (src/complex.rs:55-57), arg(z) - carrier (examples/fm_disc.rs:33-41); `tab`: the atan2
// reciprocal table.  `prev.replace(x)` of a `None` gives 0 instead (fm_disc.rs:33-35): the callers select, each where it knows.  Both role
// kernels call this; FmDiscProc::step keeps the same lines written out (see there).
__device__ __forceinline__ int32_t fm_disc_dev(cplx_bits x, cplx_bits prev, int32_t carrier, const uint32_t *tab)
{
    const int32_t cim = int32_t(0u - uint32_t(prev.y));
    const int64_t re = int64_t(uint64_t(int64_t(x.x) * prev.x) - uint64_t(int64_t(x.y) * cim));
    const int64_t im = int64_t(uint64_t(int64_t(x.x) * cim) + uint64_t(int64_t(x.y) * prev.x));
    return int32_t(uint32_t(atan2_dev(int32_t(im >> 32), int32_t(re >> 32), tab)) - uint32_t(carrier));
}

struct FmDiscProc {
    using In = cplx_bits;
    using Out = int32_t;
    static constexpr bool HAS_IN = true;
    static constexpr int LDS_WORDS = 32;  // atan2 reciprocal table
    static constexpr int IN_DIV = 1;
    static constexpr int COST = 130;
    struct Params {
        int32_t carrier;
        bq::SecI32 sec;
    };
    const uint32_t *tab;
    uint32_t has_prev;
    int32_t pre, pim;
    uint32_t s[4];
    static __device__ __forceinline__ void fill_shared(uint32_t *sh, int tid, int n)
    {
        for (int i = tid; i < 32; i += n) sh[i] = d_atan2_table[i];
    }
    __device__ __forceinline__ void set_shared(const uint32_t *sh) { tab = sh; }
    __device__ __forceinline__ void load(const Params &, const uint32_t *st, size_t lanes, size_t lane)
    {
        has_prev = st[lane];
        pre = int32_t(st[lanes + lane]);
        pim = int32_t(st[2 * lanes + lane]);
#pragma unroll
        for (int w = 0; w < 4; w++) s[w] = st[size_t(3 + w) * lanes + lane];
    }
    __device__ __forceinline__ void store(const Params &, uint32_t *st, size_t lanes, size_t lane)
    {
        st[lane] = has_prev;
        st[lanes + lane] = uint32_t(pre);
        st[2 * lanes + lane] = uint32_t(pim);
#pragma unroll
        for (int w = 0; w < 4; w++) st[size_t(3 + w) * lanes + lane] = s[w];
    }
    __device__ __forceinline__ Out step(const Params &p, In x)
    {
        int32_t d = 0;
        // `prev.replace(x)`: None -> 0 (fm_disc.rs:33-35)
        // (fm_disc_dev written out on the two scalars of the state: through the function, stream_frame_major<FmDiscProc, 24> comes out with the
        // two products of `re` in the other order and other registers — the same values, but not the same code as before the function existed)
        const int32_t cim = int32_t(0u - uint32_t(pim));  // conj (src/complex.rs:55-57)
        const int64_t re = int64_t(uint64_t(int64_t(x.x) * pre) - uint64_t(int64_t(x.y) * cim));
        const int64_t im = int64_t(uint64_t(int64_t(x.x) * cim) + uint64_t(int64_t(x.y) * pre));
        const int32_t a = atan2_dev(int32_t(im >> 32), int32_t(re >> 32), tab);
        d = has_prev ? int32_t(uint32_t(a) - uint32_t(p.carrier)) : 0;
        has_prev = 1u;
        pre = x.x, pim = x.y;
        return bq::Df1I32<false>::step(p.sec, s, d);
    }
};

// FM discriminator on role waves (round 3, FRAME_MAJOR).  One thread per lane is ~55 VALU instructions per sample on a single
// wave per SIMD at 65536 lanes (0.44 of the HBM peak, issue-bound) — but only the deemphasis biquad is a recurrence: the
// discriminator `arg(x[f] * conj(x[f-1])) - carrier` needs nothing but the previous INPUT sample, which is in the buffer (the
// state's `prev` only for frame 0).  So a workgroup of NF + 1 waves owns 64 lanes: front wave w computes the discriminator of
// frames [w FPW, (w + 1) FPW) of every tile of T = NF FPW frames (it loads those FPW rows plus the one before them) into an
// LDS tile, the last wave runs the biquad down the previous tile and stores y; one workgroup barrier per tile, tiles double
// buffered, whole tiles without per-frame predicates.  Five waves per SIMD instead of one, the same per-sample functions
// (fm_disc_dev — FmDiscProc::step's lines —, bq::Df1I32) in the same order: results are those of FmDiscProc bit for bit.
// (registers: left alone the compiler spends 245 VGPRs on hoisted loads and ONE workgroup fits a CU — 1.01 ms at the C2 shape,
// slower than the stream kernel; four workgroups per CU need <= 96)
#ifdef IDSP_FMD_ABL_NOSTORE  // tools/exp_lm_ablate.sh (UNIT=fm_disc): timing variants, conditions never true at run time
#define IDSP_FMD_ST_ON (frames == 1)
#else
#define IDSP_FMD_ST_ON true
#endif
#ifdef IDSP_FMD_ABL_NOLOAD
#define IDSP_FMD_LD_ON (frames == 1)
#else
#define IDSP_FMD_LD_ON true
#endif
#ifndef IDSP_FMD_WPE
#define IDSP_FMD_WPE 5
#endif
template <int NF>
__global__ __launch_bounds__(kWave *(NF + 1)) __attribute__((amdgpu_waves_per_eu(IDSP_FMD_WPE, IDSP_FMD_WPE))) void fm_disc_waves_kernel(const FmDiscProc::Params prm, uint32_t *st, const cplx_bits *x, int32_t *y,
                                                                        const size_t lanes, const size_t frames, const size_t xl, const size_t yl)
{
    constexpr int FPW = 8, T = NF * FPW;
    __shared__ int32_t tile[2][T][kWave];
    __shared__ uint32_t tab[32];
    const int wave = __builtin_amdgcn_readfirstlane(int(threadIdx.x) / kWave), lid = int(threadIdx.x) % kWave;
    if (threadIdx.x < 32) tab[threadIdx.x] = d_atan2_table[threadIdx.x];
    __syncthreads();
    const size_t lane = size_t(blockIdx.x) * kWave + lid;
    const bool active = lane < lanes;
    const size_t la = active ? lane : lanes - 1;  // idle threads of the last workgroup shadow a valid lane, stores masked
    const size_t nfull = frames / T;
    const int ntail = int(frames - nfull * T);
    if (wave < NF) {
        const cplx_bits *xp = x + la;
        const uint32_t has_prev0 = st[la];
        const cplx_bits prev0 = {int32_t(st[lanes + la]), int32_t(st[2 * lanes + la])};
        const int j0 = wave * FPW;  // first frame of this wave inside a tile
        cplx_bits cur[FPW + 1], nxt[FPW + 1];  // [0]: the frame before this wave's first
        auto fetch = [&](size_t k, cplx_bits(&dst)[FPW + 1], auto full) __attribute__((always_inline)) {
            const size_t f0 = k * T + j0;
#pragma unroll
            for (int j = 0; j <= FPW; j++) {
                if (j == 0 && f0 == 0) {
                    dst[0] = prev0;  // frame -1 is the state's `prev`
                } else if ((decltype(full)::value || j0 + j - 1 < ntail) && IDSP_FMD_LD_ON) {
                    dst[j] = nt_load<true>(xp + (f0 + j - 1) * xl);
                }
            }
        };
        if (nfull)
            fetch(0, cur, std::true_type{});
        else
            fetch(0, cur, std::false_type{});
        for (size_t k = 0; k < nfull; k++) {
            if (k + 1 < nfull)
                fetch(k + 1, nxt, std::true_type{});
            else if (ntail)
                fetch(k + 1, nxt, std::false_type{});
#pragma unroll
            for (int j = 0; j < FPW; j++) {
                int32_t d = fm_disc_dev(cur[j + 1], cur[j], prm.carrier, tab);
                if (j == 0 && k == 0 && wave == 0) d = has_prev0 ? d : 0;  // `prev` was None: 0 (fm_disc.rs:33-35)
                tile[k & 1][j0 + j][lid] = d;
            }
#pragma unroll
            for (int j = 0; j <= FPW; j++) cur[j] = nxt[j];
            lds_barrier();  // tile k complete; the biquad wave has finished tile k - 1
        }
        if (ntail) {
            for (int j = 0; j < FPW && j0 + j < ntail; j++) {
                int32_t d = fm_disc_dev(cur[j + 1], cur[j], prm.carrier, tab);
                if (j == 0 && nfull == 0 && wave == 0) d = has_prev0 ? d : 0;
                tile[nfull & 1][j0 + j][lid] = d;
            }
            lds_barrier();
        }
        lds_barrier();  // pairs with the biquad wave's last interval
        if (wave == 0 && active) {
            const cplx_bits last = xp[(frames - 1) * xl];
            st[lane] = 1u;
            st[lanes + lane] = uint32_t(last.x);
            st[2 * lanes + lane] = uint32_t(last.y);
        }
    } else {
        uint32_t s[4];
#pragma unroll
        for (int w = 0; w < 4; w++) s[w] = st[size_t(3 + w) * lanes + la];
        int32_t *yp = y + la;
        lds_barrier();  // tile 0
        for (size_t k = 0; k < nfull; k++) {
            int32_t v[T];
#pragma unroll
            for (int f = 0; f < T; f++) v[f] = tile[k & 1][f][lid];
#pragma unroll
            for (int f = 0; f < T; f++) {
                // (no `if (active)`: an idle thread of the last workgroup shadows lane `lanes - 1` — same input, same state, the
                // same value to the same address — and a predicate per store is a branch per sample in the ISA)
                const int32_t o = bq::Df1I32<false>::step(prm.sec, s, v[f]);
                if (IDSP_FMD_ST_ON) nt_store<true>(yp + (k * T + f) * yl, o);
            }
            lds_barrier();
        }
        if (ntail) {
            for (int f = 0; f < ntail; f++) {
                const int32_t o = bq::Df1I32<false>::step(prm.sec, s, tile[nfull & 1][f][lid]);
                if (active) nt_store<true>(yp + (nfull * T + f) * yl, o);
            }
            lds_barrier();
        }
        if (active) {
#pragma unroll
            for (int w = 0; w < 4; w++) st[size_t(3 + w) * lanes + lane] = s[w];
        }
    }
}


// FM discriminator on role waves, LANE_MAJOR (round 4).  Same roles as above — four front waves with eight frames of a 32-frame
// tile each, a fifth wave with the deemphasis biquad one tile behind — but every global access moves whole 128-byte lines, as in
// the LaneMajor lock-in (lockin_waves.h): the input tile (two lines of 16 `Complex<i32>` per lane) arrives by LDS-DMA one tile
// ahead, eight threads per line, pieces swizzled so that a thread's ds_read_b128 of its own row are conflict free; a front-wave
// thread reads its eight samples and the one before them from LDS (wave 0 carries the last sample of the tile before in a
// register), a barrier frees the slot and the requests of the next tile fly during the arithmetic (one slot: 34 KiB of LDS, four
// workgroups per CU — with two slots and one barrier per tile, 51 KiB and three: 0.98 ms); the discriminator values go into one ROW per lane (pitch 36 words), the biquad wave
// turns its row into outputs in place and the wave then re-reads the rows line-wise — eight threads per lane — and stores eight
// whole lines per instruction.  Two workgroup barriers per tile.  Whole tiles on 16-byte aligned rows; everything else stays on
// the tile kernel (stream_lane_major<FmDiscProc>), whose 64 different lines per access are what it is bound by (1.25 ms at
// 65536 lanes x 4096 frames; the FrameMajor role kernel with per-thread vectors on LaneMajor rows: 2.30 ms, round 3).
__global__ __launch_bounds__(kWave * 5) void fm_disc_waves_lm_kernel(const FmDiscProc::Params prm, uint32_t *st, const cplx_bits *x, int32_t *y,
                                                                     const size_t lanes, const size_t frames, const size_t pitch,
                                                                     const unsigned skew, const unsigned skew_shift, const unsigned skew_mod)
{
    constexpr int NF = 4, FPW = 8, T = NF * FPW, RS = T + 4;
    // start-up stagger (lockin_waves.h, "lanes in phase"): workgroup b waits ((b >> shift) % mod) * skew ticks of 10 ns
    if (const long long d = blockIdx.x < 1024 ? (long long)(skew) * ((blockIdx.x >> skew_shift) % skew_mod) : 0) {  // the first round only
        const long long t0 = wall_clock64();
        // (bounded: an s_sleep(8) is at least 0.2 us = 20 ticks, so d / 8 rounds are more than enough even if the counter stood still)
        for (long long spins = d / 8 + 16; spins > 0 && wall_clock64() - t0 < d; spins--) __builtin_amdgcn_s_sleep(8);
    }
    typedef int32_t i32x4 __attribute__((ext_vector_type(4)));
    __shared__ __attribute__((aligned(16))) int32_t tile[2][kWave * RS];
    __shared__ __attribute__((aligned(16))) uint32_t xs[2][kWave * 32];  // [line of the tile][64 rows x 128 bytes]: ONE slot, 34 KiB in all, four workgroups per CU
    __shared__ uint32_t tab[32];
    const int wave = __builtin_amdgcn_readfirstlane(int(threadIdx.x) / kWave), lid = int(threadIdx.x) % kWave;
    if (threadIdx.x < 32) tab[threadIdx.x] = d_atan2_table[threadIdx.x];
    const size_t lane = size_t(blockIdx.x) * kWave + lid;
    const bool active = lane < lanes;
    const size_t la = active ? lane : lanes - 1;  // idle threads of the last workgroup shadow a valid lane, stores masked
    const size_t ntiles = frames / T;             // launcher: whole tiles of rows `pitch` elements apart (the rest of a row: the tile kernel)
    if (wave < NF) {
        const uint32_t has_prev0 = st[la];
        cplx_bits carry = {int32_t(st[lanes + la]), int32_t(st[2 * lanes + la])};  // wave 0: the sample before the tile
        __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): the state has landed before the first DMA request is counted
        // instruction j = 4 wave + g of the 16 of a tile: line j / 8 of the tile, rows of lanes j % 8 + 8 (lid / 8), piece (lid % 8) ^ (j % 8)
        auto dma = [&](size_t k) {
            if (!IDSP_FMD_LD_ON) return;
#pragma unroll
            for (int g = 0; g < 4; g++) {
                const int j = 4 * wave + g, line = j >> 3, jj = j & 7;
                size_t gl = size_t(blockIdx.x) * kWave + size_t(jj + 8 * (lid / 8));
                gl = gl < lanes ? gl : lanes - 1;
                glds16(x + gl * pitch + k * T + size_t(line * 16 + ((lid % 8) ^ jj) * 2),
                       uint32_t(reinterpret_cast<uintptr_t>(&xs[line][jj * 256])));
            }
        };
        const uint32_t own = uint32_t((lid % 8) * 8 + lid / 8) * 128, sw = uint32_t(lid % 8);  // own row; piece p sits at 16 (p ^ sw)
        auto piece = [&](int line, int p) {
            return *reinterpret_cast<const i32x4 *>(reinterpret_cast<const char *>(&xs[line][0]) + own + ((uint32_t(p) ^ sw) * 16));
        };
        dma(0);
        wait_vmcnt<0>();
        lds_barrier();  // the table, tile 0
        const int line = wave >> 1, p0 = (wave & 1) * 4;
        for (size_t k = 0; k < ntiles; k++) {
            const int slot = int(k & 1);
            cplx_bits cur[FPW + 1];
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const i32x4 a = piece(line, p0 + q);
                cur[1 + 2 * q] = cplx_bits{a.x, a.y}, cur[2 + 2 * q] = cplx_bits{a.z, a.w};
            }
            if (wave == 0) {
                cur[0] = carry;
                const i32x4 a = piece(1, 7);  // frame 31 of this tile: the sample before the next one
                carry = cplx_bits{a.z, a.w};
            } else {
                const i32x4 a = wave == 2 ? piece(0, 7) : piece(line, p0 - 1);
                cur[0] = cplx_bits{a.z, a.w};
            }
            lds_barrier();  // every front wave holds its samples of tile k: the slot is free
            if (k + 1 < ntiles) dma(k + 1);
            int32_t d[FPW];
#pragma unroll
            for (int j = 0; j < FPW; j++) d[j] = fm_disc_dev(cur[j + 1], cur[j], prm.carrier, tab);
            if (k == 0 && wave == 0) d[0] = has_prev0 ? d[0] : 0;  // `prev` was None: 0 (fm_disc.rs:33-35)
            i32x4 *row = reinterpret_cast<i32x4 *>(&tile[slot][lid * RS + wave * FPW]);
            row[0] = i32x4{d[0], d[1], d[2], d[3]};
            row[1] = i32x4{d[4], d[5], d[6], d[7]};
            wait_vmcnt<0>();  // this wave's share of tile k + 1 has landed (it had the whole interval)
            lds_barrier();    // tile k complete, tile k + 1 in LDS; the biquad wave has finished tile k - 1
        }
        if (wave == 0 && active) {
            const cplx_bits last = x[lane * pitch + frames - 1];
            st[lane] = 1u;
            st[lanes + lane] = uint32_t(last.x);
            st[2 * lanes + lane] = uint32_t(last.y);
        }
    } else {
        uint32_t s[4];
#pragma unroll
        for (int w = 0; w < 4; w++) s[w] = st[size_t(3 + w) * lanes + la];
        lds_barrier();  // pairs with the front waves' first barrier
        for (size_t k = 0; k <= ntiles; k++) {
            if (k < ntiles) lds_barrier();  // the front waves' slot hand-over of interval k
            if (k == 0) {
                lds_barrier();  // tile 0 complete
                continue;
            }
            const size_t kt = k - 1;  // the tile this wave turns into outputs during interval k
            int32_t *rowp = &tile[kt & 1][lid * RS];
            int32_t v[T];
#pragma unroll
            for (int q = 0; q < T / 4; q++) {
                const i32x4 a = reinterpret_cast<const i32x4 *>(rowp)[q];
                v[4 * q] = a.x, v[4 * q + 1] = a.y, v[4 * q + 2] = a.z, v[4 * q + 3] = a.w;
            }
#pragma unroll
            for (int f = 0; f < T; f++) v[f] = bq::Df1I32<false>::step(prm.sec, s, v[f]);
#pragma unroll
            for (int q = 0; q < T / 4; q++) reinterpret_cast<i32x4 *>(rowp)[q] = i32x4{v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]};
            // line-wise: in instruction u thread t holds frames 4 (t % 8) .. of lane 8 u + t / 8 (LDS operations of one wave stay in order)
#pragma unroll
            for (int u = 0; u < 8; u++) {
                const int ll = u * 8 + lid / 8;
                const size_t gl = size_t(blockIdx.x) * kWave + size_t(ll);
                const i32x4 a = *reinterpret_cast<const i32x4 *>(&tile[kt & 1][ll * RS + (lid % 8) * 4]);
                if (gl < lanes && IDSP_FMD_ST_ON) __builtin_nontemporal_store(a, reinterpret_cast<i32x4 *>(y + gl * pitch + kt * T) + lid % 8);
            }
            if (k < ntiles) lds_barrier();  // tile k complete
        }
        if (active) {
#pragma unroll
            for (int w = 0; w < 4; w++) st[size_t(3 + w) * lanes + lane] = s[w];
        }
    }
}

}  // namespace
}  // namespace idsp

using namespace idsp;

extern "C" {

// plan_fm_disc (readout_plan.h) says which kernels, this runs them
int idsp_fm_disc_i32(const idsp_fm_disc *cfg, void *state, const int32_t *x, int32_t *y, size_t lanes, size_t frames,
                     int layout, void *stream)
{
    int rc = check_stream_args(cfg, 1, state, x, y, lanes, frames, layout);
    if (rc) return rc;
    if (cfg->deemph.frac < 0 || cfg->deemph.frac > 31) return fail(IDSP_EINVAL, "deemph frac = %d not in 0..31", cfg->deemph.frac);
    if (lanes == 0 || frames == 0) return IDSP_OK;
    FmDiscProc::Params p;
    p.carrier = cfg->carrier;
    bq::Fill{&cfg->deemph}(p.sec, 0);
    FmDiscCall call;
    call.lanes = lanes, call.frames = frames, call.layout = layout;
    call.x = reinterpret_cast<uintptr_t>(x), call.y = reinterpret_cast<uintptr_t>(y);
    call.tuned_device = layout == IDSP_LANE_MAJOR && stagger_tuned_device();  // read for the LaneMajor role kernel only
    const FmDiscPlan plan = plan_fm_disc(call, fm_disc_switches());
    const hipStream_t s = as_stream(stream);
    uint32_t *const st = static_cast<uint32_t *>(state);
    const cplx_bits *const xc = reinterpret_cast<const cplx_bits *>(x);
    switch (plan.form) {
        case FmDiscForm::WavesFm:
            note_kernel(fm_disc_plan_name(plan));
            if (plan.front_waves == 3)
                hipLaunchKernelGGL((fm_disc_waves_kernel<3>), dim3(plan.grid), dim3(kWave * 4), 0, s, p, st, xc, y, lanes, frames, lanes, lanes);
            else
                hipLaunchKernelGGL((fm_disc_waves_kernel<4>), dim3(plan.grid), dim3(kWave * 5), 0, s, p, st, xc, y, lanes, frames, lanes, lanes);
            return launch_status();
        case FmDiscForm::WavesLm:
        case FmDiscForm::WavesLmTail:
            // the whole tiles of every row at the call's row pitch; WavesLmTail: the tile kernel on the rest of each row behind it (same stream;
            // the state carries over as between two calls)
            note_kernel("fm_disc_waves_lm_kernel");
            hipLaunchKernelGGL(fm_disc_waves_lm_kernel, dim3(plan.grid), dim3(kWave * 5), 0, s, p, st, xc, y, lanes, plan.body, frames, plan.skew,
                               plan.skew_shift, plan.skew_mod);
            if ((rc = launch_status()) || plan.form == FmDiscForm::WavesLm) return rc;
            rc = launch_stream<FmDiscProc>(p, state, xc + plan.body, y + plan.body, lanes, plan.tail, layout, s, Pitch{frames, frames});
            if (rc == IDSP_OK) note_kernel(fm_disc_plan_name(plan));
            return rc;
        default: return launch_stream<FmDiscProc>(p, state, xc, y, lanes, frames, layout, s);
    }
}

}  // extern "C"
