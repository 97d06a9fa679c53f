"""Float kernels on the IEEE edge values: signed zeros, subnormals, huge values that overflow, inf and NaN.

`assert_same_float` is the comparison rule, `special_x` / `special_state` the generators (one kind of data per lane,
kind = lane % 8, so that a poisoned lane cannot hide the others and every 8-lane group, wave and tile holds every kind),
`classes` the census of a result, `POISON` a finite fill for GPU outputs.  The case tables below are one list for both
sides: tests/test_float_special_oracle.py runs them on the CPU (oracle against a per-sample numpy restatement, plus the
conditions every case must meet); a GPU module comparing HIP with the oracle takes the same tables, `prepare`, `invoke`,
`run_oracle` and `check_conditions`, and each case's `kernel` (the start of `idsp_last_kernel()` to assert).

Test infrastructure only."""
from __future__ import annotations

import ctypes as C
import types
import zlib

import numpy as np

from idsp_amd import _abi
from tests import _harness as H

FM, LM = H.FM, H.LM
F32, F64 = np.float32, np.float64
# Finite fill of GPU output buffers: a NaN fill would compare equal wherever the oracle's result is NaN, so an element the
# kernel never wrote could pass there.  `assert_poison_absent` makes "every element was written" hold at those positions too.
POISON = {F32: np.uint32(0x7F7FDEAD), F64: np.uint64(0x7FEFDEADBEEF5EED)}
NAN_CAP = 0.5  # at most this share of a case's outputs / float state words may be NaN, or the case checks too little


def _uint(dtype):
    return np.uint32 if np.dtype(dtype) == np.dtype(F32) else np.uint64


def bits(a):
    a = np.ascontiguousarray(a)
    assert a.dtype in (np.dtype(F32), np.dtype(F64)), a.dtype
    return a.view(_uint(a.dtype))


def assert_same_float(want, got, what, where=None):
    """float32 / float64 arrays are the same when their NaN masks are identical and every non-NaN element is bit-identical
    on the uint32 / uint64 view — so +0 and -0 differ, and subnormals count like any other value.

    NaN sign and payload are deliberately NOT compared: an invalid operation on x86 yields the negative default NaN
    (0xFFC00000) where the GPU yields a positive one, the rules for propagating an operand's payload differ between the
    two, and the reference language does not specify NaN bits.  The same rule holds for written-back float state words.
    `where(flat index) -> str` names the first differing element (lane, frame, kind of data) in the message."""
    want, got = np.ascontiguousarray(want), np.ascontiguousarray(got)
    assert want.dtype == got.dtype and want.shape == got.shape, (what, want.dtype, got.dtype, want.shape, got.shape)
    nw, ng = np.isnan(want), np.isnan(got)
    bad = (nw != ng) | (~nw & ~ng & (bits(want) != bits(got)))
    if bad.any():
        i = int(np.flatnonzero(bad.reshape(-1))[0])
        w, g = want.reshape(-1)[i], got.reshape(-1)[i]
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements differ; first at flat index {i}"
                             f"{' ' + where(i) if where else ''}: want {w!r} ({int(bits(want).reshape(-1)[i]):#x}), "
                             f"got {g!r} ({int(bits(got).reshape(-1)[i]):#x})")


def poison(n, dtype):
    """n elements of the finite poison pattern as a numpy array of `dtype`."""
    return np.full(int(n), POISON[np.dtype(dtype).type], dtype=_uint(dtype)).view(dtype)


def assert_poison_absent(y, what):
    """The expected result must not hold the poison pattern, or an unwritten element could equal it."""
    assert not (bits(y) == POISON[y.dtype.type]).any(), (what, "the oracle's output holds the poison pattern")


def _consts(dt):
    fi = np.finfo(dt)
    if dt == F32:
        return types.SimpleNamespace(huge=[3e38, -3e38, 1e30], scale=2e-38, mant=23, sub=[1e-41, -3e-42], fi=fi)
    return types.SimpleNamespace(huge=[1.7e308, -1.7e308, 1e300], scale=4e-308, mant=52, sub=[1e-310, -3e-320], fi=fi)


def _zeros(rng, shape, dt, zero):
    if zero is not None:
        return np.full(shape, zero, dt)
    return np.where(rng.integers(0, 2, size=shape) == 1, dt(-0.0), dt(0.0)).astype(dt)


def _subnormals(rng, shape, dt):
    c, u = _consts(dt), _uint(dt)
    mag = rng.integers(1, 1 << c.mant, size=shape, dtype=np.uint64)
    sign = rng.integers(0, 2, size=shape, dtype=np.uint64) << np.uint64(8 * np.dtype(dt).itemsize - 1)
    return (mag | sign).astype(u).view(dt)


def special_x(rng, frames, lanes, dtype, zero=None):
    """([frames, lanes] array, kind[lanes]); kind = lane % 8:
      0 standard normal (control)            4 standard normal, one +-inf at frame frames // 2
      1 random +0 / -0 (`zero`: all that)    5 standard normal, one NaN at frame frames // 2
      2 random subnormals of either sign     6 standard normal * 2e-38 (f64: 4e-308): products land in the subnormal range
      3 huge values (sums overflow)          7 standard normal, 10 % from {+-0, two subnormals, +-MAX, +-MIN}"""
    dt = np.dtype(dtype).type
    c = _consts(dt)
    kind = np.arange(lanes) % 8
    x = rng.standard_normal((frames, lanes)).astype(dt)
    col = [np.flatnonzero(kind == k) for k in range(8)]
    x[:, col[1]] = _zeros(rng, (frames, col[1].size), dt, zero)
    x[:, col[2]] = _subnormals(rng, (frames, col[2].size), dt)
    x[:, col[3]] = rng.choice(np.array(c.huge, dt), size=(frames, col[3].size))
    x[frames // 2, col[4]] = np.where(rng.integers(0, 2, size=col[4].size) == 1, dt(np.inf), dt(-np.inf))
    x[frames // 2, col[5]] = dt(np.nan)
    x[:, col[6]] = x[:, col[6]] * dt(c.scale)
    edge = np.array([0.0, -0.0, c.sub[0], c.sub[1], c.fi.max, -c.fi.max, c.fi.tiny, -c.fi.tiny], dt)
    pick = rng.random((frames, col[7].size)) < 0.1
    x[:, col[7]] = np.where(pick, rng.choice(edge, size=pick.shape), x[:, col[7]])
    return x, kind


def special_chunks(rng, frames, lanes, rate, dtype, zero=None):
    """[frames, lanes, rate] for the multi-rate entries, whose element is a lane's whole chunk of `rate` consecutive
    samples (include/idsp_hip.h: FRAME_MAJOR x[(f*lanes + l)*R + k]): lane l's stream of frames * rate samples is of
    kind l % 8 throughout."""
    x, kind = special_x(rng, frames * rate, lanes, dtype, zero)
    return np.ascontiguousarray(x.reshape(frames, rate, lanes).transpose(0, 2, 1)), kind


def state_words(v):
    """float values [values, lanes] -> uint32 state planes [words, lanes] (f64: value v -> words 2v low, 2v + 1 high)."""
    v = np.ascontiguousarray(v)
    if v.dtype == np.dtype(F32):
        return v.view(np.uint32).copy()
    u = v.view(np.uint64)
    st = np.empty((2 * v.shape[0], v.shape[1]), np.uint32)
    st[0::2] = (u & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    st[1::2] = (u >> np.uint64(32)).astype(np.uint32)
    return st


def state_values(st, dtype):
    """uint32 state planes [words, lanes] -> the float values they hold [values, lanes]."""
    st = np.ascontiguousarray(st)
    if np.dtype(dtype) == np.dtype(F32):
        return st.view(F32)
    return (st[0::2].astype(np.uint64) | (st[1::2].astype(np.uint64) << np.uint64(32))).view(F64)


def special_state(rng, words, lanes, kind, dtype, zero=None):
    """uint32 [words, lanes] of float state: standard normal; +-0 in kind-1 lanes (`zero`: all that), subnormals in
    kind-2 lanes, scaled by 2e-38 (f64: 4e-308) in kind-6 lanes."""
    dt = np.dtype(dtype).type
    values = words // (np.dtype(dt).itemsize // 4)
    v = rng.standard_normal((values, lanes)).astype(dt)
    l1, l2, l6 = (np.flatnonzero(kind == k) for k in (1, 2, 6))
    v[:, l1] = _zeros(rng, (values, l1.size), dt, zero)
    v[:, l2] = _subnormals(rng, (values, l2.size), dt)
    v[:, l6] = v[:, l6] * dt(_consts(dt).scale)
    return state_words(v)


def classes(y):
    """Census of a float array: NaN share and the counts of +-inf, -0, +0, subnormal and normal elements."""
    y = np.asarray(y)
    tiny = np.finfo(y.dtype).tiny
    mag = np.abs(y)
    zero = y == 0
    return {"nan": float(np.isnan(y).mean()) if y.size else 0.0, "inf": int(np.isinf(y).sum()),
            "-0": int((zero & np.signbit(y)).sum()), "+0": int((zero & ~np.signbit(y)).sum()),
            "subnormal": int(((mag > 0) & (mag < tiny)).sum()), "normal": int((np.isfinite(y) & (mag >= tiny)).sum())}


# ------------------------------------------------------------------------------------------------------------ cases
# Clamp rows (u, min, max): every u is NaN-free, one is -0.0.  `v < lo ? lo : (v > hi ? hi : v)` passes a NaN v through,
# returns -0 for v = -0 between bounds of +-0, and is the identity between -inf and +inf, for +-inf too.
CLAMPS = {"finite": (0.05, -0.7, 0.9), "open": (-0.0, -np.inf, np.inf), "zeros": (0.01, -0.0, 0.0), "pzero": (-0.0, 0.0, 0.0)}

# op -> (float values of state per section, extra values, form)
STREAM = {"biquad_{t}_df1": (4, 0, "df1"), "biquad_{t}_df1_clamp": (4, 0, "df1"), "biquad_{t}_df2t": (2, 0, "df2t"),
          "biquad_{t}_df2t_clamp": (2, 0, "df2t"), "cascade_{t}_df1": (2, 2, "cascade"), "normal_{t}_df1": (4, 0, "normal")}
TYPES = {"f32": F32, "f64": F64}


def _case(cid, call, op, dtype, layout, lanes, frames, **kw):
    c = types.SimpleNamespace(id=f"{cid}-{'FM' if layout == FM else 'LM'}-{lanes}x{frames}", call=call, op=op, dtype=dtype,
                              layout=layout, lanes=lanes, frames=frames, n=1, clamp=None, coef="random", rin=1, rout=1,
                              kernel=None, pitch=None, inplace=call in ("stream", "bylane"), cfg=None)
    c.__dict__.update(kw)
    return c


# Start of `idsp_last_kernel()` asserted per case.  FrameMajor, dense rows: the f32 single sections, `cascade` and `normal` at one
# section dispatch like i32 DF1 (4-byte samples, cheap, LDS-eligible), so their kernels are the rows of
# tests/test_gpu_dispatch_table.py::I32_FM; three f32 sections are not LDS-eligible and 8-byte samples never are (register-window
# kernel), but f64 takes the staged single-wave kernel below 49152 lanes (idsp_amd/csrc/lane_stream.h, dispatch_thresholds.h).
SWEEP = "stream_frame_major_sweep["
FEW = " + stream_frame_major_few (lanes % 4, second stream)"
# FrameMajor lane counts of tests/test_gpu_dispatch_table.py: (lanes, frames)
FM_BIG = [(65536, 64), (131072, 64), (65537, 64), (65552, 64), (24576, 96), (16384, 96), (8176, 257)]
FM_F32 = {
    65536: SWEEP + "1 block/workgroup]<", 131072: SWEEP + "2 blocks/workgroup]<", 65537: "stream_frame_major_lds[XCD-contiguous blocks]<",
    65552: "stream_frame_major_sweep + stream_frame_major_staged (remainder, second stream)<", 24576: SWEEP + "1 block/workgroup]<",
    16384: "stream_frame_major_staged[32 lanes/wave]<", 8176: "stream_frame_major_staged[16 lanes/wave]<",
}
FM_F64 = {24576: "stream_frame_major_staged[64 lanes/wave]<", 16384: "stream_frame_major_staged[32 lanes/wave]<",
          8176: "stream_frame_major_staged[16 lanes/wave]<"}


def _fm_kernel(dtype, n, lanes):
    if lanes < 8176:
        return "stream_frame_major"  # the small ragged shapes: the launcher family only
    if dtype == F32:
        return FM_F32[lanes] if n == 1 else "stream_frame_major<"
    return FM_F64.get(lanes, "stream_frame_major<")


def _lm_kernel(dtype, frames, pitch=None):
    """tests/test_gpu_lane_major_staged.py: the staged kernel on 16-byte rows of 128 bytes or more, else the 4-byte tile kernel."""
    size = np.dtype(dtype).itemsize
    if ((pitch or frames) * size) % 16 == 0 and frames * size >= 128:
        return "stream_lane_major_staged"
    return "stream_lane_major<"


LM_BIG = [(65536, 64), (32768, 64), (16384, 96)]


def _big(tn, form, n, ck):
    """Which stream configurations also run at the big FrameMajor lane counts: every f32 form and clamp row at one section,
    f32 DF1 at three; of f64 (the same templates on two-word samples) DF1 and the +-0-clamped DF2T."""
    if tn == "f32":
        return n == 1 or (form == "df1" and ck is None)
    return n == 1 and (form, ck) in (("df1", None), ("df2t", "zeros"))


def small_shapes():
    from tests.test_gpu_parity import SHAPES

    return list(SHAPES)


def lane_major_shapes():
    from tests.test_gpu_lane_major_staged import SHAPES

    return list(SHAPES)  # (lanes, frames, pitch)


def stream_cases():
    """biquad_{f32,f64}_{df1,df2t}[_clamp] at n = 1 and 3, cascade_*_df1, normal_*_df1: both layouts, the small ragged shapes,
    the FrameMajor lane counts of every kernel family and the LaneMajor staged-kernel shapes."""
    out = []
    small, lm = small_shapes(), lane_major_shapes()
    for tn, dt in TYPES.items():
        for pat, (vals, extra, form) in STREAM.items():
            op = pat.format(t=tn)
            clamps = list(CLAMPS) if op.endswith("_clamp") else [None]
            for ci, ck in enumerate(clamps):
                for n in (1, 3):
                    tag = f"{op}-n{n}" + (f"-{ck}" if ck else "")
                    kw = dict(n=n, clamp=ck, form=form, values=vals * n + extra)
                    for si, (lanes, frames) in enumerate(small):
                        if si % 2 != (n == 3) and ck not in (None, "finite"):
                            continue  # the +-0 / open clamp rows take every other small shape, alternating with n
                        for layout in (FM, LM):
                            k = "stream_frame_major" if layout == FM else _lm_kernel(dt, frames)
                            out.append(_case(tag, "stream", op, dt, layout, lanes, frames, kernel=k, **kw))
                    if ck in (None, "zeros") and (n == 1 or tn == "f32"):
                        for lanes, frames, _ in lm:
                            out.append(_case(tag, "stream", op, dt, LM, lanes, frames, kernel=_lm_kernel(dt, frames), **kw))
                    if not _big(tn, form, n, ck):
                        continue
                    for lanes, frames in FM_BIG:
                        if (ck in ("finite", "open", "pzero") and lanes not in (65536, 16384)) or (n == 3 and lanes not in (65536, 131072)):
                            continue  # the +-0 rows (and the unclamped forms) take every lane count
                        out.append(_case(tag, "stream", op, dt, FM, lanes, frames, kernel=_fm_kernel(dt, n, lanes), **kw))
                    if (tn, form, ck, n) == ("f32", "df2t", None, 1):  # from 512 frames up to 24576 lanes: the compute + mover pair kernel
                        out.append(_case(tag, "stream", op, dt, FM, 16384, 512, kernel="stream_frame_major_pair[", **kw))
                    if n == 1 and (form, ck) in ((("df1", None), ("df2t", "zeros")) if tn == "f32" else (("df1", None),)):
                        for lanes, frames in LM_BIG:
                            out.append(_case(tag, "stream", op, dt, LM, lanes, frames, kernel="stream_lane_major_staged", **kw))
            if op.endswith("_clamp"):
                continue
            # signed zeros: all five coefficients positive, kind-1 lanes of x and state all -0 -> -0 out, throughout
            for n in (1, 3):
                kw = dict(n=n, form=form, values=vals * n + extra, coef="positive")
                fm = [(65, 47), (4096, 50)] + ([(65536, 64)] if n == 1 else []) + ([(16384, 96)] if (tn, form, n) == ("f32", "df2t", 1) else [])
                for layout, shapes in ((FM, fm), (LM, [(65, 47), (1000, 513)])):
                    for lanes, frames in shapes:
                        k = _fm_kernel(dt, n, lanes) if layout == FM else _lm_kernel(dt, frames)
                        out.append(_case(f"{op}-n{n}-positive", "stream", op, dt, layout, lanes, frames, kernel=k, **kw))
    # one `_pitch` twin with a non-dense pitch: the padded LaneMajor rows of tests/test_gpu_lane_major_staged.py
    for tn, dt in TYPES.items():
        for lanes, frames, pitch in lm:
            if pitch != frames:
                out.append(_case(f"biquad_{tn}_df1_clamp_pitch-n1-zeros", "stream", f"biquad_{tn}_df1_clamp", dt, LM, lanes, frames,
                                 kernel=_lm_kernel(dt, frames, pitch), n=1, clamp="zeros", form="df1", values=4, pitch=pitch))
    return out


def bylane_cases():
    """The eight float `_bylane` entries: per-lane coefficients; clamped entries cycle the four clamp rows over 8-lane groups."""
    out = []
    shapes = [(1, 1), (63, 23), (65, 47), (257, 64), (100, 65), (1028, 77), (512, 300), (4096, 50)]
    for tn, dt in TYPES.items():
        for pat in ("biquad_{t}_df1", "biquad_{t}_df1_clamp", "biquad_{t}_df2t", "biquad_{t}_df2t_clamp"):
            op = pat.format(t=tn)
            vals, _, form = STREAM[pat]
            for coef in ("random",) if op.endswith("_clamp") else ("random", "positive"):
                for i, (lanes, frames) in enumerate(shapes):
                    n = (1, 3)[i % 2]
                    kw = dict(n=n, form=form, values=vals * n, coef=coef, clamp="cycle" if op.endswith("_clamp") else None)
                    for layout in (FM, LM):
                        k = "stream_frame_major" if layout == FM else _lm_kernel(dt, frames)
                        out.append(_case(f"{op}_bylane-n{n}-{coef}", "bylane", op, dt, layout, lanes, frames, kernel=k, **kw))
                if coef == "random":
                    kw = dict(n=1, form=form, values=vals, coef=coef, clamp="cycle" if op.endswith("_clamp") else None)
                    for lanes, frames in ((65536, 64), (16384, 96)):
                        out.append(_case(f"{op}_bylane-n1-{coef}", "bylane", op, dt, FM, lanes, frames, kernel=_fm_kernel(dt, 1, lanes), **kw))
                    out.append(_case(f"{op}_bylane-n1-{coef}", "bylane", op, dt, LM, 1000, 516, kernel=_lm_kernel(dt, 516), **kw))
    return out


C3 = {("dec", 16384, FM): "hbf_dec_ring[FrameMajor]", ("dec", 16384, LM): "hbf_dec_blk[LaneMajor]"}


def hbf_cases():
    """hbf_dec_f32 / hbf_int_f32 for /2 ... /32 and both tap sets on the ring / block shapes of test_gpu_parity.hbf_base_shapes()
    plus 16384 lanes (/16: the C3 kernels); the f64 entries; one custom all-positive tap set per decimator (generic-taps
    kernel; the only way a decimator's kind-1 lanes give -0, the built-in taps alternating in sign)."""
    from tests.test_gpu_parity import hbf_base_shapes

    out = []
    for kind in ("dec", "int"):
        for tap_set in (0, 1):
            for stages in (1, 2, 3, 4, 5):
                shapes = hbf_base_shapes(stages) + ([(16384, 64)] if stages == 4 and tap_set == 0 else [])
                for lanes, frames in shapes:
                    for layout in (FM, LM):
                        r = 1 << stages
                        out.append(_case(f"hbf_{kind}_f32-set{tap_set}-s{stages}", "cfg", f"hbf_{kind}_f32", F32, layout, lanes, frames,
                                         rin=r if kind == "dec" else 1, rout=1 if kind == "dec" else r, hbf=(kind, tap_set, stages),
                                         kernel=C3.get((kind, lanes, layout), f"hbf_{kind}_")))
        for tap_set, stages in ((0, 1), (0, 4), (1, 3), (1, 5)):
            ch = 2048 >> stages
            for lanes, frames in [(1, 1), (3, ch + 1), (17, 40), (64, 70), (300, 9)]:
                for layout in (FM, LM):
                    r = 1 << stages
                    out.append(_case(f"hbf_{kind}_f64-set{tap_set}-s{stages}", "cfg", f"hbf_{kind}_f64", F64, layout, lanes, frames,
                                     rin=r if kind == "dec" else 1, rout=1 if kind == "dec" else r, hbf=(kind, tap_set, stages),
                                     kernel=f"hbf_{kind}_f64_kernel"))
    for tn, dt in TYPES.items():
        for lanes, frames in ((17, 40), (64, 70)):
            for layout in (FM, LM):
                out.append(_case(f"hbf_dec_{tn}-positive-taps", "cfg", f"hbf_dec_{tn}", dt, layout, lanes, frames, rin=4, rout=1,
                                 hbf=("dec", "positive", 2), coef="positive",
                                 kernel="hbf_dec_" if tn == "f32" else "hbf_dec_f64_kernel"))
    return out


def fir_cases():
    """fir_sym_f32 / fir_sym_f64, kinds 0-3 (Type I-IV), 1 to 32 one-sided taps; one all-positive symmetric tap set."""
    out = []
    for tn, dt in TYPES.items():
        k = "fir_sym_kernel" if tn == "f32" else "fir_sym_f64_kernel"
        for kind in (0, 1, 2, 3):
            for m in (1, 4, 23, 32):
                for lanes, frames in [(1, 1), (3, 255), (5, 2049), (17, 300), (64, 70)]:
                    for layout in (FM, LM):
                        out.append(_case(f"fir_sym_{tn}-kind{kind}-m{m}", "cfg", f"fir_sym_{tn}_process", dt, layout, lanes, frames,
                                         fir=(kind, m), kernel=k))
        for kind in (0, 1):
            for layout in (FM, LM):
                out.append(_case(f"fir_sym_{tn}-kind{kind}-m4-positive", "cfg", f"fir_sym_{tn}_process", dt, layout, 64, 70,
                                 fir=(kind, 4), coef="positive", kernel=k))
    return out


def _lockin_kernel(layout, frames):
    """tests/test_gpu_lockin_generic.py: FrameMajor always the multi-wave kernel; LaneMajor from 32 frames on 16-byte rows (a stream
    kernel takes the last frames % 16), the one-thread-per-lane stream kernels below; rows off the 16-byte grid: either."""
    if layout == FM or (frames >= 32 and frames % 4 == 0):
        return "lockin_waves_kernel"
    return "stream_lane_major" if frames < 32 else ("lockin_waves_kernel", "stream_lane_major")


def lockin_cases():
    """lockin_f32_biquad_lo_process with both x and lo special, on the shapes of tests/test_gpu_lockin_generic.py."""
    shapes = [(1, 1), (3, 5), (64, 33), (65, 128), (200, 257), (1024, 64), (4099, 19)]
    out = []
    for n in (1, 2, 4):
        for coef in ("random", "positive"):
            for lanes, frames in shapes if coef == "random" else shapes[3:5]:
                for layout in (FM, LM):
                    out.append(_case(f"lockin_f32_biquad_lo-n{n}-{coef}", "lo", "lockin_f32_biquad_lo_process", F32, layout, lanes, frames,
                                     n=n, rout=2, values=8 * n, coef=coef, form="lockin", kernel=_lockin_kernel(layout, frames)))
    return out


TABLES = {"stream": stream_cases, "bylane": bylane_cases, "hbf": hbf_cases, "fir": fir_cases, "lockin": lockin_cases}


# ----------------------------------------------------------------------------------------------------------- inputs
def _rows(rng, n, coef):
    """n x 5 coefficients, f32-representable (so the same rows serve f64): |a1| + |a2| < 1 keeps every section stable."""
    lo, hi = (0.05, 0.45) if coef == "positive" else (-0.5, 0.5)
    return rng.uniform(lo, hi, size=(n, 5)).astype(F32).astype(F64)


def prepare(case):
    """Inputs of a case, seeded by its id: cfg (ctypes), rows / coef / taps (numbers for the restatement), state (uint32
    [words, lanes]), x and lo for the two consecutive calls (logical [frames, lanes, chunk]), kind[lanes]."""
    rng = np.random.default_rng(zlib.crc32(case.id.encode()))
    dt, lanes, frames = case.dtype, case.lanes, case.frames
    f32 = dt == F32
    inp = types.SimpleNamespace(cfg=None, coef=None, rows=None, clamp=None, taps=None, lo=[None, None])
    zero = -0.0 if case.coef == "positive" else None
    w = np.dtype(dt).itemsize // 4
    if case.call in ("stream", "lo"):
        inp.rows = _rows(rng, case.n, case.coef)
        if case.clamp:
            inp.clamp = CLAMPS[case.clamp]
            mk = H.biquad_clamp_f32 if f32 else H.biquad_clamp_f64
            inp.cfg = mk([(r.tolist(),) + inp.clamp for r in inp.rows])
        else:
            inp.cfg = (H.biquad_f32 if f32 else H.biquad_f64)([r.tolist() for r in inp.rows])
        words = case.values * w
    elif case.call == "bylane":
        lo_, hi_ = (0.05, 0.45) if case.coef == "positive" else (-0.5, 0.5)
        cv = 8 if case.clamp else 5
        inp.coef = np.zeros((case.n, cv, lanes), dt)
        inp.coef[:, :5] = rng.uniform(lo_, hi_, size=(case.n, 5, lanes)).astype(dt)
        if case.clamp:
            sets = np.array([CLAMPS[k] for k in ("finite", "open", "zeros", "pzero")], dt)  # [4, (u, min, max)]
            inp.coef[:, 5:] = sets[(np.arange(lanes) // 8) % 4].T[None]
        words = case.values * w
    elif getattr(case, "hbf", None):
        kind, tap_set, stages = case.hbf
        inp.cfg = _abi.HbfCascadeF32() if f32 else _abi.HbfCascadeF64()
        if tap_set == "positive":
            inp.cfg.stages = stages
            for s, m in enumerate((3, 7)[:stages]):
                inp.cfg.m[s] = m
                for k, v in enumerate(rng.uniform(0.02, 0.3, size=m).astype(F32)):
                    inp.cfg.taps[s][k] = float(v)
        else:
            assert H.oracle().fn[f"hbf_{kind}_cascade" + ("" if f32 else "_f64")](tap_set, stages, C.byref(inp.cfg)) == 0
        inp.taps = [np.array(inp.cfg.taps[s][:inp.cfg.m[s]], dt) for s in range(inp.cfg.stages)]
        words = H.oracle().fn[f"hbf_{kind}_state_words" + ("" if f32 else "_f64")](C.byref(inp.cfg))
    else:
        kind, m = case.fir
        inp.cfg = _abi.FirSymF32() if f32 else _abi.FirSymF64()
        inp.cfg.kind, inp.cfg.m = kind, m
        t = rng.uniform(0.02, 0.3, size=m) if case.coef == "positive" else rng.standard_normal(m) * 0.3
        for k, v in enumerate(t.astype(F32)):
            inp.cfg.taps[k] = float(v)
        inp.taps = np.array(inp.cfg.taps[:m], dt)
        words = H.oracle().fn["fir_sym_state_words" + ("" if f32 else "_f64")](C.byref(inp.cfg))
    assert words > 0
    inp.x = []
    for rep in range(2):
        x, inp.kind = special_chunks(rng, frames, lanes, case.rin, dt, zero)
        inp.x.append(x)
    if case.call == "lo":  # the -0 case needs x * lo = -0 in the kind-1 lanes: x = -0, lo = +0
        inp.lo = [special_chunks(rng, frames, lanes, 2, dt, 0.0 if zero is not None else None)[0] for rep in range(2)]
    inp.state = special_state(rng, words, lanes, inp.kind, dt, zero)
    return inp


def to_flat(a, layout):
    """logical [frames, lanes, chunk] -> the flat buffer of `layout`."""
    return np.ascontiguousarray(a if layout == FM else a.transpose(1, 0, 2)).reshape(-1)


def from_flat(flat, layout, frames, lanes, chunk):
    if layout == FM:
        return flat.reshape(frames, lanes, chunk)
    return np.ascontiguousarray(flat.reshape(lanes, frames, chunk).transpose(1, 0, 2))


def invoke(lib, with_stream, case, inp, st, x, lo, y, coef=None, pitch=None):
    """One ABI call on the oracle (numpy arrays) or the engine (device tensors; `with_stream`)."""
    p = H._ptr
    geo = (case.lanes, case.frames, case.layout) + ((None,) if with_stream else ())
    if case.call == "stream":
        cfg = C.cast(inp.cfg, C.c_void_p)
        if pitch:
            return lib.fn[case.op + "_pitch"](cfg, case.n, p(st), p(x), pitch, p(y), pitch, *geo)
        return lib.fn[case.op](cfg, case.n, p(st), p(x), p(y), *geo)
    if case.call == "bylane":
        return lib.fn[case.op + "_bylane"](p(inp.coef if coef is None else coef), case.n, p(st), p(x), p(y), *geo)
    if case.call == "lo":
        return lib.fn[case.op](C.cast(inp.cfg, C.c_void_p), case.n, p(st), p(x), p(lo), p(y), *geo)
    return lib.fn[case.op](C.byref(inp.cfg), p(st), p(x), p(y), *geo)


def run_oracle(case, inp):
    """[(y [frames, lanes, chunk], state uint32 [words, lanes])] of the two consecutive calls on the CPU oracle."""
    o = H.oracle()
    st, out = inp.state.copy(), []
    for x, lo in zip(inp.x, inp.lo):
        y = np.empty(case.lanes * case.frames * case.rout, case.dtype)
        rc = invoke(o, False, case, inp, st, to_flat(x, case.layout), None if lo is None else to_flat(lo, case.layout), y)
        assert rc == 0, (case.id, rc)
        out.append((from_flat(y, case.layout, case.frames, case.lanes, case.rout), st.copy()))
    return out


def where(case, inp, shape):
    """Decoder of a flat index into a logical [frames, lanes, chunk] or a [values, lanes] array for assertion messages."""
    def f(i):
        idx = np.unravel_index(i, shape)
        lane = int(idx[1])
        names = ("frame", "lane", "k") if len(shape) == 3 else ("state value", "lane")
        return "(" + ", ".join(f"{n} {int(v)}" for n, v in zip(names, idx)) + f", kind {int(inp.kind[lane])})"
    return f


# ------------------------------------------------------------------------------------------------------- conditions
def zero_bounds(case):
    """Clamp rows whose bounds are both zeros: every output is +-0 (or NaN), whatever the data."""
    return case.clamp in ("zeros", "pzero")


# (case id, call) of the decimator rows whose single inf the oracle turns to NaN before the output: the stage that takes the
# inf on its odd branch gives one inf per tap, of the taps' alternating signs, and the next stage sums those.  17 calls of the
# 898 decimator calls with 8 lanes and 8 frames or more; there the narrowed form is asserted: NaN in a kind-4 lane, no inf.
INF_LOST = {
    ("hbf_dec_f32-set0-s4-FM-17x40", 1), ("hbf_dec_f32-set0-s4-LM-17x40", 1), ("hbf_dec_f32-set1-s5-FM-17x40", 1),
    ("hbf_dec_f32-set1-s5-LM-17x40", 1), ("hbf_dec_f32-set1-s5-FM-8x130", 1), ("hbf_dec_f32-set1-s5-LM-8x130", 1),
    ("hbf_dec_f32-set1-s5-FM-20x70", 0), ("hbf_dec_f32-set1-s5-FM-20x70", 1), ("hbf_dec_f32-set1-s5-LM-20x70", 1),
    ("hbf_dec_f32-set1-s5-FM-16x31", 1), ("hbf_dec_f32-set1-s5-LM-16x31", 1), ("hbf_dec_f64-set0-s4-FM-17x40", 1),
    ("hbf_dec_f64-set0-s4-LM-17x40", 1), ("hbf_dec_f64-set1-s5-FM-17x40", 1), ("hbf_dec_f64-set1-s5-LM-17x40", 1),
    ("hbf_dec_f64-set1-s5-FM-64x70", 1), ("hbf_dec_f64-set1-s5-LM-64x70", 1),
}


def check_conditions(case, inp, res):
    """The conditions a case must meet ON THE ORACLE so that the comparison checks something; returns the census of all
    outputs and state of the case (for the per-entry union).  They are no tolerances: a case that misses one is changed.

    Per call: the NaN cap.  Per call with 8 lanes and 8 frames or more: NaN present; +-inf present where no finite clamp
    bound removes it (unclamped, the open row, per-lane rows, which hold open rows from 16 lanes on); at least half of the
    kind-0 lanes entirely normal.  Narrowed, each with its assertion:
      * the second call of a recursive form (biquad, cascade, normal, lock-in arms) starts from the state the first call's inf
        has turned to NaN, so +-inf is asserted on the first call, and on the second that every kind-4 lane stays non-finite;
      * the decimator calls of INF_LOST;
      * clamp rows whose bounds are both zeros (which the clamp edges need) can only give +-0 or NaN: there the control lanes
        are asserted to be entirely +-0."""
    census = {"nan": 0.0, "inf": 0, "-0": 0, "+0": 0, "subnormal": 0, "normal": 0}
    recursive = case.call in ("stream", "bylane", "lo")
    for rep, (y, st) in enumerate(res):
        cy, cs = classes(y), classes(state_values(st, case.dtype))
        assert cy["nan"] <= NAN_CAP and cs["nan"] <= NAN_CAP, (case.id, rep, "NaN cap", cy["nan"], cs["nan"])
        for k in census:
            census[k] = max(census[k], cy[k]) if k == "nan" else census[k] + cy[k] + cs[k]
        if case.lanes < 8 or case.frames < 8:
            continue
        assert cy["nan"] > 0, (case.id, rep, "no NaN in the expected output")
        if case.clamp in (None, "open", "cycle"):
            open_row = (np.arange(case.lanes) // 8) % 4 == 1 if case.clamp == "cycle" else True  # per-lane rows: finite bounds elsewhere
            k4 = y[:, (inp.kind == 4) & open_row]
            if (case.id, rep) in INF_LOST:
                assert cy["inf"] == 0 and np.isnan(k4).any(), (case.id, rep, "listed in INF_LOST")
            elif recursive and rep == 1:
                assert (~np.isfinite(k4)).any(axis=(0, 2)).all(), (case.id, rep, "kind-4 lanes after an inf")
            else:
                assert cy["inf"] > 0, (case.id, rep, "no inf in the expected output")
        ctrl = y[:, inp.kind == 0]
        if zero_bounds(case):
            assert (ctrl == 0).all(), (case.id, rep, "control lanes")
        else:
            tiny = np.finfo(case.dtype).tiny
            whole = (np.isfinite(ctrl) & (np.abs(ctrl) >= tiny)).all(axis=(0, 2))
            assert 2 * int(whole.sum()) >= whole.size, (case.id, rep, "control lanes entirely normal", int(whole.sum()), whole.size)
    if case.coef == "positive" and getattr(case, "form", None) != "normal":
        # all coefficients positive, kind-1 lanes of x and state all -0: the output there is -0 throughout
        for y, _ in res:
            z = y[:, inp.kind == 1]
            assert z.size == 0 or ((z == 0) & np.signbit(z)).all(), (case.id, "-0 lanes")
    return census
