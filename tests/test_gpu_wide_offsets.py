"""Both sides of the launchers' 32-bit offset guards, and frame counts past 2^31.

Several FrameMajor / LaneMajor kernels address global memory as a wave-uniform 64-bit base plus a 32-bit per-thread byte offset; their
launchers keep those offsets in range with size guards (row pitch, in bytes, against 2^26 / 2^28; the sweep kernel's frames per segment
against 2^32).  Each case here runs a pitched biquad entry just inside and just outside one guard, checks the valid outputs and the
written-back state bit for bit against the CPU oracle, pins the kernel the dispatch took (`idsp_last_kernel()`), and counts, over the whole
allocation, the elements of y that differ from the sentinel: they must all lie in the valid region.

Every tensor starts 2 GiB into its allocation, behind a sentinel-filled lead-in, and the rest of the allocation is sentinel-filled too:
an offset that wrapped at 32 bits lands between the wave's base and the intended address, a sign-extended one at most 2 GiB below the
base — inside the allocation either way, so a broken guard shows up here as a parity or stray-write failure, not as a page fault."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from idsp_amd import _abi
from tests import _harness as H
from tests.test_gpu_pitch import init_state, sample, tdtype

pytestmark = pytest.mark.gpu
FM, LM = H.FM, H.LM
DEV = "cuda:0"
SENT = -1234567
LEAD = 2 << 30  # bytes of sentinel before the first element
PEAK = 24 << 30  # device memory per test
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def stable_sections(kind, count):
    """`count` low-pass sections (stable: float outputs stay finite over any number of frames, so NaN payloads never enter a comparison)"""
    o = H.oracle()
    out = []
    for k in range(count):
        sos = (C.c_double * 6)(*o.lowpass_sos(0.01 * (k + 1)))
        q = kind()
        assert o.fn["biquad_f32_from_sos_f64" if kind is _abi.BiquadF32 else "biquad_f64_from_sos"](sos, C.byref(q)) == 0
        out.append(q)
    return (kind * count)(*out)


def procs(rng, chain=False, f64=False):
    """(entry, cfg, sections, state words per section, dtype): one cheap i32 section and one f32 DF2T section; a 2-section chain, an f64 section"""
    ri = [(rng.integers(-(1 << 29), 1 << 29, size=5).tolist(), 29) for _ in range(2)]
    out = [("biquad_i32_df1", H.biquad_i32(ri[:1]), 1, 4, np.int32), ("biquad_f32_df2t", stable_sections(_abi.BiquadF32, 1), 1, 2, np.float32)]
    if chain:
        out.append(("biquad_i32_df1", H.biquad_i32(ri), 2, 4, np.int32))
    if f64:
        out.append(("biquad_f64_df2t", stable_sections(_abi.BiquadF64, 1), 1, 4, np.float64))
    return out


def wide_buffer(t, rows, pitch):
    """a sentinel-filled allocation with `rows` rows of `pitch` elements starting LEAD bytes into it; (allocation, rows view)"""
    esz = torch.empty(0, dtype=t).element_size()
    lead = LEAD // esz
    b = torch.full((lead + rows * pitch + 64,), SENT, dtype=t, device=DEV)
    return b, b[lead:lead + rows * pitch].view(rows, pitch)


def not_sentinel(t):
    """elements of t that differ from the sentinel, counted on the device (in pieces of 2^26: a reduction over a whole allocation at
    once would hold a mask and its int64 sum the size of the allocation)"""
    flat = t.reshape(-1)
    return sum(int(torch.count_nonzero(piece != SENT)) for piece in flat.split(1 << 26))


def run_wide(gpu, rng, proc, lanes, frames, layout, xp, yp, inplace):
    """one pitched call on wide buffers; checks parity, state and stray writes, returns the kernel name"""
    op, cfg, n, words, dt = proc
    o = H.oracle()
    row, rows = (frames, lanes) if layout == LM else (lanes, frames)
    xh = sample(rng, dt, lanes * frames).reshape(rows, row)
    want = np.empty_like(xh)
    st0 = init_state(rng, dt, words * n, lanes)
    so = st0.copy()
    assert o.stream(op, cfg, n, so, xh, want, lanes, frames, layout) == 0
    t = tdtype(dt)
    xb, xv = wide_buffer(t, rows, xp)
    xv[:, :row] = torch.from_numpy(xh).to(DEV)
    if inplace:
        assert xp == yp
        yb, yv = xb, xv
    else:
        yb, yv = wide_buffer(t, rows, yp)
    sg = torch.from_numpy(st0.view(np.int32)).to(DEV)
    rc = gpu.fn[op + "_pitch"](C.cast(cfg, C.c_void_p), n, C.c_void_p(sg.data_ptr()), C.c_void_p(xv.data_ptr()), xp, C.c_void_p(yv.data_ptr()), yp,
                               lanes, frames, layout, None)
    torch.cuda.synchronize()
    assert rc == 0, (op, gpu.err())
    kernel = gpu.last_kernel()
    where = (op, n, lanes, frames, layout, xp, yp, inplace, kernel)
    got = yv[:, :row].cpu().numpy()
    assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), where  # integers exact, floats 0 ULP
    assert np.array_equal(sg.cpu().numpy().view(np.uint32), so), where + ("state",)
    # every element of y's allocation that is not the sentinel lies in the valid region
    assert not_sentinel(yb) == int(torch.count_nonzero(yv[:, :row] != SENT)), where + ("stray writes",)
    if not inplace:
        assert torch.equal(xv[:, :row].cpu(), torch.from_numpy(xh)), where + ("x changed",)
    del xb, xv, yb, yv, sg
    torch.cuda.empty_cache()
    return kernel


def sides(gpu, rng, procs_, lanes, frames, layout, inside, outside, want_in, want_out, out_of_place=True, mixed_frames=None):
    """run every processor at row bytes `inside` and `outside` (None: no outside) for both x and y, out of place and in place, then out of
    place with x inside and y outside and the reverse (`mixed_frames` frames: the guards check xl and yl each, and either one outside
    must take the outside kernel); returns the (case, kernel) pairs whose kernel name is not the pinned one"""
    bad = []
    for proc in procs_:
        esz = np.dtype(proc[4]).itemsize
        for pitch_bytes, want in ((inside, want_in), (outside, want_out)):
            if pitch_bytes is None:
                continue
            pitch = pitch_bytes // esz
            for inplace in (False, True) if out_of_place else (True,):
                k = run_wide(gpu, rng, proc, lanes, frames, layout, pitch, pitch, inplace)
                if not (want(k) if callable(want) else k.startswith(want)):
                    bad.append((proc[0], proc[2], pitch_bytes, inplace, k))
        if outside is not None:
            for xb, yb in ((inside, outside), (outside, inside)):
                k = run_wide(gpu, rng, proc, lanes, mixed_frames or frames, layout, xb // esz, yb // esz, False)
                if not (want_out(k) if callable(want_out) else k.startswith(want_out)):
                    bad.append((proc[0], proc[2], (xb, yb), False, k))
    return bad


@pytest.fixture
def peak(request):
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    yield
    torch.cuda.empty_cache()
    used = torch.cuda.max_memory_allocated()
    print("\npeak device memory %s: %.2f GiB" % (request.node.name, used / 2 ** 30))  # (shown with pytest -s)
    assert used <= PEAK, used


def test_frame_major_staged_row_guard(gpu, peak):
    """lane_stream.h:1825 `xl * sz < 2^28` / `yl * sz < 2^28` (FrameMajor staged kernel, 16 lanes/wave: up to 15 row pitches + 1 KiB
    inside a tile): 4096 lanes x 17 frames at row bytes 2^28 - 64 (staged) and 2^28 (the register-window kernel); i32 DF1, f32 DF2T,
    a 2-section i32 chain and an f64 DF2T section (8-byte samples: the same byte guard)."""
    rng = np.random.default_rng(1)
    bad = sides(gpu, rng, procs(rng, chain=True, f64=True), 4096, 17, FM, (1 << 28) - 64, 1 << 28,
                "stream_frame_major_staged[16 lanes/wave]<", "stream_frame_major<")
    assert not bad, bad


def test_round_split_row_guard(gpu, peak):
    """lane_stream.h:1743 `xl * 4 < 2^28` / `yl * 4 < 2^28` (whole rounds on the sweep kernel + remainder on the staged kernel): 65552 lanes
    x 16 frames at row bytes 2^28 - 64 (split) and 2^28 (one sweep of narrow blocks)."""
    rng = np.random.default_rng(2)
    bad = sides(gpu, rng, procs(rng, chain=True), 65552, 16, FM, (1 << 28) - 64, 1 << 28,
                "stream_frame_major_sweep + stream_frame_major_staged (remainder, second stream)<", "stream_frame_major_sweep[2 blocks/workgroup]<")
    assert not bad, bad


def test_sweep_frames_per_segment_guard(gpu, peak):
    """fm_sweep.h:597 `((f - 1) * kSweepT * max(xl, yl) + 256) * 4 < 2^32` (`xvoff` of the several-frames-per-segment sweep,
    fm_sweep.h:191): 32768 lanes x 24 frames in place (128-lane blocks: up to 2 frames per segment) at pitch 2^27 - 48 elements
    (2 frames per segment, the largest offset 2^32 - 512 bytes) and 2^27 - 32 (2^32: 1 frame per segment); x and y at different pitches
    out of place with 16 frames."""
    rng = np.random.default_rng(3)
    sweep = "stream_frame_major_sweep[1 block/workgroup]<"
    # (equal pitches in place only: x and y of 12 GiB each would not fit out of place; the guard takes max(xl, yl))
    bad = sides(gpu, rng, procs(rng, chain=True), 32768, 24, FM, ((1 << 27) - 48) * 4, ((1 << 27) - 32) * 4,
                lambda k: k.startswith(sweep) and k.endswith("> [2 frames/segment]"), lambda k: k.startswith(sweep) and k.endswith("> [1 frame/segment]"),
                out_of_place=False, mixed_frames=16)
    assert not bad, bad


def test_sweep_one_frame_per_segment_past_4_gib(gpu, peak):
    """fm_sweep.h:597 (the other kernel form): a lane block of 65536 lanes x 70 frames at pitch 2^24 + 64 elements — full 256-lane
    blocks, one frame per segment, row offsets past 4 GiB (size_t in the kernel)."""
    rng = np.random.default_rng(4)
    bad = sides(gpu, rng, procs(rng), 65536, 70, FM, ((1 << 24) + 64) * 4, None,
                lambda k: k.startswith("stream_frame_major_sweep[1 block/workgroup]<") and not k.endswith("/segment]"), None)
    assert not bad, bad


def test_lds_dma_off_grid_past_4_gib(gpu, peak):
    """lane_stream.h:1743 and :1825 on their outside (row bytes 2^28 + 16, off the 64-byte grid): 65540 lanes x 17 frames at pitch
    2^26 + 4 elements go to the XCD-contiguous LDS-DMA kernel, whose row offsets are 64-bit."""
    rng = np.random.default_rng(5)
    bad = sides(gpu, rng, procs(rng), 65540, 17, FM, ((1 << 26) + 4) * 4, None, "stream_frame_major_lds[XCD-contiguous blocks]<", None)
    assert not bad, bad


LM_SNIPPET = r"""
import json, sys
import numpy as np, torch
sys.path.insert(0, %r)
from idsp_amd import _abi
from tests import _harness as H
from tests.test_gpu_wide_offsets import procs, sides, LM
gpu = H.engine()
rng = np.random.default_rng(6)
torch.cuda.reset_peak_memory_stats()
bad = sides(gpu, rng, procs(rng, chain=True, f64=True), 65, 300, LM, (1 << 26) - 16, 1 << 26, "stream_lane_major_staged<", "stream_lane_major<")
print(json.dumps({"bad": bad, "peak": torch.cuda.max_memory_allocated()}))
"""


def test_lane_major_staged_row_guard(gpu):  # (the peak is measured in the subprocess)
    """lane_stream.h:1646-1648 `xl * isz < 2^26` / `yl * osz < 2^26` (LaneMajor staged kernel: 64 rows span less than 4 GiB,
    lane_stream.h:906-909): 65 lanes x 300 frames with 64 lanes per wave forced (IDSP_DIAG=1 IDSP_LM_LANES_PER_WAVE=64, read once per
    process: a subprocess) at row bytes 2^26 - 16 (staged) and 2^26 (the tile kernel); i32 DF1, f32 DF2T, a 2-section chain, f64 DF2T."""
    env = dict(os.environ, IDSP_DIAG="1", IDSP_LM_LANES_PER_WAVE="64")
    r = subprocess.run([sys.executable, "-c", LM_SNIPPET % ROOT], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert not res["bad"], res["bad"]
    print("\npeak device memory test_lane_major_staged_row_guard (subprocess): %.2f GiB" % (res["peak"] / 2 ** 30))
    assert res["peak"] <= PEAK, res["peak"]


# ------------------------------------------------------------------------------------------------ frame counts past 2^31
FRAMES = (1 << 31) + 77
CHUNK = 1 << 24


def chunk_x(k, dt, seed):
    """frames [k CHUNK, (k + 1) CHUNK) of x, generated on the device from a seed of their own (so they can be made again after an in-place call)"""
    n = min(CHUNK, FRAMES - k * CHUNK)
    g = torch.Generator(device=DEV)
    g.manual_seed(seed * 100003 + k)
    if dt == np.int32:
        return torch.randint(-(1 << 31), 1 << 31, (n,), dtype=torch.int64, device=DEV, generator=g).to(torch.int32)
    return torch.randn(n, dtype=torch.float32, device=DEV, generator=g)


def long_single_lane(gpu, proc, layout, inplace, seed, want_kernel):
    op, cfg, n, words, dt = proc
    o = H.oracle()
    t = tdtype(dt)
    nch = (FRAMES + CHUNK - 1) // CHUNK
    x = torch.empty(FRAMES, dtype=t, device=DEV)
    for k in range(nch):
        x[k * CHUNK:(k + 1) * CHUNK] = chunk_x(k, dt, seed)
    y = x if inplace else torch.full((FRAMES,), SENT, dtype=t, device=DEV)
    st0 = init_state(np.random.default_rng(seed), dt, words * n, 1)
    sg = torch.from_numpy(st0.view(np.int32)).to(DEV)
    assert gpu.stream(op, cfg, n, sg, x, y, 1, FRAMES, layout) == 0, gpu.err()
    torch.cuda.synchronize()
    kernel = gpu.last_kernel()
    assert kernel.startswith(want_kernel), kernel
    so = st0.copy()
    for k in range(nch):
        xc = chunk_x(k, dt, seed).cpu().numpy()
        want = np.empty_like(xc)
        assert o.stream(op, cfg, n, so, xc, want, 1, len(xc), layout) == 0
        got = y[k * CHUNK:k * CHUNK + len(xc)].cpu().numpy()
        assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), (op, k, int(np.flatnonzero(got.view(np.uint8) != want.view(np.uint8))[0]))
    assert np.array_equal(sg.cpu().numpy().view(np.uint32), so), (op, "state")


def test_frame_count_past_2_31_frame_major_few(gpu, peak):
    """one lane, 2^31 + 77 frames, i32 DF1 FrameMajor out of place on stream_frame_major_few (frame counters: size_t outside the tile
    loops' int counters)"""
    rng = np.random.default_rng(7)
    long_single_lane(gpu, procs(rng)[0], FM, False, 7, "stream_frame_major_few<")


def test_frame_count_past_2_31_lane_major(gpu, peak):
    """one lane, 2^31 + 77 frames, f32 DF2T LaneMajor in place on stream_lane_major (a row of 8 GiB is past the staged kernel's guard,
    lane_stream.h:1646)"""
    rng = np.random.default_rng(8)
    long_single_lane(gpu, procs(rng)[1], LM, True, 8, "stream_lane_major<")


# ------------------------------------------------------------------- families without `_pitch` entries: dense tensors past 2^32 bytes
def dense_subset(gpu, rng, op, cfg, words, lanes, frames, layout, x, y, want_kernel, float_state=False):
    """one call on dense tensors behind LEAD bytes of sentinel: x = (dtype, samples per lane and frame, "bits" | "normal") or None (DDS),
    y = (dtype, samples per lane and frame); FrameMajor rows are frames of lanes x width, LaneMajor rows lanes of frames x width.  A subset
    of lanes — the first 256, the last 256, 256 others — is gathered on the device and compared with the oracle (lanes never interact),
    the state planes likewise; then the stray-write count over y's whole allocation"""
    o = H.oracle()
    tt = {np.dtype(np.int32): torch.int32, np.dtype(np.int64): torch.int64, np.dtype(np.float32): torch.float32}
    rows = frames if layout == FM else lanes

    def buffers(dt, width):
        return wide_buffer(tt[np.dtype(dt)], rows, (lanes if layout == FM else frames) * width)

    def gather(v, width, it):  # the lanes `it` of a rows view, as the dense tensor of those lanes alone
        if layout == FM:
            return v.view(frames, lanes, width)[:, it, :].reshape(frames, -1).cpu().numpy()
        return v[it, :].cpu().numpy()

    g = torch.Generator(device=DEV)
    g.manual_seed(int(rng.integers(1 << 30)))
    if x is not None:
        x_dt, x_width, kind = x
        xb, xv = buffers(x_dt, x_width)
        step = max(1, (256 << 20) // (xv.shape[1] * xv.element_size()))
        for r in range(0, rows, step):  # a quarter GiB at a time: random bit patterns, or normal floats (no NaN payloads to compare)
            piece = xv[r:r + step]
            if kind == "bits":
                piece.view(torch.uint8).copy_(torch.randint(0, 256, tuple(piece.view(torch.uint8).shape), dtype=torch.uint8, device=DEV, generator=g))
            else:
                piece.copy_(torch.randn(tuple(piece.shape), dtype=piece.dtype, device=DEV, generator=g))
    y_dt, y_width = y
    yb, yv = buffers(y_dt, y_width)
    if float_state:
        st0 = rng.standard_normal((words, lanes)).astype(np.float32).view(np.uint32)
    else:
        st0 = rng.integers(0, 1 << 32, size=(words, lanes), dtype=np.uint64).astype(np.uint32)
    sg = torch.from_numpy(st0.view(np.int32)).to(DEV)
    if x is None:
        rc = gpu.fn[op](C.c_void_p(sg.data_ptr()), C.c_void_p(yv.data_ptr()), lanes, frames, layout, None)
    else:
        rc = gpu.fn[op](C.byref(cfg), C.c_void_p(sg.data_ptr()), C.c_void_p(xv.data_ptr()), C.c_void_p(yv.data_ptr()), lanes, frames, layout, None)
    torch.cuda.synchronize()
    assert rc == 0, (op, gpu.err())
    kernel = gpu.last_kernel()
    where = (op, lanes, frames, layout, kernel)
    assert kernel.startswith(want_kernel), where
    assert not_sentinel(yb) == not_sentinel(yv), where + ("stray writes",)
    mid = rng.choice(np.arange(256, lanes - 256), 256, replace=False)
    idx = np.unique(np.concatenate([np.arange(256), np.arange(lanes - 256, lanes), mid]))
    it = torch.from_numpy(idx).to(DEV)
    so = np.ascontiguousarray(st0[:, idx])
    want = np.empty((frames * idx.size * y_width,), y_dt)
    if x is None:
        assert o.fn[op](H._ptr(so), H._ptr(want), idx.size, frames, layout) == 0
    else:
        xs = np.ascontiguousarray(gather(xv, x_width, it))
        assert o.cfgcall(op, cfg, so, xs, want, idx.size, frames, layout) == 0
    got = gather(yv, y_width, it).reshape(-1)
    assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), where  # integers exact, floats 0 ULP
    assert np.array_equal(sg.view(words, lanes)[:, it].cpu().numpy().view(np.uint32), so), where + ("state",)
    del yb, yv, sg
    if x is not None:
        del xb, xv, piece
    torch.cuda.empty_cache()
    return kernel


@pytest.mark.parametrize("op, y_width, y_dt, want", [
    ("lockin_i32_process", 2, np.int32, "lockin_waves_kernel"),
    ("lockin_i32_arg", 1, np.int32, "lockin_stages_kernel[16 waves per 128 lanes]"),
    ("lockin_i32_norm_sqr", 1, np.int64, "lockin_waves_kernel"),
])
def test_lockin_frame_major_past_4_gib(gpu, peak, op, y_width, y_dt, want):
    """lock-in, FrameMajor, 2^20 lanes x 1040 frames (x: 2^32 + 2^28 bytes): the IQ form and the fused `arg` / `norm_sqr` read-outs,
    whose waves address x and y through a wave-uniform base (lockin_waves.h)"""
    rng = np.random.default_rng(9)
    cfg = H.lockin_cfg([[int(rng.integers(1, 1 << 24)), -int(rng.integers(1, 1 << 29))] for _ in range(2)])
    dense_subset(gpu, rng, op, cfg, 18, 1 << 20, 1040, FM, (np.int32, 1, "bits"), (y_dt, y_width), want)


def test_dds_frame_major_past_4_gib(gpu, peak):
    """DDS, FrameMajor, 2^20 lanes x 520 frames (y: [re, im] per lane and frame, 2^32 + 2^28 bytes; dds.hip's processor on the
    register-window stream kernel at this shape)"""
    rng = np.random.default_rng(11)
    dense_subset(gpu, rng, "dds_i32", None, 2, 1 << 20, 520, FM, None, (np.int32, 2), "stream_frame_major<idsp::(anonymous namespace)::DdsProcT<false>>")


@pytest.mark.parametrize("kind, layout, lanes, frames, want", [
    ("dec", FM, 16384, 4160, "hbf_dec_ring[FrameMajor]"),
    ("dec", LM, 16400, 4096, "hbf_dec_blk[LaneMajor]"),
    ("int", FM, 16384, 4160, "hbf_int_block_fm<"),
    ("int", LM, 16400, 4096, "hbf_int_wave[LaneMajor]"),
], ids=["dec-FM", "dec-LM", "int-FM", "int-LM"])
def test_hbf_past_4_gib(gpu, peak, kind, layout, lanes, frames, want):
    """half-band /16 (4 stages, f32) on the 16-rate side past 2^32 bytes: 16384 x 4160 x 16 FrameMajor, 16400 lanes x 65536 frames
    LaneMajor (just past C3) — hbf_ring.h / hbf_blk.h / hbf_wave.h address through wave-uniform bases"""
    rng = np.random.default_rng(12 + 2 * layout + (kind == "int"))
    cfg = _abi.HbfCascadeF32()
    assert gpu.fn["hbf_%s_cascade" % kind](0, 4, C.byref(cfg)) == 0
    words = gpu.fn["hbf_%s_state_words" % kind](C.byref(cfg))
    x, y = ((np.float32, 16, "normal"), (np.float32, 1)) if kind == "dec" else ((np.float32, 1, "normal"), (np.float32, 16))
    dense_subset(gpu, rng, "hbf_%s_f32" % kind, cfg, words, lanes, frames, layout, x, y, want, float_state=True)


@pytest.mark.parametrize("kind, dt, layout, frames, want", [
    ("dec", np.int32, FM, 1040, "cic_dec_kernel"),
    ("dec", np.int64, FM, 520, "cic_dec_kernel"),
    ("dec", np.int32, LM, 1040, "cic_dec_ring[LaneMajor]"),
    ("int", np.int32, FM, 1040, "cic_int_ring[FrameMajor]"),
], ids=["dec-i32-FM", "dec-i64-FM", "dec-i32-LM", "int-i32-FM"])
def test_cic_past_4_gib(gpu, peak, kind, dt, layout, frames, want):
    """Cic /16 (order 3), 65536 lanes, the 16-rate side past 2^32 bytes (2^32 + 2^28): the decimator's generic kernel (FrameMajor: each
    lane's 16 inputs of an output frame side by side) and wave-per-lane ring (LaneMajor, cic_ring.h), the interpolator's ring kernel"""
    rng = np.random.default_rng(20 + 2 * layout + (kind == "int") + 4 * (dt == np.int64))
    cfg = _abi.Cic(3, 1, 15)
    words = gpu.fn["cic_state_words"](C.byref(cfg), 64 if dt == np.int64 else 32)
    x, y = ((dt, 16, "bits"), (dt, 1)) if kind == "dec" else ((dt, 1, "bits"), (dt, 16))
    dense_subset(gpu, rng, "cic_%s_%s" % (kind, "i64" if dt == np.int64 else "i32"), cfg, words, 65536, frames, layout, x, y, want)


# ------------------------------------------------ entries held to a numpy specification (no CPU oracle): PFB, CORDIC, batch LO, RPLL, unwrapper
def dense_subset_np(gpu, rng, call, spec, st0, lanes, layout, xs, y, want_kernel, subset=256):
    """`dense_subset` for the entries whose reference is a numpy specification.  xs: inputs [(dtype, frames, samples per lane and frame,
    "bits" | "normal"), ..]; y = (dtype, frames, samples per lane and frame); st0 [words, lanes] uint32 or None.  call(state, inputs, y) -> rc on
    device tensors; spec(state subset, [input subset [frames, n, width], ..]) -> [y frames, n, width], state subset updated.  The first `subset`
    lanes, the last `subset` and `subset` others are compared, their state planes likewise; then the stray-write count over y's allocation."""
    tt = {np.dtype(np.int32): torch.int32, np.dtype(np.int64): torch.int64, np.dtype(np.float32): torch.float32}

    def buffers(dt, frames, width):
        return wide_buffer(tt[np.dtype(dt)], frames if layout == FM else lanes, (lanes if layout == FM else frames) * width)

    def gather(v, frames, width, it):  # the lanes `it` as [frames, n, width]
        if layout == FM:
            return v.view(frames, lanes, width)[:, it, :].cpu().numpy()
        return np.ascontiguousarray(np.swapaxes(v[it, :].cpu().numpy().reshape(it.numel(), frames, width), 0, 1))

    g = torch.Generator(device=DEV)
    g.manual_seed(int(rng.integers(1 << 30)))
    keep, views = [], []
    for dt, frames, width, kind in xs:
        xb, xv = buffers(dt, frames, width)
        for piece in xv.reshape(-1).split((64 << 20)):  # a quarter GiB at a time: random bit patterns, or normal floats (no NaN payloads to compare)
            if kind == "bits":
                piece.view(torch.uint8).copy_(torch.randint(0, 256, (piece.numel() * piece.element_size(),), dtype=torch.uint8, device=DEV, generator=g))
            else:
                piece.copy_(torch.randn((piece.numel(),), dtype=piece.dtype, device=DEV, generator=g))
        del piece
        keep.append(xb), views.append(xv)
    y_dt, y_frames, y_width = y
    yb, yv = buffers(y_dt, y_frames, y_width)
    sg = None if st0 is None else torch.from_numpy(st0.view(np.int32)).to(DEV)
    rc = call(sg, views, yv)
    torch.cuda.synchronize()
    assert rc == 0, gpu.err()
    kernel = gpu.last_kernel()
    where = (lanes, layout, xs, y, kernel)
    assert kernel.startswith(want_kernel), where
    assert not_sentinel(yb) == not_sentinel(yv), where + ("stray writes",)
    mid = rng.integers(subset, lanes - subset, size=subset)  # (drawn with replacement: `lanes` may be half a billion elements)
    idx = np.unique(np.concatenate([np.arange(subset), np.arange(lanes - subset, lanes), mid]))
    it = torch.from_numpy(idx).to(DEV)
    so = None if st0 is None else np.ascontiguousarray(st0[:, idx])
    want = spec(so, [gather(v, x[1], x[2], it) for v, x in zip(views, xs)])
    got = gather(yv, y_frames, y_width, it)
    assert got.shape == want.reshape(got.shape).shape and np.array_equal(got.view(np.uint8), np.ascontiguousarray(want).reshape(got.shape).view(np.uint8)), where
    if st0 is not None:
        assert np.array_equal(sg.view(st0.shape[0], lanes)[:, it].cpu().numpy().view(np.uint32), so), where + ("state",)
    del keep, views, xv, xb, yb, yv, sg
    torch.cuda.empty_cache()
    return kernel


def _p(t):
    return C.c_void_p(t.data_ptr())


@pytest.mark.parametrize("layout, lanes, frames, want", [
    (FM, 65536, 2112, "pfb_frame_major[segment 256 frames]<taps 8>"),
    (LM, 16400, 8192, "pfb_lane_major[tile 256 frames]<taps 8>"),
], ids=["FM", "LM"])
def test_pfb_past_4_gib(gpu, peak, layout, lanes, frames, want):
    """idsp_pfb_f32_process, 8 taps with the DFT, out of place: 65536 lanes x 2112 frames FrameMajor (x and y 2^32 + 2^27 bytes each) and
    16400 lanes x 8192 frames LaneMajor (just past 2^32) — pfb_frame_major / pfb_lane_major index frames of 32 bytes on their own (pfb.h)"""
    from tests import _pfb_spec as PF
    from tests.test_gpu_pfb import make_cfg

    rng = np.random.default_rng(30 + layout)
    taps = 8
    coeff = rng.standard_normal((taps, 4)).astype(np.float32)
    cfg = make_cfg(coeff, 1)
    st0 = PF.random_state(rng, taps, lanes)
    dense_subset_np(gpu, rng, lambda sg, xv, yv: gpu.fn["pfb_f32_process"](C.byref(cfg), _p(sg), _p(xv[0]), _p(yv), lanes, frames, layout, None),
                    lambda so, xi: PF.bank_np(coeff, 1, so, xi[0].reshape(frames, -1, 4, 2)), st0, lanes, layout,
                    [(np.float32, frames, 8, "normal")], (np.float32, frames, 8), want)


@pytest.mark.parametrize("name", ["cos_sin", "sqrt_atan2", "div"])
def test_cordic_past_4_gib(gpu, peak, name):
    """n = 2^29 + 2^25 + 3 elements of cordic_kernel: xy 2^32 + 2^28 + 24 bytes; a rotating and a vectoring pair-output form (out as large) and a
    word-output form (`div`; both cos_sin and sqrt_atan2 return pairs).  Elementwise: the first 2^16, the last 2^16 and 2^16 other elements are compared"""
    from tests import _cordic_spec as CS

    n = (1 << 29) + (1 << 25) + 3
    pair = CS.FUNCTIONS[name][2]
    rng = np.random.default_rng(40 + pair)
    dense_subset_np(gpu, rng, lambda sg, xv, yv: gpu.fn["cordic_%s_i32" % name](_p(xv[0]), _p(xv[1]), _p(yv), n, None),
                    lambda so, xi: CS.function_np(name, xi[0][0], xi[1][0, :, 0]), None, n, FM,
                    [(np.int32, 1, 2, "bits"), (np.int32, 1, 1, "bits")], (np.int32, 1, 2 if pair else 1), "cordic_kernel<%s>[four elements per thread]" % name,
                    subset=1 << 16)


@pytest.mark.parametrize("layout, lanes, updates, want", [
    (FM, 1 << 20, 65, "accu_lo_kernel[FrameMajor]"),
    (LM, 65536, 1040, "accu_lo_kernel[LaneMajor]"),
], ids=["FM", "LM"])
def test_accu_lo_past_4_gib(gpu, peak, layout, lanes, updates, want):
    """idsp_accu_lo_i32 with batch_log2 = 3: `lo` of 2^20 lanes x 520 samples FrameMajor and 65536 lanes x 8320 samples LaneMajor (2^32 + 2^28 bytes) —
    accu_lo_kernel computes `lo + r * cols * 2` and the accu index on its own (rpll.hip)"""
    from tests import _rpll_spec as RS

    k = 3
    lo_cfg = (k, 3, 12345)
    rng = np.random.default_rng(50 + layout)
    dense_subset_np(gpu, rng, lambda sg, xv, yv: gpu.fn["accu_lo_i32"](C.byref(_abi.AccuLo(*lo_cfg)), _p(xv[0]), _p(yv), lanes, updates, layout, None),
                    lambda so, xi: RS.accu_lo_np(lo_cfg, xi[0]), None, lanes, layout, [(np.int32, updates, 2, "bits")], (np.int32, updates << k, 2), want)


def test_rpll_frame_major_past_4_gib(gpu, peak):
    """idsp_rpll_i32, FrameMajor, 2^20 lanes x 520 frames (ts and accu 2^32 + 2^28 bytes each): the only 8-byte-in processor on the register-window
    stream kernel at a large lane count"""
    from tests import _rpll_spec as RS

    lanes, frames, cfg = 1 << 20, 520, (8, 23, 22)
    rng = np.random.default_rng(60)
    dense_subset_np(gpu, rng, lambda sg, xv, yv: gpu.fn["rpll_i32"](C.byref(_abi.Rpll(*cfg)), _p(sg), _p(xv[0]), _p(yv), lanes, frames, FM, None),
                    lambda so, xi: RS.rpll_np(cfg, so, xi[0]), RS.random_state(rng, lanes), lanes, FM, [(np.int32, frames, 2, "bits")], (np.int32, frames, 2),
                    "stream_frame_major<idsp::(anonymous namespace)::RpllProc>")


def test_unwrap_phase_frame_major_past_4_gib(gpu, peak):
    """idsp_unwrap_i32_phase, FrameMajor, 2^20 lanes x 520 frames: 4-byte rows in, 8-byte rows out (y 2^32 + 2^28 bytes) on the register-window kernel"""
    from tests import _phase_spec as PS

    lanes, frames = 1 << 20, 520
    rng = np.random.default_rng(61)
    dense_subset_np(gpu, rng, lambda sg, xv, yv: gpu.fn["unwrap_i32_phase"](_p(sg), _p(xv[0]), _p(yv), lanes, frames, FM, None),
                    lambda so, xi: PS.unwrap_np(so, xi[0][:, :, 0], mode=1)[:, :, None], PS.random_state(rng, 2, lanes), lanes, FM,
                    [(np.int32, frames, 1, "bits")], (np.int64, frames, 1), "stream_frame_major<idsp::(anonymous namespace)::UnwrapProc<1>>")
