"""include/idsp_hip.h: "`stream` is a `hipStream_t` ... Calls are asynchronous on that stream" -- held for every processing entry, under
the arrangement of tests/_on_stream.py: decoys in the device buffers, the true inputs copied in on a stream S behind a device-side delay,
the call with `stream = S`, the results read back on S.  A call counts only when it was ARMED (the delay was still running when the call
returned): a launch that went to another stream then computed from the decoy, and a call that waits for the device cannot be armed.

  * control (first, own process): the engine is deliberately handed NULL under the same arrangement and must LOSE -- the read-back is
    the oracle's output for the decoy.  It proves that the arrangement bites on this runtime.
  * replays: the parity files once more, each in a child process with IDSP_TEST_STREAM=1 (tests/_backends.py and the `_pitch` runners of
    tests/test_gpu_frame_major_staged.py / test_gpu_lane_major_staged.py then go through the arrangement).  Deselected with -k, because
    they start pytest themselves: test_fm_disc.py::test_fm_disc_other_forms, test_gpu_lane_major_staged.py::
    test_polar_lockin_on_the_staged_kernel_without_the_row_split and ::test_every_lanes_per_wave_form_on_the_ragged_shapes.  Calls a
    file makes on the engine directly (error paths, `test_concurrent_streams_distinct_states`, the unaligned-base cases) stay as
    they are.
  * direct cases for entries that do not go through `GpuBackend`, two consecutive calls on one state, bit for bit with the state.
  * two callers that share the thread's one second stream (idsp_amd/csrc/common.h `side_stream`).
  * asynchrony probe: the second call of a shape is armed at the first attempt with the base delay.

REPLAYS below holds, per file, the entries that must have been armed and the blind calls allowed.  The blind calls, read off the tallies:
test_gpu_parity.py 4 -- test_empty_and_error_paths' three rejected calls (frac = 32, layout 7, nine cascade sections: x and the state
are zeros, nothing is launched) and test_atan2_parity_all_octants' empty call; test_gpu_cic.py 2 -- the two rejected calls of
test_cic_errors_and_helpers (zeros); test_fm_disc.py 2 -- the rejected frac = 32 call of test_fm_disc_gpu_parity, once per layout
(zeros).  Every other call of the eight files has an input or a state that differs from the decoy.

Measured on an MI355X, one run each (profiles/NOTES.md, "The caller's stream"): pytest's own time of the plain file / wall time of the
replay case (interpreter start included) / calls, armed at first try, retried, blind; bound = 2 x plain + calls x 80 us:
    test_gpu_parity.py             10.40 s / 13.36 s / 5883, 5831, 52, 4
    test_gpu_bylane.py              3.96 s /  5.74 s / 1235, 1231, 4, 0
    test_gpu_cic.py                 2.59 s /  4.05 s / 362, 352, 10, 2
    test_gpu_normal_wdf.py          2.79 s /  5.05 s / 289, 284, 5, 0
    test_fm_disc.py                 2.84 s /  4.32 s / 94, 92, 2, 2
    test_gpu_duo.py                15.68 s / 18.31 s / 124, 89, 35, 0
    test_gpu_round_split.py         2.79 s /  4.93 s / 18, 1, 17, 0
    test_gpu_lane_major_staged.py   2.89 s /  4.45 s / 487, 473, 14, 0"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from idsp_amd import _abi
from tests import _harness as H

pytestmark = pytest.mark.gpu
FM, LM = H.FM, H.LM
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


def _child(code, env=None, timeout=600):
    return subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, **(env or {})), capture_output=True, text=True, timeout=timeout)


# ---------------------------------------------------------------------------------------------------------------- control
def control_child(priority=0):
    """in a process of its own: biquad_i32_df1, 1000 lanes x 64 frames, FrameMajor, under the arrangement but with stream = NULL"""
    import torch

    from tests import _on_stream as OS
    from tests._guard import Guards

    o, e = H.oracle(), H.engine()
    rng = np.random.default_rng(1)
    lanes, frames = 1000, 64
    cfg = H.biquad_i32([(rng.integers(-(1 << 29), 1 << 29, size=5).tolist(), 29)])
    x = rng.integers(-(1 << 30), 1 << 30, size=(frames, lanes), dtype=np.int32)
    st = rng.integers(0, 1 << 32, size=(4, lanes), dtype=np.uint64).astype(np.uint32)
    true_y, decoy_y = np.empty_like(x), np.empty_like(x)
    assert o.stream("biquad_i32_df1", cfg, 1, st.copy(), x, true_y, lanes, frames, FM) == 0
    assert o.stream("biquad_i32_df1", cfg, 1, np.zeros_like(st), np.zeros_like(x), decoy_y, lanes, frames, FM) == 0
    out = {"armed": False, "first": None}
    for null_stream in (False, True):  # the first run loads the code object and shows that the same call on S is right
        c = OS.Call("biquad_i32_df1 (control)", Guards(DEV), OS.Arrangement(priority))
        xs, ys, ss = c.stage("x", x, readonly=True), c.out("y", x.size, torch.int32, -77), c.stage("state", st)
        c.read(ys)
        try:
            rc, (y,) = c.run(lambda s: e.stream("biquad_i32_df1", cfg, 1, ss, xs, ys, lanes, frames, FM, s), null_stream=null_stream)
        except OS.NotArmed as err:
            out["error"] = str(err)
            break
        y = y.view(np.int32).reshape(x.shape)
        torch.cuda.synchronize()
        key = "null" if null_stream else "on S"
        out[key] = {"rc": rc, "is_decoy": bool(np.array_equal(y, decoy_y)), "is_true": bool(np.array_equal(y, true_y)), "poison_left": int((y == -77).sum())}
        out["armed"], out["first"] = bool(c.armed), c.first
    print("CONTROL " + json.dumps(out))


def test_control_a_launch_on_the_null_stream_loses(gpu):
    r = _child("from tests.test_gpu_callers_stream import control_child; control_child()")
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("CONTROL ")][-1][8:])
    assert out["armed"] and "error" not in out, out
    assert out["on S"] == {"rc": 0, "is_decoy": False, "is_true": True, "poison_left": 0}, out
    assert out["null"]["rc"] == 0 and out["null"]["is_decoy"] and not out["null"]["is_true"], out


# ---------------------------------------------------------------------------------------------------------------- replays
BIQUADS = ["biquad_i32_df1", "biquad_i32_df1_clamp", "biquad_i32_dither", "biquad_i32_dither_clamp", "biquad_i32_wide", "biquad_i32_wide_clamp",
           "biquad_f32_df1", "biquad_f32_df1_clamp", "biquad_f32_df2t", "biquad_f32_df2t_clamp",
           "biquad_f64_df1", "biquad_f64_df1_clamp", "biquad_f64_df2t", "biquad_f64_df2t_clamp"]
# file -> (-k expression or None, entries that must have been armed at least once, blind calls allowed)
REPLAYS = {
    "tests/test_gpu_parity.py": (None, BIQUADS + ["cascade_i32_df1", "cascade_f32_df1", "cascade_f64_df1", "hbf_dec_f32", "hbf_int_f32", "fir_sym_f32_process",
                                                  "cossin_i32", "atan2_i32", "dds_i32", "lowpass_i32", "lockin_i32_process", "lockin_i32_arg", "lockin_i32_norm_sqr"], 4),
    "tests/test_gpu_bylane.py": (None, [b + "_bylane" for b in BIQUADS], 0),
    "tests/test_gpu_cic.py": (None, ["cic_dec_i32", "cic_dec_i64", "cic_int_i32", "cic_int_i64"], 2),
    "tests/test_gpu_normal_wdf.py": (None, ["normal_i32_df1", "normal_f32_df1", "normal_f64_df1", "wdf_i32"], 0),
    "tests/test_fm_disc.py": ("not other_forms", ["fm_disc_i32"], 2),
    "tests/test_gpu_duo.py": (None, ["biquad_i32_df1_pitch", "biquad_f32_df2t_pitch", "cascade_i32_df1_pitch", "cascade_f32_df1_pitch", "wdf_i32",
                                     "biquad_i32_df1_bylane", "biquad_f32_df1_bylane"], 0),
    "tests/test_gpu_round_split.py": (None, ["biquad_i32_df1_pitch", "biquad_f32_df1_pitch", "biquad_i32_df1_bylane", "biquad_f32_df2t_clamp_bylane"], 0),
    "tests/test_gpu_lane_major_staged.py": ("not without_the_row_split and not every_lanes_per_wave_form",
                                            [b + "_pitch" for b in BIQUADS] + ["cascade_i32_df1", "cascade_f32_df1", "cascade_f64_df1", "normal_i32_df1", "normal_f32_df1",
                                                                              "lowpass_i32", "dds_i32", "lockin_i32_arg"], 0),
}


@pytest.mark.parametrize("path", list(REPLAYS))
def test_replay_on_the_callers_stream(gpu, path, tmp_path):
    deselect, entries, blind_allowed = REPLAYS[path]
    tally_file = str(tmp_path / "tally.json")
    env = dict(os.environ, IDSP_TEST_STREAM="1", IDSP_TEST_STREAM_TALLY=tally_file)
    cmd = [sys.executable, "-m", "pytest", path, "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider"] + (["-k", deselect] if deselect else [])
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0 and " passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    with open(tally_file) as f:
        t = json.load(f)
    print("TALLY", path, json.dumps({k: t[k] for k in ("calls", "armed_first", "retried", "blind", "median_host_us", "p99_host_us", "max_host_us")}), json.dumps(t["entries"]))
    assert t["calls"] == t["armed_first"] + t["retried"] > 0, t
    missing = [e for e in entries if t["entries"].get(e, {}).get("armed", 0) < 1]
    assert not missing, (missing, sorted(t["entries"]))
    assert t["blind"] <= blind_allowed, {e: v["blind"] for e, v in t["entries"].items() if v["blind"]}


# ----------------------------------------------------------------------------------------------------------- direct cases
def run_two(entry, st0, ins, ynum, ytd, fill, gpu_call, ref_call):
    """Two consecutive calls of `entry` on one state under the arrangement, each against the oracle bit for bit, state included.
    ins: per call {role: numpy} of read-only inputs; gpu_call(state, {role: tensor}, y, stream) -> rc; ref_call(state, {role: numpy}) ->
    y (numpy; advances the state).  -> the Call objects"""
    import torch

    from tests import _on_stream as OS
    from tests._guard import Guards

    e = H.engine()
    so, sg, calls = st0.copy(), st0.copy(), []
    for rep in range(2):
        want = ref_call(so, ins[rep])
        g = Guards(DEV)
        c = OS.Call(entry, g)
        ts = {k: c.stage(k, v, readonly=True) for k, v in ins[rep].items()}
        y, s = c.read(c.out("y", ynum, ytd, fill)), c.read(c.stage("state", sg))
        rc, (yb, sb) = c.run(lambda strm: gpu_call(s, ts, y, strm))
        torch.cuda.synchronize()
        g.check((entry, rep, e.last_kernel()))
        assert rc == 0, (entry, e.err())
        sg = sb.view(np.uint32).reshape(st0.shape)
        assert np.array_equal(yb, np.ascontiguousarray(want).reshape(-1).view(np.uint8)), (entry, rep, e.last_kernel())
        assert np.array_equal(sg, so), (entry, rep, "state", e.last_kernel())
        calls.append(c)
    return calls


@pytest.mark.parametrize("layout", [FM, LM])
@pytest.mark.parametrize("name", ["hbf_dec_f64", "hbf_int_f64", "fir_sym_f64_process"])
def test_f64_half_band_and_fir(gpu, name, layout):
    import torch

    from tests.test_gpu_hbf_f64 import state_f64

    o, e = H.oracle(), H.engine()
    rng = np.random.default_rng(2000 + layout)
    lanes, frames = 17, 40
    if name.startswith("hbf"):
        kind = name[4:7]
        cfg = _abi.HbfCascadeF64()
        assert o.fn[f"hbf_{kind}_cascade_f64"](0, 2, C.byref(cfg)) == 0
        words = o.fn[f"hbf_{kind}_state_words_f64"](C.byref(cfg))
        nin, nout = (frames * 4, frames) if kind == "dec" else (frames, frames * 4)
    else:
        cfg = _abi.FirSymF64()
        cfg.kind, cfg.m = 0, 23
        for k, v in enumerate(rng.standard_normal(23) * 0.3):
            cfg.taps[k] = v
        words = o.fn["fir_sym_state_words_f64"](C.byref(cfg))
        nin = nout = frames

    def ref(so, i):
        yo = np.empty(lanes * nout)
        assert o.cfgcall(name, cfg, so, i["x"], yo, lanes, frames, layout) == 0
        return yo

    run_two(name, state_f64(rng, words, lanes), [{"x": rng.standard_normal(lanes * nin)} for _ in range(2)], lanes * nout, torch.float64, float("nan"),
            lambda s, t, y, strm: e.cfgcall(name, cfg, s, t["x"], y, lanes, frames, layout, strm), ref)


@pytest.mark.parametrize("layout", [FM, LM])
@pytest.mark.parametrize("lanes,frames", [(200, 257), (1024, 64)])
@pytest.mark.parametrize("name", ["lockin_i32_biquad_process", "lockin_i32_lo_process", "lockin_i32_biquad_lo_process", "lockin_f32_biquad_lo_process"])
def test_lockin_generic(gpu, name, lanes, frames, layout):
    import torch

    from tests import _lockin_generic_cases as G

    o, e = H.oracle(), H.engine()
    rng = np.random.default_rng(3000 + layout + lanes)
    n, f32 = 2, name.startswith("lockin_f32")
    lo_form = "_lo_" in name
    if name == "lockin_i32_lo_process":
        cfg, n = H.lockin_cfg([[1 << 22, -(1 << 27)]] * 2), None
        words = o.fn["lockin_state_words"](C.byref(cfg)) - 2
    else:
        cfg = (G.sections_f32 if f32 else G.sections_i32)(n, rng)[0]
        words = 8 * n + (0 if lo_form else 2)
    if f32:
        st = rng.standard_normal((words, lanes)).astype(np.float32).view(np.uint32)
        ins = [{"x": rng.standard_normal(lanes * frames).astype(np.float32), "lo": rng.standard_normal(lanes * frames * 2).astype(np.float32)} for _ in range(2)]
    else:
        st = rng.integers(-(1 << 20), 1 << 20, (words, lanes)).astype(np.int32).view(np.uint32)
        ins = [{"x": rng.integers(-(1 << 28), 1 << 28, lanes * frames, dtype=np.int32),
                "lo": rng.integers(-(1 << 31), (1 << 31) - 1, lanes * frames * 2, dtype=np.int64).astype(np.int32)} for _ in range(2)]
    if not lo_form:
        ins = [{"x": i["x"]} for i in ins]
    ydt = np.float32 if f32 else np.int32

    def ref(so, i):
        yo = np.empty(lanes * frames * 2, ydt)
        rc = G.call_lo(o, name, cfg, n, so, i["x"], i["lo"], yo, lanes, frames, layout, False) if lo_form else o.stream(name, cfg, n, so, i["x"], yo, lanes, frames, layout)
        assert rc == 0
        return yo

    def call(s, t, y, strm):
        if lo_form:
            return G.call_lo(e, name, cfg, n, s, t["x"], t["lo"], y, lanes, frames, layout, True, strm)
        return e.stream(name, cfg, n, s, t["x"], y, lanes, frames, layout, strm)

    run_two(name, st, ins, lanes * frames * 2, torch.float32 if f32 else torch.int32, -77, call, ref)


@pytest.mark.parametrize("layout", [FM, LM])
def test_pitch_twin_of_a_stream_entry(gpu, layout):
    """biquad_f32_df2t_pitch, five sections (two passes, the second in place on the padded y), rows padded by 5 / 9 elements, 3 elements in"""
    from tests import _on_stream as OS
    from tests import test_gpu_pitch as P

    o = H.oracle()
    rng = np.random.default_rng(4000 + layout)
    op, cfg, n, words, dt = [c for c in P.cases(rng) if c[0] == "biquad_f32_df2t" and c[2] == 5][0]
    lanes, frames, xpad, ypad, off = 70, 130, 5, 9, 3
    row, rows = (frames, lanes) if layout == LM else (lanes, frames)
    so = P.init_state(rng, dt, words * n, lanes)
    sg = so.copy()
    for rep in range(2):
        xh = P.sample(rng, dt, lanes * frames).reshape(rows, row)
        want = np.empty_like(xh)
        assert o.stream(op, cfg, n, so, xh, want, lanes, frames, layout) == 0
        full, decoy = (np.full(rows * (row + xpad) + off, P.SENT, dtype=dt) for _ in range(2))
        full[off:].reshape(rows, row + xpad)[:, :row], decoy[off:].reshape(rows, row + xpad)[:, :row] = xh, 0
        rc, yh, sg, _ = OS.pitch_call(gpu, op + "_pitch", cfg, n, sg, full, decoy, off, row + xpad, row + ypad, rows * (row + ypad) + off, lanes, frames, layout,
                                      False, P.SENT)
        assert rc == 0, gpu.err()
        yv = yh[off:].reshape(rows, row + ypad)
        assert np.array_equal(yv[:, :row].view(np.uint8), want.view(np.uint8)) and np.array_equal(sg, so), (layout, rep)
        assert (yv[:, row:] == P.SENT).all() and (yh[:off] == P.SENT).all(), "padding of y must stay untouched"


@pytest.mark.parametrize("layout", [FM, LM])
def test_pitch_twin_of_a_bylane_entry(gpu, layout):
    """biquad_i32_df1_bylane_pitch, three sections (two passes of at most two), rows padded by 8 / 20 elements"""
    import torch

    from tests import _bylane_cases as B
    from tests import _on_stream as OS
    from tests._backends import OracleBackend
    from tests._guard import Guards
    from tests.test_gpu_pitch import SENT

    ob = OracleBackend()
    rng = np.random.default_rng(4100 + layout)
    op, lanes, frames, nsec, frac, words = "biquad_i32_df1", 300, 41, 3, 29, 4
    row, rows = (frames, lanes) if layout == LM else (lanes, frames)
    xp, yp = row + 8, row + 20
    coef = B.coef_planes(rng, np.int32, nsec, lanes, False, frac)
    so = B.init_state(rng, np.int32, words * nsec, lanes)
    sg = so.copy()
    for rep in range(2):
        xh = B.samples(rng, np.int32, lanes * frames)
        rc, want = ob.bylane(op, coef, frac, nsec, so, xh, lanes, frames, layout)
        assert rc == 0
        full, decoy = (np.full((rows, xp), SENT, dtype=np.int32) for _ in range(2))
        full[:, :row], decoy[:, :row] = np.asarray(xh).reshape(rows, row), 0
        g = Guards(DEV)
        c = OS.Call(op + "_bylane_pitch", g)
        xb, cd = c.stage("x", full, readonly=True, decoy=decoy), c.stage("coef", coef, readonly=True)
        yb, sd = c.read(c.out("y", rows * yp, torch.int32, SENT)), c.read(c.stage("state", sg))
        rc, (yh, sh) = c.run(lambda s: gpu.fn[op + "_bylane_pitch"](H._ptr(cd), frac, nsec, H._ptr(sd), H._ptr(xb), xp, H._ptr(yb), yp, lanes, frames, layout, s))
        torch.cuda.synchronize()
        g.check((op, layout, rep))
        assert rc == 0, gpu.err()
        yv, sg = yh.view(np.int32).reshape(rows, yp), sh.view(np.uint32).reshape(so.shape)
        assert np.array_equal(yv[:, :row], np.asarray(want).reshape(rows, row)) and np.array_equal(sg, so), (layout, rep)
        assert (yv[:, row:] == SENT).all()


@pytest.mark.parametrize("what", ["wdf_i32 x 6", "cascade_f32_df1 x 8", "biquad_f32_df1 x 6"])
def test_chains_in_place(gpu, what):
    """300 lanes x 200 frames, in place, both layouts: six Wdf sections and six biquad sections are two passes (four, then two in place
    on y); a `Cascade` is one launch whatever its length (1 .. 8 sections, idsp_amd/csrc/biquad_host.h `run_cascade`), so its longest
    stands here."""
    from tests import _nw_cases as W
    from tests._backends import GpuBackend, OracleBackend

    ob, gb = OracleBackend(), GpuBackend(on_stream=True)
    rng = np.random.default_rng(5000)
    lanes, frames = 300, 200
    op, k = what.split(" x ")
    k = int(k)
    if op == "wdf_i32":
        cfg = W.wdf_array(W.random_wdf(rng, k))
        words = gb.helper("wdf_state_words", C.cast(cfg, C.c_void_p), k)
        mk = lambda: rng.integers(W.I32_MIN, W.I32_MAX, size=lanes * frames, dtype=np.int64, endpoint=True).astype(np.int32)  # noqa: E731
        init = rng.integers(0, 1 << 32, size=(words, lanes), dtype=np.uint64).astype(np.uint32)
    else:
        cfg = H.biquad_f32([(rng.standard_normal(5) * 0.3).tolist() for _ in range(k)])
        words = 2 + 2 * k if op.startswith("cascade") else 4 * k
        mk = lambda: rng.standard_normal(lanes * frames).astype(np.float32)  # noqa: E731
        init = rng.standard_normal((words, lanes)).astype(np.float32).view(np.uint32)
    for layout in (FM, LM):
        so, sg = init.copy(), init.copy()
        for rep in range(2):
            x = mk()
            rco, yo = ob.stream(op, cfg, k, so, x.copy(), lanes, frames, layout, inplace=True)
            rcg, yg = gb.stream(op, cfg, k, sg, x.copy(), lanes, frames, layout, inplace=True)
            assert rco == 0 and rcg == 0, gpu.err()
            assert gb.last_call.armed and not gb.last_call.blind
            assert np.array_equal(yo.view(np.uint32), yg.view(np.uint32)) and np.array_equal(so, sg), (what, layout, rep, gpu.last_kernel())


def test_fm_disc_lane_major_body_and_tail(gpu):
    """(130, 48) LaneMajor: the whole 32-frame tile of every row on the role-wave kernel, the last 16 frames on the tile kernel behind it"""
    from tests.test_fm_disc import _cfg, _x
    from tests._backends import GpuBackend, OracleBackend

    ob, gb = OracleBackend(), GpuBackend(on_stream=True)
    rng = np.random.default_rng(6000)
    lanes, frames = 130, 48
    cfg = _cfg(rng)
    init = np.zeros((7, lanes), np.uint32)
    init[0, ::3] = 1
    init[1:] = rng.integers(0, 1 << 32, size=(6, lanes), dtype=np.uint64).astype(np.uint32)
    so, sg = init.copy(), init.copy()
    for rep in range(2):
        x = _x(rng, lanes * frames)
        rco, yo = ob.cfgcall("fm_disc_i32", cfg, so, x, (lanes * frames,), np.int32, lanes, frames, LM)
        rcg, yg = gb.cfgcall("fm_disc_i32", cfg, sg, x, (lanes * frames,), np.int32, lanes, frames, LM)
        assert rco == 0 and rcg == 0, gpu.err()
        k = gpu.last_kernel()
        assert k.startswith("fm_disc_waves_lm_kernel") and k.endswith("(last frames % 32)"), k
        assert np.array_equal(yo, yg) and np.array_equal(so, sg), rep


# ------------------------------------------------------------------------------------------- two callers, one second stream
def test_two_callers_share_the_threads_second_stream(gpu):
    """Two streams, each with its own delay, buffers and state; three calls each of biquad_i32_df1 at 65536 + 8192 lanes x 64 frames
    (whole rounds + remainder on the second stream) interleaved call by call, and on the second caller's stream clamp_wrap_i32 at 65540
    lanes (the last lanes % 4 on the second stream) behind them: the fork and join events of the one side stream are re-recorded by every
    call, for both callers in turn."""
    import torch

    from tests import _on_stream as OS
    from tests import _stream_proc_cases as SP
    from tests.test_gpu_pitch import cases
    from tests.test_gpu_round_split import is_split

    o = H.oracle()
    rng = np.random.default_rng(7000)
    op, cfg, n, words, dt = [c for c in cases(rng) if c[0] == "biquad_i32_df1" and c[2] == 1][0]
    lanes, frames, calls = 65536 + 8192, 64, 3
    xs = [rng.integers(-(1 << 30), 1 << 30, size=(frames, lanes), dtype=np.int32) for _ in range(2)]
    sts = [rng.integers(0, 1 << 32, size=(4, lanes), dtype=np.uint64).astype(np.uint32) for _ in range(2)]
    wants = []
    for x, st in zip(xs, sts):
        so, y = st.copy(), np.empty_like(x)
        for _ in range(calls):  # the same x three times, the state carried on
            assert o.stream(op, cfg, 1, so, x, y, lanes, frames, FM) == 0
        wants.append((y, so))
    cl, cf = 65540, 64
    ccfg, cx, cst = SP.make_inputs("clamp", cl, cf, 7001)
    cafter = cst.copy()
    cwant = SP.spec_run("clamp", ccfg, cafter, cx, cf)
    arrs = [OS.Arrangement(), OS.Arrangement()]
    for attempt in range(OS.ATTEMPTS):
        cs, bufs = [], []
        for i in range(2):
            c = OS.Call(f"{op} (caller {i})", arr=arrs[i])
            xd, yd, sd = (torch.empty((frames, lanes), dtype=torch.int32, device=DEV), torch.empty((frames, lanes), dtype=torch.int32, device=DEV),
                          torch.empty((4, lanes), dtype=torch.int32, device=DEV))
            c.load(xd, xs[i]), c.load(sd, sts[i]), c.poison(yd, -77), c.read(yd), c.read(sd)
            cs.append(c), bufs.append((xd, yd, sd))
        cxd, cyd, csd = (torch.empty((cf, cl), dtype=torch.int32, device=DEV), torch.empty((cf, cl), dtype=torch.int32, device=DEV),
                         torch.empty(cst.shape, dtype=torch.int32, device=DEV))
        cs[1].load(cxd, cx), cs[1].load(csd, cst.view(np.int32)), cs[1].poison(cyd, SP.POISON), cs[1].read(cyd), cs[1].read(csd)
        for c in cs:
            c.prepare()
        torch.cuda.synchronize()
        for c in cs:
            c.open(OS.DELAY_US * (8 << attempt))  # seven calls and the copies of two callers behind one delay each
        kernels = []
        for _ in range(calls):
            for c, (xd, yd, sd) in zip(cs, bufs):
                assert c.launch(lambda s: gpu.stream(op, cfg, 1, sd, xd, yd, lanes, frames, FM, s)) == 0, gpu.err()
                kernels.append(gpu.last_kernel())
        assert cs[1].launch(lambda s: SP.call_form(gpu, "clamp", ccfg, csd.data_ptr(), cxd.data_ptr(), cyd.data_ptr(), cl, cf, FM, stream=s.value)) == 0, gpu.err()
        armed = [not c.event.query() for c in cs]  # both delays still running now that every call has returned
        kernels.append(gpu.last_kernel())
        for c in cs:
            c.close()
        got = [c.collect() for c in cs]
        torch.cuda.synchronize()
        if all(armed):
            break
    assert all(armed), ("a call blocked the host", armed)
    assert all(is_split(k) for k in kernels[:-1]) and "second stream" in kernels[-1], kernels
    for i in range(2):
        y, s = got[i][0].view(np.int32).reshape(frames, lanes), got[i][1].view(np.uint32).reshape(4, lanes)
        assert np.array_equal(y, wants[i][0]) and np.array_equal(s, wants[i][1]), f"caller {i}"
    assert np.array_equal(got[1][2].view(np.int32).reshape(cwant.shape), cwant) and np.array_equal(got[1][3].view(np.uint32).reshape(cst.shape), cafter), "clamp_wrap_i32"


# ------------------------------------------------------------------------------------------------------- asynchrony probe
def _probe(gb, ob, entry, rng):
    """-> (run(back end, state, rng of the inputs) -> (rc, y), the initial state) for one shape of `entry`"""
    if entry == "biquad_f32_df2t":
        lanes, frames = 1000, 64
        cfg = H.biquad_f32([(rng.standard_normal(5) * 0.3).tolist()])
        st = rng.standard_normal((2, lanes)).astype(np.float32).view(np.uint32)
        return (lambda be, s, r: be.stream(entry, cfg, 1, s, r.standard_normal(lanes * frames).astype(np.float32), lanes, frames, FM)), st
    if entry == "wdf_i32":
        from tests import _nw_cases as W

        lanes, frames = 1000, 64
        cfg = W.wdf_array(W.random_wdf(rng, 2))
        st = rng.integers(0, 1 << 32, size=(gb.helper("wdf_state_words", C.cast(cfg, C.c_void_p), 2), lanes), dtype=np.uint64).astype(np.uint32)
        return (lambda be, s, r: be.stream(entry, cfg, 2, s, r.integers(-(1 << 31), 1 << 31, size=lanes * frames, dtype=np.int64).astype(np.int32), lanes, frames, FM)), st
    if entry == "hbf_dec_f32":
        lanes, frames = 300, 64
        cfg = _abi.HbfCascadeF32()
        assert H.oracle().fn["hbf_dec_cascade"](0, 2, C.byref(cfg)) == 0
        st = rng.standard_normal((H.oracle().fn["hbf_dec_state_words"](C.byref(cfg)), lanes)).astype(np.float32).view(np.uint32)
        return (lambda be, s, r: be.cfgcall(entry, cfg, s, r.standard_normal(lanes * frames * 4).astype(np.float32), (lanes * frames,), np.float32, lanes, frames, FM)), st
    if entry == "cic_dec_i64":
        from tests import _cic_cases as K

        lanes, frames = 300, 64
        cfg = _abi.Cic(3, 1, 7)
        st = K.random_state(rng, K.state_words(ob, cfg, np.int64), lanes)
        return (lambda be, s, r: K.run(be, "dec", np.int64, cfg, s, K.samples(r, np.int64, lanes * frames * 8), lanes, frames, FM)), st
    if entry == "lockin_i32_process":
        lanes, frames = 1000, 64
        cfg = H.lockin_cfg([[1 << 22, -(1 << 27)]] * 2)
        st = rng.integers(0, 1 << 32, size=(H.oracle().fn["lockin_state_words"](C.byref(cfg)), lanes), dtype=np.uint64).astype(np.uint32)
        assert st.shape[0] == 2 + 2 * 2 * 2 * 2  # phase and frequency, then two arms of `cascade` low-passes of `order` two-word integrators
        return (lambda be, s, r: be.cfgcall(entry, cfg, s, r.integers(-(1 << 28), 1 << 28, lanes * frames, dtype=np.int32), (lanes * frames * 2,), np.int32, lanes, frames, FM)), st
    from tests.test_fm_disc import _cfg, _x

    assert entry == "fm_disc_i32"
    lanes, frames = 1000, 64
    cfg = _cfg(rng)
    st = rng.integers(0, 1 << 32, size=(7, lanes), dtype=np.uint64).astype(np.uint32)
    st[0] = 1
    return (lambda be, s, r: be.cfgcall(entry, cfg, s, _x(r, lanes * frames), (lanes * frames,), np.int32, lanes, frames, FM)), st


@pytest.mark.parametrize("entry", ["biquad_f32_df2t", "hbf_dec_f32", "cic_dec_i64", "lockin_i32_process", "wdf_i32", "fm_disc_i32"])
def test_second_call_does_not_wait_for_the_device(gpu, entry):
    """One entry of each launcher family: the first call of a shape may load a code object (and is then retried with a longer delay);
    the second is armed at the first attempt with the base delay -- the call returned while the device-side delay in front of its
    inputs was still running, so nothing inside it waits for the stream."""
    from tests._backends import GpuBackend, OracleBackend

    ob, gb = OracleBackend(), GpuBackend(on_stream=True)
    run, so = _probe(gb, ob, entry, np.random.default_rng(8000))
    sg = so.copy()
    for seed in (1, 2):
        rco, yo = run(ob, so, np.random.default_rng(seed))
        rcg, yg = run(gb, sg, np.random.default_rng(seed))
        assert rco == 0 and rcg == 0, (entry, gpu.err())
        assert np.array_equal(np.asarray(yo).view(np.uint8), np.asarray(yg).view(np.uint8)) and np.array_equal(so, sg), (entry, seed)
    assert gb.last_call.first and gb.last_call.armed and not gb.last_call.blind, (entry, gb.last_call.host_us)
