"""The passes of a long chain on the device: one entry per family of tests/_biquad_pass_cases.py at kDuoMinLanes lanes x 33 frames, FRAME_MAJOR,
dense, out of place, each with more sections than one launch takes (the cascade: its full length).  Outputs and written-back state against
the oracle bit for bit — every pass has to start at its own sections' coefficients and state words and the later ones have to run in place
on y —, and the last launch on the kernel the table's last pass names (`idsp_last_kernel()` shows the last launch only; the schedule as a
whole is pinned on the CPU by tests/test_biquad_pass_plan.py).  Slice composition: dsp-process/src/compose.rs:43-77; `ByLane`: compose.rs:363-390;
`Cascade`: src/iir/biquad.rs:339-364; `Wdf`: src/iir/wdf.rs:178-214.  The 16-bit entry has no oracle entry: its reference is
tests/_biquad_i16_spec.py, as in tests/test_gpu_biquad_i16.py."""
import ctypes as C

import numpy as np
import pytest

from tests import _biquad_pass_cases as P
from tests import _harness as H
from tests.test_gpu_pitch import init_state, sample

pytestmark = pytest.mark.gpu
LANES, FRAMES = P.LO, 33
DUO = "stream_frame_major_duo<"


def _run(gpu, rng, entry, n):
    """one call of `entry` with n sections on both back ends -> (y, state) wanted, (y, state) got"""
    from tests._backends import GpuBackend, OracleBackend

    ob, gb = OracleBackend(), GpuBackend()
    if entry == "biquad_i16_df1":
        from tests import test_gpu_biquad_i16 as I16

        secs, x, st, want, want_st = I16._case(n, False, LANES, FRAMES, 612)
        y, got_st, _ = I16.run(gpu, secs, I16.FM, st, x)
        return (want, want_st), (y, got_st)
    if entry == "biquad_i32_df1_bylane":
        from tests import _bylane_cases as B

        coef = B.coef_planes(rng, np.int32, n, LANES, False, 29)
        x, init = B.samples(rng, np.int32, LANES * FRAMES), B.init_state(rng, np.int32, 4 * n, LANES)
        so, sg = init.copy(), init.copy()
        rco, yo = ob.bylane("biquad_i32_df1", coef, 29, n, so, x.copy(), LANES, FRAMES, H.FM)
        rcg, yg = gb.bylane("biquad_i32_df1", coef, 29, n, sg, x.copy(), LANES, FRAMES, H.FM)
    else:
        if entry == "wdf_i32":
            from tests import _nw_cases as W

            secs = W.random_wdf(rng, n)
            for sec in secs:  # orders 1 .. 4: the two-wave form
                sec.n = 1 + sec.n % 4
                sec.m &= (1 << (4 * sec.n)) - 1
            cfg = W.wdf_array(secs)
            words, dt = gb.helper("wdf_state_words", C.cast(cfg, C.c_void_p), n), np.int32
        elif entry == "biquad_f64_df1":
            cfg, words, dt = H.biquad_f64([(rng.standard_normal(5) * 0.3).tolist() for _ in range(n)]), 8 * n, np.float64
        elif entry == "biquad_i32_wide_clamp":
            cfg = H.biquad_clamp_i32([(rng.integers(-(1 << 29), 1 << 29, size=5).tolist(), 29, 77, -(1 << 28), 1 << 28) for _ in range(n)])
            words, dt = 6 * n, np.int32
        else:  # biquad_i32_df1, cascade_i32_df1
            cfg = H.biquad_i32([(rng.integers(-(1 << 28), 1 << 28, size=5).tolist(), 29) for _ in range(n)])
            words, dt = (2 + 2 * n if entry.startswith("cascade") else 4 * n), np.int32
        x, init = sample(rng, dt, LANES * FRAMES), init_state(rng, dt, words, LANES)
        so, sg = init.copy(), init.copy()
        rco, yo = ob.stream(entry, cfg, n, so, x.copy(), LANES, FRAMES, H.FM)
        rcg, yg = gb.stream(entry, cfg, n, sg, x.copy(), LANES, FRAMES, H.FM)
    assert rco == 0 and rcg == 0, H.engine().err()
    return (yo, so), (yg, sg)


@pytest.mark.parametrize("entry,family,n", P.GPU_ROWS, ids=["%s-%d" % (e, n) for e, _, n in P.GPU_ROWS])
def test_long_chains_against_the_oracle(gpu, entry, family, n):
    schedule = P.schedule_of(family, n)
    assert len(schedule) >= 2 or family == "cascade_i32", schedule
    (want, want_st), (got, got_st) = _run(gpu, np.random.default_rng(610 + n), entry, n)
    kernel = gpu.fn["last_kernel"]().decode()
    assert kernel.startswith(DUO) == (schedule[-1][1] != 0), (entry, n, schedule, kernel)
    assert np.array_equal(np.asarray(got).view(np.uint8), np.asarray(want).view(np.uint8)), (entry, n, kernel)
    assert np.array_equal(got_st, want_st), (entry, n, "state", kernel)
