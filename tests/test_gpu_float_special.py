"""Float kernels on signed zeros, subnormals, huge values, inf and NaN: HIP through the C ABI against the CPU oracle under
`assert_same_float` (identical NaN masks, every other element bit-identical, so +0 / -0 and subnormals count), on outputs
and on the written-back float state.  Both layouts, out of place and y == x, every call followed by a second one that
continues from the written-back state (which by then holds +-0, subnormals, inf and NaN).  Output buffers are filled with
a finite poison pattern that the expected output is asserted not to contain, so "every element was written" holds where
the expected value is NaN too.  Every case asserts the start of `idsp_last_kernel()`, so a dispatch change cannot silently
drop a kernel family from this coverage; the families reached are printed and checked at the end.

The cases, their inputs and the conditions they meet on the oracle are those of tests/_float_special.py, checked without a
GPU by tests/test_float_special_oracle.py."""
import time

import numpy as np
import pytest
import torch

from tests import _float_special as S
from tests.test_float_special_oracle import PARAMS, entry_cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REACHED = set()

# kernel families this module must keep reaching: the float-capable ones of tests/test_gpu_dispatch_table.py, the half-band kernels
# of its C3 shape, and the kernels that are an entry's only one.  The half-band wave and block kernels of the smaller shapes are
# printed with the rest.
FAMILIES = [
    "stream_frame_major_sweep[", "stream_frame_major_sweep + stream_frame_major_staged", "stream_frame_major_lds[", "stream_frame_major_few<",
    "stream_frame_major_staged[", "stream_frame_major_pair[", "stream_frame_major<", "stream_lane_major_staged", "stream_lane_major<",
    "hbf_dec_ring[FrameMajor]", "hbf_dec_blk[LaneMajor]", "hbf_dec_f64_kernel", "hbf_int_f64_kernel", "fir_sym_kernel", "fir_sym_f64_kernel",
    "lockin_waves_kernel",
]


def dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(DEV)


def run_gpu(gpu, case, inp, inplace):
    """[(y [frames, lanes, chunk], state uint32 [words, lanes], kernel name)] of the two consecutive calls on the GPU."""
    lanes, frames, pitch = case.lanes, case.frames, case.pitch
    st = dev(inp.state)
    coef = None if inp.coef is None else dev(inp.coef)
    out = []
    for x, lo in zip(inp.x, inp.lo):
        xf = S.to_flat(x, case.layout)
        if pitch:  # LaneMajor rows of `frames` samples at a pitch of `pitch`: the padding is poison and must stay so
            buf = S.poison(lanes * pitch, case.dtype).reshape(lanes, pitch)
            buf[:, :frames] = xf.reshape(lanes, frames)
            xf = buf.reshape(-1)
        xd = dev(xf)
        yd = xd if inplace else dev(S.poison(lanes * pitch if pitch else lanes * frames * case.rout, case.dtype))
        lod = None if lo is None else dev(S.to_flat(lo, case.layout))
        rc = S.invoke(gpu, True, case, inp, st, xd, lod, yd, coef=coef, pitch=pitch)
        torch.cuda.synchronize()
        assert rc == 0, (case.id, rc, gpu.err())
        kernel = gpu.last_kernel()
        y = yd.cpu().numpy()
        if pitch:
            y = y.reshape(lanes, pitch)
            assert (S.bits(y[:, frames:]) == S.POISON[case.dtype]).all(), (case.id, kernel, "row padding must stay untouched")
            y = np.ascontiguousarray(y[:, :frames]).reshape(-1)
        out.append((S.from_flat(y, case.layout, frames, lanes, case.rout), st.cpu().numpy().view(np.uint32).copy(), kernel))
    if coef is not None:
        assert np.array_equal(coef.cpu().numpy(), inp.coef), (case.id, "coefficients are read-only")
    return out


@pytest.mark.parametrize("table,entry", PARAMS, ids=[p[1] for p in PARAMS])
def test_hip_meets_oracle_on_special_values(gpu, table, entry):
    t0 = time.time()
    kernels, wrong = set(), []
    cases = entry_cases(table, entry)
    for case in cases:
        inp = S.prepare(case)
        want = S.run_oracle(case, inp)
        S.check_conditions(case, inp, want)
        for y, _ in want:
            S.assert_poison_absent(y, case.id)
        for inplace in (False, True) if case.inplace else (False,):
            got = run_gpu(gpu, case, inp, inplace)
            for rep, ((yo, so), (yg, sg, kernel)) in enumerate(zip(want, got)):
                what = f"{case.id} {'y == x' if inplace else 'out of place'} call {rep} [{kernel}]"
                kernels.add(kernel.split("<")[0] + "<")
                if " + stream_frame_major_few" in kernel:  # the last lanes % 4 lanes, on a second stream
                    kernels.add("stream_frame_major_few<")
                few = case.layout == S.FM and case.dtype == S.F32 and case.lanes == 65537  # lanes % 4 beside the rest
                if not kernel.startswith(case.kernel) or (few and not kernel.endswith(S.FEW)):
                    wrong.append((what, case.kernel))
                S.assert_same_float(yo, yg, what + ": output", S.where(case, inp, yo.shape))
                svo, svg = S.state_values(so, case.dtype), S.state_values(sg, case.dtype)
                S.assert_same_float(svo, svg, what + ": state", S.where(case, inp, svo.shape))
    REACHED.update(kernels)
    print(f"{entry}: {len(cases)} cases, {time.time() - t0:.1f} s, kernels {sorted(kernels)}")
    assert not wrong, (len(wrong), wrong[:10])


def test_kernel_families_reached():
    """Runs after the cases above (file order): the distinct kernel names they recorded, and the families that must be there."""
    print("kernel families reached:", sorted(REACHED))
    if not REACHED:
        pytest.fail("run this module as a whole: no case has run before this test")
    missing = [f for f in FAMILIES if not any(k.startswith(f) for k in REACHED)]
    assert not missing, missing
