"""The `stream` argument of the entries added since the biquad family: each is launched three times back to back on a stream of the
caller's, on one state, and the last output and the state are read back ON THAT STREAM, asynchronously, with no device-wide
synchronisation anywhere.  The inputs are uploaded on the same stream, so a launch that went to the null stream instead, or a call
that forks to the library's second stream and forgets the join (idsp_clamp_wrap_i32 at 65540 lanes is a round split,
idsp_amd/csrc/lane_stream.h), is not ordered behind its inputs or in front of the read-back.

As tests/test_gpu_round_split.py::test_call_stays_ordered_on_the_callers_stream does for the biquad.  (A race need not lose: the
test cannot prove the ordering, it can only catch its absence.)"""
import ctypes as C

import numpy as np
import pytest
import torch

from idsp_amd import _abi
from tests import _cordic_spec as CS
from tests import _float_special as F
from tests import _pfb_spec as PF
from tests import _rpll_spec as RS
from tests import _stream_proc_cases as SP
from tests import test_gpu_pfb as TP

pytestmark = pytest.mark.gpu
FM = SP.FM
CALLS = 3


def pinned(shape, dtype):
    """a pinned host buffer, made BEFORE the launches: pinning takes milliseconds, the kernels tens of microseconds"""
    return torch.empty(tuple(shape), dtype=dtype).pin_memory()


def queue_copies(hosts, tensors):
    """inside the caller's stream context, directly behind the last call: asynchronous copies on that stream, nothing else in between"""
    for h, t in zip(hosts, tensors):
        h.copy_(t, non_blocking=True)


@pytest.mark.parametrize("form,lanes,frames", [("clamp", 65540, 64), ("pll2", 1000, 256), ("rpll", 1000, 256), ("sweep", 1000, 256)])
def test_stream_processors(gpu, form, lanes, frames):
    cfg, x, st = SP.make_inputs(form, lanes, CALLS * frames, 900 + SP.FORMS.index(form))
    after = st.copy()
    want = SP.spec_run(form, cfg, after, x, CALLS * frames)
    s = torch.cuda.Stream()
    width = SP.out_width(form)
    hosts = [pinned((frames * lanes * width,), torch.int32), pinned(st.shape, torch.int32)]
    with torch.cuda.stream(s):
        sd = torch.from_numpy(st.view(np.int32)).to("cuda")
        xs = [None] * CALLS if x is None else [torch.from_numpy(np.ascontiguousarray(x[i * frames:(i + 1) * frames])).to("cuda") for i in range(CALLS)]
        yd = torch.full((frames * lanes * width,), SP.POISON, dtype=torch.int32, device="cuda")
        rcs = []
        for i in range(CALLS):
            rc = SP.call_form(gpu, form, cfg, sd.data_ptr(), None if xs[i] is None else xs[i].data_ptr(), yd.data_ptr(), lanes, frames, FM, stream=s.cuda_stream)
            rcs.append(rc)
        queue_copies(hosts, (yd, sd))
    s.synchronize()
    assert rcs == [0] * CALLS, (rcs, gpu.err())
    k = gpu.last_kernel()
    y, sg = (h.numpy() for h in hosts)
    e = SP.expected_kernel(form, FM, lanes, frames)
    assert k.startswith(e) and k.endswith(e.suffix or ">"), (k, e, e.suffix)
    if form == "clamp":
        assert "second stream" in k, k
    assert np.array_equal(y.reshape(want[-frames:].shape), want[-frames:]), (form, k)
    assert np.array_equal(sg.view(np.uint32), after), (form, k, "state")


def test_accu_lo(gpu):
    lanes, updates, lo_cfg = 1000, 256, (2, 3, 12345)
    rng = np.random.default_rng(910)
    accu = [RS.adversarial_accu(rng, updates, lanes) for _ in range(CALLS)]
    want = RS.accu_lo_np(lo_cfg, accu[-1])
    s = torch.cuda.Stream()
    hosts = [pinned(((updates << lo_cfg[0]) * lanes * 2,), torch.int32)]
    rcs = []
    with torch.cuda.stream(s):
        ads = [torch.from_numpy(a).to("cuda") for a in accu]
        ld = torch.full(((updates << lo_cfg[0]) * lanes * 2,), SP.POISON, dtype=torch.int32, device="cuda")
        for ad in ads:
            rc = gpu.fn["accu_lo_i32"](C.byref(_abi.AccuLo(*lo_cfg)), C.c_void_p(ad.data_ptr()), C.c_void_p(ld.data_ptr()), lanes, updates, FM, C.c_void_p(s.cuda_stream))
            rcs.append(rc)
        queue_copies(hosts, (ld,))
    s.synchronize()
    assert rcs == [0] * CALLS, (rcs, gpu.err())
    assert gpu.last_kernel() == "accu_lo_kernel[FrameMajor]"
    lo = hosts[0].numpy()
    assert np.array_equal(lo.reshape(want.shape), want)


def test_pfb(gpu):
    lanes, frames, taps = 1000, 256, 8
    rng = np.random.default_rng(911)
    coeff = rng.standard_normal((taps, 4)).astype(np.float32)
    st = PF.random_state(rng, taps, lanes)
    x = rng.standard_normal((CALLS * frames, lanes, 4, 2)).astype(np.float32)
    after = st.copy()
    want = PF.bank_np(coeff, 1, after, x)
    cfg = TP.make_cfg(coeff, 1)
    s = torch.cuda.Stream()
    hosts = [pinned((lanes * frames * 8,), torch.float32), pinned(st.shape, torch.int32)]
    rcs = []
    with torch.cuda.stream(s):
        sd = torch.from_numpy(st.view(np.int32)).to("cuda")
        xs = [torch.from_numpy(np.ascontiguousarray(x[i * frames:(i + 1) * frames]).reshape(-1)).to("cuda") for i in range(CALLS)]
        yd = torch.from_numpy(F.poison(lanes * frames * 8, np.float32)).to("cuda")
        for xd in xs:
            rc = gpu.fn["pfb_f32_process"](C.byref(cfg), C.c_void_p(sd.data_ptr()), C.c_void_p(xd.data_ptr()), C.c_void_p(yd.data_ptr()), lanes, frames, FM,
                                           C.c_void_p(s.cuda_stream))
            rcs.append(rc)
        queue_copies(hosts, (yd, sd))
    s.synchronize()
    assert rcs == [0] * CALLS, (rcs, gpu.err())
    assert gpu.last_kernel() == TP.NAMES[(FM, False)].format(T=TP.T, taps=taps)
    y, sg = (h.numpy() for h in hosts)
    TP.same(want[-frames:], y.reshape(frames, lanes, 4, 2), after, sg.view(np.uint32), ("stream argument",))


def test_cordic_cos_sin(gpu):
    n = 1000 * 256
    rng = np.random.default_rng(912)
    data = [(rng.integers(-(1 << 31), 1 << 31, size=(n, 2), dtype=np.int64).astype(np.int32), rng.integers(-(1 << 31), 1 << 31, size=n, dtype=np.int64).astype(np.int32))
            for _ in range(CALLS)]
    want = CS.function_np("cos_sin", *data[-1])
    s = torch.cuda.Stream()
    hosts = [pinned((n * 2,), torch.int32)]
    rcs = []
    with torch.cuda.stream(s):
        dev = [(torch.from_numpy(xy).to("cuda"), torch.from_numpy(z).to("cuda")) for xy, z in data]
        od = torch.full((n * 2,), SP.POISON, dtype=torch.int32, device="cuda")
        for xyd, zd in dev:
            rc = gpu.fn["cordic_cos_sin_i32"](C.c_void_p(xyd.data_ptr()), C.c_void_p(zd.data_ptr()), C.c_void_p(od.data_ptr()), n, C.c_void_p(s.cuda_stream))
            rcs.append(rc)
        queue_copies(hosts, (od,))
    s.synchronize()
    assert rcs == [0] * CALLS, (rcs, gpu.err())
    assert gpu.last_kernel() == "cordic_kernel<cos_sin>[four elements per thread]"
    out = hosts[0].numpy()
    assert np.array_equal(out.reshape(n, 2), want)
