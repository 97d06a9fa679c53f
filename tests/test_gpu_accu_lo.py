"""idsp_accu_lo_i32 on the GPU, through the C ABI, against the specification (tests/_rpll_spec.py, accu_lo_np — held to the
Python-integer restatement on oracle/spec.py's cossin in tests/test_rpll_spec.py).

Every output word is compared with array_equal; outputs start poisoned, every buffer sits between guard bands, the input is held
read-only.  Bases at 0 and 8 mod 16 and odd lane / frame counts put rows on and off the 16-byte grid of the kernel's stores."""
import ctypes as C

import numpy as np
import pytest
import torch

from idsp_amd import _abi
from idsp_amd._abi import RPLL  # the feature's prototype table
from tests import _harness as H
from tests import _rpll_spec as S
from tests._guard import Guards

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POISON = -77
KERNELS = {}

LANES = [1, 63, 64, 65, 1000, 16385]
UPDATES = [1, 3, 33]


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def to_layout(a, layout):
    return np.ascontiguousarray(a if layout == H.FM else np.swapaxes(a, 0, 1))


def from_layout(flat, layout, frames, lanes):
    a = flat.reshape((frames, lanes, 2) if layout == H.FM else (lanes, frames, 2))
    return np.ascontiguousarray(a if layout == H.FM else np.swapaxes(a, 0, 1))


def gpu_run(gpu, lo_cfg, accu, layout, off_in=0, off_out=0):
    """accu [updates, lanes, 2] int32 -> lo [updates << k, lanes, 2]; off_*: bytes between the 512-byte grid and the buffers"""
    updates, lanes = accu.shape[:2]
    frames = updates << lo_cfg[0]
    g = Guards(DEV)
    ad = g.upload("accu", to_layout(accu, layout), off=off_in, readonly=True)
    ld = g.full("lo", frames * lanes * 2, torch.int32, POISON, off=off_out)
    rc = gpu.fn["accu_lo_i32"](C.byref(_abi.AccuLo(*lo_cfg)), _ptr(ad), _ptr(ld), lanes, updates, layout, None)
    assert rc == 0, gpu.err()
    torch.cuda.synchronize()
    k = KERNELS[(layout, lanes, updates, lo_cfg[0])] = gpu.last_kernel()
    g.check((lo_cfg, layout, lanes, updates, off_in, off_out, k))
    assert "accu_lo" in k, k
    return from_layout(ld.cpu().numpy(), layout, frames, lanes)


@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("updates", UPDATES)
def test_equals_the_spec(gpu, lanes, updates):
    """every (lanes, updates) with k and harmonic walking their grids; both layouts, bases at 0 and 8 mod 16 on either side"""
    rng = np.random.default_rng(1000 * updates + lanes)
    ks = [k for k in S.LO_K if (updates << k) * lanes <= 1 << 22]  # k = 10 where the output stays small
    for i, k in enumerate(ks):
        h = S.LO_HARMONICS[(i + lanes + updates) % len(S.LO_HARMONICS)]
        lo_cfg = (k, h, int(rng.integers(-(1 << 31), 1 << 31)))
        accu = S.adversarial_accu(rng, updates, lanes)
        want = S.accu_lo_np(lo_cfg, accu)
        for layout in (H.FM, H.LM):
            for off_in, off_out in ((0, 0), (8, 8), (0, 8)) if i % 2 == 0 else ((8, 0),):
                got = gpu_run(gpu, lo_cfg, accu, layout, off_in, off_out)
                assert np.array_equal(got, want), (lo_cfg, layout, lanes, updates, off_in, off_out)


@pytest.mark.parametrize("k", S.LO_K)
def test_every_harmonic(gpu, k):
    rng = np.random.default_rng(k)
    accu = S.adversarial_accu(rng, 3, 65)
    for h in S.LO_HARMONICS:
        lo_cfg = (k, h, int(rng.integers(-(1 << 31), 1 << 31)))
        want = S.accu_lo_np(lo_cfg, accu)
        for layout in (H.FM, H.LM):
            assert np.array_equal(gpu_run(gpu, lo_cfg, accu, layout), want), (lo_cfg, layout)


def test_row_ranges_equal_the_whole(gpu):
    """no state: a call on rows [u0, u1) equals those rows of a longer call"""
    rng = np.random.default_rng(4)
    accu = S.adversarial_accu(rng, 9, 130)
    for k in (0, 3):
        lo_cfg = (k, 3, 12345)
        for layout in (H.FM, H.LM):
            whole = gpu_run(gpu, lo_cfg, accu, layout)
            assert np.array_equal(whole, S.accu_lo_np(lo_cfg, accu))
            for u0, u1 in ((0, 1), (2, 7), (8, 9)):
                assert np.array_equal(gpu_run(gpu, lo_cfg, accu[u0:u1], layout), whole[u0 << k:u1 << k]), (k, layout, u0, u1)


def test_every_phase_of_a_2_16_grid(gpu):
    """one update of 2^10 samples on 64 lanes: lane l starts at phase l 2^26 and steps by 2^16, so the 2^16 samples hold every
    multiple of 2^16 once — every octant and every entry of either table (a wrong table half shows)"""
    lanes, k = 64, 10
    accu = np.zeros((1, lanes, 2), np.int32)
    accu[0, :, 0] = ((np.arange(lanes, dtype=np.int64) << 26) - (1 << 16)).astype(np.uint32).view(np.int32)  # next() pre-increments
    accu[0, :, 1] = 1 << (16 + k)
    phases = S.accu_lo_phase_np((k, 1, 0), accu)
    assert np.array_equal(np.sort(phases.reshape(-1)), np.arange(1 << 16, dtype=np.uint32) << 16)
    want = S.accu_lo_np((k, 1, 0), accu)
    for layout in (H.FM, H.LM):
        assert np.array_equal(gpu_run(gpu, (k, 1, 0), accu, layout), want), layout


def test_rejected_calls_write_nothing(gpu):
    rng = np.random.default_rng(5)
    lanes, updates, k = 64, 4, 3
    g = Guards(DEV)
    ad = g.upload("accu", S.adversarial_accu(rng, updates + 1, lanes), readonly=True)
    ld = g.full("lo", ((updates << k) + 1) * lanes * 2, torch.int32, POISON)
    g.freeze("lo")
    c = _abi.AccuLo(k, 1, 0)
    for layout in (H.FM, H.LM):
        for a_p, l_p in ((ad.data_ptr(), ad.data_ptr()), (ad.data_ptr() + 4, ld.data_ptr()), (ad.data_ptr(), ld.data_ptr() + 4),
                         (ld.data_ptr() + 8 * lanes, ld.data_ptr())):
            rc = gpu.fn["accu_lo_i32"](C.byref(c), C.c_void_p(a_p), C.c_void_p(l_p), lanes, updates, layout, None)
            assert rc == _abi.IDSP_EINVAL and gpu.err(), (layout, a_p, l_p)
    torch.cuda.synchronize()
    g.check("rejected idsp_accu_lo_i32 calls")


def test_dispatch(gpu):
    if not KERNELS:
        gpu_run(gpu, (3, 1, 0), S.adversarial_accu(np.random.default_rng(0), 3, 65), H.FM)
    assert "accu_lo_i32" in RPLL
    for key in sorted(KERNELS):
        print(key, KERNELS[key])
