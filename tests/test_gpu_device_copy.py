"""`idsp_device_copy` (include/idsp_hip.h, idsp_amd/csrc/api_util.hip) against a plain host copy: every path it has — the byte
kernel alone (dst and src not congruent mod 16, including a size past one sweep of its capped grid of 65535 x 16 blocks, so that its
grid-stride loop runs), and the 16-byte chunk kernel with its byte-kernel head and tail (congruent, including piece counts on both sides
of the chunk kernel's grid cap of 2048 workgroups, a ragged last workgroup on the capped grid, and a size past 2^32 bytes) — with guard bytes on both sides left untouched, and the contract:
overlap in either order is IDSP_EINVAL, touching buffers and dst == src are fine, NULL only with 0 bytes."""
import ctypes as C

import numpy as np
import pytest
import torch

from idsp_amd import _abi

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64  # guard bytes before and after each region (plus the 0..15 byte offset)


def copy(gpu, dst, src, n, stream=None):
    return gpu.fn["device_copy"](C.c_void_p(dst), C.c_void_p(src), n, stream)


def pattern(n, seed):
    """n random bytes on the device (a seeded generator: the same bytes on every run)"""
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return torch.randint(0, 256, (n,), dtype=torch.uint8, device=DEV, generator=g)


def check_copy(gpu, n, doff, soff, seed=0):
    """copy n bytes from src + soff to dst + doff; the copied bytes equal the source, everything else of both buffers is unchanged"""
    size = n + 2 * GUARD + 16
    src, dst = pattern(size, seed), pattern(size, seed + 1)
    d, s = GUARD + doff, GUARD + soff
    torch.cuda.synchronize()
    assert copy(gpu, dst.data_ptr() + d, src.data_ptr() + s, n) == _abi.IDSP_OK, gpu.err()
    torch.cuda.synchronize()
    assert torch.equal(dst[d:d + n], src[s:s + n]), (n, doff, soff, "copied bytes")
    # the originals are regenerated rather than cloned: the 4 GiB case stays within four buffers' worth of memory
    dst0 = pattern(size, seed + 1)
    assert torch.equal(dst[:d], dst0[:d]) and torch.equal(dst[d + n:], dst0[d + n:]), (n, doff, soff, "guard bytes of dst")
    del dst, dst0
    assert torch.equal(src, pattern(size, seed)), (n, doff, soff, "src changed")


@pytest.mark.parametrize("n", [0, 1, 15, 16, 17, 4097])
def test_small_sizes_every_offset_pair(gpu, n):
    """dst and src offsets 0..15 each: congruent pairs take head + 16-byte chunks + tail, the others the byte kernel alone"""
    for doff in range(16):
        for soff in range(16):
            check_copy(gpu, n, doff, soff, seed=n * 256 + doff * 16 + soff)


@pytest.mark.parametrize("n, doff, soff", [
    (2048 * 2048 * 16 + 5, 0, 0),     # 2^22 pieces and a 5-byte tail: the first count on the capped grid (2048 workgroups of 2048 pieces)
    (2048 * 2048 * 16 + 5, 3, 3),     # a head of 13 bytes, 2^22 - 1 pieces: the last count below the cap, a ragged last workgroup
    (2048 * 2048 * 16 + 16 + 7, 0, 0),  # 2^22 + 1 pieces on the capped grid: 2049 per workgroup, the last one clamped to n
    (2 ** 28 + 4099, 1, 6),           # not congruent: the byte kernel's capped grid strides over the bytes more than once
    (2 ** 28 + 4099, 11, 0),
])
def test_large_sizes(gpu, n, doff, soff):
    check_copy(gpu, n, doff, soff, seed=n % 1000 + doff)


def test_past_4_gib_congruent(gpu):
    """2^32 + 21 bytes at offsets 5 / 5: a head of 11 bytes, 2^28 + 0 pieces, a tail of 10 bytes, byte offsets past 32 bits"""
    n, off = 2 ** 32 + 21, 5
    torch.cuda.empty_cache()
    check_copy(gpu, n, off, off, seed=77)
    torch.cuda.empty_cache()


def test_overlap_is_rejected_and_touching_is_fine(gpu):
    buf = pattern(4096, 3)
    b0 = buf.clone()
    a = buf.data_ptr()
    for dst, src, n in ((a + 100, a, 101), (a, a + 100, 101), (a + 1, a, 4000), (a, a + 1, 4000), (a + 64, a, 65), (a, a + 64, 65)):
        assert copy(gpu, dst, src, n) == _abi.IDSP_EINVAL, (dst - a, src - a, n)
    torch.cuda.synchronize()
    assert torch.equal(buf, b0), "a rejected copy wrote"
    # touching but disjoint, both orders
    assert copy(gpu, a + 100, a, 100) == _abi.IDSP_OK, gpu.err()
    torch.cuda.synchronize()
    want = b0.clone()
    want[100:200] = b0[0:100]
    assert torch.equal(buf, want)
    assert copy(gpu, a + 1000, a + 1100, 100) == _abi.IDSP_OK, gpu.err()
    torch.cuda.synchronize()
    want[1000:1100] = want[1100:1200].clone()
    assert torch.equal(buf, want)
    # dst == src: nothing to do
    assert copy(gpu, a + 7, a + 7, 3000) == _abi.IDSP_OK, gpu.err()
    torch.cuda.synchronize()
    assert torch.equal(buf, want)


def test_null_pointers(gpu):
    buf = torch.zeros(64, dtype=torch.uint8, device=DEV)
    assert gpu.fn["device_copy"](None, None, 0, None) == _abi.IDSP_OK
    assert gpu.fn["device_copy"](None, C.c_void_p(buf.data_ptr()), 0, None) == _abi.IDSP_OK
    assert gpu.fn["device_copy"](None, C.c_void_p(buf.data_ptr()), 1, None) == _abi.IDSP_EINVAL
    assert gpu.fn["device_copy"](C.c_void_p(buf.data_ptr()), None, 1, None) == _abi.IDSP_EINVAL
    assert gpu.fn["device_copy"](None, None, 16, None) == _abi.IDSP_EINVAL


def test_non_default_stream(gpu):
    """the copy runs on the caller's stream: idsp_stream_sync on that stream is all it takes before the host reads the result"""
    n, d, s = 1 << 20 | 9, GUARD + 3, GUARD + 3
    src = pattern(n + 2 * GUARD, 11)
    dst = torch.zeros(n + 2 * GUARD, dtype=torch.uint8, device=DEV)
    want = src[s:s + n].cpu()
    torch.cuda.synchronize()
    st = torch.cuda.Stream(device=DEV)
    h = C.c_void_p(st.cuda_stream)
    assert copy(gpu, dst.data_ptr() + d, src.data_ptr() + s, n, h) == _abi.IDSP_OK, gpu.err()
    assert gpu.fn["stream_sync"](h) == _abi.IDSP_OK, gpu.err()
    # read back with a plain host copy (hipMemcpy of the raw pointer: no torch stream ordering involved)
    got = np.empty(n + 2 * GUARD, np.uint8)
    assert gpu.fn["device_d2h"](C.c_void_p(got.ctypes.data), C.c_void_p(dst.data_ptr()), n + 2 * GUARD, h) == _abi.IDSP_OK
    assert gpu.fn["stream_sync"](h) == _abi.IDSP_OK
    assert np.array_equal(got[d:d + n], want.numpy()) and not got[:d].any() and not got[d + n:].any()
