"""The six idsp_cordic_*_i32 entries on the GPU, through the C ABI, against the numpy specification (tests/_cordic_spec.py).

Every case allocates through tests/_guard.py (0xA5 bands checked, inputs frozen unless the call is in place, outputs poisoned),
compares every output word with `array_equal` and asserts the kernel's name: four elements per thread when xy, z and out all sit on
the 16-byte grid, one element per thread otherwise.

`N_SECOND_TRIP`: the launcher caps the grid at 2048 workgroups of 256 threads (kCordicMaxBlocks, idsp_amd/csrc/cordic.hip), each
thread taking four elements per trip of the grid-stride loop, so one trip covers 2048 * 256 * 4 = 2^21 elements.  2^21 + 3 * 1024
+ 7 gives the first three workgroups a second trip and leaves a ragged tail of 7 % 4 = 3 single elements; in the
one-element-per-thread form the same count is four trips and a fifth for some."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from idsp_amd import _abi
from idsp_amd._abi import CORDIC  # noqa: F401  (the feature's prototype table)
from tests import _cordic_spec as S
from tests import _harness as H
from tests._guard import Guards

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POISON = -77
NAMES = list(S.FUNCTIONS)
N_SECOND_TRIP = (1 << 21) + 3 * 1024 + 7
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KAT = json.load(open(os.path.join(ROOT, "tests", "golden", "cordic_kat.json")))


def _ptr(t):
    return C.c_void_p(None if t is None else t.data_ptr())


def kernel_name(name, *offsets):
    form = "four elements per thread" if all(o % 16 == 0 for o in offsets) else "one element per thread"
    return f"cordic_kernel<{name}>[{form}]"


def gpu_run(gpu, name, xy, z=None, *, xy_off=0, z_off=0, out_off=0, inplace=False):
    """xy int32 [n, 2], z int32 [n] or None -> what the entry wrote, [n, 2] or [n].  The offsets are bytes off the 16-byte grid."""
    pair = S.FUNCTIONS[name][2]
    n = xy.shape[0]
    g = Guards(DEV)
    xd = g.upload("xy", xy.reshape(-1), off=xy_off, readonly=not (inplace and pair))
    zd = None if z is None else g.upload("z", z, off=z_off, readonly=not (inplace and not pair))
    if inplace:
        od, out_off = (xd, xy_off) if pair else (zd, z_off)
    else:
        od = g.full("out", n * (2 if pair else 1), torch.int32, POISON, off=out_off)
    rc = gpu.fn[f"cordic_{name}_i32"](_ptr(xd), _ptr(zd), _ptr(od), n, None)
    assert rc == 0, gpu.err()
    torch.cuda.synchronize()
    what = (name, n, "z" if z is not None else "z = NULL", xy_off, z_off, out_off, "in place" if inplace else "")
    g.check(what)
    assert gpu.last_kernel() == kernel_name(name, xy_off, out_off, *([] if z is None else [z_off])), what
    got = od.cpu().numpy()
    return got.reshape(n, 2) if pair else got


def random_words(rng, shape):
    return rng.integers(S.I32_MIN, 1 << 31, size=shape, dtype=np.int64).astype(np.int32)


def same(want, got, what):
    assert want.dtype == got.dtype == np.int32 and np.array_equal(want, got), (what, np.flatnonzero((want != got).reshape(-1))[:8])


@pytest.mark.parametrize("name", NAMES)
def test_corner_triples(gpu, name):
    """all 17^3 triples of the reference's fixed values (:179-197): i32::MIN, +-0x7fffffff, +-2^30, ..."""
    v = np.array(S.FIXED_VALUES, np.int64)
    x, y, z = (g.reshape(-1).astype(np.int32) for g in np.meshgrid(v, v, v, indexing="ij"))
    xy = np.stack([x, y], axis=-1)
    same(S.function_np(name, xy, z), gpu_run(gpu, name, xy, z), (name, "corners"))
    same(S.function_np(name, xy[:289 * 17:17]), gpu_run(gpu, name, xy[:289 * 17:17]), (name, "corners, z = NULL"))


@pytest.mark.parametrize("name", NAMES)
def test_random_words_and_lengths(gpu, name):
    """n = 1, 3, 4, 5, 255, 1023, 1024, 1025 with z and with z = NULL"""
    rng = np.random.default_rng(11)
    for n in (1, 3, 4, 5, 255, 1023, 1024, 1025):
        xy, z = random_words(rng, (n, 2)), random_words(rng, n)
        same(S.function_np(name, xy, z), gpu_run(gpu, name, xy, z), (name, n))
        same(S.function_np(name, xy), gpu_run(gpu, name, xy), (name, n, "z = NULL"))


@pytest.mark.parametrize("name", NAMES)
def test_second_trip_of_the_grid_stride_loop(gpu, name):
    """N_SECOND_TRIP elements (module docstring).  The data repeats with the prime period 4099, so the specification runs on one period
    and every output word is still compared."""
    rng = np.random.default_rng(12)
    period = 4099
    bxy, bz = random_words(rng, (period, 2)), random_words(rng, period)
    reps = -(-N_SECOND_TRIP // period)
    xy, z = np.tile(bxy, (reps, 1))[:N_SECOND_TRIP], np.tile(bz, reps)[:N_SECOND_TRIP]
    want = S.function_np(name, bxy, bz)
    want = np.tile(want, (reps, 1) if want.ndim == 2 else reps)[:N_SECOND_TRIP]
    same(want, gpu_run(gpu, name, xy, z), (name, "second trip"))
    if name in ("cos_sin", "div"):  # the one-element-per-thread form, pair and word results
        same(want, gpu_run(gpu, name, xy, z, xy_off=8), (name, "second trip, one element per thread"))


def test_empty_call(gpu):
    """n == 0 returns IDSP_OK before any pointer check and writes nothing"""
    g = Guards(DEV)
    xd = g.upload("xy", np.arange(8, dtype=np.int32), readonly=True)
    od = g.upload("out", np.full(8, POISON, np.int32), readonly=True)
    for name in NAMES:
        f = gpu.fn[f"cordic_{name}_i32"]
        assert f(_ptr(xd), None, _ptr(od), 0, None) == 0 and f(None, None, None, 0, None) == 0
        assert f(C.c_void_p(xd.data_ptr() + 4), None, C.c_void_p(xd.data_ptr() + 4), 0, None) == 0
    torch.cuda.synchronize()
    g.check("n == 0")


@pytest.mark.parametrize("name", NAMES)
def test_base_addresses(gpu, name):
    """xy and a pair out 0 or 8 bytes off the 16-byte grid, z and a word out 0, 4, 8 or 12 bytes off; n = 1027 = 256 fours + 3"""
    rng = np.random.default_rng(13)
    n, pair = 1027, S.FUNCTIONS[name][2]
    xy, z = random_words(rng, (n, 2)), random_words(rng, n)
    want, want0 = S.function_np(name, xy, z), S.function_np(name, xy)
    for xy_off in (0, 8):
        for out_off in ((0, 8) if pair else (0, 4, 8, 12)):
            for z_off in (0, 4, 8, 12):
                same(want, gpu_run(gpu, name, xy, z, xy_off=xy_off, z_off=z_off, out_off=out_off), (name, xy_off, z_off, out_off))
            same(want0, gpu_run(gpu, name, xy, xy_off=xy_off, out_off=out_off), (name, xy_off, "z = NULL", out_off))


@pytest.mark.parametrize("name", NAMES)
def test_in_place(gpu, name):
    """out == xy (pair functions) and out == z (mul, div) equal the out-of-place call, in both kernel forms"""
    rng = np.random.default_rng(14)
    pair = S.FUNCTIONS[name][2]
    for n in (5, 1027, 4096):
        xy, z = random_words(rng, (n, 2)), random_words(rng, n)
        want = S.function_np(name, xy, z)
        for off in ((0, 8) if pair else (0, 4)):
            out = gpu_run(gpu, name, xy, z, xy_off=off if pair else 0, z_off=0 if pair else off, out_off=off)
            got = gpu_run(gpu, name, xy, z, xy_off=off if pair else 0, z_off=0 if pair else off, inplace=True)
            same(want, got, (name, n, off, "in place"))
            same(out, got, (name, n, off, "in place against out of place"))
        if pair:
            same(S.function_np(name, xy), gpu_run(gpu, name, xy, inplace=True), (name, n, "in place, z = NULL"))


def test_argument_errors(gpu):
    """every forbidden overlap, a 4-byte-misaligned xy or pair out and NULL pointers: IDSP_EINVAL with a message, nothing written"""
    n = 16
    g = Guards(DEV)
    xd = g.upload("xy", np.arange(4 * n, dtype=np.int32), readonly=True)
    zd = g.upload("z", np.arange(2 * n, dtype=np.int32), readonly=True)
    od = g.upload("out", np.full(4 * n, POISON, np.int32), readonly=True)
    x, z, o = xd.data_ptr(), zd.data_ptr(), od.data_ptr()
    for name in NAMES:
        pair = S.FUNCTIONS[name][2]
        rows = [("xy NULL", None, z, o), ("out NULL", x, z, None), ("xy and z NULL", None, None, o),
                ("xy 4 bytes off", x + 4, z, o), ("out one row behind xy", x, z, x + 8), ("out one row in front of xy", x + 8, z, x),
                ("out over the end of xy", x, None, x + 8 * n - 8), ("out one word behind z", x, z, z + 8), ("out in front of z", x, z + 8, z)]
        rows += [("pair out 4 bytes off", x, z, o + 4), ("pair out == z", x, z, z)] if pair else [("word out == xy", x, z, x), ("word out inside xy", x, None, x + 16)]
        for what, xp, zp, op in rows:
            rc = gpu.fn[f"cordic_{name}_i32"](C.c_void_p(xp), C.c_void_p(zp), C.c_void_p(op), n, None)
            assert rc == _abi.IDSP_EINVAL and gpu.err(), (name, what, rc)
    torch.cuda.synchronize()
    g.check("argument errors")


def test_meanmax_rot_on_the_device(gpu):
    """the cases of `meanmax_rot` (:201-223) through idsp_cordic_cos_sin_i32: bit-equal to the specification, so the reference's
    bounds (mean < 5, max < 24) hold for what the device wrote"""
    b = KAT["bounds"]["meanmax_rot"]
    total, x, y, z, xy, zi = S.rot_cases(S.test_values(b["random"], 42))
    got = gpu_run(gpu, "cos_sin", xy, zi)
    same(S.function_np("cos_sin", xy, zi), got, "meanmax_rot")
    e = S.rot_errors(got, x, y, z)
    assert e.sum() / total < b["mean"] and e.max() < b["max"]


def test_meanmax_vect_on_the_device(gpu):
    """the cases of `meanmax_vect` (:225-245) through idsp_cordic_sqrt_atan2_i32 with z = NULL (the reference passes 0)"""
    b = KAT["bounds"]["meanmax_vect"]
    total, x, y, xy = S.vect_cases(S.test_values(b["random"], 42))
    got = gpu_run(gpu, "sqrt_atan2", xy)
    same(S.function_np("sqrt_atan2", xy), got, "meanmax_vect")
    e = S.vect_errors(got, x, y)
    assert e.sum() / total < b["mean"] and e.max() < b["max"]


@pytest.mark.parametrize("layout", [H.FM, H.LM])
def test_polar_read_out_of_a_dds_stream(gpu, layout):
    """idsp_dds_i32 rows -> idsp_cordic_sqrt_atan2_i32 with z = NULL: magnitude and phase of an engine stream in one pass"""
    rng = np.random.default_rng(15)
    lanes, frames = 65, 300
    st = torch.from_numpy(random_words(rng, (2, lanes))).to(DEV)
    g = Guards(DEV)
    iq = g.full("iq", lanes * frames * 2, torch.int32, POISON)
    assert gpu.fn["dds_i32"](_ptr(st), _ptr(iq), lanes, frames, layout, None) == 0, gpu.err()
    g.freeze("iq")
    out = g.full("out", lanes * frames * 2, torch.int32, POISON)
    assert gpu.fn["cordic_sqrt_atan2_i32"](_ptr(iq), None, _ptr(out), lanes * frames, None) == 0, gpu.err()
    torch.cuda.synchronize()
    g.check("dds -> sqrt_atan2")
    assert gpu.last_kernel() == kernel_name("sqrt_atan2", 0)
    rows = iq.cpu().numpy().reshape(-1, 2)
    assert not (rows == POISON).all(axis=1).any()
    same(S.function_np("sqrt_atan2", rows), out.cpu().numpy().reshape(-1, 2), "dds -> sqrt_atan2")


def test_offsets_past_32_bits(gpu):
    """n = 2^29 + 5: xy and out are 4 GiB + 40 bytes each, z 2 GiB + 20.  Inputs are made on the device; the first 4096 and the last
    4096 + 5 elements are compared with the specification."""
    n, head, tail = (1 << 29) + 5, 4096, 4096 + 5
    try:
        xy = torch.randint(-(1 << 31), (1 << 31) - 1, (n, 2), dtype=torch.int32, device=DEV)
        z = torch.randint(-(1 << 31), (1 << 31) - 1, (n,), dtype=torch.int32, device=DEV)
        out = torch.full((n, 2), POISON, dtype=torch.int32, device=DEV)
    except torch.OutOfMemoryError as e:  # pragma: no cover
        pytest.skip(f"10 GiB of device memory are not available: {e}")
    assert gpu.fn["cordic_cos_sin_i32"](_ptr(xy), _ptr(z), _ptr(out), n, None) == 0, gpu.err()
    torch.cuda.synchronize()
    assert gpu.last_kernel() == kernel_name("cos_sin", 0)
    for sl in (slice(0, head), slice(n - tail, n)):
        same(S.function_np("cos_sin", xy[sl].cpu().numpy(), z[sl].cpu().numpy()), out[sl].cpu().numpy(), ("past 4 GiB", sl))
    del xy, z, out
    torch.cuda.empty_cache()
