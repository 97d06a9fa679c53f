"""The Python mirrors of the CORDIC family (idsp_amd.process.cordic_*) give the same words as direct calls of the C ABI on one small
shape each, and their validation raises before anything is launched."""
import ctypes as C

import pytest
import torch

from idsp_amd import process as P
from idsp_amd._abi import CORDIC  # noqa: F401  (the feature's prototype table)
from tests import _cordic_spec as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _ptr(t):
    return C.c_void_p(None if t is None else t.data_ptr())


def words(shape, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randint(-(1 << 31), (1 << 31) - 1, shape, generator=g, dtype=torch.int64).to(torch.int32).to(DEV)


@pytest.mark.parametrize("name", list(S.FUNCTIONS))
def test_python_mirror(gpu, name):
    pair = S.FUNCTIONS[name][2]
    fn = getattr(P, "cordic_" + name)
    xy, z = words((7, 93, 2), 1), words((7, 93), 2)  # a [frames, lanes] block of `Complex<i32>`
    n = 7 * 93
    for zz in (z, None):
        want = torch.full((7, 93, 2) if pair else (7, 93), -77, dtype=torch.int32, device=DEV)
        assert gpu.fn[f"cordic_{name}_i32"](_ptr(xy), _ptr(zz), _ptr(want), n, None) == 0, gpu.err()
        torch.cuda.synchronize()
        got = fn(xy, zz)
        assert got.shape == want.shape and got.dtype == torch.int32 and torch.equal(got, want)
        out = torch.full_like(want, -77)
        assert fn(xy, zz, out=out) is out and torch.equal(out, want)
    # in place: out = xy (pair) / out = z (word)
    if pair:
        a = xy.clone()
        assert fn(a, z, out=a) is a and torch.equal(a, fn(xy, z))
    else:
        a = z.clone()
        assert fn(xy, a, out=a) is a and torch.equal(a, fn(xy, z))


def test_gains(gpu):
    assert P.cordic_circular_gain() == S.circular_gain() and P.cordic_hyperbolic_gain() == S.hyperbolic_gain()


def test_python_mirror_rejects_misuse(gpu):
    xy, z = words((8, 2), 3), words((8,), 4)
    before = gpu.last_kernel()
    for name in S.FUNCTIONS:
        fn, pair = getattr(P, "cordic_" + name), S.FUNCTIONS[name][2]
        bad = [
            lambda: fn(xy.cpu(), z),                                  # CPU tensor
            lambda: fn(xy.to(torch.int64), z),                        # dtype
            lambda: fn(words((8, 3), 5), z),                          # rows are not pairs
            lambda: fn(words((8, 4), 5)[:, :2], z),                   # not contiguous
            lambda: fn(xy, words((7,), 6)),                           # z of another length
            lambda: fn(xy, z.to(torch.int64)),                        # z dtype
            lambda: fn(xy, z, out=torch.empty((8,) if pair else (8, 2), dtype=torch.int32, device=DEV)),  # out of the other kind
            lambda: fn(xy, z, out=torch.empty((8, 2) if pair else (8,), dtype=torch.float32, device=DEV)),
            lambda: fn(torch.empty((), dtype=torch.int32, device=DEV), None),
        ]
        for k, call in enumerate(bad):
            with pytest.raises(ValueError):
                call()
        # an overlap the library refuses arrives as IdspError, also before any launch
        with pytest.raises(P.IdspError):
            both = words((16, 2), 7)
            fn(both[:8], z, out=(both.reshape(-1)[8:24].reshape(8, 2) if pair else both.reshape(-1)[8:16]))
    assert gpu.last_kernel() == before  # nothing was launched
