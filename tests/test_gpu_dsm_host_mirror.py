"""idsp_amd.process.Dsm / DsmLanes on torch tensors against tests/_dsm_spec.py, and the C++ mirrors of include/idsp_hip.hpp against
direct calls of the C ABI on one small shape (tests/cpp/test_dsm_gpu.cpp, compiled here with plain g++ against the C ABI only)."""
import os
import subprocess

import numpy as np
import pytest
import torch

from idsp_amd import process as P
from idsp_amd._abi import DSM  # noqa: F401  (the feature's prototype table)
from tests import _dsm_spec as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LANES, FRAMES = 65, 37


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to(DEV)


@pytest.mark.parametrize("order", [0, 1, 3, 8])
def test_python_mirror(gpu, order):
    rng = np.random.default_rng(order)
    x1, x2 = S.inputs(rng, FRAMES, LANES), S.inputs(rng, FRAMES + 3, LANES)
    st = np.zeros((2 * order, LANES), np.uint32)
    want1, want2 = S.dsm_np(order, st, x1), S.dsm_np(order, st, x2)
    d = P.Dsm(order).lanes(LANES)
    assert isinstance(d, P.DsmLanes) and d.state.shape == (2 * order, LANES) and d.state.dtype == torch.int32 and not d.state.any()
    # `.block`: FrameMajor [frames, lanes] ...
    y1 = torch.full((FRAMES, LANES), -77, dtype=torch.int8, device=DEV)
    assert d.block(_dev(x1), y1) is y1
    assert gpu.last_kernel().startswith("dsm_frame_major")
    # ... then `.process_view` LaneMajor on the same state
    y2 = torch.full(((FRAMES + 3) * LANES,), -77, dtype=torch.int8, device=DEV)
    d.process_view(P.View(_dev(x2.T), P.LaneMajor, LANES), P.ViewMut(y2, P.LaneMajor, LANES))
    assert gpu.last_kernel().startswith("dsm_lane_major")
    torch.cuda.synchronize()
    assert np.array_equal(y1.cpu().numpy(), want1)
    assert np.array_equal(y2.cpu().numpy().reshape(LANES, FRAMES + 3).T, want2)
    assert np.array_equal(d.state.cpu().numpy().view(np.uint32), st)
    # FrameMajor views go the same way
    d.reset()
    assert not d.state.any()
    y3 = torch.full((FRAMES * LANES,), -77, dtype=torch.int8, device=DEV)
    d.process_view(P.View(_dev(x1), P.FrameMajor, LANES), P.ViewMut(y3, P.FrameMajor, LANES))
    assert np.array_equal(y3.cpu().numpy().reshape(FRAMES, LANES), want1)


def test_python_mirror_errors(gpu):
    d = P.Dsm(3).lanes(LANES)
    x = torch.zeros((FRAMES, LANES), dtype=torch.int32, device=DEV)
    y = torch.zeros((FRAMES, LANES), dtype=torch.int8, device=DEV)
    before = d.state.clone()
    for bad_x, bad_y in [(x.cpu(), y), (x, y.cpu()),                                     # CPU tensors
                         (x.to(torch.int64), y), (x, y.to(torch.int32)), (x, y.to(torch.uint8)),   # dtypes
                         (x[:, :-1].contiguous(), y), (x, y[:-1]), (x.reshape(-1), y.reshape(-1)),  # shapes
                         (x.t(), y)]:                                                    # not contiguous
        with pytest.raises(ValueError):
            d.block(bad_x, bad_y)
    with pytest.raises(ValueError):
        d.inplace(x)
    with pytest.raises(ValueError):
        d.inplace_view(P.ViewMut(x, P.LaneMajor, LANES))
    with pytest.raises(ValueError):
        d.process_view(P.View(x, P.LaneMajor, LANES), P.View(y, P.LaneMajor, LANES))       # y is not a ViewMut
    with pytest.raises(ValueError):
        d.process_view(P.View(x, P.LaneMajor, LANES), P.ViewMut(y, P.FrameMajor, LANES))   # layouts differ
    with pytest.raises(ValueError):
        d.process_view(P.View(x, P.LaneMajor, LANES), P.ViewMut(y[:-1], P.LaneMajor, LANES - 1))
    torch.cuda.synchronize()
    assert torch.equal(d.state, before) and not y.any()


def test_cpp_mirror(gpu):
    exe = os.path.join(ROOT, "build", "test_dsm_gpu")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Iinclude", "tests/cpp/test_dsm_gpu.cpp", "-Lidsp_amd/lib", "-lidsp_hip",
                    "-Wl,-rpath,$ORIGIN/../idsp_amd/lib", "-o", exe], cwd=ROOT, check=True)
    r = subprocess.run([exe], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "dsm host-mirror tests passed" in r.stdout
