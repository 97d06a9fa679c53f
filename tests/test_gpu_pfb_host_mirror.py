"""The host mirrors of the polyphase channelizer give the same bytes as direct calls of the C ABI: idsp_amd.process.PolyphaseBank
on torch tensors (block / inplace / LaneMajor views, state continued between them) and the C++ class of include/idsp_hip.hpp
(tests/cpp/test_pfb_host.cpp, compiled here with plain g++ against the C ABI only)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from idsp_amd import _abi
from idsp_amd import process as P
from idsp_amd._abi import PFB  # noqa: F401  (the feature's prototype table)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def abi(gpu, cfg, sd, xd, yd, lanes, frames, layout):
    rc = gpu.fn["pfb_f32_process"](C.byref(cfg), C.c_void_p(sd.data_ptr()), C.c_void_p(xd.data_ptr()), C.c_void_p(yd.data_ptr()),
                                   lanes, frames, layout, None)
    assert rc == 0, gpu.err()
    torch.cuda.synchronize()


def same_bytes(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("dft", [False, True])
@pytest.mark.parametrize("taps", [3, 8])
def test_python_mirror(gpu, taps, dft):
    lanes, frames = 65, 256 + 9
    op = P.PolyphaseBank.prototype(taps, dft=dft).lanes(lanes)
    cfg = _abi.PfbF32()
    assert gpu.fn["pfb_prototype_f32"](taps, C.byref(cfg)) == 0
    cfg.dft = int(dft)
    assert bytes(op.cfg) == bytes(cfg) and op.state.shape == (8 * taps + 1, lanes) and not op.state.any()
    assert np.array_equal(np.array(op.coeff, np.float32), np.array([[cfg.coeff[t][m] for m in range(4)] for t in range(taps)], np.float32))
    g = torch.Generator(device="cpu").manual_seed(taps)
    sd = torch.zeros((8 * taps + 1, lanes), dtype=torch.int32, device=DEV)
    # Process::block: FrameMajor [frames, lanes, 4, 2]
    x = torch.randn((frames, lanes, 4, 2), generator=g).to(DEV)
    y, want = torch.full_like(x, 7.0), torch.full_like(x, 7.0)
    op.block(x, y)
    abi(gpu, cfg, sd, x, want, lanes, frames, P.FrameMajor)
    assert same_bytes(y, want) and torch.equal(op.state, sd)
    # ViewProcess::process_view on LaneMajor views of width 8 continues the same state
    xl = torch.randn((lanes, 100, 8), generator=g).to(DEV)
    yl, wl = torch.full_like(xl, 7.0), torch.full_like(xl, 7.0)
    op.process_view(P.View(xl, P.LaneMajor, lanes, width=8), P.ViewMut(yl, P.LaneMajor, lanes, width=8))
    abi(gpu, cfg, sd, xl, wl, lanes, 100, P.LaneMajor)
    assert same_bytes(yl, wl) and torch.equal(op.state, sd)
    # Inplace::inplace
    x3 = torch.randn((33, lanes, 4, 2), generator=g).to(DEV)
    xy = x3.clone()
    op.inplace(xy)
    abi(gpu, cfg, sd, x3, x3, lanes, 33, P.FrameMajor)
    assert same_bytes(xy, x3) and torch.equal(op.state, sd)
    assert torch.equal(op.head(), sd[8 * taps]) and int(op.head().max()) < taps
    op.reset()
    assert not op.state.any()


def test_python_mirror_rejects_misuse(gpu):
    with pytest.raises(ValueError):
        P.PolyphaseBank([[0.25] * 4] * 17)
    with pytest.raises(ValueError):
        P.PolyphaseBank([[0.25] * 3])
    with pytest.raises(P.IdspError):
        P.PolyphaseBank.prototype(0)
    op = P.PolyphaseBank([[0.25] * 4] * 2).lanes(8)
    good = torch.zeros((4, 8, 4, 2), dtype=torch.float32, device=DEV)
    with pytest.raises(ValueError):
        op.block(good, torch.zeros((5, 8, 4, 2), dtype=torch.float32, device=DEV))
    with pytest.raises(ValueError):
        op.block(good.to(torch.float64), good)
    with pytest.raises(ValueError):
        op.block(torch.zeros((4, 8, 4, 2)), good)  # CPU tensor


def test_cpp_mirror(gpu):
    exe = os.path.join(ROOT, "build", "test_pfb_host")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Iinclude", "tests/cpp/test_pfb_host.cpp", "-Lidsp_amd/lib", "-lidsp_hip",
                    "-Wl,-rpath,$ORIGIN/../idsp_amd/lib", "-o", exe], cwd=ROOT, check=True)
    r = subprocess.run([exe], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "polyphase host-mirror tests passed" in r.stdout
