"""idsp_amd.process.RPLLConfig / RPLLLanes / accu_lo on torch tensors and the C++ mirrors of include/idsp_hip.hpp against direct
calls of the C ABI on one small shape, `phase()` / `frequency()` included (tests/cpp/test_rpll_gpu.cpp, compiled here with plain
g++ against the C ABI only)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from idsp_amd import _abi
from idsp_amd import process as P
from idsp_amd._abi import RPLL  # noqa: F401  (the feature's prototype table)
from tests import _rpll_spec as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LANES, UPDATES, K = 65, 17, 3


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def test_python_mirror(gpu):
    rng = np.random.default_rng(1)
    ts_np = S.adversarial_ts(rng, UPDATES, LANES)
    for layout in (P.FrameMajor, P.LaneMajor):
        ts = torch.from_numpy(np.ascontiguousarray(ts_np if layout == P.FrameMajor else np.swapaxes(ts_np, 0, 1))).to(DEV)
        raw = torch.zeros((4, LANES), dtype=torch.int32, device=DEV)
        want_a = torch.full((UPDATES * LANES * 2,), -77, dtype=torch.int32, device=DEV)
        want_lo = torch.full(((UPDATES << K) * LANES * 2,), -77, dtype=torch.int32, device=DEV)
        assert gpu.fn["rpll_i32"](C.byref(_abi.Rpll(8, 23, 22)), _ptr(raw), _ptr(ts), _ptr(want_a), LANES, UPDATES, layout, None) == 0, gpu.err()
        assert gpu.fn["accu_lo_i32"](C.byref(_abi.AccuLo(K, 3, -99)), _ptr(want_a), _ptr(want_lo), LANES, UPDATES, layout, None) == 0, gpu.err()
        torch.cuda.synchronize()
        r = P.RPLLConfig(8, 23, 22).lanes(LANES)
        assert r.state.shape == (4, LANES) and not r.state.any()
        got_a, got_lo = torch.full_like(want_a, -77), torch.full_like(want_lo, -77)
        assert r.process(ts, got_a, UPDATES, layout) is got_a
        assert P.accu_lo(got_a, got_lo, LANES, UPDATES, K, harmonic=3, offset=-99, layout=layout) is got_lo
        assert torch.equal(got_a, want_a) and torch.equal(got_lo, want_lo) and torch.equal(r.state, raw)
        assert torch.equal(r.phase(), raw[3]) and torch.equal(r.frequency(), raw[2])
    # the spec, once
    st = np.zeros((4, LANES), np.uint32)
    accu = S.rpll_np((8, 23, 22), st, ts_np)
    assert np.array_equal(raw.cpu().numpy().view(np.uint32), st)
    assert np.array_equal(np.swapaxes(want_lo.cpu().numpy().reshape(LANES, UPDATES << K, 2), 0, 1), S.accu_lo_np((K, 3, -99), accu))
    for bad in ((-1, 9, 8), (8, 8, 8), (8, 33, 8), (8, 9, 7), (8, 9, 40), (31, 32, 31)):
        with pytest.raises(ValueError):
            P.RPLLConfig(*bad)
    with pytest.raises(ValueError):
        P.accu_lo(got_a, got_lo, LANES, UPDATES, 25)
    with pytest.raises(ValueError):
        P.accu_lo(got_a, got_lo[:-2], LANES, UPDATES, K)
    with pytest.raises(ValueError):
        r.process(ts.cpu(), got_a, UPDATES)  # CPU tensor
    with pytest.raises(P.IdspError):
        r.process(got_a, got_a, UPDATES)  # ts == accu


def test_cpp_mirror(gpu):
    exe = os.path.join(ROOT, "build", "test_rpll_gpu")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Iinclude", "tests/cpp/test_rpll_gpu.cpp", "-Lidsp_amd/lib", "-lidsp_hip",
                    "-Wl,-rpath,$ORIGIN/../idsp_amd/lib", "-o", exe], cwd=ROOT, check=True)
    r = subprocess.run([exe], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "rpll host-mirror tests passed" in r.stdout
