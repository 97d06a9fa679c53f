"""idsp_amd.process.Sweep / SweepOsc on torch tensors and the C++ mirrors of include/idsp_hip.hpp against direct calls
of the C ABI on one small shape, `emitted()` included (tests/cpp/test_sweep_gpu.cpp, compiled here with plain g++ against the C ABI
only)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from idsp_amd import process as P
from idsp_amd._abi import SWEEP  # noqa: F401  (the feature's prototype table)
from tests import _sweep_spec as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LANES, FRAMES = 65, 17


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _sweeps():
    """per-lane (rate, state) tensors: the reference test's sweep, with lanes that end after 3, after 1 and before the call"""
    fit = P.Sweep.fit(0.3, 3000.0, 3.0)
    assert (fit.rate, fit.state) == S.fit(0.3, 3000.0, 3.0)
    rate = torch.full((LANES,), fit.rate, dtype=torch.int32)
    state = torch.full((LANES,), fit.state, dtype=torch.int64)
    rate[1], state[1] = 1 << 30, 1 << 62
    rate[2], state[2] = (1 << 31) - 1, (1 << 62) + 12345
    rate[64], state[64] = 1, -(1 << 63)
    return fit, rate, state


def _emitted_want():
    e = np.full(LANES, FRAMES, np.int64)
    e[1], e[2], e[64] = 3, 1, 0
    return e


def test_sweep_osc(gpu):
    fit, rate, state = _sweeps()
    st = torch.from_numpy(S.pack([int(v) for v in state], [int(v) for v in rate]).view(np.int32)).to(DEV)
    for layout in (P.FrameMajor, P.LaneMajor):
        raw = st.clone()
        want = torch.full((FRAMES * LANES * 2,), -77, dtype=torch.int32, device=DEV)
        assert gpu.fn["sweep_i32"](_ptr(raw), _ptr(want), LANES, FRAMES, layout, None) == 0, gpu.err()
        torch.cuda.synchronize()
        osc = P.SweepOsc(LANES, rate, state)
        assert osc.state.shape == (7, LANES) and torch.equal(osc.state, st)
        got = torch.full_like(want, -77)
        assert osc.generate(got, FRAMES, layout) is got
        assert torch.equal(got, want) and torch.equal(osc.state, raw)
        assert osc.emitted().dtype == torch.int64 and np.array_equal(osc.emitted().cpu().numpy(), _emitted_want())
    # one `Sweep` for every lane; a scalar pair
    a, b = P.SweepOsc(8, fit), P.SweepOsc(8, fit.rate, fit.state)
    assert torch.equal(a.state, b.state) and int(a.state[4, 3]) == fit.rate
    with pytest.raises(ValueError):
        a.generate(torch.zeros(8 * 4 * 2 + 1, dtype=torch.int32, device=DEV), 4)
    with pytest.raises(ValueError):
        a.generate(torch.zeros(8 * 4 * 2, dtype=torch.int32), 4)  # CPU tensor
    with pytest.raises(ValueError):
        P.Sweep.fit(0.6, 1.0, 1.0)


def test_cpp_mirror(gpu):
    exe = os.path.join(ROOT, "build", "test_sweep_gpu")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Iinclude", "tests/cpp/test_sweep_gpu.cpp", "-Lidsp_amd/lib", "-lidsp_hip",
                    "-Wl,-rpath,$ORIGIN/../idsp_amd/lib", "-o", exe], cwd=ROOT, check=True)
    r = subprocess.run([exe], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "sweep host-mirror tests passed" in r.stdout
