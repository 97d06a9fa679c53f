"""idsp_amd.process.LockinLo.process_accu on torch tensors and idsp_hip::AccuLo::lockin_view (include/idsp_hip.hpp) against the
chain they fuse, accu_lo -> LockinLo.process, on one small shape per layout (tests/cpp/test_lockin_accu_gpu.cpp, compiled here
with plain g++ against the C ABI only)."""
import os
import subprocess

import numpy as np
import pytest
import torch

from idsp_amd import process as P
from idsp_amd._abi import RPLL
from tests import _lockin_accu_cases as LA
from tests import _rpll_spec as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LANES, UPDATES, K = 65, 9, 3


def test_python_mirror(gpu):
    assert "lockin_i32_accu_process" in RPLL
    rng = np.random.default_rng(2)
    accu_np, x_np = S.adversarial_accu(rng, UPDATES, LANES), LA.adversarial_x(rng, UPDATES << K, LANES)
    arms = [P.Lowpass([1 << 21, -(1 << 26)]), P.Lowpass([1 << 20, -(1 << 27)])]
    for layout in (P.FrameMajor, P.LaneMajor):
        put = lambda a: torch.from_numpy(np.ascontiguousarray(a if layout == P.FrameMajor else np.swapaxes(a, 0, 1))).to(DEV)  # noqa: E731
        x, accu = put(x_np), put(accu_np)
        a, b = P.LockinLo(arms, LANES), P.LockinLo(arms, LANES)
        a.state.copy_(torch.from_numpy(LA.random_state(rng, 2, 2, LANES).view(np.int32)))
        b.state.copy_(a.state)
        lo = torch.full(((UPDATES << K) * LANES * 2,), -77, dtype=torch.int32, device=DEV)
        want, got = torch.full_like(lo, -77), torch.full_like(lo, -78)
        P.accu_lo(accu, lo, LANES, UPDATES, K, harmonic=3, offset=-99, layout=layout)
        a.process(x, lo, want, layout)
        assert b.process_accu(x, accu, got, K, harmonic=3, offset=-99, layout=layout) is got
        assert torch.equal(got, want) and torch.equal(a.state, b.state), layout
        with pytest.raises(ValueError):
            b.process_accu(x, accu, got, 25)
        with pytest.raises(ValueError):
            b.process_accu(x, accu, got[:-2], K)
        with pytest.raises(ValueError):
            b.process_accu(x, accu.cpu(), got, K)
        with pytest.raises(P.IdspError):
            b.process_accu(x, got[:accu.numel()], got, K)  # accu inside y
        assert torch.equal(a.state, b.state), "a rejected call moved the state"


def test_cpp_mirror(gpu):
    exe = os.path.join(ROOT, "build", "test_lockin_accu_gpu")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Iinclude", "tests/cpp/test_lockin_accu_gpu.cpp", "-Lidsp_amd/lib", "-lidsp_hip",
                    "-Wl,-rpath,$ORIGIN/../idsp_amd/lib", "-o", exe], cwd=ROOT, check=True, timeout=120)
    r = subprocess.run([exe], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "lockin_accu host-mirror tests passed" in r.stdout
