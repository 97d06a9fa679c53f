"""The half-band and Cic entries held to the table of tests/_resample_plan_cases.py on the GPU: every `gpu` row is one real call through
`GpuBackend` (guard bands, poisoned outputs; under IDSP_TEST_STREAM=1 the arrangement of tests/_on_stream.py) on random inputs and a random
state; `idsp_last_kernel()` must start with the row's name, and outputs and written-back state must equal the oracle's — bit for bit
(`assert_same_float` for the f32 half-band, `np.array_equal` for Cic).  tests/test_resample_plan.py holds `plan_hbf` / `plan_cic` to the same
rows without a GPU, launch parameters included; the Cic tile form, whose recorded name is the plain lane kernel's, is told apart there only.

A misaligned row puts its own buffer one element off the 16-byte grid.  Rows with switches run in a fresh child process per switch set (the
library reads them once per process), as tests/test_gpu_lockin_plan.py does.  Reference: src/hbf.rs:142-236, src/cic.rs:34-201."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from idsp_amd import _abi
from tests import _cic_cases as K
from tests import _harness as H
from tests import _resample_plan_cases as R
from tests._backends import GpuBackend, OracleBackend
from tests._float_special import assert_same_float

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCH_SETS = sorted({json.dumps(c.sw, sort_keys=True) for c in R.HBF_CASES + R.CIC_CASES if c.gpu and c.sw})
# the table's names hold unless another dispatch is in force: IDSP_TEST_MISALIGN moves every buffer, and IDSP_DIAG lets the environment
# choose (the children of test_switches run under exactly the switches of their rows: there the names hold)
NAMES_HOLD = not os.environ.get("IDSP_TEST_MISALIGN") and (__name__ == "__main__" or not os.environ.get("IDSP_DIAG"))


class RowBackend(GpuBackend):
    """GpuBackend whose buffers of a given role ("x", "y") start `offs[role]` bytes into their allocation"""
    offs = {}

    def _row_off(self, role, itemsize):
        return self.offs.get(role) or self._off(itemsize)

    def _alloc(self, n, dtype, role="y"):
        return self.g.empty(role, int(n), dtype, self._row_off(role, self.torch.empty(0, dtype=dtype).element_size()))

    def _up(self, a, role, readonly=False):
        a = np.ascontiguousarray(a)
        return self.g.upload(role, a, self._row_off(role, a.dtype.itemsize), readonly)

    def _stage(self, c, a, role, readonly=False):
        a = np.ascontiguousarray(a)
        return c.stage(role, a, self._row_off(role, a.dtype.itemsize), readonly)

    def _out(self, c, n, dtype, fill):
        return c.out("y", n, dtype, fill, self._row_off("y", self.torch.empty(0, dtype=dtype).element_size()))


def hbf_row(ob, gb, c, rng):
    if c.tap_set >= 0:
        cfg = _abi.HbfCascadeF32()
        assert H.oracle().fn[f"hbf_{c.kind}_cascade"](c.tap_set, c.stages, C.byref(cfg)) == 0
    else:  # tap counts without a specialised instance
        cfg = H.hbf_cfg([(rng.standard_normal(m) * 0.3).astype(np.float32).tolist() for m in (7, 1, 9, 4, 5)[:c.stages]])
    rate = 1 << c.stages
    words = H.oracle().fn[f"hbf_{c.kind}_state_words"](C.byref(cfg))
    nin, nout = (c.frames * rate, c.frames) if c.kind == "dec" else (c.frames, c.frames * rate)
    so = rng.standard_normal(size=(words, c.lanes)).astype(np.float32).view(np.uint32)
    sg = so.copy()
    x = rng.standard_normal(size=c.lanes * nin).astype(np.float32)
    layout = H.LM if c.layout == "LM" else H.FM
    gb.offs = {"x" if c.kind == "dec" else "y": c.off}
    rco, yo = ob.cfgcall(f"hbf_{c.kind}_f32", cfg, so, x, (c.lanes * nout,), np.float32, c.lanes, c.frames, layout)
    rcg, yg = gb.cfgcall(f"hbf_{c.kind}_f32", cfg, sg, x, (c.lanes * nout,), np.float32, c.lanes, c.frames, layout)
    assert rco == 0 and rcg == 0, (R.hbf_line(c), H.engine().err())
    took = H.engine().last_kernel()
    assert not NAMES_HOLD or took.startswith(c.name), (R.hbf_line(c), took, c.name)
    assert_same_float(yo, yg, R.hbf_line(c))
    assert_same_float(so.view(np.float32), sg.view(np.float32), (R.hbf_line(c), "state"))


def cic_row(ob, gb, c, rng):
    dtype = np.int64 if c.bits == 64 else np.int32
    cfg = _abi.Cic(c.order, 1 + c.order % 4, c.rate)
    words = K.state_words(gb, cfg, dtype)
    so = K.random_state(rng, words, c.lanes)
    sg = so.copy()
    x = K.samples(rng, dtype, c.lanes * c.frames * (c.rate + 1 if c.kind == "dec" else 1))
    layout = K.LM if c.layout == "LM" else K.FM
    gb.offs = {"x": c.off[0], "y": c.off[1]}
    rco, yo = K.run(ob, c.kind, dtype, cfg, so, x, c.lanes, c.frames, layout)
    rcg, yg = K.run(gb, c.kind, dtype, cfg, sg, x, c.lanes, c.frames, layout)
    assert rco == 0 and rcg == 0, (R.cic_line(c), H.engine().err())
    took = H.engine().last_kernel()
    assert not NAMES_HOLD or took.startswith(c.name), (R.cic_line(c), took, c.name)
    assert np.array_equal(yo, yg), R.cic_line(c)
    assert np.array_equal(so, sg), (R.cic_line(c), "state")


def run_rows(rows):
    ob, gb, rng = OracleBackend(), RowBackend(), np.random.default_rng(2718)
    for c in rows:
        (hbf_row if isinstance(c, R.Hbf) else cic_row)(ob, gb, c, rng)


@pytest.mark.parametrize("family,kind", [(f, k) for f in ("hbf", "cic32", "cic64") for k in ("dec", "int")])
def test_default_dispatch(gpu, family, kind):
    if family == "hbf":
        rows = [c for c in R.HBF_CASES if c.gpu and not c.sw and c.kind == kind]
    else:
        rows = [c for c in R.CIC_CASES if c.gpu and not c.sw and c.kind == kind and c.bits == int(family[3:])]
    assert rows
    run_rows(rows)


@pytest.mark.parametrize("switches", SWITCH_SETS, ids=lambda s: ",".join(k[5:] for k in json.loads(s) if k != "IDSP_DIAG"))
def test_switches(gpu, switches):
    env = dict(os.environ, **json.loads(switches))
    r = subprocess.run([sys.executable, "-m", "tests.test_gpu_resample_plan", switches], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("rows ok"), r.stdout[-3000:] + r.stderr[-3000:]


if __name__ == "__main__":  # the child of test_switches: the rows of one switch set, which the parent has put into the environment
    rows = [c for c in R.HBF_CASES + R.CIC_CASES if c.gpu and c.sw and json.dumps(c.sw, sort_keys=True) == sys.argv[1]]
    assert rows
    run_rows(rows)
    print(len(rows), "rows ok")
