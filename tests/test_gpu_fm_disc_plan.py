"""idsp_fm_disc_i32 and idsp_dds_i32 held to the table of tests/_fm_disc_plan_cases.py on the GPU: every `gpu` row is one real call
through `GpuBackend` (guard bands, poisoned outputs; under IDSP_TEST_STREAM=1 the arrangement of tests/_on_stream.py) on random inputs and a
random state; `idsp_last_kernel()` must start with the row's name (DDS: name the row's stream processor), and outputs and written-back
state must equal the oracle's bit for bit.  tests/test_fm_disc_plan.py holds `plan_fm_disc` / `plan_dds` to the same rows without a GPU,
launch parameters included; the stagger ticks are a kernel argument, not a name, and are held there only.

A misaligned row puts its own buffer that many bytes off the 16-byte grid.  Rows with switches run in a fresh child process per switch set
(the library reads them once per process), as tests/test_gpu_resample_plan.py does.  Reference: examples/fm_disc.rs:25-50,
src/accu.rs:34-41, src/cossin.rs:14-67."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from idsp_amd import _abi
from tests import _fm_disc_plan_cases as R
from tests import _harness as H
from tests._backends import OracleBackend
from tests.test_gpu_resample_plan import RowBackend

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCH_SETS = sorted({json.dumps(c.sw, sort_keys=True) for c in R.FM_DISC_CASES + R.DDS_CASES if c.gpu and c.sw})
# the table's names hold unless another dispatch is in force: IDSP_TEST_MISALIGN moves every buffer, and IDSP_DIAG lets the environment
# choose (the children of test_switches run under exactly the switches of their rows: there the names hold)
NAMES_HOLD = not os.environ.get("IDSP_TEST_MISALIGN") and (__name__ == "__main__" or not os.environ.get("IDSP_DIAG"))
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1


def fm_disc_row(ob, gb, c, rng):
    cfg = _abi.FmDisc()
    cfg.carrier = int(rng.integers(I32_MIN, I32_MAX))
    cfg.deemph.ba[:] = [int(v) for v in rng.integers(-(1 << 29), 1 << 29, size=5)]
    cfg.deemph.frac = int(rng.integers(20, 31))
    init = np.zeros((7, c.lanes), np.uint32)
    init[0, ::3] = 1  # two lanes of three start without a previous sample
    init[1:] = rng.integers(0, 1 << 32, size=(6, c.lanes), dtype=np.uint64).astype(np.uint32)
    so, sg = init.copy(), init.copy()
    layout = H.LM if c.layout == "LM" else H.FM
    gb.offs = {"x": c.off[0], "y": c.off[1]}
    for part in range(2):  # the second call continues from the state the first wrote back
        x = rng.integers(I32_MIN, I32_MAX, size=2 * c.lanes * c.frames, dtype=np.int64, endpoint=True).astype(np.int32)
        rco, yo = ob.cfgcall("fm_disc_i32", cfg, so, x, (c.lanes * c.frames,), np.int32, c.lanes, c.frames, layout)
        rcg, yg = gb.cfgcall("fm_disc_i32", cfg, sg, x, (c.lanes * c.frames,), np.int32, c.lanes, c.frames, layout)
        assert rco == 0 and rcg == 0, (R.fm_disc_line(c), H.engine().err())
        took = H.engine().last_kernel()
        assert not NAMES_HOLD or (took.startswith(c.name) and (took == c.name or c.name == "stream_")), (R.fm_disc_line(c), took, c.name)
        assert np.array_equal(yo, yg), (R.fm_disc_line(c), part)
        assert np.array_equal(so, sg), (R.fm_disc_line(c), part, "state")


def dds_row(ob, gb, c, rng):
    st = rng.integers(0, 1 << 32, size=(2, c.lanes), dtype=np.uint64).astype(np.uint32)
    so, sg = st.copy(), st.copy()
    layout = H.LM if c.layout == "LM" else H.FM
    gb.offs = {}
    rco, yo = ob.dds(so, c.lanes, c.frames, layout)
    rcg, yg = gb.dds(sg, c.lanes, c.frames, layout)
    assert rco == 0 and rcg == 0, (R.dds_line(c), H.engine().err())
    took = H.engine().last_kernel()
    assert not NAMES_HOLD or (took.startswith("stream_") and "::" + c.proc + ">" in took), (R.dds_line(c), took, c.proc)
    assert np.array_equal(yo, yg), R.dds_line(c)
    assert np.array_equal(so, sg), (R.dds_line(c), "state")


def run_rows(rows):
    ob, gb, rng = OracleBackend(), RowBackend(), np.random.default_rng(1618)
    for c in rows:
        (fm_disc_row if isinstance(c, R.FmDisc) else dds_row)(ob, gb, c, rng)


@pytest.mark.parametrize("family,layout", [(f, lay) for f in ("fm_disc", "dds") for lay in ("FM", "LM")])
def test_default_dispatch(gpu, family, layout):
    rows = [c for c in (R.FM_DISC_CASES if family == "fm_disc" else R.DDS_CASES) if c.gpu and not c.sw and c.layout == layout]
    assert rows
    run_rows(rows)


@pytest.mark.parametrize("switches", SWITCH_SETS, ids=lambda s: ",".join("%s=%s" % (k[5:], v) for k, v in json.loads(s).items() if k != "IDSP_DIAG"))
def test_switches(gpu, switches):
    env = dict(os.environ, **json.loads(switches))
    r = subprocess.run([sys.executable, "-m", "tests.test_gpu_fm_disc_plan", switches], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("rows ok"), r.stdout[-3000:] + r.stderr[-3000:]


if __name__ == "__main__":  # the child of test_switches: the rows of one switch set, which the parent has put into the environment
    rows = [c for c in R.FM_DISC_CASES + R.DDS_CASES if c.gpu and c.sw and json.dumps(c.sw, sort_keys=True) == sys.argv[1]]
    assert rows
    run_rows(rows)
    print(len(rows), "rows ok")
