"""Self-test of tests/_guard.py without any kernel of the library: one byte changed by torch indexing just before or just behind
the valid region, or inside a read-only input, must fail `Guards.check` with the buffer's role, the side and that byte's position;
untouched buffers must pass.  With and without an offset of the view inside its allocation."""
import numpy as np
import pytest
import torch

from tests import _guard

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("off_elems", [0, 1, 3])  # the view starts this many elements into the 512-byte grid
@pytest.mark.parametrize("dtype,n", [(torch.int32, 37), (torch.float32, 1), (torch.int64, 5), (torch.float64, 129)])
def test_one_byte_on_either_side_is_found_and_named(gpu, dtype, n, off_elems):
    item = torch.empty(0, dtype=dtype).element_size()
    off, nbytes = off_elems * item, n * item

    def fresh():
        g = _guard.Guards()
        x = g.upload("x", np.arange(11, dtype=np.int32), off=4 if off else 0, readonly=True)
        y = g.full("y", n, dtype, -77 if dtype in (torch.int32, torch.int64) else float("nan"), off=off)
        s = g.upload("state", np.arange(6, dtype=np.uint32).reshape(2, 3))
        return g, x, y, s

    g, x, y, s = fresh()
    assert y.data_ptr() % 512 == off and y.numel() == n and y.dtype == dtype and s.shape == (2, 3)
    torch.cuda.synchronize()
    g.check("untouched")
    y.fill_(3)  # writing the whole valid region, and the state, is what a call does
    s.fill_(-1)
    torch.cuda.synchronize()
    g.check("valid regions written")

    raw, lo, hi = g.bufs[1].raw, g.bufs[1].lo, g.bufs[1].hi
    assert (lo, hi) == (_guard.G + off, _guard.G + off + nbytes)
    for at, side, rel in ((lo - 1, "before", -1), (hi, "after", nbytes), (0, "before", -lo), (raw.numel() - 1, "after", nbytes + _guard.G - 1)):
        g, x, y, s = fresh()
        g.bufs[1].raw[at] = 0  # what a stray store of zeros, or of one poison byte, leaves
        torch.cuda.synchronize()
        with pytest.raises(_guard.GuardError) as err:
            g.check("some_op")
        msg = str(err.value)
        assert "some_op" in msg and "`y`" in msg and side in msg and f"offset {rel:+d} " in msg, msg

    # the first changed byte is the one reported; state and x are named by their roles
    g, x, y, s = fresh()
    g.bufs[2].raw[g.bufs[2].hi + 3] = 1
    g.bufs[2].raw[g.bufs[2].hi + 9] = 1
    with pytest.raises(_guard.GuardError, match=r"`state`.*after.*offset \+27 "):  # 24 bytes of state, then byte 3 of the band
        g.check("op")
    g, x, y, s = fresh()
    x[7] = 5
    with pytest.raises(_guard.GuardError, match=r"`x`: read-only input modified.*offset \+28 .*inside"):
        g.check("op")
    g, x, y, s = fresh()
    g.bufs[0].raw[g.bufs[0].lo - 2] = 7
    with pytest.raises(_guard.GuardError, match=r"`x`: stray write before.*offset -2 "):
        g.check("op")


def test_sentinel_is_no_poison_and_no_zero(gpu):
    g = _guard.Guards()
    assert int(g.empty("a", 1, torch.int32)[0]) not in (0, -77)
    f = float(g.empty("b", 1, torch.float32)[0])
    d = float(g.empty("c", 1, torch.float64)[0])
    assert f == f and f != 0 and d == d and d != 0
    assert int(g.empty("d", 1, torch.int64)[0]) not in (0, -77)
    assert _guard.G % 512 == 0
    e = g.empty("e", 0, torch.int32)  # empty buffers (zero frames) are legal and checked
    assert e.numel() == 0
    torch.cuda.synchronize()
    g.check("empty")
