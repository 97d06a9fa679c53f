"""The phase consumers, the RPLL and the swept sine on every kernel `launch_stream` can send them to: the case table of
tests/_stream_proc_cases.py through the C ABI, each case on guarded buffers (tests/_guard.py) with poisoned outputs and random
states, every output element and state word compared with the specification by array_equal, and the kernel the call took held to
`expected_kernel` — the launcher's conditions restated from its source — prefix and suffix.

Two passes: buffers on torch's 512-byte grid (or where the case puts them), and x, y and state each one element into their
allocations.  Forms whose output element is 4 bytes also run in place.  The entries with kernels of their own (PFB, batch LO,
CORDIC) get the offset pass their own files lack.

`test_kernels_reached` prints, per form and layout, the distinct kernels the cases ran on (pytest -s)."""
import collections
import ctypes as C
import re

import numpy as np
import pytest
import torch

from idsp_amd import _abi
from tests import _cordic_spec as CS
from tests import _float_special as F
from tests import _harness as H
from tests import _pfb_spec as PF
from tests import _rpll_spec as RS
from tests import _stream_proc_cases as SP
from tests import test_gpu_accu_lo as TA
from tests import test_gpu_cordic as TC
from tests import test_gpu_pfb as TP
from tests._guard import Guards

pytestmark = pytest.mark.gpu
FM, LM = SP.FM, SP.LM
DEV = SP.DEV
REACHED = collections.defaultdict(set)  # (form, layout) -> kernel names with the processor's name cut out


def one_element_off(form):
    t = SP.TRAITS[form]
    return (t.in_bytes if t.has_in else 0, t.out_bytes, 4)


def _params():
    seen, out = set(), []
    for c in sorted(SP.CASES, key=lambda c: (c.form, c.lanes, c.frames, c.layout, c.x_off)):
        for name, off in (("grid", (c.x_off, c.y_off, 0)), ("one element off", one_element_off(c.form))):
            key = (c.form, c.layout, c.lanes, c.frames, off)
            if key not in seen:
                seen.add(key)
                out.append(pytest.param(c, off, id="%s-%s-%dx%d-%s-x%d-y%d" % (c.form, "FM" if c.layout == FM else "LM", c.lanes, c.frames, name.split()[0], off[0], off[1])))
    return out


def check_name(k, form, layout, lanes, frames, x_off, y_off, what):
    e = SP.expected_kernel(form, layout, lanes, frames, x_off, y_off)
    assert k.startswith(e), (what, k, "expected", e)
    assert k.endswith(e.suffix if e.suffix else ">"), (what, k, "expected the suffix", e.suffix)
    assert SP.TRAITS[form].proc in k, (what, k)
    REACHED[(form, layout)].add(re.sub(r"<.*>", "<P>", k))


def run_case(gpu, c, off, inplace):
    cfg, x, st, after, want = SP.reference(c.form, c.lanes, c.frames)
    names = []
    sg = st.copy()
    got = SP.run_form(gpu, c.form, cfg, sg, x, c.frames, c.layout, inplace=inplace, off=off, record=lambda n, k: names.append(k))
    what = (c, off, "in place" if inplace else "", names[0])
    assert got.dtype == want.dtype and got.shape == want.shape, what
    assert np.array_equal(got, want), what + (np.argwhere(got != want)[:4].tolist(),)
    assert np.array_equal(sg, after), what + ("state", np.argwhere(sg != after)[:4].tolist())
    # in place the input is also the output: y's offset is x's
    check_name(names[0], c.form, c.layout, c.lanes, c.frames, off[0], off[0] if inplace else off[1], what)


@pytest.mark.parametrize("c,off", _params())
def test_case(gpu, c, off):
    run_case(gpu, c, off, False)
    if c.form in SP.FOUR_BYTE and off[0] == off[1]:
        run_case(gpu, c, off, True)


@pytest.mark.parametrize("form", SP.FORMS)
def test_two_uneven_chunks_equal_one_call(gpu, form):
    cases = [c for c in SP.CASES if c.form == form and c.frames >= 2]
    for c in (cases[0], cases[len(cases) // 2], cases[-1]):
        cfg, x, st, after, want = SP.reference(c.form, c.lanes, c.frames)
        first = max(1, c.frames // 3)
        s1, s2 = st.copy(), st.copy()
        whole = SP.run_form(gpu, form, cfg, s1, x, c.frames, c.layout)
        parts = SP.run_form(gpu, form, cfg, s2, x, c.frames, c.layout, chunks=[first, c.frames - first])
        assert np.array_equal(whole, parts) and np.array_equal(s1, s2), (c, first)
        assert np.array_equal(whole, want) and np.array_equal(s1, after), c


@pytest.mark.parametrize("form", ["unwrap1", "pll2", "rpll", "sweep"])
def test_pairs_off_the_8_byte_grid_are_rejected_and_write_nothing(gpu, form):
    """an x or y of 8-byte elements that sits 4 bytes off the 8-byte grid is a caller error (include/idsp_hip.h): IDSP_EINVAL, and
    no byte of any buffer moves"""
    lanes, frames = 64, 16
    cfg, x, st, _, _ = SP.reference(form, lanes, frames + 1)
    t = SP.TRAITS[form]
    g = Guards(DEV)
    sd = g.upload("state", st, readonly=True)
    x0 = g.upload("x", x, readonly=True).data_ptr() if t.has_in else 0  # (the generator has no input: its x is ignored)
    yd = g.full("y", (frames + 1) * lanes * 2, torch.int32, SP.POISON)
    g.freeze("y")
    rows = [(x0, yd.data_ptr() + 4)] + ([(x0 + 4, yd.data_ptr()), (x0 + 4, yd.data_ptr() + 4)] if t.has_in and t.in_bytes == 8 else [])
    for layout in (FM, LM):
        for xp, yp in rows:
            rc = SP.call_form(gpu, form, cfg, sd.data_ptr(), xp, yp, lanes, frames, layout)
            assert rc == _abi.IDSP_EINVAL and gpu.err(), (form, layout, xp - x0, yp - yd.data_ptr(), rc)
        assert SP.call_form(gpu, form, cfg, sd.data_ptr(), x0, yd.data_ptr() + 8, lanes, 0, layout) == 0  # an empty call on the grid: nothing to do
    torch.cuda.synchronize()
    g.check(("rejected calls", form))


def test_kernels_reached(gpu):
    """Per form and layout, the kernels the cases ran on: printed (pytest -s; profiles/NOTES.md holds a copy), and held to what the table
    promises — every kernel `expected_kernel` names for a case of the table was reached, with its name asserted, on this GPU.  `REACHED` is
    filled by test_case; a case it does not hold yet (this test run alone, or first) is run here, so the assertion never rests on the order."""
    def key(e):
        return e[:-1] + "<P>" + e.suffix

    for c in SP.CASES:
        if key(SP.expected_kernel(c.form, c.layout, c.lanes, c.frames, c.x_off, c.y_off)) not in REACHED[(c.form, c.layout)]:
            run_case(gpu, c, (c.x_off, c.y_off, 0), False)
    for (form, layout), names in sorted(REACHED.items()):
        print(form, "FM" if layout == FM else "LM", len(names))
        for n in sorted(names):
            print("   ", n)
    for form in SP.FORMS:
        for layout in (FM, LM):
            want = {key(SP.expected_kernel(c.form, c.layout, c.lanes, c.frames, c.x_off, c.y_off)) for c in SP.CASES if (c.form, c.layout) == (form, layout)}
            assert want <= REACHED[(form, layout)], (form, layout, sorted(want - REACHED[(form, layout)]))
    for form in ("clamp", "unwrap0"):
        assert len(REACHED[(form, FM)]) >= 12, sorted(REACHED[(form, FM)])


# ------------------------------------------------------------------------------------------------ entries with kernels of their own
def pfb_run(gpu, cfg, st, x, layout, off, inplace=False):
    """tests/test_gpu_pfb.py's gpu_run with x, y and state `off` bytes into their allocations"""
    frames, lanes = x.shape[:2]
    g = Guards(DEV)
    sd = g.upload("state", st, off=off)
    xd = g.upload("x", TP.to_layout(x, layout), off=off, readonly=not inplace)
    yd = xd if inplace else g.upload("y", F.poison(lanes * frames * 8, np.float32), off=off)
    rc = gpu.fn["pfb_f32_process"](C.byref(cfg), C.c_void_p(sd.data_ptr()), C.c_void_p(xd.data_ptr()), C.c_void_p(yd.data_ptr()), lanes, frames, layout, None)
    assert rc == 0, gpu.err()
    torch.cuda.synchronize()
    name = gpu.last_kernel()
    g.check((name, lanes, frames, off, inplace))
    assert name == TP.NAMES[(layout, inplace)].format(T=TP.T, taps=cfg.taps), name
    st[...] = sd.cpu().numpy().view(np.uint32).reshape(st.shape)
    return TP.from_layout(yd.cpu().numpy(), layout, frames, lanes)


@pytest.mark.parametrize("layout", [FM, LM])
@pytest.mark.parametrize("off", [16, 32])
def test_pfb_bases_off_the_allocation_grid(gpu, layout, off):
    """x, y and state 16 and 32 bytes into their allocations (the entry asks for 16-byte alignment; 4 and 8 bytes off are rejected in
    tests/test_gpu_pfb.py): odd lane counts, frames across two time tiles, out of place and in place"""
    rng = np.random.default_rng(100 * off + layout)
    for taps, lanes, frames in ((8, 65, 2 * TP.T + 3), (3, 29, 7), (16, 200, TP.T + 1)):
        coeff = rng.standard_normal((taps, 4)).astype(np.float32)
        st = PF.random_state(rng, taps, lanes)
        x = rng.standard_normal((frames, lanes, 4, 2)).astype(np.float32)
        for dft, inplace in ((0, False), (1, False), (1, True)):
            sw, sg = st.copy(), st.copy()
            want = PF.bank_np(coeff, dft, sw, x)
            got = pfb_run(gpu, TP.make_cfg(coeff, dft), sg, x, layout, off, inplace)
            TP.same(want, got, sw, sg, (taps, layout, lanes, frames, dft, off, inplace))


@pytest.mark.parametrize("layout", [FM, LM])
def test_accu_lo_bases_16_and_32_bytes_off(gpu, layout):
    """accu and lo 16 and 32 bytes into their allocations, alone and mixed with 8 (tests/test_gpu_accu_lo.py has 0 and 8): rows on and off
    the 16-byte grid of the kernel's stores, odd lane and update counts, k = 0 and k > 0"""
    rng = np.random.default_rng(7 + layout)
    for lanes, updates, k in ((65, 3, 3), (1000, 5, 0), (63, 33, 1), (16385, 1, 3)):
        lo_cfg = (k, RS.LO_HARMONICS[(lanes + k) % len(RS.LO_HARMONICS)], int(rng.integers(-(1 << 31), 1 << 31)))
        accu = RS.adversarial_accu(rng, updates, lanes)
        want = RS.accu_lo_np(lo_cfg, accu)
        for off_in, off_out in ((16, 16), (32, 32), (16, 32), (32, 8), (8, 16)):
            got = TA.gpu_run(gpu, lo_cfg, accu, layout, off_in, off_out)
            assert np.array_equal(got, want), (lo_cfg, layout, lanes, updates, off_in, off_out)
            assert TA.KERNELS[(layout, lanes, updates, k)] == ("accu_lo_kernel[LaneMajor]" if layout == LM else "accu_lo_kernel[FrameMajor]")


@pytest.mark.parametrize("name", TC.NAMES)
def test_cordic_short_calls_at_bases_off_the_grid(gpu, name):
    """n = 1, 3, 4, 5 and 1027 (the kernel's body of n / 4 fours and its tail of n % 4 elements, each alone and together) with every buffer on
    the 16-byte grid — four elements per thread — and 4 or 8 bytes off it — one element per thread; tests/test_gpu_cordic.py has the short
    lengths on the grid only and the offsets at n = 1027 only.  The runner asserts the kernel's name from the offsets."""
    rng = np.random.default_rng(21)
    pair = CS.FUNCTIONS[name][2]
    for n in (1, 3, 4, 5, 1027):
        xy, z = TC.random_words(rng, (n, 2)), TC.random_words(rng, n)
        want, want0 = CS.function_np(name, xy, z), CS.function_np(name, xy)
        for xy_off, z_off, out_off in ((0, 0, 0), (8, 8, 8), (0, 4, 8 if pair else 4), (8, 0, 0), (0, 0, 8)):
            TC.same(want, TC.gpu_run(gpu, name, xy, z, xy_off=xy_off, z_off=z_off, out_off=out_off), (name, n, xy_off, z_off, out_off))
            assert ("four" in gpu.last_kernel()) == (xy_off == z_off == out_off == 0), gpu.last_kernel()
        TC.same(want0, TC.gpu_run(gpu, name, xy, xy_off=8, out_off=8), (name, n, "z = NULL", 8))
        TC.same(want0, TC.gpu_run(gpu, name, xy), (name, n, "z = NULL", 0))
        assert "four" in gpu.last_kernel(), gpu.last_kernel()
