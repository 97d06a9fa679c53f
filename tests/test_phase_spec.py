"""The phase consumers without a GPU: the specification (tests/_phase_spec.py) against what the reference asserts in its own unit
tests (tests/golden/phase_kat.json: src/unwrap.rs:202-270, src/pll.rs:117-150), its two restatements against each other on random
and adversarial inputs, and the host-side pieces of the library and of idsp_amd.process (coefficient builders, argument checks,
`overflowing_sub`, `saturating_scale`) against the specification.  The library loads without a GPU."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

from idsp_amd import _abi
from idsp_amd._abi import PHASE  # the feature's prototype table
from tests import _phase_spec as S

KAT = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "phase_kat.json")))


def _fn():
    from idsp_amd._lib import load

    return load()[0]


# ------------------------------------------------------------------------------------------- the reference's own rows
def test_fixture_is_complete():
    assert len(KAT["overflowing_sub"]["rows"]) == 19 and len(KAT["saturating_scale"]["rows"]) == 22 and KAT["saturating_scale"]["shift"] == 8


def test_overflowing_sub_rows_on_the_scalar_spec():
    for x0, x1, wrap in KAT["overflowing_sub"]["rows"]:
        dx, w = S.overflowing_sub(x1, x0)
        assert w == wrap, (x0, x1)
        assert dx == S.w32(x1 - x0)                       # src/unwrap.rs:228-230: i32::overflowing_sub agrees
        assert (w != 0) == (not S.I32_MIN <= x1 - x0 <= S.I32_MAX)


def test_saturating_scale_rows_on_the_scalar_spec():
    shift = KAT["saturating_scale"]["shift"]
    for lo, hi, res in KAT["saturating_scale"]["rows"]:
        assert S.saturating_scale(lo, hi, shift) == res, (lo, hi)


def test_overflowing_sub_rows_on_the_host_function():
    from idsp_amd.process import overflowing_sub

    for x0, x1, wrap in KAT["overflowing_sub"]["rows"]:
        assert overflowing_sub(x1, x0) == (S.w32(x1 - x0), wrap), (x0, x1)


def test_saturating_scale_rows_on_the_host_function():
    from idsp_amd.process import saturating_scale

    shift = KAT["saturating_scale"]["shift"]
    for lo, hi, res in KAT["saturating_scale"]["rows"]:
        assert saturating_scale(lo, hi, shift) == res, (lo, hi)
    with pytest.raises(ValueError):
        saturating_scale(0, 0, 0)


def test_host_functions_equal_the_spec_on_random_arguments():
    from idsp_amd.process import overflowing_sub, saturating_scale

    rng = np.random.default_rng(3)
    edge = [S.I32_MIN, S.I32_MIN + 1, -1, 0, 1, S.I32_MAX - 1, S.I32_MAX]
    for _ in range(4000):
        a, b = (int(rng.choice(edge)) if rng.random() < 0.3 else int(rng.integers(S.I32_MIN, S.I32_MAX + 1)) for _ in range(2))
        assert overflowing_sub(a, b) == S.overflowing_sub(a, b)
        shift = int(rng.integers(1, 32))  # (shift 32 is `lo >> 32` on an i32: a panic in the reference's debug build)
        hi = int(rng.integers(-(1 << shift), (1 << shift) + 1)) if rng.random() < 0.7 else b
        assert saturating_scale(a, hi, shift) == S.saturating_scale(a, hi, shift)


# ---------------------------------------------------------------------------------------- convergence (src/pll.rs:117-150)
def _abs32(v):
    return S.w32(abs(S.w32(v)))  # `W<i32>::abs`: wrapping


@pytest.mark.parametrize("name", ["converge_pll", "converge_narrow"])
def test_convergence_on_the_scalar_spec(name):
    k = KAT[name]
    ba = S.pll_from_bandwidth(k["bandwidth"], k["split"])
    s, acc, step = S.PLLState(), k["accu_state"], k["accu_step"]
    worst_f = worst_p = 0
    for i in range(k["n"]):
        acc = S.w32(acc + step)
        y = S.pll_process(ba, s, acc)
        if i > k["bounds_apply_for_i_greater_than"]:
            df, dp = _abs32(step + s.frequency()), _abs32(acc + y)
            worst_f, worst_p = max(worst_f, df), max(worst_p, dp)
            assert df <= k["frequency_bound"] and dp <= k["phase_bound"], (i, df, dp)
    print(name, "worst |step + frequency|", worst_f, "worst |x + y|", worst_p)


@pytest.mark.parametrize("name", ["converge_pll", "converge_narrow"])
def test_convergence_on_the_numpy_spec(name):
    k = KAT[name]
    ba = S.pll_from_bandwidth(k["bandwidth"], k["split"])
    n, step = k["n"], k["accu_step"]
    x = ((np.arange(1, n + 1, dtype=np.uint64) * np.uint64(step) + np.uint64(k["accu_state"])) & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32)
    st = np.zeros((S.PLL_WORDS, 1), np.uint32)
    out = S.pll_np(ba, st, x.reshape(n, 1), output=2).astype(np.int64)
    wrap_abs = lambda v: np.abs(((v + (1 << 31)) % (1 << 32)) - (1 << 31))  # noqa: E731  (no i32::MIN occurs below the bounds)
    sel = np.arange(n) > k["bounds_apply_for_i_greater_than"]
    assert (wrap_abs(step + out[sel, 0, 1]) <= k["frequency_bound"]).all()
    assert (wrap_abs(x.astype(np.int64)[sel] + out[sel, 0, 0]) <= k["phase_bound"]).all()


def test_coefficients_of_the_convergence_tests():
    """not reference-asserted: derived here from the spec's f32 restatement; the third coefficient of the wide loop saturates"""
    wide = S.pll_from_bandwidth(5e-2, 4.0)
    assert wide[2] == S.I32_MIN and wide[0] < 0 < wide[1]
    narrow = S.pll_from_bandwidth(8e-5, 4.0)
    assert all(S.I32_MIN < v < S.I32_MAX for v in narrow) and narrow[0] < 0 < narrow[1] and narrow[2] < 0
    fn = _fn()
    for bw, want in ((5e-2, wide), (8e-5, narrow)):
        ba = (C.c_int32 * 3)()
        assert fn["pll_from_bandwidth"](bw, 4.0, ba) == 0 and list(ba) == want


# ------------------------------------------------------------------------------------------------- scalar == numpy
def _scalar_run(form, ba, st, x):
    """the scalar spec lane by lane on word-plane state; returns outputs shaped like the numpy spec's and the final words"""
    frames, lanes = x.shape
    words = st.shape[0]
    out_state = np.empty_like(st)
    if form in ("pll0", "pll1"):
        y = np.empty((frames, lanes), np.int64)
    elif form == "pll2":
        y = np.empty((frames, lanes, 2), np.int64)
    else:
        y = np.empty((frames, lanes), np.int64)
    for l in range(lanes):
        w = [int(st[i, l]) for i in range(words)]
        if form.startswith("pll"):
            s = S.PLLState.from_words(w)
            for f in range(frames):
                ph = S.pll_process(ba, s, int(x[f, l]))
                if form == "pll0":
                    y[f, l] = ph
                elif form == "pll1":
                    y[f, l] = s.frequency()
                else:
                    y[f, l] = (ph, s.frequency())
        elif form.startswith("unwrap"):
            s = S.Unwrapper.from_words(w)
            for f in range(frames):
                dx = s.process(int(x[f, l]))
                y[f, l] = dx if form == "unwrap0" else s.phase()
        else:
            s = S.ClampWrap.from_words(w)
            for f in range(frames):
                y[f, l] = s.process(int(x[f, l]))
        out_state[:, l] = s.words()
    return y, out_state


def _numpy_run(form, ba, st, x):
    if form.startswith("pll"):
        return S.pll_np(ba, st, x, output=int(form[-1]))
    if form.startswith("unwrap"):
        return S.unwrap_np(st, x, mode=int(form[-1]))
    return S.clamp_wrap_np(st, x)


FORMS = ["pll0", "pll1", "pll2", "unwrap0", "unwrap1", "clamp"]
WORDS = {"pll0": 9, "pll1": 9, "pll2": 9, "unwrap0": 2, "unwrap1": 2, "clamp": 2}


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("zero_state", [True, False])
def test_scalar_equals_numpy(form, zero_state):
    rng = np.random.default_rng(2 * FORMS.index(form) + int(zero_state))
    lanes, frames = 40, 300
    for trial in range(3):
        ba = S.random_ba(rng)
        x = S.adversarial_phases(rng, frames, lanes) if trial else rng.integers(S.I32_MIN, S.I32_MAX + 1, size=(frames, lanes)).astype(np.int32)
        st = np.zeros((WORDS[form], lanes), np.uint32) if zero_state else S.random_state(rng, WORDS[form], lanes)
        ys, ss = _scalar_run(form, ba, st.copy(), x)
        sn = st.copy()
        yn = _numpy_run(form, ba, sn, x)
        assert np.array_equal(ys, yn.astype(np.int64)), (form, trial)
        assert np.array_equal(ss, sn), (form, trial)


def test_numpy_spec_in_chunks_equals_one_call():
    rng = np.random.default_rng(11)
    x = S.adversarial_phases(rng, 200, 17)
    for form in FORMS:
        ba = S.random_ba(rng)
        st = S.random_state(rng, WORDS[form], 17)
        a, b = st.copy(), st.copy()
        whole = _numpy_run(form, ba, a, x)
        parts = np.concatenate([_numpy_run(form, ba, b, x[:7]), _numpy_run(form, ba, b, x[7:130]), _numpy_run(form, ba, b, x[130:])])
        assert np.array_equal(whole, parts) and np.array_equal(a, b), form


def test_unwrapper_wraps_read_out():
    rng = np.random.default_rng(5)
    st = S.random_state(rng, 2, 500)
    st[1, :100] = rng.integers(-3, 3, size=100).astype(np.int32).view(np.uint32)  # a few wraps either way
    for shift in (1, 8, 31, 32, 33, 40):
        want = [S.Unwrapper.from_words(st[:, l]).wraps(shift) for l in range(st.shape[1])]
        assert np.array_equal(S.unwrap_wraps_np(st, shift), np.array(want, dtype=np.int32)), shift


# ------------------------------------------------------------------------------------------------ library, host side
def test_phase_table_is_exported():
    assert set(PHASE) == {"clamp_wrap_i32", "unwrap_i32", "unwrap_i32_phase", "pll_state_words", "pll_i32", "pll_from_zpk", "pll_from_bandwidth"}
    assert set(PHASE) <= set(_abi.UTILS) and set(PHASE) <= set(_abi.exported_names()) and set(PHASE) <= set(_fn())
    assert not set(PHASE) & (set(_abi.PROCESSING) | set(_abi.HELPERS))  # product only: the checker library has no twin


def test_pll_state_words():
    assert _fn()["pll_state_words"]() == 9 == _abi.PLL_STATE_WORDS == S.PLL_WORDS


def _special(rng):
    r = rng.random()
    if r < 0.04:
        return math.nan
    if r < 0.08:
        return math.inf * (1 if rng.random() < 0.5 else -1)
    if r < 0.2:
        return float(rng.uniform(-1, 1)) * 10.0 ** float(rng.uniform(0, 12))  # saturating
    if r < 0.3:
        return float(rng.uniform(-1, 1)) * 10.0 ** float(rng.uniform(-12, 0))
    return float(rng.uniform(-2, 2))


def test_library_coefficient_builders_equal_the_f32_spec():
    fn = _fn()
    rng = np.random.default_rng(7)
    saturated = nans = 0
    for _ in range(4000):
        z, p, g = _special(rng), _special(rng), _special(rng)
        ba = (C.c_int32 * 3)()
        assert fn["pll_from_zpk"](z, p, g, ba) == 0
        want = S.pll_from_zpk(z, p, g)
        assert list(ba) == want, (z, p, g)
        saturated += any(v in (S.I32_MIN, S.I32_MAX) for v in want)
        nans += any(math.isnan(v) for v in (z, p, g))
        bw = float(rng.uniform(7e-5, 5e-2)) if rng.random() < 0.7 else _special(rng)
        split = float(rng.uniform(1, 8)) if rng.random() < 0.8 else _special(rng)
        assert fn["pll_from_bandwidth"](bw, split, ba) == 0
        assert list(ba) == S.pll_from_bandwidth(bw, split), (bw, split)
    assert saturated > 100 and nans > 100
    # ties round away from zero, and the argument is narrowed to f32 first
    for v, want in ((1.5 / 2 ** 32, 2), (-1.5 / 2 ** 32, -2), (0.5 / 2 ** 32, 1), (-0.5 / 2 ** 32, -1), (0.5, S.I32_MAX), (-0.5, S.I32_MIN), (0.1, int(np.float32(0.1) * np.float32(2.0 ** 32)))):
        ba = (C.c_int32 * 3)()
        assert fn["pll_from_zpk"](0.0, 1.0, v, ba) == 0 and ba[0] == want == S.q32_from_f32(v), v
    assert fn["pll_from_zpk"](0.0, 0.0, 0.0, None) == _abi.IDSP_EINVAL
    assert fn["pll_from_bandwidth"](0.01, 4.0, None) == _abi.IDSP_EINVAL


def test_host_mirror_builders_use_the_library():
    from idsp_amd.process import PLL

    assert PLL.from_bandwidth(5e-2, 4.0).ba == S.pll_from_bandwidth(5e-2, 4.0)
    assert PLL.from_zpk(0.9, 0.5, -0.01).ba == S.pll_from_zpk(0.9, 0.5, -0.01)
    assert PLL([1 << 31, -1, 5]).ba == [S.I32_MIN, -1, 5]
    with pytest.raises(ValueError):
        PLL([1, 2])


def test_argument_checks_return_einval():
    """a null pointer, an unknown layout and an unknown `output` are IDSP_EINVAL before anything touches a device"""
    fn = _fn()
    E = _abi.IDSP_EINVAL
    buf = (C.c_int32 * 64)()
    p = C.cast(buf, C.c_void_p)
    ba = (C.c_int32 * 3)(1, 2, 3)
    for name in ("clamp_wrap_i32", "unwrap_i32", "unwrap_i32_phase"):
        assert fn[name](None, p, p, 4, 4, 0, None) == E, name
        assert fn[name](p, None, p, 4, 4, 0, None) == E, name
        assert fn[name](p, p, None, 4, 4, 0, None) == E, name
        assert fn[name](p, p, p, 4, 4, 2, None) == E, name
        assert fn[name](p, p, p, 4, 4, -1, None) == E, name
    assert fn["pll_i32"](None, p, p, p, 4, 4, 0, 0, None) == E
    assert fn["pll_i32"](ba, None, p, p, 4, 4, 0, 0, None) == E
    assert fn["pll_i32"](ba, p, None, p, 4, 4, 0, 0, None) == E
    assert fn["pll_i32"](ba, p, p, None, 4, 4, 0, 0, None) == E
    assert fn["pll_i32"](ba, p, p, p, 4, 4, 2, 0, None) == E
    assert fn["pll_i32"](ba, p, p, p, 4, 4, 0, 3, None) == E
    assert fn["pll_i32"](ba, p, p, p, 4, 4, 0, -1, None) == E
    assert b"output" in fn["last_error"]()
    # nothing to do: no launch, no device needed
    for name in ("clamp_wrap_i32", "unwrap_i32", "unwrap_i32_phase"):
        assert fn[name](p, p, p, 0, 4, 0, None) == 0 and fn[name](p, p, p, 4, 0, 1, None) == 0
    assert fn["pll_i32"](ba, p, p, p, 0, 4, 0, 2, None) == 0 and fn["pll_i32"](ba, p, p, p, 4, 0, 1, 0, None) == 0


def test_host_mirror_rejects_cpu_tensors():
    import torch

    from idsp_amd.process import ClampWrap, PLL, Unwrapper

    for make in (lambda: PLL([1, 2, 3]).lanes(4, device="cpu"), lambda: Unwrapper().lanes(4, device="cpu"), lambda: ClampWrap().lanes(4, device="cpu")):
        with pytest.raises(ValueError):
            make()
    with pytest.raises(ValueError):
        PLL([1, 2, 3]).lanes(4, output="amplitude")
    with pytest.raises(ValueError):
        Unwrapper().lanes(4, output="wraps")
    del torch
