"""The swept-sine specification (tests/_sweep_spec.py) against itself, against the reference's own figures
(tests/golden/sweep_kat.json, from src/sweptsine.rs:197-235) and against the library's host functions.  No GPU.

The issue's table of corner states calls `negative state, any rate` never ending and `i64::MIN, negative rate` ending going down.
The arithmetic of `Sweep::next` says otherwise — a negative state with a POSITIVE rate grows downwards and ends, with a negative rate
it decays and never ends (at i64::MIN too) — and the golden file records what the arithmetic gives, row by row."""
import ctypes as C
import json
import math
import os
import subprocess

import numpy as np
import pytest

from idsp_amd import _abi
from idsp_amd._abi import SWEEP  # noqa: F401  (the feature's prototype table)
from oracle import spec as O
from tests import _sweep_spec as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KAT = json.load(open(os.path.join(ROOT, "tests", "golden", "sweep_kat.json")))


def isclose(a, b, rtol, atol):
    return abs(a - b) <= atol + rtol * abs(b)


# ---- the two restatements
def test_cossin_np_is_oracle_spec_cossin():
    rng = np.random.default_rng(0)
    edges = np.array([o * (1 << 29) + d for o in range(8) for d in (-2, -1, 0, 1, 2, 1 << 14, (1 << 14) - 1, 1 << 22, (1 << 22) - 1)], np.int64)
    ph = np.concatenate([edges, rng.integers(0, 1 << 32, 60000), np.arange(0, 1 << 32, 65537 * 3)]).astype(np.uint32).view(np.int32)
    c, s = S.cossin_np(ph)
    want = np.array([O.cossin(int(p)) for p in ph], np.int64)
    assert np.array_equal(c, want[:, 0]) and np.array_equal(s, want[:, 1])
    assert not ((c == 0) & (s == 0)).any()  # (0, 0) marks an ended lane: cossin never returns it


@pytest.mark.parametrize("frames", [1, 3, 17, 257])
def test_generator_restatements_agree(frames):
    rng = np.random.default_rng(frames)
    for variant in range(3):
        st = S.population(rng, 203, frames, boundary=max(frames // 2, 1), variant=variant)
        a, b = st.copy(), st.copy()
        assert np.array_equal(S.osc_int(a, frames), S.osc_np(b, frames)) and np.array_equal(a, b)
        inside, before, never = S.classify(st, b, frames)
        assert before.any() and never.any() and (inside.any() or frames == 1)
        assert np.array_equal(a[4], st[4])  # the rate never moves
        # ended is ended: more frames change nothing
        c = b.copy()
        more = S.osc_np(c, 5)
        gone = S.ended_np(b)
        assert gone.any() and not more[:, gone].any() and np.array_equal(c[:, gone], b[:, gone])


def test_chunks_equal_one_call():
    rng = np.random.default_rng(5)
    st = S.population(rng, 64, 33, boundary=9)
    a, b = st.copy(), st.copy()
    whole = S.osc_np(a, 33)
    parts = np.concatenate([S.osc_np(b, 9), S.osc_np(b, 1), S.osc_np(b, 23)])
    assert np.array_equal(whole, parts) and np.array_equal(a, b)


# ---- the reference's own figures
def test_reference_fit_and_descriptors():
    rate, state = S.fit(KAT["fit"]["stop"], KAT["fit"]["harmonics"], KAT["fit"]["cycles"])
    assert rate == KAT["fit"]["rate"] == 0x22F40 and state == KAT["fit"]["state"] == (rate * 3) << 32
    assert isclose(S.delay(rate, KAT["delay"]["harmonic"]), KAT["delay"]["value"], 0.0, KAT["delay"]["tol"])
    assert isclose(S.cycles_f(rate, state), KAT["cycles"]["value"], 0.0, KAT["cycles"]["tol"])
    assert S.state_f(rate, state) == S.continuous(rate, state, 0.0) * S.rate_f(rate)  # :208
    stop, harmonics = np.float32(0.3), np.float32(3000.0)
    assert stop * np.float32(0.99) <= np.float32(S.state_f(rate, state)) * harmonics <= np.float32(1.01) * stop  # :210
    length = S.delay(rate, 3000.0)
    assert stop * np.float32(0.99) <= np.float32(S.continuous(rate, state, length) * S.rate_f(rate)) <= np.float32(1.01) * stop  # :211-214
    # zero crossings and wraps, 0 included (:217-220; delay(0) = -inf, continuous(-inf) = 0)
    worst = 0.0
    for h in range(KAT["zero_crossings"]["harmonics"]):
        d = -math.inf if h == 0 else S.delay(rate, float(h))
        p = S.continuous(rate, state, d)
        worst = max(worst, abs(p - h * 3.0))
        assert isclose(p, h * 3.0, 0.0, KAT["zero_crossings"]["tol"]), (h, p)
    print("zero crossings: worst", worst)


def test_reference_phase_bound_and_end():
    """:221-234: the running sum of the sweep (post-increment, the sum taken before the sample is added) stays within 5e-5 turns of
    the analytic phase for the first `delay(harmonics)` samples; the sweep ends after 255515 samples"""
    rate, state = S.fit(*S.KAT_FIT)
    n = KAT["phase"]["frames"]
    assert n == int(S.delay(rate, 3000.0))
    p, s, got = 0, state, np.empty(n)
    for t in range(n):
        got[t] = p / 2.0 ** 64
        p = O.i64(p + s)
        s = S.sweep_next_int(s, rate)
    err = got - S.cycles_f(rate, state) * np.exp(S.rate_f(rate) * np.arange(n, dtype=np.float64))
    err = np.abs(err - np.round(err))
    print("phase error: worst", err.max())
    assert err.max() <= KAT["phase"]["tol"]
    assert S.remaining_int(state, rate, 300000) == KAT["total_emitted"] == S.KAT_TOTAL
    # and through the generator: accu after k samples is that sum, emitted counts them
    st = S.pack(state, rate)
    S.osc_np(st, 1000)
    assert S.unpack_lane(st, 0) == (_advance(state, rate, 1000), rate, _sum(state, rate, 1000), 1000)


def _advance(state, rate, n):
    for _ in range(n):
        state = S.sweep_next_int(state, rate)
    return state


def _sum(state, rate, n):
    a = 0
    for _ in range(n):
        a, state = O.i64(a + state), S.sweep_next_int(state, rate)
    return a


def test_corner_states():
    assert [(c["state"], c["rate"]) for c in KAT["corners"]] == [tuple(c) for c in S.CORNERS]
    horizon = KAT["horizon"]
    for c in KAT["corners"]:
        assert S.remaining_int(c["state"], c["rate"], horizon) == c["emitted"], c
    # the rows the issue names
    by = {(c["state"], c["rate"]): c["emitted"] for c in KAT["corners"]}
    assert by[(1 << 62, 1 << 30)] == 3 and by[((1 << 62) + 12345, (1 << 31) - 1)] == 1
    assert by[(S.I64_MAX, 1)] is None and by[(S.I64_MAX - (1 << 31) + 1, 0)] is None and by[(0, 12345)] is None
    assert by[(S.I64_MIN, 1)] == 0 and by[(S.I64_MIN, -1)] is None
    # both restatements, all corners as lanes of one state, past every end
    st = S.pack([c[0] for c in S.CORNERS], [c[1] for c in S.CORNERS], accu=[(1 << 63) - 5, -3], emitted=[(1 << 64) - 2, S.M32])
    a, b = st.copy(), st.copy()
    assert np.array_equal(S.osc_int(a, 12), S.osc_np(b, 12)) and np.array_equal(a, b)
    e = (S.emitted_of(b) - S.emitted_of(st)).astype(np.int64)
    assert [int(v) for v in e] == [12 if c["emitted"] is None else min(12, c["emitted"]) for c in KAT["corners"]]


# ---- the library's host side: needs the built library (`make all`), no GPU
FIT_GRID = [(stop, h, c) for stop in (0.0, 1e-9, 0.01, 0.25, 0.3, 0.49999997, 0.5, 0.50000006, -0.0, -1e-9, 0.6, math.nan, math.inf)
            for h in (0.0, 0.5, 1.0, 7.0, 3000.0, 1e6, 3e9, math.inf, math.nan, -3.0)
            for c in (0.0, 0.5, 0.99, 1.0, 1.5, 2.9, 3.0, 123.0, 1e5, 4.3e9, 1e19, -1.0, math.nan, math.inf)]


def test_fit_is_the_spec_fit():
    from idsp_amd._lib import load

    fn, _ = load()
    seen = set()
    for stop, h, c in FIT_GRID:
        rate, state = C.c_int32(-7), C.c_int64(-7)
        rc = fn["sweep_fit"](stop, h, c, C.byref(rate), C.byref(state))
        try:
            want = S.fit(stop, h, c)
        except ValueError as e:
            assert rc == _abi.IDSP_EINVAL and fn["last_error"]().decode() == str(e), (stop, h, c)
            assert (rate.value, state.value) == (-7, -7)
            seen.add(str(e))
            continue
        assert rc == 0 and (rate.value, state.value) == want, (stop, h, c, rate.value, state.value, want)
        seen.add("ok")
    assert seen == {"ok", "Stop out of bounds", "Start out of bounds"}
    assert fn["sweep_fit"](math.nan, 1.0, 1.0, C.byref(C.c_int32()), C.byref(C.c_int64())) == _abi.IDSP_EINVAL
    assert fn["last_error"]().decode() == "Stop out of bounds"
    assert fn["sweep_fit"](0.3, 3000.0, 3.0, None, None) == _abi.IDSP_EINVAL
    assert fn["sweep_state_words"]() == _abi.SWEEP_STATE_WORDS == S.WORDS == 7
    assert set(_abi.SWEEP) <= set(_abi.UTILS)


def test_descriptors_meet_the_reference_tolerances():
    """the f64 descriptors and `inverse_filter` against the spec with the reference test's tolerances (isclose(.., 0.0, 1e-2) on
    lengths and cycles, 1e-10 on phases in cycles; f32 results to a few units of f32 precision): libm is not part of the contract"""
    from idsp_amd._lib import load

    fn, _ = load()
    for args in ((0.3, 3000.0, 3.0), (0.5, 1e6, 1.0), (0.01, 7.0, 123.0), (0.25, 1e5, 2.9)):
        rate, state = S.fit(*args)
        assert isclose(fn["sweep_rate"](rate), S.rate_f(rate), 1e-12, 0.0)
        for h in (1.0, 2.0, 7.5, args[1]):
            assert isclose(fn["sweep_delay"](rate, h), S.delay(rate, h), 0.0, 1e-2)
            assert isclose(fn["sweep_continuous"](rate, state, S.delay(rate, h)), h * S.cycles_f(rate, state), 1e-10, 1e-10)
        assert isclose(fn["sweep_octave"](rate), S.octave(rate), 0.0, 1e-2) and isclose(fn["sweep_decade"](rate), S.decade(rate), 0.0, 1e-2)
        assert isclose(fn["sweep_cycles"](rate, state), S.cycles_f(rate, state), 0.0, 1e-2)
        assert isclose(fn["sweep_state"](rate, state), S.state_f(rate, state), 1e-12, 0.0)
        assert fn["sweep_state"](rate, state) == fn["sweep_continuous"](rate, state, 0.0) * fn["sweep_rate"](rate)  # :208
        for f in (1e-4, 1e-3, 0.01, 0.1, 0.3):
            out = (C.c_float * 2)()
            assert fn["sweep_inverse_filter"](rate, state, f, C.cast(out, C.c_void_p)) == 0
            want = S.inverse_filter(rate, state, f)
            # |H| = 2 rate sqrt(f / rate) exactly up to f32 rounding; the angle is 2 pi turns with |turns| up to ~f / rate * 20, so one f32
            # ulp of turns (2^-23 |turns|) moves the result by amp * 2 pi * 2^-23 |turns|: allow four of those
            amp = abs(want)
            turns = abs(0.125 - (f / S.rate_f(rate)) * (1.0 - math.log(f / S.rate_f(rate) / S.cycles_f(rate, state))))
            tol = amp * (4 * 2 * math.pi * 2.0 ** -23 * max(turns, 1.0) + 1e-6)
            assert abs(complex(out[0], out[1]) - want) <= tol, (args, f, out[0], out[1], want, tol)
            assert isclose(math.hypot(out[0], out[1]), amp, 1e-5, 0.0)
    assert fn["sweep_inverse_filter"](1, 1, 0.1, None) == _abi.IDSP_EINVAL


def test_cpp_host_mirror():
    """tests/cpp/test_sweep_host.cpp: `idsp::Sweep` of include/idsp_hip.hpp — fit, its two errors, the descriptors — and the
    argument errors of idsp_sweep_i32, before anything touches a device (plain g++ against the C ABI)"""
    exe = os.path.join(ROOT, "build", "test_sweep_host")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Iinclude", "tests/cpp/test_sweep_host.cpp", "-Lidsp_amd/lib", "-lidsp_hip",
                    "-Wl,-rpath,$ORIGIN/../idsp_amd/lib", "-o", exe], cwd=ROOT, check=True)
    r = subprocess.run([exe], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "sweep host tests passed" in r.stdout
