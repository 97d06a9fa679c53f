"""The RPLL / batch-LO specification (tests/_rpll_spec.py) against itself, against the reference's own limits
(tests/golden/rpll_kat.json, from src/rpll.rs:105-289) and against the library's argument checks.  No GPU.

Figures (this file prints them): the `default` case meets its four limits at 0.155, 0.0029, 0.72 and 0.0030 of them; the spreads of
the six noisy cases (numpy noise, the one seed of the golden file) are 0.1 to 0.4 % of theirs; the chain's worst component error over the five shapes
of the issue is printed by test_chain_recovers_the_tone (bound 3e-3, examples/ddc_lockin.rs:105-109)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from idsp_amd import _abi
from idsp_amd._abi import RPLL  # noqa: F401  (the feature's prototype table)
from tests import _harness as H
from tests import _rpll_spec as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KAT = S.kat()
CASES = {c["name"]: c for c in KAT["cases"]}


# ---- the two restatements
@pytest.mark.parametrize("cfg", S.CONFIGS)
def test_rpll_restatements_agree(cfg):
    rng = np.random.default_rng(sum(cfg))
    seen_neg = seen_min = seen_max = False
    for density in (0.0, 1.0, 1 / 3):
        ts = S.adversarial_ts(rng, 60, 31, density)
        st = S.random_state(rng, 31)
        if density == 1.0:  # dx = i32::MIN and dx < 0 on the first sample of lanes 0 and 1
            ts[0, 0, 1] = (int(st[0, 0]) ^ 0x80000000) - (1 << 32) if (int(st[0, 0]) ^ 0x80000000) >= 1 << 31 else int(st[0, 0]) ^ 0x80000000
            dx = (ts[:, :, 1].astype(np.int64) - np.concatenate([st[0].view(np.int32)[None, :], ts[:-1, :, 1]]).astype(np.int64) + (1 << 31)) % (1 << 32) - (1 << 31)
            seen_neg, seen_min = seen_neg or (dx < 0).any(), seen_min or (dx == -(1 << 31)).any()
            seen_max = seen_max or (st[1] == S.M32).any()
        a, b = st.copy(), st.copy()
        ya, yb = S.rpll_int(cfg, a, ts), S.rpll_np(cfg, b, ts)
        assert np.array_equal(ya, yb) and np.array_equal(a, b), (cfg, density)
        if density == 0.0:  # all None: only y moves, by f per sample
            assert np.array_equal(a[:3], st[:3]) and np.array_equal(a[3], st[3] + np.uint32(60) * st[2])
    assert seen_neg and seen_min and seen_max


def test_rpll_chunks_and_default_state():
    rng = np.random.default_rng(3)
    ts = S.adversarial_ts(rng, 50, 9)
    a, b = np.zeros((4, 9), np.uint32), np.zeros((4, 9), np.uint32)
    whole = S.rpll_np((8, 9, 8), a, ts)
    parts = np.concatenate([S.rpll_np((8, 9, 8), b, ts[:1]), S.rpll_np((8, 9, 8), b, ts[1:33]), S.rpll_np((8, 9, 8), b, ts[33:])])
    assert np.array_equal(whole, parts) and np.array_equal(a, b)
    assert np.array_equal(whole[-1, :, 0].view(np.uint32), a[3]) and np.array_equal(whole[-1, :, 1].view(np.uint32), a[2])  # phase(), frequency()


@pytest.mark.parametrize("k", S.LO_K)
def test_accu_lo_restatements_agree(k):
    rng = np.random.default_rng(k)
    for h in S.LO_HARMONICS:
        offset = int(rng.integers(-(1 << 31), 1 << 31))
        accu = S.adversarial_accu(rng, 3 if k < 10 else 1, 7)
        assert (accu[:, ::3, 1] < 0).all()  # steps with the top bit set: a logical shift differs from an arithmetic one
        got = S.accu_lo_np((k, h, offset), accu)
        assert np.array_equal(S.accu_lo_int((k, h, offset), accu), got), (k, h)
        if k > 0 and h == 1:  # ... and it does differ: sample 0 of every update with an ARITHMETIC shift of the step
            arith = (accu[..., 0].astype(np.int64) + offset + (accu[..., 1].astype(np.int64) >> k)) & S.M32
            assert (S.accu_lo_phase_np((k, h, offset), accu)[::1 << k] != arith)[:, ::3].all()
    # rows [u0, u1) of a call equal those rows of the whole
    accu = S.adversarial_accu(rng, 5, 4)
    whole = S.accu_lo_np((k, 3, 77), accu)
    assert np.array_equal(S.accu_lo_np((k, 3, 77), accu[1:4]), whole[1 << k:4 << k])


# ---- the reference's own cases
def _limits(c):
    return np.array(c["limits"], np.float32)


def test_reference_default_case():
    """src/rpll.rs:208-213: no noise, so it is reproducible without Rust's RNG — all four limits hold"""
    c = CASES["default"]
    m = S.harness_case_int(c, KAT["n"], KAT["seed"])
    rel = np.abs(m) / _limits(c)
    print("default: measured", m, "relative", rel)
    assert (rel <= 1.0).all(), (m, rel)
    assert np.allclose(m, c["measured"], rtol=1e-6, atol=0.0)


def test_vectorised_harness_is_the_scalar_one():
    """`Harness` over lanes + rpll_np give the figures of the scalar loop (no noise: nothing depends on the generator)"""
    c = CASES["default"]
    cfg, n = tuple(c["cfg"]), 4096
    h = S.Harness(cfg, [c["period"], 990 // 3, 500], [c["next"], 351, 0], [0, 0, 0])
    assert h.lockable().all()
    st = np.zeros((4, 3), np.uint32)
    ts, _ = h.timestamps(S.t_settle(cfg))
    S.rpll_np(cfg, st, ts)
    ts, book = h.timestamps(n)
    got = S.Harness.stats(*h.errors(S.rpll_np(cfg, st, ts), book))
    for lane, (period, nxt) in enumerate(((c["period"], c["next"]), (330, 351), (500, 0))):
        want = S.harness_case_int(dict(cfg=cfg, period=period, next=nxt, noise=0), n, 0)
        assert np.array_equal(got[:, lane], want), (lane, got[:, lane], want)


@pytest.mark.parametrize("name", ["noisy", "narrow_fast", "narrow_slow", "wide_fast", "wide_slow", "batch_fast_narrow"])
def test_reference_noisy_cases(name):
    """src/rpll.rs:215-289 with numpy noise: the two spreads (indices 1 and 3) against the reference's limits; the two means are
    recorded in the golden file and not asserted (they depend on the noise realisation: 0.15 to 3.0 times the limit with this seed)"""
    c = CASES[name]
    m = S.harness_case_int(c, KAT["n"], KAT["seed"])
    rel = np.abs(m) / _limits(c)
    print(name, "measured", m, "relative", rel)
    assert rel[1] <= 1.0 and rel[3] <= 1.0, (m, rel)
    assert np.allclose(m, c["measured"], rtol=1e-6, atol=0.0), (m, c["measured"])


# ---- the chain on the specification
CHAIN = [((8, 9, 8), 333, 3, 1, 4096), ((8, 9, 8), 333, 3, 3, 4096), ((8, 9, 8), 333, 0, 1, 4096), ((8, 9, 8), 333, 8, 1, 512),
         ((8, 10, 9), 990, 3, 2, 4096)]


@pytest.mark.parametrize("cfg,period,k,h,updates", CHAIN)
def test_chain_recovers_the_tone(cfg, period, k, h, updates):
    """mean of x cos and x sin over the last quarter within 3e-3 of (0.5 cos phi, -0.5 sin phi): the reference's own bound for its
    DDC example (examples/ddc_lockin.rs:105-109)"""
    lanes = 8
    ts, tone, phi, _ = S.chain_case(cfg, [period] * lanes, k, h, updates, seed=period + 10 * k + h)
    assert updates // 4 * 3 >= S.t_settle(cfg)
    st = np.zeros((4, lanes), np.uint32)
    lo = S.accu_lo_np((k, h, 0), S.rpll_np(cfg, st, ts)).astype(np.float64) / 2.0 ** 31
    q = tone.shape[0] // 4 * 3
    i_mean, q_mean = (tone[q:] * lo[q:, :, 0]).mean(axis=0), (tone[q:] * lo[q:, :, 1]).mean(axis=0)
    err = max(np.abs(i_mean - 0.5 * np.cos(phi)).max(), np.abs(q_mean + 0.5 * np.sin(phi)).max())
    print("chain", cfg, period, k, h, updates, "worst error", err)
    assert err <= 3e-3, err


def test_chain_through_the_lock_in():
    """the CPU form of the device chain's assertion (tests/test_gpu_rpll.py, test_chain_on_the_device): the spec's LO into the checker library's
    lockin_i32_lo_process; atan2(mean Q, mean I) over the last quarter within 1e-2 rad of -phi on every lane (3e-3 on components
    of 0.5, times sqrt 2, rounded up; independent of scale)"""
    from tests import _rpll_chain as G

    case = G.chain()
    worst = 0.0
    for h in G.HARMONICS:
        worst = max(worst, G.phase_error(case, h, case["want"][h]).max())
    print("chain through the lock-in: worst |arg + phi|", worst)
    assert worst <= 1e-2


# ---- the library's argument checks: host-only paths, nothing is launched
def _rpll(fn, cfg, lanes=0, frames=0, state=None, ts=None, accu=None, layout=0):
    return fn["rpll_i32"](C.byref(_abi.Rpll(*cfg)), state, ts, accu, lanes, frames, layout, None)


def _lo(fn, cfg, lanes=0, updates=0, accu=None, lo=None, layout=0):
    return fn["accu_lo_i32"](C.byref(_abi.AccuLo(*cfg)), accu, lo, lanes, updates, layout, None)


def test_entry_validation():
    from idsp_amd._lib import load

    fn, _ = load()
    assert fn["rpll_state_words"]() == _abi.RPLL_STATE_WORDS == S.WORDS == 4
    assert set(_abi.RPLL) <= set(_abi.UTILS)
    inside = [(0, 1, 0), (30, 31, 30), (0, 32, 31), (30, 32, 61), (30, 31, 61), (8, 9, 8), (8, 9, 39), (0, 1, 31)]
    outside = [(-1, 9, 8), (31, 32, 31), (8, 8, 8), (8, 33, 8), (0, 0, 0), (8, 9, 7), (8, 9, 40), (30, 32, 62), (0, 1, 32), (0, 1, -1)]
    for cfg in S.CONFIGS + inside:
        assert S.cfg_ok(cfg) and _rpll(fn, cfg) == 0, cfg
    for cfg in outside:
        assert not S.cfg_ok(cfg) and _rpll(fn, cfg) == _abi.IDSP_EINVAL and fn["last_error"](), cfg
    assert fn["rpll_i32"](None, None, None, None, 0, 0, 0, None) == _abi.IDSP_EINVAL
    assert _rpll(fn, (8, 9, 8), layout=2) == _abi.IDSP_EINVAL
    # pointers are only compared before anything is launched: NULL, misaligned, overlapping
    ok = dict(lanes=4, frames=4, state=0x10000, ts=0x20000, accu=0x30000)
    for bad in (dict(state=None), dict(ts=None), dict(accu=None), dict(ts=0x20004), dict(accu=0x30004), dict(accu=0x20000),
                dict(accu=0x20000 + 4 * 4 * 8 - 8), dict(ts=0x30000 + 8)):
        assert _rpll(fn, (8, 9, 8), **{**ok, **bad}) == _abi.IDSP_EINVAL, bad

    for k in (0, 24):
        assert _lo(fn, (k, 1, 0)) == 0
        assert _lo(fn, (k, 1, 0), updates=(1 << 40) >> k) == 0 and _lo(fn, (k, 1, 0), updates=((1 << 40) >> k) + 1) == _abi.IDSP_EINVAL
    for k in (-1, 25):
        assert _lo(fn, (k, 1, 0)) == _abi.IDSP_EINVAL
    assert fn["accu_lo_i32"](None, None, None, 0, 0, 0, None) == _abi.IDSP_EINVAL
    assert _lo(fn, (3, 1, 0), layout=2) == _abi.IDSP_EINVAL
    ok = dict(lanes=4, updates=2, accu=0x20000, lo=0x30000)
    for bad in (dict(accu=None), dict(lo=None), dict(accu=0x20004), dict(lo=0x30004), dict(lo=0x20000), dict(lo=0x20000 + 4 * 2 * 8 - 8),
                dict(accu=0x30000 + (4 * 16 * 8) - 8)):
        assert _lo(fn, (3, 1, 0), **{**ok, **bad}) == _abi.IDSP_EINVAL, bad


def test_rust_structs_match_ctypes():
    """rust/idsp-hip-sys/src/rpll.rs is what tools/gen_rust_sys.py generates, and its `#[repr(C)]` field lists imply ctypes' sizes"""
    import re
    import sys

    src = open(os.path.join(ROOT, "rust", "idsp-hip-sys", "src", "rpll.rs")).read()
    gen = subprocess.run([sys.executable, "-c", "import sys; sys.path.insert(0, 'tools'); import gen_rust_sys as g; sys.stdout.write(g.generate_side('rpll'))"],
                         cwd=ROOT, capture_output=True, text=True, check=True).stdout
    assert gen == src, "rust/idsp-hip-sys/src/rpll.rs is stale: run python tools/gen_rust_sys.py"
    found = {name: re.findall(r"pub (\w+): (.+),", body) for name, body in re.findall(r"pub struct (\w+) \{\n(.*?)\n\}", src, flags=re.S)}
    assert found == {"IdspRpll": [("dt2", "i32"), ("shift_frequency", "i32"), ("shift_phase", "i32")],
                     "IdspAccuLo": [("batch_log2", "i32"), ("harmonic", "i32"), ("offset", "i32")]}
    assert C.sizeof(_abi.Rpll) == C.sizeof(_abi.AccuLo) == 12
    assert [f[0] for f in _abi.Rpll._fields_] == [f[0] for f in found["IdspRpll"]] and [f[0] for f in _abi.AccuLo._fields_] == [f[0] for f in found["IdspAccuLo"]]
    lib = open(os.path.join(ROOT, "rust", "idsp-hip-sys", "src", "lib.rs")).read()
    assert "mod rpll;\npub use rpll::*;" in lib and "cfg: *const IdspRpll" in lib and "cfg: *const IdspAccuLo" in lib


def test_cpp_host_mirror():
    """tests/cpp/test_rpll_host.cpp: `RPLLConfig` / `AccuLo` of include/idsp_hip.hpp — the same validation — and the empty calls
    and argument errors of the two entries, before anything touches a device (plain g++ against the C ABI)"""
    exe = os.path.join(ROOT, "build", "test_rpll_host")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Iinclude", "tests/cpp/test_rpll_host.cpp", "-Lidsp_amd/lib", "-lidsp_hip",
                    "-Wl,-rpath,$ORIGIN/../idsp_amd/lib", "-o", exe], cwd=ROOT, check=True)
    r = subprocess.run([exe], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "rpll host tests passed" in r.stdout
