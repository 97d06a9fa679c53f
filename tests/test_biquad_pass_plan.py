"""The passes of the biquad section chains, the per-lane banks, the cascade, the Wdf chain and the 16-bit chains without a GPU: `next_pass`
(idsp_amd/csrc/biquad_pass_plan.h) run through build/stream_plan_cli (tests/cpp/stream_plan_cli.cpp, plain g++, verb `passes`) over the table
of tests/_biquad_pass_cases.py, whose expectations were written from the five loops that decided this before (line numbers there).  The
entries themselves are held to the same table on the GPU by tests/test_gpu_biquad_passes.py.

Reference: the slice composition `[C] x [S]` (dsp-process/src/compose.rs:43-77) runs its stages one after the other over the whole block; a
pass is a group of consecutive stages fused into one launch."""
import os
import subprocess

import pytest

from tests import _biquad_pass_cases as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LO, HI4 = P.LO, P.HI4


@pytest.fixture(scope="module")
def cli():
    subprocess.run(["make", "-s", "build/stream_plan_cli"], cwd=ROOT, check=True)
    exe = os.path.join(ROOT, "build", "stream_plan_cli")

    def run(lines):
        r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stderr
        out = r.stdout.split("\n")[:-1]
        assert len(out) == len(lines) and not any(o.startswith("error") for o in out), [o for o in out if o.startswith("error")][:3]
        return out

    return run


def test_the_table(cli):
    got = cli([P.line(*r[:5]) for r in P.ROWS])
    bad = [(r, g) for r, g in zip(P.ROWS, got) if g != r[5]]
    assert not bad, (len(bad), bad[:5])
    assert {r[0] for r in P.ROWS} == set(P.FAMILIES)


def test_lane_thresholds(cli):
    """kDuoMinLanes and kDuo4MaxLanes at value - 4 and value (the cap is `lanes <= kDuo4MaxLanes`: value and value + 4), for every family: the
    smallest section count that asks for two waves, and 4 sections where that is another count"""
    def ask(f, n, lanes):
        return "+" in cli([P.line(f, n, lanes)])[0].split(" ")[0]

    for f, (_, _, _, _, (_, max_duo, duo_min)) in P.FAMILIES.items():
        if not max_duo:
            assert not any(ask(f, n, lanes) for n in (2, 4, 5, 8) for lanes in (LO, HI4, HI4 + 4)), f
            continue
        assert [ask(f, duo_min, LO - 4), ask(f, duo_min, LO)] == [False, True], f
        assert not ask(f, duo_min - 1, LO), f
        capped = f in P.PLAIN  # biquad_sections.h:752 asked duo_wanted(4, ...) for these alone: every other family's four ask as five do
        if max_duo >= 4 and duo_min <= 4:
            assert [ask(f, 4, HI4 - 4), ask(f, 4, HI4), ask(f, 4, HI4 + 4)] == [True, True, not capped], f
        if max_duo >= 5:
            assert [ask(f, 5, HI4), ask(f, 5, HI4 + 4), ask(f, 5, 1 << 20)] == [True, True, True], f


def test_every_schedule_covers_its_sections(cli):
    """n = 1 .. 20 at lane counts on both sides of both thresholds, both layouts, with and without the two-wave kernel: the passes sum to n
    (the cascade's 8 at most), none is empty, none exceeds its family's rule, a two-wave pass is at least the family's minimum and is
    split ceil(m / 2) + floor(m / 2)"""
    cases = [(f, n, lanes, layout, sw) for f in P.FAMILIES for n in range(1, 21) for lanes in (64, LO - 4, LO, HI4, HI4 + 4, 1 << 20)
             for layout in ("FM", "LM") for sw in ((), P.DUO_OFF) if not (P.FAMILIES[f][0] == "cascade" and n > 8)]
    got = cli([P.line(*c) for c in cases])
    for (f, n, lanes, layout, sw), g in zip(cases, got):
        max_single, max_duo, duo_min = P.FAMILIES[f][4]
        passes = [[int(v) for v in p.split("+")] for p in g.split(" ")]
        assert sum(sum(p) for p in passes) == n and all(v >= 1 for p in passes for v in p), (f, n, lanes, g)
        for p in passes:
            if len(p) == 1:
                assert p[0] <= max_single, (f, n, lanes, g)
            else:
                m = sum(p)
                assert len(p) == 2 and duo_min <= m <= max_duo and p == [(m + 1) // 2, m // 2], (f, n, lanes, g)
                assert layout == "FM" and lanes >= LO and not sw, (f, n, lanes, layout, sw, g)
        # every pass but the last is as wide as its kind allows: nothing is left for a later launch that this one could have taken
        for p in passes[:-1]:
            assert sum(p) == (max_duo if len(p) == 2 else max_single), (f, n, lanes, g)
