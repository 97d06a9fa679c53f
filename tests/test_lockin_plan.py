"""The dispatch of the eight lock-in entries without a GPU: `plan_lockin` (idsp_amd/csrc/lockin_plan.h) run through build/stream_plan_cli
(tests/cpp/stream_plan_cli.cpp, plain g++) over the table of tests/_lockin_plan_cases.py, whose expectations were written from the
dispatch as it stood before the choice moved into that header.  tests/test_gpu_lockin_plan.py holds the real entries to the same rows.

Reference: src/lockin.rs:11-39 (the function every one of these kernels computes)."""
import os
import re
import subprocess

import pytest

from tests import _lockin_plan_cases as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def answers():
    subprocess.run(["make", "-s", "build/stream_plan_cli"], cwd=ROOT, check=True)
    lines = [L.cli_line(c) for c in L.CASES]
    r = subprocess.run([os.path.join(ROOT, "build", "stream_plan_cli")], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    out = r.stdout.split("\n")[:-1]
    assert len(out) == len(lines) and not any(o.startswith("error") for o in out), [o for o in out if o.startswith("error")][:3]
    return out


def test_every_row(answers):
    bad = [(L.cli_line(c), got, c.name + "\t" + c.params) for c, got in zip(L.CASES, answers) if got != c.name + "\t" + c.params]
    assert not bad, (len(bad), bad[:8])


def test_the_table_is_whole():
    assert len({L.cli_line(c) for c in L.CASES}) == len(L.CASES), "a call twice"
    entries = {"process", "arg", "norm_sqr", "biquad_process", "lo_process", "biquad_lo_process", "f32_biquad_lo_process", "accu_process"}
    assert {(c.entry, c.layout) for c in L.CASES} == {(e, lay) for e in entries for lay in ("FM", "LM")}
    switches = {"IDSP_LOCKIN_NO_WAVES", "IDSP_LOCKIN_WAVES", "IDSP_LOCKIN_NO_LM_TAIL", "IDSP_LOCKIN_NO_STAGES", "IDSP_LOCKIN_STAGE_GROUPS", "IDSP_LOCKIN_NO_SKEW",
                "IDSP_LOCKIN_NO_DMA", "IDSP_LOCKIN_B", "IDSP_SPLIT_MAX_LANES"}
    assert {k for c in L.CASES for k in c.sw} - {"IDSP_DIAG"} == switches
    # ... and those are the switches the header reads
    text = open(os.path.join(ROOT, "idsp_amd", "csrc", "lockin_plan.h")).read()
    assert set(re.findall(r'(?:on|num)\("(IDSP_\w+)"', text)) == switches
    # what runs on the GPU is small: 65600 lanes x 48 frames at the most, and the stagger's long calls stay here
    for c in L.CASES:
        assert not c.gpu or (c.lanes <= 65600 and 1 <= c.frames <= 48 and not c.tuned), c
    phase = [c for c in L.CASES if c.entry == "process" and c.layout == "LM" and c.lanes == 4096 and not c.sw and c.off == (0, 0)]
    assert {c.frames for c in phase} >= {16, 20, 28, 30, 32, 36, 48}


def lockin_thresholds():
    """the names under the lock-in heading of dispatch_thresholds.h -> value"""
    text = open(os.path.join(ROOT, "idsp_amd", "csrc", "dispatch_thresholds.h")).read()
    section = text[text.index("// ---- lock-in"):]
    out = {}
    for m in re.finditer(r"constexpr\s+(?:size_t|int|unsigned)\s+([^;]+);", section):
        for item in m.group(1).split(","):
            name, value = re.fullmatch(r"\s*(k\w+)\s*=\s*(\d+)\s*", item).groups()
            out[name] = int(value)
    return out


def test_every_lockin_threshold_is_compared_on_both_sides():
    """For each name: the last value on the one side and the first on the other (a workgroup of 64 lanes apart for the lane counts), as
    the condition that reads it is written, and the rows that must hold them — for each read-out where all three read it."""
    T = lockin_thresholds()
    lowpass = [c for c in L.CASES if c.entry in L.READOUTS and not c.sw]

    def lanes_of(entry, pred=lambda c: True):
        return {c.lanes for c in lowpass if c.entry == entry and c.layout == "FM" and pred(c)}

    sides = {
        # `lanes <= value`
        "kSplitMaxLanes": lambda v: all({v, v + 64} <= lanes_of(e, lambda c: c.b == 1) for e in L.READOUTS) and
        {v, v + 64} <= {c.lanes for c in lowpass if c.entry == "process" and c.name.startswith("stream_")} and
        {v, v + 64} <= {c.lanes for c in L.CASES if c.entry == "accu_process"},
        "kLockinSixWavesMaxLanes": lambda v: all({v, v + 64} <= lanes_of(e, lambda c: c.b == 1) for e in L.READOUTS),
        "kLockinStagesOneGroupMaxLanes": lambda v: all({v, v + 64} <= lanes_of(e, lambda c: c.b == 2 and c.frames == 16 and c.off == (0, 0)) for e in L.READOUTS),
        # `lanes > value`, `lanes <= value`
        "kLockinB16MinLanes": lambda v: all({v, v + 64} <= lanes_of(e) for e in L.READOUTS),
        "kLockinB16MaxLanes": lambda v: all({v, v + 64} <= lanes_of(e) for e in L.READOUTS),
        # `order * cascade < value`: the products next to 6 are 4 and 6
        "kLockinSixWavesArmWeight": lambda v: v == 6 and {4, 6} <= {c.a * c.b for c in lowpass if c.entry == "arg" and c.lanes == 32768 and c.b != 2},
        # `lanes >= value`: not theirs
        "kLockinWavesMaxLanes": lambda v: {v - 64, v} <= {c.lanes for c in L.CASES if c.layout == "FM"} and {v - 64, v} <= {c.lanes for c in L.CASES if c.layout == "LM"},
        # `frames >= value` of rows with frames % 4 == 0 that are not whole batches: 28 and 36 around 32
        "kLockinTailMinFrames": lambda v: all({v - 4, v + 4} <= {c.frames for c in lowpass if c.entry == e and c.layout == "LM" and c.off == (0, 0)} for e in L.READOUTS),
    }
    assert set(sides) == set(T), sorted(set(sides) ^ set(T))
    assert not [name for name, ok in sides.items() if not ok(T[name])]
    # the rows were written on the header's values as they stand
    assert (T["kSplitMaxLanes"], T["kLockinSixWavesMaxLanes"], T["kLockinStagesOneGroupMaxLanes"], T["kLockinB16MinLanes"], T["kLockinB16MaxLanes"],
            T["kLockinWavesMaxLanes"], T["kLockinTailMinFrames"]) == (L.SPLIT_MAX, 16384, 16384, 49152, 65536, 1 << 28, 32)
