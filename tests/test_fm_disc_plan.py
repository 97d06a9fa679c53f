"""The dispatch of idsp_fm_disc_i32 and idsp_dds_i32 without a GPU: `plan_fm_disc` / `plan_dds` (idsp_amd/csrc/readout_plan.h) run through
build/stream_plan_cli (tests/cpp/stream_plan_cli.cpp, plain g++) over the table of tests/_fm_disc_plan_cases.py, whose expectations were
written from the two entries as they stood before the choice moved into that header.  tests/test_gpu_fm_disc_plan.py holds the real
entries to the same rows.

Reference: examples/fm_disc.rs:25-50, src/accu.rs:34-41 and src/cossin.rs:14-67 (the functions every one of these kernels computes)."""
import os
import re
import subprocess

import pytest

from tests import _fm_disc_plan_cases as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ask(lines):
    subprocess.run(["make", "-s", "build/stream_plan_cli"], cwd=ROOT, check=True)
    r = subprocess.run([os.path.join(ROOT, "build", "stream_plan_cli")], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    out = r.stdout.split("\n")[:-1]
    assert len(out) == len(lines) and not any(o.startswith("error") for o in out), [o for o in out if o.startswith("error")][:3]
    return out


def fm_want(c):
    return c.name + "\t" + c.params


def dds_want(c):
    return "stream_<" + c.proc + ">\t" + c.params


@pytest.mark.parametrize("cases,line,want", [(R.FM_DISC_CASES, R.fm_disc_line, fm_want), (R.DDS_CASES, R.dds_line, dds_want)], ids=["fm_disc", "dds"])
def test_every_row(cases, line, want):
    got = ask([line(c) for c in cases])
    bad = [(line(c), g, want(c)) for c, g in zip(cases, got) if g != want(c)]
    assert not bad, (len(bad), bad[:8])


def test_the_table_is_whole():
    assert len({R.fm_disc_line(c) for c in R.FM_DISC_CASES}) == len(R.FM_DISC_CASES) and len({R.dds_line(c) for c in R.DDS_CASES}) == len(R.DDS_CASES), "a call twice"
    for cases in (R.FM_DISC_CASES, R.DDS_CASES):
        assert {c.layout for c in cases} == {"FM", "LM"} and {c.layout for c in cases if c.gpu and not c.sw} == {"FM", "LM"}
    # the switches: each with IDSP_DIAG=1 and without, and they are the ones the header reads
    for cases, switches in ((R.FM_DISC_CASES, R.FM_DISC_SWITCHES), (R.DDS_CASES, R.DDS_SWITCHES)):
        for diag in (True, False):
            assert {k for c in cases if c.sw and ("IDSP_DIAG" in c.sw) == diag for k in c.sw} - {"IDSP_DIAG"} == switches
    text = open(os.path.join(ROOT, "idsp_amd", "csrc", "readout_plan.h")).read()
    assert set(re.findall(r'num\("(IDSP_\w+)"', text)) == R.FM_DISC_SWITCHES and set(re.findall(r'env\("(IDSP_\w+)"\)', text)) == R.DDS_SWITCHES
    # the four recorded names of the discriminator's own kernels, and the stream launcher's for the rest
    assert {c.name for c in R.FM_DISC_CASES} == {"stream_", "fm_disc_waves_kernel<3>", "fm_disc_waves_kernel<4>", "fm_disc_waves_lm_kernel",
                                                 "fm_disc_waves_lm_kernel + stream_lane_major (last frames % 32)"}
    # forced wave counts 0, 3, 4 and 5 in both layouts, with IDSP_DIAG=1 and without
    assert {(c.sw["IDSP_FM_DISC_WAVES"], c.layout, "IDSP_DIAG" in c.sw) for c in R.FM_DISC_CASES if "IDSP_FM_DISC_WAVES" in c.sw} == \
        {(n, lay, d) for n in "0345" for lay in ("FM", "LM") for d in (True, False)}
    # what runs on the GPU is small, runs on whatever device is there, and relies on no switch the library would not honour
    for c in R.FM_DISC_CASES:
        assert not c.gpu or (c.lanes <= 81921 and c.frames <= 2064 and c.lanes * c.frames <= 81921 * 8 and not c.tuned and (not c.sw or "IDSP_DIAG" in c.sw)), c
    for c in R.DDS_CASES:
        assert not c.gpu or (c.lanes <= 81921 and 0 < c.frames <= 2064 and c.lanes * c.frames <= 40961 * 256 and (not c.sw or "IDSP_DIAG" in c.sw)), c
    # every form of both plans on the GPU under the default dispatch (three front waves need the switch)
    form = lambda c: re.match(r"form=(\w+)", c.params).group(1)
    assert {form(c) for c in R.FM_DISC_CASES if c.gpu and not c.sw} == {"Stream", "WavesFm", "WavesLm", "WavesLmTail"}
    assert {c.proc for c in R.DDS_CASES if c.gpu and not c.sw} == {"DdsSplitProcT<true>", "DdsSplitProcT<false>", "DdsProcT<false>"}
    assert any(c.gpu and c.name == "fm_disc_waves_kernel<3>" for c in R.FM_DISC_CASES)


def thresholds(heading="// ---- FM discriminator and DDS"):
    """the names under a heading of dispatch_thresholds.h (the last one: to the end of the file) -> value"""
    text = open(os.path.join(ROOT, "idsp_amd", "csrc", "dispatch_thresholds.h")).read()
    section = text[text.index(heading):]
    assert section.count("// ---- ") == 1, "the section is the last of the file"
    out = {}
    for m in re.finditer(r"constexpr\s+(?:uint64_t|int32_t)\s+([^;]+);", section):
        for item in m.group(1).split(","):
            name, value = re.fullmatch(r"\s*(k\w+)\s*=\s*(0x[0-9a-f]+|\d+)\s*", item).groups()
            out[name] = int(value, 0)
    return out


def test_every_readout_threshold_is_compared_on_both_sides():
    """For each name of the section: the last value on the one side and the first on the other, as the condition that reads it is written,
    and the rows that must hold them (default dispatch, buffers on the 16-byte grid)."""
    T = thresholds()
    fmd = [c for c in R.FM_DISC_CASES if not c.sw and c.off == (0, 0)]
    dds = [c for c in R.DDS_CASES if not c.sw]

    def has(cases, **want):
        """a row with these fields or launch parameters"""
        def value(c, k):
            par = dict(kv.split("=") for kv in c.params.split())
            return (par[k] if k == "form" else int(par[k])) if k in par else getattr(c, k)
        return any(all(value(c, k) == v for k, v in want.items()) for c in cases)

    sides = {
        # `lanes <= value`, FrameMajor
        "kFmDiscWavesMaxLanes": lambda v: has(fmd, layout="FM", lanes=v, form="WavesFm", waves=4) and has(fmd, layout="FM", lanes=v + 1, form="Stream"),
        # `frames >= value`, FrameMajor
        "kFmDiscFmMinFrames": lambda v: has(fmd, layout="FM", frames=v - 1, form="Stream") and has(fmd, layout="FM", frames=v, form="WavesFm"),
        # `frames >= value` and `body = frames - frames % value`, LaneMajor: one tile, one tile and a half, two tiles
        "kFmDiscLmTile": lambda v: has(fmd, layout="LM", frames=v - 1, form="Stream") and has(fmd, layout="LM", frames=v, form="WavesLm", body=v, tail=0) and
        has(fmd, layout="LM", frames=v + v // 2, form="WavesLmTail", body=v, tail=v // 2) and has(fmd, layout="LM", frames=2 * v, form="WavesLm", body=2 * v),
        # `frames % value == 0`, LaneMajor from 32 frames: 32 + 1, 32 + 8 and 32 + 16
        "kFmDiscLmRowMultiple": lambda v: has(fmd, layout="LM", frames=2 * v + 1, form="Stream") and has(fmd, layout="LM", frames=2 * v + v // 2, form="Stream") and
        has(fmd, layout="LM", frames=3 * v, form="WavesLmTail"),
        # `lanes < value`, LaneMajor
        "kFmDiscLmMaxLanes": lambda v: has(fmd, layout="LM", lanes=v - 1, form="WavesLm") and has(fmd, layout="LM", lanes=v, form="Stream"),
        # `frames >= value`, FrameMajor, two threads per lane
        "kDdsCircleMinFrames": lambda v: has(dds, layout="FM", frames=v - 1, split=1, circle=0) and has(dds, layout="FM", frames=v, split=1, circle=1) and
        has(dds, layout="LM", frames=v, circle=0) and has(dds, layout="FM", frames=v, split=0, circle=0),
    }
    assert set(sides) == set(T), sorted(set(sides) ^ set(T))
    assert not [name for name, ok in sides.items() if not ok(T[name])]
    # the rows were written on the header's values as they stand
    assert T == {"kFmDiscWavesMaxLanes": 81920, "kFmDiscFmMinFrames": 8, "kFmDiscLmTile": 32, "kFmDiscLmRowMultiple": 16, "kFmDiscLmMaxLanes": 1 << 28,
                 "kDdsCircleMinFrames": 256}
    # ... and the names of other sections that the two plans read: the two addresses on the 16-byte grid, the two-thread split, the stagger window
    text = open(os.path.join(ROOT, "idsp_amd", "csrc", "dispatch_thresholds.h")).read()
    other = {name: int(re.search(r"\b%s = (\d+)" % name, text).group(1)) for name in
             ("kPieceBytes", "kSplitMaxLanes", "kStaggerMinWorkgroups", "kStaggerMinFrames", "kStaggerMaxFrames", "kFmDiscStaggerTicks")}
    assert other == {"kPieceBytes": 16, "kSplitMaxLanes": 40960, "kStaggerMinWorkgroups": 512, "kStaggerMinFrames": 2048, "kStaggerMaxFrames": 8192, "kFmDiscStaggerTicks": 1200}
    off = [c for c in R.FM_DISC_CASES if not c.sw and c.layout == "LM" and c.frames == 64]
    assert all(has(off, off=o, form="Stream") for o in ((4, 0), (8, 0), (0, 4), (0, 8))) and has(off, off=(0, 0), form="WavesLm")
    assert all(has(dds, layout=lay, lanes=40960, split=1) and has(dds, layout=lay, lanes=40961, split=0) for lay in ("FM", "LM"))
    tuned = [c for c in fmd if c.tuned and c.layout == "LM"]
    ticks = other["kFmDiscStaggerTicks"]
    assert has(tuned, lanes=511 * 64, frames=2048, skew=0) and has(tuned, lanes=511 * 64 + 1, frames=2048, skew=ticks) and has(tuned, lanes=512 * 64, frames=2048, skew=ticks)
    assert has(tuned, frames=2032, skew=0) and has(tuned, frames=2047, form="Stream") and has(tuned, frames=8192, skew=ticks) and has(tuned, frames=8208, skew=0, body=8192)
    assert has(fmd, tuned=False, lanes=512 * 64, frames=2048, skew=0) and has(fmd, tuned=False, lanes=512 * 64, frames=8192, skew=0)
