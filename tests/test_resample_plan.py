"""The dispatch of the half-band and Cic entries without a GPU: `plan_hbf` / `plan_cic` (idsp_amd/csrc/resample_plan.h) run through
build/stream_plan_cli (tests/cpp/stream_plan_cli.cpp, plain g++) over the table of tests/_resample_plan_cases.py, whose expectations were
written from the dispatch as it stood before the choice moved into that header.  tests/test_gpu_resample_plan.py holds the real entries
to the same rows.

Reference: src/hbf.rs:142-236 and src/cic.rs:34-201 (the functions every one of these kernels computes)."""
import os
import re
import subprocess

import pytest

from tests import _resample_plan_cases as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBF_SWITCHES = {"IDSP_HBF_GENERIC", "IDSP_HBF_NO_BLK", "IDSP_HBF_NO_RING", "IDSP_HBF_NO_BLOCK_FM"}
CIC_SWITCHES = {"IDSP_CIC_NO_RING", "IDSP_CIC_NO_LM_TILES"}


def ask(lines):
    subprocess.run(["make", "-s", "build/stream_plan_cli"], cwd=ROOT, check=True)
    r = subprocess.run([os.path.join(ROOT, "build", "stream_plan_cli")], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    out = r.stdout.split("\n")[:-1]
    assert len(out) == len(lines) and not any(o.startswith("error") for o in out), [o for o in out if o.startswith("error")][:3]
    return out


@pytest.mark.parametrize("cases,line", [(R.HBF_CASES, R.hbf_line), (R.CIC_CASES, R.cic_line)], ids=["hbf", "cic"])
def test_every_row(cases, line):
    got = ask([line(c) for c in cases])
    bad = [(line(c), g, c.name + "\t" + c.params) for c, g in zip(cases, got) if g != c.name + "\t" + c.params]
    assert not bad, (len(bad), bad[:8])


def test_the_table_is_whole():
    assert len({R.hbf_line(c) for c in R.HBF_CASES}) == len(R.HBF_CASES) and len({R.cic_line(c) for c in R.CIC_CASES}) == len(R.CIC_CASES), "a call twice"
    assert {(c.kind, c.layout) for c in R.HBF_CASES} == {(k, lay) for k in ("dec", "int") for lay in ("FM", "LM")}
    assert {(c.kind, c.bits, c.layout) for c in R.CIC_CASES} == {(k, b, lay) for k in ("dec", "int") for b in (32, 64) for lay in ("FM", "LM")}
    # the switches: each with IDSP_DIAG=1 and without, and they are the ones the header reads
    for cases, switches in ((R.HBF_CASES, HBF_SWITCHES), (R.CIC_CASES, CIC_SWITCHES)):
        for diag in (True, False):
            assert {k for c in cases if ("IDSP_DIAG" in c.sw) == diag for k in c.sw} - {"IDSP_DIAG"} == switches
    text = open(os.path.join(ROOT, "idsp_amd", "csrc", "resample_plan.h")).read()
    assert set(re.findall(r'on\("(IDSP_\w+)"', text)) == HBF_SWITCHES | CIC_SWITCHES
    # IDSP_HBF_NO_BLK on a LaneMajor decimator: the generic kernel (neither the ring nor the wave kernels take LaneMajor decimators)
    no_blk = [c for c in R.HBF_CASES if c.sw == {"IDSP_DIAG": "1", "IDSP_HBF_NO_BLK": "1"} and c.kind == "dec" and c.layout == "LM"]
    assert no_blk and all(c.name == R.GENERIC["dec"] for c in no_blk)
    # what runs on the GPU is small, and no GPU row relies on a switch the library would not honour
    for c in R.HBF_CASES:
        assert not c.gpu or (c.lanes <= 176 and c.frames in ((1024 >> c.stages) + 3, (1024 >> c.stages) + 4) and (not c.sw or "IDSP_DIAG" in c.sw)), c
    for c in R.CIC_CASES:
        assert not c.gpu or (c.lanes <= 1024 and c.frames <= 449 and (not c.sw or "IDSP_DIAG" in c.sw)), c
    # every form of both plans on the GPU under the default dispatch (the tile form's recorded name is the plain lane kernel's: this
    # file tells them apart, the GPU row checks the values)
    form = lambda c: re.match(r"form=(\w+)", c.params).group(1)
    assert {form(c) for c in R.HBF_CASES if c.gpu and not c.sw} == {"Generic", "BlkLm", "RingFm", "BlockFm", "WaveFm", "WaveLm"}
    for kind in ("dec", "int"):
        forms = {form(c) for c in R.CIC_CASES if c.gpu and not c.sw and c.kind == kind}
        assert forms == {"RingLm", "LaneTiles", "Lane"} | ({"RingFm"} if kind == "int" else set()), (kind, forms)


def thresholds():
    """the names under the half-band and Cic headings of dispatch_thresholds.h -> value"""
    text = open(os.path.join(ROOT, "idsp_amd", "csrc", "dispatch_thresholds.h")).read()
    section = text[text.index("// ---- half-band"):text.index("// ---- lock-in")]
    assert "// ---- Cic" in section
    out = {}
    for m in re.finditer(r"constexpr\s+(?:uint64_t|int32_t)\s+([^;]+);", section):
        for item in m.group(1).split(","):
            name, value = re.fullmatch(r"\s*(k\w+)\s*=\s*(0x[0-9a-f]+|\d+)\s*", item).groups()
            out[name] = int(value, 0)
    return out


def test_every_resample_threshold_is_compared_on_both_sides():
    """For each name: the last value on the one side and the first on the other, as the condition that reads it is written, and the
    rows that must hold them (default dispatch, and the form the row takes must be the one the name decides about)."""
    T = thresholds()
    hbf = [c for c in R.HBF_CASES if not c.sw]
    cic = [c for c in R.CIC_CASES if not c.sw]
    chunk = lambda c: (c.rate + 1) * c.bits // 8
    aligned = lambda c: c.off in (0, (0, 0))
    wide_off = lambda kind, bits: (bits // 8, 0) if kind == "dec" else (0, bits // 8)  # (x, y): the high-rate tensor one element off the grid

    def has(cases, **want):
        """a row with these fields, launch parameters (form, ppt, vpc, grid) or chunk bytes; on the 16-byte grid unless `off` is asked for"""
        def value(c, k):
            par = dict(kv.split("=") for kv in c.params.split())
            return chunk(c) if k == "chunk" else par[k] if k == "form" else int(par[k]) if k in par else getattr(c, k)
        return any(all(value(c, k) == v for k, v in want.items()) for c in cases if "off" in want or aligned(c))

    sides = {
        # `address % 16 == 0`: the wide buffer of every half-band form and of the Cic rings, both tensors of the Cic tiles; LaneMajor rows of whole
        # pieces, `frames * R * 4 % 16 == 0` (one stage, odd and even frame counts)
        "kPieceBytes": lambda v: v == 16 and all(has(hbf, kind=k, layout=lay, off=4, form="Generic") for k in ("dec", "int") for lay in ("FM", "LM")) and
        all(has(hbf, kind=k, layout="LM", stages=1, frames=f, form=form) for k, pair in (("dec", ((515, "Generic"), (516, "BlkLm"))), ("int", ((515, "Generic"), (516, "WaveLm"))))
            for f, form in pair) and
        all(has(cic, kind=k, bits=b, lanes=64, frames=8, off=off, form=form, vpc=vpc) and has(cic, kind=k, bits=b, lanes=7, frames=127, off=off, form=ring)
            for k in ("dec", "int") for b in (32, 64)
            for off, form, vpc, ring in (((0, 0), "LaneTiles", 4, "RingLm"), (wide_off(k, b), "Lane", 0, "Lane"), (wide_off(k, b)[::-1], "Lane", 4, "RingLm"))),
        # `lanes <= value`
        "kGridMaxLanes": lambda v: has(hbf, kind="dec", lanes=v, form="BlkLm") and has(hbf, kind="dec", lanes=v + 1, form="Generic") and
        all(has(cic, kind=k, bits=b, lanes=v, form="RingLm") and has(cic, kind=k, bits=b, lanes=v + 1, form="LaneTiles") for k in ("dec", "int") for b in (32, 64)) and
        all(has(cic, kind="int", bits=b, layout="FM", lanes=v + 1, form="Lane") for b in (32, 64)),
        # `stages >= value`, FrameMajor
        "kHbfFmMinStages": lambda v: all(has(hbf, kind=k, layout="FM", stages=v - 1, form="Generic") and has(hbf, kind=k, layout="FM", stages=v, form="BlockFm") for k in ("dec", "int")),
        # `stages == value`, on whole 16-lane groups
        "kHbfRingStages": lambda v: has(hbf, layout="FM", stages=v, lanes=144, form="RingFm") and all(has(hbf, kind="dec", layout="FM", stages=s, lanes=16, form="BlockFm") for s in (v - 1, v + 1)),
        # `lanes % value == 0`: 16 k and 16 k + 8, 4 k and 4 k + 2
        "kHbfRingLanes": lambda v: has(hbf, stages=4, lanes=9 * v, form="RingFm") and has(hbf, kind="dec", layout="FM", stages=4, lanes=9 * v + v // 2, form="BlockFm"),
        "kHbfBlockLanes": lambda v: all(has(hbf, kind=k, lanes=9 * v, form="BlockFm") and has(hbf, kind=k, lanes=9 * v + v // 2, form="WaveFm") for k in ("dec", "int")),
        # `chunk >= value` (8 bytes is no whole piece), `chunk <= value` (256 bytes), a power of two between (48 bytes is whole pieces)
        "kCicRingMinChunkBytes": lambda v: all(has(cic, kind=k, bits=b, chunk=v, frames=64, form="RingLm") and has(cic, kind=k, bits=b, chunk=v // 2, frames=64, form="Lane", vpc=0)
                                               for k in ("dec", "int") for b in (32, 64)),
        "kCicRingMaxChunkBytes": lambda v: all(has(cic, kind=k, bits=b, chunk=v, form="RingLm") and has(cic, kind=k, bits=b, chunk=2 * v, frames=64, form="LaneTiles") and
                                               has(cic, kind=k, bits=b, chunk=48, frames=64, form="Lane") for k in ("dec", "int") for b in (32, 64)),
        # `frames >= value`
        "kCicRingMinFrames": lambda v: all(has(cic, kind=k, bits=b, layout="LM", frames=v, form="RingLm") and has(cic, kind=k, bits=b, layout="LM", frames=v - 1, form="Lane")
                                           for k in ("dec", "int") for b in (32, 64)) and
        all(has(cic, kind="int", bits=b, layout="FM", frames=v, form="RingFm") and has(cic, kind="int", bits=b, layout="FM", frames=v - 1, form="Lane") for b in (32, 64)),
        # `lanes % value == 0`: 16 k and 16 k + 8
        "kCicRingFmLanes": lambda v: all(has(cic, bits=b, lanes=9 * v, form="RingFm") and has(cic, bits=b, layout="FM", kind="int", lanes=9 * v + v // 2, form="Lane") for b in (32, 64)),
        # `lanes % value == 0`: 64 k and 64 k + 1, the tile form
        "kCicBlockLanes": lambda v: all(has(cic, kind=k, bits=b, lanes=2 * v, form="LaneTiles") and has(cic, kind=k, bits=b, layout="LM", lanes=2 * v + 1, form="Lane")
                                        for k in ("dec", "int") for b in (32, 64)),
        # `frames >= value / vpc` (vpc = 4: 3 and 4 frames; vpc = 1: 15 and 16) and `vectors per chunk <= value` (16 and 32 of them)
        "kCicTileVecs": lambda v: all(has(cic, kind=k, bits=b, chunk=64, frames=v // 4 - 1, form="Lane") and has(cic, kind=k, bits=b, chunk=64, frames=v // 4, form="LaneTiles") and
                                      has(cic, kind=k, bits=b, chunk=16, frames=v - 1, form="Lane") and has(cic, kind=k, bits=b, chunk=16, frames=v, form="LaneTiles") and
                                      has(cic, kind=k, bits=b, chunk=16 * v, form="LaneTiles") and has(cic, kind=k, bits=b, chunk=32 * v, form="Lane")
                                      for k in ("dec", "int") for b in (32, 64)),
    }
    assert set(sides) == set(T), sorted(set(sides) ^ set(T))
    assert not [name for name, ok in sides.items() if not ok(T[name])]
    # the rows were written on the header's values as they stand
    assert T == {"kPieceBytes": 16, "kGridMaxLanes": (1 << 31) - 1, "kHbfFmMinStages": 2, "kHbfRingStages": 4, "kHbfRingLanes": 16, "kHbfBlockLanes": 4,
                 "kCicRingMinChunkBytes": 16, "kCicRingMaxChunkBytes": 128, "kCicRingMinFrames": 64, "kCicRingFmLanes": 16, "kCicBlockLanes": 64, "kCicTileVecs": 16}


def test_plan_hbf_agrees_with_the_restatement_of_the_parity_suite():
    """`hbf_expected_kernel` of tests/test_gpu_parity.py (the Python restatement test_hbf_parity asserts on the GPU) and `plan_hbf` name the
    same kernel for every HBF_CASES x hbf_shapes call, on aligned buffers and one element off the grid."""
    from tests import test_gpu_parity as P

    calls = [(kind, lay, ts, s, lanes, frames, aligned) for kind in ("dec", "int") for lay in ("FM", "LM") for _, ts, s in P.HBF_CASES
             for lanes, frames in P.hbf_shapes(s) for aligned in (True, False)]
    got = ask(["hbf %s %d %d %d %d %s %d" % (kind, ts, s, lanes, frames, lay, 0 if aligned else 4) for kind, lay, ts, s, lanes, frames, aligned in calls])
    bad = []
    for (kind, lay, ts, s, lanes, frames, aligned), g in zip(calls, got):
        want = P.hbf_expected_kernel(True, kind, P.LM if lay == "LM" else P.FM, ts, s, lanes, frames, aligned)
        if g.split("\t")[0] != want:
            bad.append((kind, lay, ts, s, lanes, frames, aligned, g, want))
    assert len(calls) == 2 * 2 * 10 * 25 * 2 and not bad, (len(bad), bad[:5])
