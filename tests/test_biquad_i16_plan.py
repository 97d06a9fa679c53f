"""`plan_biquad_i16` (idsp_amd/csrc/biquad_i16_plan.h), the pure function that picks the kernel form and the grid of a pass of
idsp_biquad_i16_df1 / _df1_clamp, through tests/cpp/biquad_i16_plan_cli.cpp: plain g++, neither HIP nor the library nor a GPU.  The
table is the rule of include/idsp_hip.h; tests/test_gpu_biquad_i16.py holds the device to the same rule by idsp_last_kernel()."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAMES = "biquad_i16_frame_major"
DWORDS, HALVES = "biquad_i16_lane_major[dword runs]", "biquad_i16_lane_major[half runs]"
A = 0x7F0000001000  # a device address on the 4 KiB grid


@pytest.fixture(scope="module")
def cli():
    exe = os.path.join(ROOT, "build", "biquad_i16_plan_cli")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Iinclude", "tests/cpp/biquad_i16_plan_cli.cpp", "-o", exe], cwd=ROOT, check=True)

    def ask(*cases):
        text = "".join(" ".join(str(v) for v in c) + "\n" for c in cases)
        r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60, check=True)
        out = []
        for ln in r.stdout.splitlines():
            name, rest = ln.split("\t")
            out.append((name, dict((k, int(v)) for k, v in (kv.split("=") for kv in rest.split()))))
        assert len(out) == len(cases), r.stdout
        return out

    return ask


def test_frame_major_has_one_form(cli):
    """one lane per thread whatever the alignment; one wave per workgroup below 65536 lanes, four from there"""
    cases = [
        ("FM", 65536, A, A + 0x100000, 65536, 65536, 256, 256),   # the headline shape: 1024 waves
        ("FM", 65536, A, A, 65536, 65536, 256, 256),              # in place
        ("FM", 65535, A, A + 64, 65535, 65535, 1024, 64),
        ("FM", 65537, A + 2, A + 6, 65538, 65539, 257, 256),
        ("FM", 16384, A, A + 64, 16384, 16390, 256, 64),
        ("FM", 1, A, A + 4, 2, 2, 1, 64), ("FM", 64, A, A + 4, 64, 64, 1, 64), ("FM", 65, A + 2, A + 4, 65, 65, 2, 64),
        ("FM", 1 << 31, A, A + 4, 1 << 31, 1 << 31, 1 << 23, 256),
    ]
    for (name, p), c in zip(cli(*[c[:6] for c in cases]), cases):
        assert name == FRAMES and p["form"] == 1 and p["grid"] == c[6] and p["block"] == c[7], (c, name, p)


def test_lane_major_forms(cli):
    cases = [
        ("LM", 65536, A, A + 0x100000, 4096, 4096, DWORDS, 1024),
        ("LM", 65537, A, A, 4097 + 1, 4097 + 1, DWORDS, 1025),   # odd frame counts live in the pitch: the form depends on the pitch alone
        ("LM", 1, A, A + 4, 2, 2, DWORDS, 1),
        ("LM", 64, A, A + 4, 4097, 4098, HALVES, 1),             # a dense odd row
        ("LM", 65, A + 2, A + 4, 4096, 4096, HALVES, 2),
        ("LM", 65, A, A + 6, 4096, 4096, HALVES, 2),
        ("LM", 65, A, A + 8, 4096, 4099, HALVES, 2),
    ]
    for (name, p), c in zip(cli(*[c[:6] for c in cases]), cases):
        assert name == c[6] and p["grid"] == c[7] and p["block"] == 64, (c, name, p)


def test_every_residue_agrees_with_the_rule(cli):
    """all 2 x 4 x 4 x 2 x 2 x 2 combinations of layout, address residues, pitch parities and lane parity against the rule, restated"""
    cases, want = [], []
    for layout in ("FM", "LM"):
        for xo in (0, 2, 4, 6):
            for yo in (0, 2, 4, 6):
                for xl in (1000, 1001):
                    for yl in (1000, 1003):
                        for lanes in (998, 999):
                            cases.append((layout, lanes, A + xo, A + 0x10000 + yo, xl, yl))
                            grid4 = xo % 4 == 0 and yo % 4 == 0 and xl % 2 == 0 and yl % 2 == 0
                            if layout == "LM":
                                want.append((DWORDS if grid4 else HALVES, -(-lanes // 64)))
                            else:
                                want.append((FRAMES, -(-lanes // 64)))
    for (name, p), w, c in zip(cli(*cases), want, cases):
        assert (name, p["grid"]) == w, c


def test_measurement_switches(cli):
    """what IDSP_DIAG=1 lets a measurement override: the FrameMajor workgroup size, in whole waves up to four"""
    got = cli(("FM", 65536, A, A, 65536, 65536, "fm_block=64"), ("FM", 16384, A, A, 16384, 16384, "fm_block=256"),
              ("FM", 65536, A, A, 65536, 65536, "fm_block=100"), ("FM", 65536, A, A, 65536, 65536, "fm_block=512"),
              ("LM", 65536, A, A, 4096, 4096, "fm_block=256"))
    assert got[0] == (FRAMES, {"form": 1, "grid": 1024, "block": 64})
    assert got[1] == (FRAMES, {"form": 1, "grid": 64, "block": 256})
    assert got[2][1]["block"] == 256 and got[3][1]["block"] == 256  # not whole waves / too many: ignored
    assert got[4] == (DWORDS, {"form": 2, "grid": 1024, "block": 64})
