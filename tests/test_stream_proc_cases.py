"""The case table of tests/_stream_proc_cases.py held to its own claims, without a GPU: every kernel `expected_kernel` can return for a
form has a case, every threshold of dispatch_thresholds.h that the dispatch of these forms reads has a case next to it on each side, what
the table calls unreachable is unreachable, and the specification on every case's inputs gives an output and a state that a wrong
kernel cannot match by leaving memory alone."""
import collections

import numpy as np
import pytest

from tests import _stream_proc_cases as SP
from tests import _sweep_spec as WS

FM, LM = SP.FM, SP.LM
FRAMES = (1, 15, 16, 63, 64, 511, 512)
OFFSETS = ((0, 0), (16, 16))
# how close "next to the threshold" is, in the unit the threshold is compared in: lanes come in steps of 4, frames and waves in steps of 1
# (kStaged64Lanes is read for rows on the 64-byte grid only: dense rows of a multiple of 16 lanes)
UNIT = collections.defaultdict(lambda: 4, kSweepMinFrames=1, kPairMinFrames=1, kLdsMinWaves=1, kStaged64Lanes=16)
LANE_THRESHOLDS = sorted({v for k, v in SP.THR.items() if k not in SP.NOT_CONSULTED and UNIT[k] == 4} |
                         {SP.THR["kLdsGridCap"] * SP.K_FM_BLOCK, SP.THR["kLdsMinWaves"] * SP.K_WAVE, SP.ROUND_LANES, 2 * SP.ROUND_LANES, 3 * SP.ROUND_LANES,
                          SP.ROUND_LANES + SP.THR["kSplitTailMax"], SP.ODD_MIN_BODY})


def scan_lanes():
    near = {t + d for t in LANE_THRESHOLDS for d in range(-5, 6)}
    return sorted(l for l in set(range(4, 200001, 4)) | {1, 2, 3} | near if 1 <= l <= 200000)


@pytest.fixture(scope="module")
def scan():
    """{(form, layout): {kernel key: first shape}} and the union of the traces, over lanes 1 .. 200000 (step 4 and the neighbours of every lane
    threshold), the frame counts above and rows on and 16 bytes off the 64-byte grid"""
    keys = {(f, lay): {} for f in SP.FORMS for lay in (FM, LM)}
    traces = set()
    # the dispatch depends on the processor's traits alone: forms with equal rows share a scan
    by_traits = {}
    for f in SP.FORMS:
        by_traits.setdefault(SP.TRAITS[f]._replace(proc="", entry="", words=0), []).append(f)
    for forms in by_traits.values():
        f = forms[0]
        for lay in (FM, LM):
            lanes_ = scan_lanes() if lay == FM else sorted({l for l in scan_lanes() if l % 256 == 0} | {t + d for t in LANE_THRESHOLDS for d in (-4, 0, 4)} | {1, 65, 1000})
            for lanes in lanes_:
                for frames in FRAMES + ((14, 17, 28, 31, 32, 33) if lay == LM else ()):
                    for xo, yo in OFFSETS:
                        e, tr = SP.traced(f, lay, lanes, frames, xo, yo)
                        traces |= {(g,) + t for g in forms for t in tr}
                        for g in forms:
                            keys[(g, lay)].setdefault(SP.kernel_key(e), (lanes, frames, xo, yo))
    return keys, traces


def case_keys():
    out = collections.defaultdict(set)
    for c in SP.CASES:
        out[(c.form, c.layout)].add(SP.kernel_key(SP.expected_kernel(c.form, c.layout, c.lanes, c.frames, c.x_off, c.y_off)))
    return out


def test_every_kernel_a_form_can_reach_has_a_case(scan):
    keys, _ = scan
    have = case_keys()
    missing = [(f, lay, k, shape) for (f, lay), ks in keys.items() for k, shape in ks.items() if k not in have[(f, lay)]]
    assert not missing, missing
    # ... and that is more than the two prefixes the parity files assert
    for f in ("clamp", "unwrap0"):
        assert len(keys[(f, FM)]) >= 12 and len(keys[(f, LM)]) == 4, (f, sorted(keys[(f, FM)]))
    for (f, lay), ks in sorted(keys.items()):
        print(f, "FM" if lay == FM else "LM", len(ks), "kernels:", sorted(ks))


# Cases per (form, layout).  This is a tally, not a coverage check: it only says that nobody took a row out of the table (or slipped one in)
# without looking, also where another row reaches the same kernel; it is edited by hand with the table.  What shows that a row is NEEDED are
# the scan above (a kernel without a case), the threshold test below (a side without a case) and the named shapes of `minimum()`.
COUNTS = {("clamp", FM): 44, ("clamp", LM): 10, ("unwrap0", FM): 44, ("unwrap0", LM): 10, ("unwrap1", FM): 6, ("unwrap1", LM): 3,
          ("pll0", FM): 10, ("pll0", LM): 10, ("pll1", FM): 10, ("pll1", LM): 10, ("pll2", FM): 6, ("pll2", LM): 3,
          ("rpll", FM): 8, ("rpll", LM): 10, ("sweep", FM): 6, ("sweep", LM): 10}


def minimum():
    """the FrameMajor shapes the cheap 4-byte forms must hold at the least — (lanes, frames, bytes off the grid) — written on the thresholds by
    name, so that a changed threshold moves them instead of switching the check off.  With the header as it stands: (3, 64), (3, 63), (4, 64),
    (8193, 16), (8189, 16), (8193, 15), (65540, 16), (86016, 16), (86020, 16), (65540, 15), (200704, 16), (4, 512), (24576, 512), (24576, 511),
    (24580, 512), (24576, 16), (24572, 16), (65536, 16), (131072, 16), (32768, 16) 16 bytes off, (8192, 16), (8188, 16), (65536, 15), (1000, 15)"""
    T, R = SP.THR, SP.ROUND_LANES
    pl, pf, sl, sf, tail = T["kPairMaxLanes"], T["kPairMinFrames"], T["kSweepMinLanesFps"], T["kSweepMinFrames"], T["kSplitTailMax"]
    return [(3, 64, 0), (3, 63, 0), (4, 64, 0), (SP.ODD_MIN_BODY + 1, 16, 0), (SP.ODD_MIN_BODY - 3, 16, 0), (SP.ODD_MIN_BODY + 1, 15, 0),
            (R + 4, 16, 0), (R + tail, 16, 0), (R + tail + 4, 16, 0), (R + 4, 15, 0), (3 * R + 4096, 16, 0),
            (4, pf, 0), (pl, pf, 0), (pl, pf - 1, 0), (pl + 4, pf, 0), (sl, sf, 0), (sl - 4, sf, 0), (R, 16, 0), (2 * R, 16, 0), (32768, 16, 16),
            (T["kStaged32Lanes"], 16, 0), (T["kStaged32Lanes"] - 4, 16, 0), (R, 15, 0), (1000, 15, 0)]


def test_the_table_is_whole():
    got = collections.Counter((c.form, c.layout) for c in SP.CASES)
    assert dict(got) == COUNTS, sorted(set(got.items()) ^ set(COUNTS.items()))
    assert len(set(SP.CASES)) == len(SP.CASES) and len({c[:6] for c in SP.CASES}) == len(SP.CASES), "a shape twice"
    for f in ("clamp", "unwrap0"):
        have = {(c.lanes, c.frames, c.x_off) for c in SP.CASES if c.form == f and c.layout == FM}
        assert not set(minimum()) - have, (f, sorted(set(minimum()) - have))
    lo, hi = SP.THR["kStagedHeavyMinLanes"], SP.THR["kStagedHeavyMaxLanes"]
    for f in ("pll0", "pll1", "rpll"):
        have = {(c.lanes, c.frames) for c in SP.CASES if c.form == f and c.layout == FM}
        assert {(lo, 16), (hi, 16), (24577, 16)} <= have, f
    # the largest case moves tens of MiB at the most (the pair kernel's 512 frames x 24576 lanes, in and out)
    for c in SP.CASES:
        t = SP.TRAITS[c.form]
        assert c.lanes * c.frames * ((t.in_bytes if t.has_in else 0) + t.out_bytes) <= 100 << 20, c


def test_every_threshold_has_a_case_on_each_side(scan):
    _, scanned = scan
    consulted = {name for _, name, _, _ in scanned}
    assert consulted | set(SP.NOT_CONSULTED) == set(SP.THR) and not consulted & set(SP.NOT_CONSULTED), sorted(set(SP.THR) ^ (consulted | set(SP.NOT_CONSULTED)))
    near = set()
    for c in SP.CASES:
        _, tr = SP.traced(c.form, c.layout, c.lanes, c.frames, c.x_off, c.y_off)
        near |= {(name, above) for name, above, dist in tr if dist <= UNIT[name]}
    excused = {(name, above) for name, above, _ in SP.UNREACHABLE_SIDES}
    missing = [(name, above) for name in sorted(consulted) for above in (False, True) if (name, above) not in near | excused]
    assert not missing, missing
    # what the table excuses, no shape of the scan reaches either — and nothing is excused that a case does reach
    reached = {(name, above) for _, name, above, dist in scanned if dist <= UNIT[name]}
    assert not excused & reached and not excused & near, sorted(excused & (reached | near))


def test_unreachable_branches_are_unreachable(scan):
    keys, _ = scan
    for forms, layout, prefix, why in SP.UNREACHABLE:
        assert why
        for f in forms:
            hit = [k for k in keys[(f, layout)] if k[0].startswith(prefix)]
            assert not hit, (f, prefix, hit)
            assert not [c for c in SP.CASES if c.form == f and c.layout == layout and
                        SP.expected_kernel(c.form, c.layout, c.lanes, c.frames, c.x_off, c.y_off).startswith(prefix)]


def test_expected_kernel_at_the_pinned_biquad_free_facts():
    """three names read off the launcher by hand, as a check of the restatement's plumbing (prefix, suffix, offsets)"""
    e = SP.expected_kernel("clamp", FM, 65540, 16)
    assert (e, e.suffix) == ("stream_frame_major_lds + stream_frame_major_staged (remainder, second stream)<", "")
    e = SP.expected_kernel("unwrap0", FM, 32768, 16, 16, 16)
    assert (e, e.suffix) == ("stream_frame_major_sweep[1 block/workgroup, XCD-contiguous]<", " [2 frames/segment]")
    e = SP.expected_kernel("pll0", FM, 24577, 16)
    assert (e, e.suffix) == ("stream_frame_major_staged[32 lanes/wave]<", " + stream_frame_major_few (lanes % 4, second stream)")
    assert SP.expected_kernel("clamp", LM, 1000, 32, 4, 4) == "stream_lane_major<" and SP.expected_kernel("clamp", LM, 1000, 32) == "stream_lane_major_staged[16 lanes/wave]<"
    assert SP.expected_kernel("clamp", FM, 24576, 512, 4, 4).startswith("stream_frame_major_sweep[")
    assert SP.sweep_geometry(65536, 4) == (1, 256, 256, 1) and SP.sweep_geometry(100000, 16) == (2, 241, 208, 1) and SP.sweep_geometry(1 << 20, 16) == (16, 256, 256, 1)


SHAPES = sorted({(c.form, c.lanes, c.frames) for c in SP.CASES})


@pytest.mark.parametrize("form,lanes,frames", SHAPES)
def test_the_specification_on_the_cases_inputs(form, lanes, frames):
    cfg, x, st, after, out = SP.reference(form, lanes, frames)
    t = SP.TRAITS[form]
    assert st.shape == (t.words, lanes) and out.shape[:2] == (frames, lanes)
    assert out.dtype == (np.int64 if form == "unwrap1" else np.int32)
    assert not (out == SP.POISON).any(), "an output the poison would pass for"
    assert not np.array_equal(st, after)
    changed = (st != after).any(axis=0)
    if form == "sweep":
        ended = WS.ended_np(after)
        assert ended.mean() <= 0.5, ended.mean()
        assert changed.mean() >= 0.5  # a lane that had ended does not move
        live = (out != 0).any(axis=2)
        assert live[-1].mean() >= 0.5 and (lanes < 8 or not live[:, 4].any())
    else:
        assert changed.all(), "every lane's state moves"
    if form == "rpll":
        some = (x[..., 0] != 0).mean()
        assert 0.25 <= some <= 0.5, some
