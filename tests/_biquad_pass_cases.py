"""How the n sections of a biquad-family call are cut into launches (`next_pass`, idsp_amd/csrc/biquad_pass_plan.h): ONE hand-written table,
shared by tests/test_biquad_pass_plan.py (no GPU: the function through build/stream_plan_cli, verb `passes`) and
tests/test_gpu_biquad_passes.py (the entries themselves, for the rows of several passes).

A schedule lists the launches in order: `4+4` is one launch of the two-wave kernel (stream_frame_major_duo) with four sections on either
wave, `4` one launch of launch_stream with four sections.  The expectations were read off the five loops that decided this before the
choice moved into biquad_pass_plan.h; `biquad_sections.h:N`, `normal_wdf.hip:N` and `biquad_i16.hip:N` below are line numbers of that
revision, the parent of the commit that added this file:

  biquad_sections.h:748-780  run_chain: `md = min(n - done, 8)`; two waves when `duo_wanted(md, ...) && (md >= 5 || (!kClamp && W <= 4))` (:752),
                             splits 2+2, 3+2, 3+3, 4+3, 4+4 (:755-759); else `m = min(n - done, 4)` on one wave (:768); 4-byte samples only (:734, :749)
  biquad_sections.h:804-830  run_chain_bylane: `md = min(n - done, 4)`; two waves when `md >= 3 && duo_wanted(5, ...)` (:809), splits 2+1, 2+2
                             (:812-813); else `m = min(n - done, 2)` (:821); 4-byte samples only (:805)
  biquad_sections.h:874-893  run_cascade: one launch of all n <= 8; two waves when `n >= 5 && duo_wanted(n, ...)` (:875), splits 3+2 .. 4+4
                             (:877-880); 4-byte samples only (:874)
  normal_wdf.hip:234-246     idsp_wdf_i32: `k = min(n - done, 4)` (:235); two waves when `K >= 2 && duo_wanted(5, ...)` (:166-168), split
                             (K + 1) / 2 + K / 2 (:168); a pass that holds an order above 4 stays on one wave (:160) — the entry's rule, not the plan's
  biquad_i16.hip:76-88, biquad_i16_bylane.hip:55-67   `m = min(n - done, 4)`, never two waves
  stream_plan.h:200-204      duo_wanted(m, lanes, layout): FRAME_MAJOR, lanes >= kDuoMinLanes, not IDSP_NO_DUO (under IDSP_DIAG=1), and
                             `m >= 5 || (m == 4 && lanes <= kDuo4MaxLanes)`

Test infrastructure only."""
from tests._stream_proc_cases import THR

LO, HI4 = THR["kDuoMinLanes"], THR["kDuo4MaxLanes"]

# family -> (the verb's family, sample bytes, clamp, state words per section, (max_single, max_duo, duo_min) as the issue of this change states them)
FAMILIES = {
    # plain 4-byte chains of up to 4 state words: four sections already take two waves
    "i32_df1": ("chain", 4, 0, 4, (4, 8, 4)), "f32_df1": ("chain", 4, 0, 4, (4, 8, 4)), "f32_df2t": ("chain", 4, 0, 2, (4, 8, 4)), "normal_i32": ("chain", 4, 0, 4, (4, 8, 4)),
    # clamped, or 5 / 6 state words: from five sections
    "i32_df1_clamp": ("chain", 4, 1, 4, (4, 8, 5)), "f32_df2t_clamp": ("chain", 4, 1, 2, (4, 8, 5)), "i32_dither": ("chain", 4, 0, 5, (4, 8, 5)),
    "i32_wide": ("chain", 4, 0, 6, (4, 8, 5)), "i32_wide_clamp": ("chain", 4, 1, 6, (4, 8, 5)),
    # 8-byte samples: one wave
    "f64_df1": ("chain", 8, 0, 8, (4, 0, 0)), "f64_df2t": ("chain", 8, 0, 4, (4, 0, 0)),
    "bylane_i32": ("bylane", 4, 0, 4, (2, 4, 3)), "bylane_f64": ("bylane", 8, 0, 8, (2, 0, 0)),
    "cascade_i32": ("cascade", 4, 0, 0, (8, 8, 5)), "cascade_f64": ("cascade", 8, 0, 0, (8, 0, 0)),
    "wdf": ("wdf", 4, 0, 0, (4, 4, 2)),
    "i16": ("i16", 2, 0, 4, (4, 0, 0)),
}
PLAIN = ("i32_df1", "f32_df1", "f32_df2t", "normal_i32")
HEAVY = ("i32_df1_clamp", "f32_df2t_clamp", "i32_dither", "i32_wide", "i32_wide_clamp")
DUO_OFF = ("IDSP_DIAG=1", "IDSP_NO_DUO=1")


def _rows(families, lanes, table, layout="FM", switches=()):
    return [(f, n, lanes, layout, tuple(switches), schedule) for f in families for n, schedule in table]


# (family, n, lanes, layout, switches, schedule)
ROWS = (
    # biquad_sections.h:750-768 at kDuoMinLanes
    _rows(PLAIN, LO, [(1, "1"), (2, "2"), (3, "3"), (4, "2+2"), (5, "3+2"), (6, "3+3"), (7, "4+3"), (8, "4+4"), (9, "4+4 1"), (12, "4+4 2+2"), (13, "4+4 3+2")])
    # four sections above kDuo4MaxLanes stay on one wave, eight do not (stream_plan.h:203)
    + _rows(PLAIN, HI4 + 4, [(4, "4"), (8, "4+4"), (12, "4+4 4")]) + _rows(PLAIN, HI4, [(4, "2+2"), (12, "4+4 2+2")])
    # below kDuoMinLanes, LANE_MAJOR, IDSP_NO_DUO (honoured under IDSP_DIAG=1 only): stream_plan.h:202
    + _rows(PLAIN, LO - 4, [(4, "4"), (9, "4 4 1")]) + _rows(PLAIN, LO, [(9, "4 4 1")], "LM") + _rows(PLAIN, LO, [(9, "4 4 1")], "FM", DUO_OFF)
    + _rows(PLAIN, LO, [(9, "4+4 1")], "FM", ("IDSP_NO_DUO=1",))
    # biquad_sections.h:752, `md >= 5 || (!Sec::kClamp && Sec::W <= 4)`: the clamp forms, dither (5 words), wide (6 words)
    + _rows(HEAVY, LO, [(1, "1"), (4, "4"), (5, "3+2"), (8, "4+4"), (9, "4+4 1"), (12, "4+4 4"), (13, "4+4 3+2")]) + _rows(HEAVY, LO - 4, [(5, "4 1"), (9, "4 4 1")])
    # biquad_sections.h:734, 749: 8-byte samples have no two-wave instantiations
    + _rows(("f64_df1", "f64_df2t"), LO, [(4, "4"), (5, "4 1"), (9, "4 4 1")]) + _rows(("f64_df1",), HI4 + 4, [(9, "4 4 1")]) + _rows(("f64_df1",), 64, [(9, "4 4 1")])
    # biquad_sections.h:808-825
    + _rows(("bylane_i32",), LO, [(1, "1"), (2, "2"), (3, "2+1"), (4, "2+2"), (5, "2+2 1"), (6, "2+2 2"), (7, "2+2 2+1")])
    + _rows(("bylane_i32",), HI4 + 4, [(4, "2+2")]) + _rows(("bylane_i32",), LO - 4, [(3, "2 1"), (5, "2 2 1")]) + _rows(("bylane_i32",), LO, [(5, "2 2 1")], "LM")
    + _rows(("bylane_f64",), LO, [(3, "2 1"), (5, "2 2 1")])
    # biquad_sections.h:875-892
    + _rows(("cascade_i32",), LO, [(1, "1"), (4, "4"), (5, "3+2"), (6, "3+3"), (7, "4+3"), (8, "4+4")]) + _rows(("cascade_i32",), HI4 + 4, [(8, "4+4")])
    + _rows(("cascade_i32",), LO - 4, [(5, "5"), (8, "8")]) + _rows(("cascade_i32",), LO, [(8, "8")], "LM") + _rows(("cascade_i32",), LO, [(8, "8")], "FM", DUO_OFF)
    + _rows(("cascade_f64",), LO, [(5, "5"), (8, "8")])
    # normal_wdf.hip:166-168, 235
    + _rows(("wdf",), LO, [(1, "1"), (2, "1+1"), (3, "2+1"), (4, "2+2"), (5, "2+2 1"), (7, "2+2 2+1")]) + _rows(("wdf",), HI4 + 4, [(4, "2+2")])
    + _rows(("wdf",), LO - 4, [(2, "2"), (7, "4 3")]) + _rows(("wdf",), LO, [(7, "4 3")], "LM")
    # biquad_i16.hip:77, biquad_i16_bylane.hip:56
    + _rows(("i16",), LO, [(1, "1"), (4, "4"), (5, "4 1"), (9, "4 4 1")]) + _rows(("i16",), HI4 + 4, [(9, "4 4 1")])
)


def line(family, n, lanes, layout="FM", switches=()):
    """the `passes` line of tests/cpp/stream_plan_cli.cpp for a row"""
    verb, size, clamp, words, _ = FAMILIES[family]
    return "passes %s %d %d %d %d %d %s %s" % (verb, size, clamp, words, n, lanes, layout, " ".join(switches))


def schedule_of(family, n, lanes=LO, layout="FM", switches=()):
    """the table's schedule of a call -> list of (na, nb)"""
    (s,) = {r[5] for r in ROWS if r[:5] == (family, n, lanes, layout, tuple(switches))}
    return [tuple(int(v) for v in (p + "+0").split("+")[:2]) for p in s.split(" ")]


# The entries tests/test_gpu_biquad_passes.py runs, one per family: (entry, family, n) — rows of the default switches at kDuoMinLanes
GPU_ROWS = [("biquad_i32_df1", "i32_df1", 12), ("biquad_i32_df1", "i32_df1", 9), ("biquad_i32_wide_clamp", "i32_wide_clamp", 12), ("biquad_f64_df1", "f64_df1", 5),
            ("biquad_i32_df1_bylane", "bylane_i32", 7), ("cascade_i32_df1", "cascade_i32", 8), ("wdf_i32", "wdf", 7), ("biquad_i16_df1", "i16", 9)]
