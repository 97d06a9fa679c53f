"""Which kernel each of the eight lock-in entries takes, and with which launch parameters: one table, shared by
tests/test_lockin_plan.py (no GPU: `plan_lockin` of idsp_amd/csrc/lockin_plan.h through build/stream_plan_cli) and
tests/test_gpu_lockin_plan.py (the real entries, through `idsp_last_kernel()`).

Every expectation was written by hand from the dispatch as it stood before the choice moved into lockin_plan.h (the parent of the
commit that added this file): `lockin_waves_for` / `lockin_lm_body` and the three entries of dds.hip, `waves_take` / `lm_body` and the
four entries of lockin_generic.hip, `lockin_stage_groups`, `launch_lockin_waves_bank` and `launch_lockin_waves_in` of lockin_waves.h,
idsp_lockin_i32_accu_process of lockin_accu.hip.  None was produced by running the new function.

A row: entry (idsp_lockin_i32_<entry>, or idsp_lockin_f32_biquad_lo_process), a / b (order / cascade of `[Lowpass<a>; b]`, or n sections / 0),
lanes, frames, layout, (x, y) byte offsets from a 64-byte boundary, switches (honoured with IDSP_DIAG=1 only), what idsp_last_kernel()
reports (`stream_<Processor>` where launch_stream names the kernel: it begins with `stream_` and names that processor), the launch
parameters, and whether the row also runs on the GPU (not: 2^28 lanes, no frames, the start-up stagger — a kernel argument of calls of
2048 frames or more that no name shows — and a switch without IDSP_DIAG).  Imports neither torch nor the library."""
import collections

Case = collections.namedtuple("Case", "entry a b lanes frames layout off sw name params gpu tuned")

W4, W6 = "lockin_waves_kernel[4 waves per 64 lanes]", "lockin_waves_kernel[6 waves per 64 lanes]"
ST8, ST16 = "lockin_stages_kernel[8 waves per 64 lanes]", "lockin_stages_kernel[16 waves per 128 lanes]"
TAIL = "lockin_waves_kernel + stream kernel (last frames % 16)"
SPLIT_MAX = 40960  # thr::kSplitMaxLanes


def waves(n, batch, inp, body, skew=0):
    return "waves=%d groups=0 batch=%d in=%s skew=%d body=%d split=0" % (n, batch, inp, skew, body)


def stages(groups, body):
    return "waves=0 groups=%d batch=0 in=- skew=0 body=%d split=0" % (groups, body)


def stream(split=0):
    return "waves=0 groups=0 batch=0 in=- skew=0 body=0 split=%d" % split


def row(entry, a, b, lanes, frames, layout, name, params, off=(0, 0), sw=None, gpu=True, tuned=False):
    return Case(entry, a, b, lanes, frames, layout, off, dict(sw or {}), name, params, gpu, tuned)


READOUTS = ("process", "arg", "norm_sqr")
PROC = {"process": "LockinProc<%d, %d>", "arg": "LockinPolarProc<%d, %d, 0>", "norm_sqr": "LockinPolarProc<%d, %d, 1>"}
CASES = []

# ---- both sides of every lane threshold, one workgroup apart, per read-out: `[Lowpass<2>; 1]`, FrameMajor, 16 frames, aligned
# (dds.hip:50 `lanes <= 16384` six waves; :54 `heavy_readout && lanes <= kSplitMaxLanes && arm_weight < 6`; lockin_waves.h:883 b16)
for entry in READOUTS:
    arg = entry == "arg"
    for lanes, n, batch in ((16384, 6, 16), (16448, 6 if arg else 4, 8 if arg else 16), (40960, 6 if arg else 4, 8 if arg else 16), (41024, 4, 8),
                            (49152, 4, 8), (49216, 4, 16), (65536, 4, 16), (65600, 4, 8)):
        CASES.append(row(entry, 2, 1, lanes, 16, "FM", W6 if n == 6 else W4, waves(n, batch, "FM_DMA", 16)))
    # LaneMajor: no six waves by lane count (dds.hip:50 is FrameMajor's), kLwBLm always, DMA for four waves and not arg (lockin_waves.h:889)
    for lanes in (16384, 16448, 40960, 41024):
        n = 6 if arg and lanes <= SPLIT_MAX else 4
        CASES.append(row(entry, 2, 1, lanes, 16, "LM", W6 if n == 6 else W4, waves(n, 16, "LM_REG" if arg else "LM_DMA", 16)))
    # ... and on the stream path (20 LaneMajor frames: neither whole batches nor 32): two threads per lane for `Complex<i32>` up to kSplitMaxLanes (dds.hip:612)
    for lanes in (40960, 41024):
        split = int(entry == "process" and lanes <= SPLIT_MAX)
        CASES.append(row(entry, 2, 1, lanes, 20, "LM", "stream_<%s>" % (("LockinSplitProc<%d, %d>" if split else PROC[entry]) % (2, 1)), stream(split)))

# ---- order x cascade < 6 (dds.hip:54), arg at 32768 lanes; K != 2, which would be the stage-wave kernel's
CASES += [row("arg", 1, 4, 32768, 16, "FM", W6, waves(6, 8, "FM_DMA", 16)), row("arg", 2, 3, 32768, 16, "FM", W4, waves(4, 16, "FM_DMA", 16)),
          row("arg", 2, 4, 32768, 16, "FM", W4, waves(4, 16, "FM_DMA", 16)), row("arg", 1, 3, 32768, 16, "FM", W6, waves(6, 8, "FM_DMA", 16)),
          row("arg", 2, 3, 32768, 16, "LM", W4, waves(4, 16, "LM_REG", 16)), row("arg", 1, 4, 32768, 16, "LM", W6, waves(6, 16, "LM_REG", 16)),
          # the other read-outs do not look at it
          row("process", 1, 4, 32768, 16, "FM", W4, waves(4, 16, "FM_DMA", 16)), row("norm_sqr", 2, 3, 32768, 16, "FM", W4, waves(4, 16, "FM_DMA", 16))]

# ---- the stage-wave kernel (lockin_waves.h:810-824): K = 2, FrameMajor, frames % 16, lanes % 64, x % 16; one group up to 16384 lanes, above
# that arg only, two groups, lanes % 128
for entry in READOUTS:
    arg = entry == "arg"
    CASES += [row(entry, 2, 2, 16384, 16, "FM", ST8, stages(1, 16)), row(entry, 1, 2, 16384, 16, "FM", ST8, stages(1, 16)),
              row(entry, 2, 2, 16384, 15, "FM", W6, waves(6, 16, "FM_DMA", 15)),
              row(entry, 2, 2, 16448, 16, "FM", W6 if arg else W4, waves(6, 8, "FM_DMA", 16) if arg else waves(4, 16, "FM_DMA", 16)),
              row(entry, 2, 2, 32768, 16, "FM", ST16 if arg else W4, stages(2, 16) if arg else waves(4, 16, "FM_DMA", 16)),
              row(entry, 2, 2, 32832, 16, "FM", W6 if arg else W4, waves(6, 8, "FM_DMA", 16) if arg else waves(4, 16, "FM_DMA", 16)),
              # x 4 bytes off: no stage-wave kernel, no DMA (lockin_waves.h:893), and with the register input 8-frame batches whatever b16 says
              row(entry, 2, 2, 16384, 16, "FM", W6, waves(6, 8, "FM_REG", 16), off=(4, 0)),
              # lanes % 64: the same
              row(entry, 2, 2, 16400, 16, "FM", W6 if arg else W4, waves(6 if arg else 4, 8, "FM_REG", 16)),
              # LaneMajor: never
              row(entry, 2, 2, 16384, 16, "LM", W6 if arg else W4, waves(6 if arg else 4, 16, "LM_REG" if arg else "LM_DMA", 16))]
CASES += [row("arg", 2, 2, 65536, 16, "FM", ST16, stages(2, 16)), row("arg", 2, 2, 65600, 16, "FM", W4, waves(4, 8, "FM_DMA", 16))]

# ---- LaneMajor frame counts (dds.hip:44 whole batches; :63 body + tail from 32 frames, frames % 4), 4096 lanes
for entry in READOUTS:
    arg = entry == "arg"
    n, inp, name = (6, "LM_REG", W6) if arg else (4, "LM_DMA", W4)
    sp = "stream_<%s>" % (("LockinSplitProc<%d, %d>" if entry == "process" else PROC[entry]) % (2, 1))
    for frames in (16, 32, 48):
        CASES.append(row(entry, 2, 1, 4096, frames, "LM", name, waves(n, 16, inp, frames)))
    for frames in (20, 28, 30):
        CASES.append(row(entry, 2, 1, 4096, frames, "LM", sp, stream(int(entry == "process"))))
    CASES.append(row(entry, 2, 1, 4096, 36, "LM", TAIL, waves(n, 16, inp, 32)))
    # rows 4 bytes off (x; and y for the 4-byte read-out): the stream kernels, whole batches or not
    CASES += [row(entry, 2, 1, 4096, 32, "LM", sp, stream(int(entry == "process")), off=(4, 0)), row(entry, 2, 1, 4096, 36, "LM", sp, stream(int(entry == "process")), off=(4, 0))]
CASES += [row("arg", 2, 1, 4096, 32, "LM", "stream_<LockinPolarProc<2, 1, 0>>", stream(), off=(0, 4)), row("arg", 2, 1, 4096, 36, "LM", "stream_<LockinPolarProc<2, 1, 0>>", stream(), off=(0, 4)),
          # FrameMajor does not look at y, nor at the frame count
          row("arg", 2, 1, 4096, 36, "FM", W6, waves(6, 16, "FM_DMA", 36), off=(0, 4)), row("process", 2, 1, 4096, 1, "FM", W6, waves(6, 16, "FM_DMA", 1))]

# ---- the biquad and LO entries: four waves always (lockin_waves_biquad.hip, lockin_waves_lo.hip pass 4), the same batch and input rules
BQ_LO, BQ_LO_F = "LockinBiquadLoProc<idsp::bq::Df1I32<false>, 2>", "LockinBiquadLoProc<idsp::bq::Df1F32<false>, 2>"
for entry, a, b, bank, proc in (("biquad_process", 2, 0, "[Biquad; 2]", "LockinBiquadProc<2>"), ("lo_process", 2, 1, "[Lowpass<N>; K], LO", "LockinLoProc<2, 1>"),
                                ("biquad_lo_process", 2, 0, "[Biquad; 2], LO", BQ_LO), ("f32_biquad_lo_process", 2, 0, "[Biquad<f32>; 2], LO", BQ_LO_F)):
    wn, sn = "%s<%s>" % (W4, bank), "stream_<%s>" % proc
    CASES += [row(entry, a, b, 4096, 16, "FM", wn, waves(4, 16, "FM_DMA", 16)), row(entry, a, b, 4096, 16, "LM", wn, waves(4, 16, "LM_DMA", 16)),
              row(entry, a, b, 4096, 20, "LM", sn, stream()), row(entry, a, b, 4096, 20, "FM", wn, waves(4, 16, "FM_DMA", 20)),
              # body + tail: the biquad phase entry records the combined name, the LO entries leave the tail's stream launch (lockin_generic.hip:324, :344)
              row(entry, a, b, 4096, 36, "LM", TAIL + "<[Biquad; n]>" if entry == "biquad_process" else sn, waves(4, 16, "LM_DMA", 32)),
              row(entry, a, b, 4096, 28, "LM", sn, stream()),
              # the LO entries test x and y (8-byte aligned at the least), not lo
              row(entry, a, b, 4096, 32, "LM", sn, stream(), off=(0, 8)), row(entry, a, b, 4096, 36, "LM", sn, stream(), off=(4, 0)),
              row(entry, a, b, 4096, 16, "FM", wn, waves(4, 8, "FM_REG", 16), off=(4, 0)),
              # b16 for four waves: up to kSplitMaxLanes, and 49152 < lanes <= 65536
              row(entry, a, b, 40960, 16, "FM", wn, waves(4, 16, "FM_DMA", 16)), row(entry, a, b, 41024, 16, "FM", wn, waves(4, 8, "FM_DMA", 16)),
              row(entry, a, b, 49152, 16, "FM", wn, waves(4, 8, "FM_DMA", 16)), row(entry, a, b, 49216, 16, "FM", wn, waves(4, 16, "FM_DMA", 16)),
              row(entry, a, b, 65536, 16, "FM", wn, waves(4, 16, "FM_DMA", 16)), row(entry, a, b, 65600, 16, "FM", wn, waves(4, 8, "FM_DMA", 16)),
              # IDSP_LOCKIN_WAVES is the lowpass phase entries' alone; IDSP_LOCKIN_NO_LM_TAIL too (lockin_generic.hip `lm_body` does not read it)
              row(entry, a, b, 4096, 16, "FM", wn, waves(4, 16, "FM_DMA", 16), sw={"IDSP_LOCKIN_WAVES": "6"}),
              row(entry, a, b, 4096, 36, "LM", TAIL + "<[Biquad; n]>" if entry == "biquad_process" else sn, waves(4, 16, "LM_DMA", 32), sw={"IDSP_LOCKIN_NO_LM_TAIL": "1"}),
              row(entry, a, b, 4096, 16, "FM", sn, stream(), sw={"IDSP_LOCKIN_NO_WAVES": "1"})]
# `[Lowpass<N>; 2]` with an LO buffer is not the stage-wave kernel's
CASES.append(row("lo_process", 2, 2, 16384, 16, "FM", W4 + "<[Lowpass<N>; K], LO>", waves(4, 16, "FM_DMA", 16)))
# the `Accu` rows: the stream kernels, two threads per lane up to kSplitMaxLanes (lockin_accu.hip:58); frames = updates (batch_log2 = 0)
CASES += [row("accu_process", 2, 2, 40960, 16, lay, "stream_<LockinAccuSplitProc<2, 2>>", stream(1)) for lay in ("FM", "LM")]
CASES += [row("accu_process", 2, 2, 41024, 16, lay, "stream_<LockinAccuProc<2, 2>>", stream(0)) for lay in ("FM", "LM")]

# ---- one row per switch (lowpass phase entries)
CASES += [
    row("process", 2, 1, 4096, 16, "FM", "stream_<LockinSplitProc<2, 1>>", stream(1), sw={"IDSP_LOCKIN_NO_WAVES": "1"}),
    row("arg", 2, 1, 4096, 16, "LM", "stream_<LockinPolarProc<2, 1, 0>>", stream(), sw={"IDSP_LOCKIN_NO_WAVES": "1"}),
    row("process", 2, 1, 4096, 16, "FM", W4, waves(4, 16, "FM_DMA", 16), sw={"IDSP_LOCKIN_WAVES": "4"}),
    row("process", 2, 1, 65536, 16, "FM", W6, waves(6, 8, "FM_DMA", 16), sw={"IDSP_LOCKIN_WAVES": "6"}),
    row("norm_sqr", 2, 1, 4096, 16, "LM", W6, waves(6, 16, "LM_REG", 16), sw={"IDSP_LOCKIN_WAVES": "6"}),
    row("process", 2, 1, 4096, 16, "FM", W6, waves(6, 16, "FM_DMA", 16), sw={"IDSP_LOCKIN_WAVES": "5"}),
    row("process", 2, 1, 4096, 36, "LM", "stream_<LockinSplitProc<2, 1>>", stream(1), sw={"IDSP_LOCKIN_NO_LM_TAIL": "1"}),
    row("process", 2, 2, 16384, 16, "FM", W6, waves(6, 16, "FM_DMA", 16), sw={"IDSP_LOCKIN_NO_STAGES": "1"}),
    row("process", 2, 2, 32768, 16, "FM", ST16, stages(2, 16), sw={"IDSP_LOCKIN_STAGE_GROUPS": "2"}),
    row("arg", 2, 2, 32768, 16, "FM", ST8, stages(1, 16), sw={"IDSP_LOCKIN_STAGE_GROUPS": "1"}),
    row("process", 2, 2, 16448, 16, "FM", W4, waves(4, 16, "FM_DMA", 16), sw={"IDSP_LOCKIN_STAGE_GROUPS": "2"}),   # not whole pairs of groups: the default rule
    row("process", 2, 2, 16384, 15, "FM", W6, waves(6, 16, "FM_DMA", 15), sw={"IDSP_LOCKIN_STAGE_GROUPS": "1"}),  # when the shape allows
    row("process", 2, 1, 4096, 16, "FM", W6, waves(6, 8, "FM_REG", 16), sw={"IDSP_LOCKIN_NO_DMA": "1"}),
    row("process", 2, 1, 4096, 16, "LM", W4, waves(4, 16, "LM_REG", 16), sw={"IDSP_LOCKIN_NO_DMA": "1"}),
    row("process", 2, 1, 4096, 16, "FM", W6, waves(6, 8, "FM_DMA", 16), sw={"IDSP_LOCKIN_B": "8"}),
    row("process", 2, 1, 65600, 16, "FM", W4, waves(4, 16, "FM_DMA", 16), sw={"IDSP_LOCKIN_B": "16"}),
    row("process", 2, 1, 4100, 16, "FM", W6, waves(6, 8, "FM_REG", 16), sw={"IDSP_LOCKIN_B": "16"}),  # the register form has 8-frame batches only
    row("process", 2, 1, 4096, 16, "LM", W4, waves(4, 16, "LM_DMA", 16), sw={"IDSP_LOCKIN_B": "8"}),   # LaneMajor 16 only
    row("process", 2, 1, 16384, 20, "LM", "stream_<LockinProc<2, 1>>", stream(0), sw={"IDSP_SPLIT_MAX_LANES": "8192"}),
    row("process", 2, 1, 8192, 20, "LM", "stream_<LockinSplitProc<2, 1>>", stream(1), sw={"IDSP_SPLIT_MAX_LANES": "8192"}),
    row("arg", 2, 1, 32768, 16, "FM", W4, waves(4, 8, "FM_DMA", 16), sw={"IDSP_SPLIT_MAX_LANES": "8192"}),
    row("accu_process", 2, 2, 16384, 16, "FM", "stream_<LockinAccuProc<2, 2>>", stream(0), sw={"IDSP_SPLIT_MAX_LANES": "8192"}),
    # IDSP_LOCKIN_NO_SKEW is among the stagger rows below
]

# ---- without a GPU only
P28 = 1 << 28
CASES += [
    # 2^28 lanes (dds.hip:43, lockin_generic.hip:40), both layouts
    row("process", 2, 1, P28 - 64, 16, "FM", W4, waves(4, 8, "FM_DMA", 16), gpu=False), row("process", 2, 1, P28, 16, "FM", "stream_<LockinProc<2, 1>>", stream(0), gpu=False),
    row("arg", 2, 1, P28 - 64, 16, "LM", W4, waves(4, 16, "LM_REG", 16), gpu=False), row("arg", 2, 1, P28, 16, "LM", "stream_<LockinPolarProc<2, 1, 0>>", stream(), gpu=False),
    row("norm_sqr", 2, 1, P28 - 64, 36, "LM", TAIL, waves(4, 16, "LM_DMA", 32), gpu=False), row("norm_sqr", 2, 1, P28, 36, "LM", "stream_<LockinPolarProc<2, 1, 1>>", stream(), gpu=False),
    row("biquad_process", 1, 0, P28 - 64, 16, "FM", W4 + "<[Biquad; 1]>", waves(4, 8, "FM_DMA", 16), gpu=False),
    row("biquad_process", 1, 0, P28, 16, "FM", "stream_<LockinBiquadProc<1>>", stream(), gpu=False),
    row("lo_process", 1, 1, P28 - 64, 36, "LM", "stream_<LockinLoProc<1, 1>>", waves(4, 16, "LM_DMA", 32), gpu=False),
    row("lo_process", 1, 1, P28, 36, "LM", "stream_<LockinLoProc<1, 1>>", stream(), gpu=False),
    # no frames: the lowpass phase entries call the stream path (dds.hip:42, :612)
    row("process", 2, 2, 4096, 0, "FM", "stream_<LockinSplitProc<2, 2>>", stream(1), gpu=False), row("arg", 2, 2, 4096, 0, "LM", "stream_<LockinPolarProc<2, 2, 0>>", stream(), gpu=False),
    row("process", 2, 2, 65536, 0, "FM", "stream_<LockinProc<2, 2>>", stream(0), gpu=False),
    # a switch without IDSP_DIAG=1 is not honoured (common.h `diag_env`)
    row("process", 2, 1, 4096, 16, "FM", W6, waves(6, 16, "FM_DMA", 16), sw={"IDSP_DIAG": "0", "IDSP_LOCKIN_NO_WAVES": "1"}, gpu=False),
    # the start-up stagger (lockin_waves.h:853): LaneMajor, 512 workgroups, 2048..8192 frames of the multi-wave kernel, a tuned device, no IDSP_LOCKIN_NO_SKEW
    row("process", 2, 1, 32768, 2048, "LM", W4, waves(4, 16, "LM_DMA", 2048, 600), gpu=False, tuned=True),
    row("process", 2, 1, 32768, 2048, "LM", W4, waves(4, 16, "LM_DMA", 2048, 0), gpu=False),
    row("process", 2, 1, 32768, 2048, "LM", W4, waves(4, 16, "LM_DMA", 2048, 0), gpu=False, tuned=True, sw={"IDSP_LOCKIN_NO_SKEW": "1"}),
    row("process", 2, 1, 32704, 2048, "LM", W4, waves(4, 16, "LM_DMA", 2048, 0), gpu=False, tuned=True),
    row("arg", 2, 1, 32705, 2048, "LM", W6, waves(6, 16, "LM_REG", 2048, 600), gpu=False, tuned=True),  # 512 workgroups, the last one a single lane
    row("process", 2, 1, 32768, 2032, "LM", W4, waves(4, 16, "LM_DMA", 2032, 0), gpu=False, tuned=True),
    row("process", 2, 1, 32768, 8192, "LM", W4, waves(4, 16, "LM_DMA", 8192, 600), gpu=False, tuned=True),
    row("process", 2, 1, 32768, 8208, "LM", W4, waves(4, 16, "LM_DMA", 8208, 0), gpu=False, tuned=True),
    row("process", 2, 1, 32768, 8196, "LM", TAIL, waves(4, 16, "LM_DMA", 8192, 600), gpu=False, tuned=True),  # the kernel's frames: the body's
    row("process", 2, 1, 32768, 2048, "FM", W4, waves(4, 16, "FM_DMA", 2048, 0), gpu=False, tuned=True),
    row("biquad_lo_process", 2, 0, 65536, 4096, "LM", W4 + "<[Biquad; 2], LO>", waves(4, 16, "LM_DMA", 4096, 600), gpu=False, tuned=True),
]


def cli_line(c):
    sw = dict(c.sw)
    if sw:
        sw.setdefault("IDSP_DIAG", "1")
    return "lockin %s %d %d %d %d %s %d %d%s %s" % (c.entry, c.a, c.b, c.lanes, c.frames, c.layout, c.off[0], c.off[1], " tuned" if c.tuned else "",
                                                  " ".join("%s=%s" % kv for kv in sorted(sw.items())))
