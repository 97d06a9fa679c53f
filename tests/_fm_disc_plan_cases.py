"""Which kernel a call of idsp_fm_disc_i32 and of idsp_dds_i32 takes, and with which launch parameters: one table, shared by
tests/test_fm_disc_plan.py (no GPU: `plan_fm_disc` / `plan_dds` of idsp_amd/csrc/readout_plan.h through build/stream_plan_cli) and
tests/test_gpu_fm_disc_plan.py (the real entries, through `idsp_last_kernel()`, values against the oracle).

Every expectation was written by hand from the two entries as they stood in dds.hip before the choice moved into readout_plan.h (the
parent of the commit that added this file; the line numbers below are that file's): `idsp_fm_disc_i32` at dds.hip:607-663 and
`idsp_dds_i32` at :560-581.  None was produced by running the new functions.

FM discriminator row: lanes, frames, layout, byte offsets of (x, y) from a 16-byte boundary, whether stagger_tuned_device() holds,
switches (honoured with IDSP_DIAG=1 only), the start of what idsp_last_kernel() reports, the launch parameters, and whether the row also
runs on the GPU.  `grid` is the role kernels' (64 lanes per workgroup); `body` / `tail` are the frames of every LaneMajor row on the role
kernel / on the tile kernel behind it; `skew` / `shift` / `mod` are the LaneMajor role kernel's stagger arguments (held here only: they
are no part of a name).  The stream form has none of these: `stream_` is where every name of the stream launcher begins.
DDS row: lanes, frames, layout, switches, the stream processor (the end of the recorded name), `split= circle=`, gpu.
Not on the GPU: 2^28 lanes, a device that is not the tuned one, and a switch without IDSP_DIAG (the library reads the environment once
per process).  Imports neither torch nor the library."""
import collections

FmDisc = collections.namedtuple("FmDisc", "lanes frames layout off tuned sw name params gpu")
Dds = collections.namedtuple("Dds", "lanes frames layout sw proc params gpu")

DIAG = {"IDSP_DIAG": "1"}
FM_NAMES = {"Stream": "stream_", "WavesFm3": "fm_disc_waves_kernel<3>", "WavesFm4": "fm_disc_waves_kernel<4>", "WavesLm": "fm_disc_waves_lm_kernel",
            "WavesLmTail": "fm_disc_waves_lm_kernel + stream_lane_major (last frames % 32)"}
FM_DISC_SWITCHES = {"IDSP_FM_DISC_WAVES", "IDSP_FM_DISC_LM_WAVES", "IDSP_FMD_SKEW", "IDSP_FMD_SKEW_SHIFT", "IDSP_FMD_SKEW_MOD"}
DDS_SWITCHES = {"IDSP_DDS_NO_CIRCLE", "IDSP_SPLIT_MAX_LANES"}


def fm(lanes, frames, layout, form, waves=0, body=0, tail=0, skew=0, shift=None, mod=None, off=(0, 0), tuned=False, sw=None, gpu=True):
    """a row; the role forms launch ceil(lanes / 64) workgroups (dds.hip:624,652), the LaneMajor one with shift 4 and mod 4 (:651)"""
    role = form != "Stream"
    lm_role = form in ("WavesLm", "WavesLmTail")
    shift = (4 if lm_role else 0) if shift is None else shift
    mod = (4 if lm_role else 1) if mod is None else mod
    params = "form=%s waves=%d grid=%d body=%d tail=%d skew=%d shift=%d mod=%d" % (form, waves, (lanes + 63) // 64 if role else 0, body, tail, skew, shift, mod)
    return FmDisc(lanes, frames, layout, off, tuned, dict(sw or {}), FM_NAMES[form + (str(waves) if form == "WavesFm" else "")], params, gpu)


FM_DISC_CASES = [
    # ---- FrameMajor (dds.hip:622-623): four front waves up to 81920 lanes, the stream kernel beyond ...
    fm(81920, 8, "FM", "WavesFm", waves=4), fm(81921, 8, "FM", "Stream"),
    # ... from 8 frames
    fm(200, 7, "FM", "Stream"), fm(200, 8, "FM", "WavesFm", waves=4), fm(64, 9, "FM", "WavesFm", waves=4), fm(1, 2064, "FM", "WavesFm", waves=4),
    # ... whatever the addresses (nothing of :622-635 reads them)
    fm(200, 8, "FM", "WavesFm", waves=4, off=(4, 0)), fm(200, 8, "FM", "WavesFm", waves=4, off=(0, 8)),
    # ---- LaneMajor (dds.hip:642-643): rows of 32 frames or more, a multiple of 16; whole 32-frame tiles are the body (:644), the last 16 the tail
    fm(130, 16, "LM", "Stream"), fm(70, 31, "LM", "Stream"), fm(64, 32, "LM", "WavesLm", body=32), fm(70, 33, "LM", "Stream"), fm(64, 40, "LM", "Stream"),
    fm(64, 48, "LM", "WavesLmTail", body=32, tail=16), fm(65, 64, "LM", "WavesLm", body=64), fm(200, 2064, "LM", "WavesLmTail", body=2048, tail=16),
    # ... both buffers on the 16-byte grid (:643)
    fm(65, 64, "LM", "Stream", off=(4, 0)), fm(65, 64, "LM", "Stream", off=(8, 0)), fm(65, 64, "LM", "Stream", off=(0, 4)), fm(65, 64, "LM", "Stream", off=(0, 8)),
    fm(64, 48, "LM", "Stream", off=(8, 8)),
    # ... fewer than 2^28 lanes (:642)
    fm((1 << 28) - 1, 32, "LM", "WavesLm", body=32, gpu=False), fm(1 << 28, 32, "LM", "Stream", gpu=False),
    # (FrameMajor has no such limit: 2^28 lanes are above 81920 anyway)
    fm(1 << 28, 32, "FM", "Stream", gpu=False),
    # ---- the start-up stagger (dds.hip:653): 1200 ticks from 512 workgroups, for calls of 2048 to 8192 frames, on the tuned device only.
    # The frames are the call's, not the body's: 8208 frames are a body of 8192 and no stagger.  2047 frames are no role-kernel row at all;
    # 2032 is the last one below the window.
    fm(511 * 64, 2048, "LM", "WavesLm", body=2048, tuned=True, gpu=False), fm(511 * 64 + 1, 2048, "LM", "WavesLm", body=2048, skew=1200, tuned=True, gpu=False),
    fm(512 * 64, 2048, "LM", "WavesLm", body=2048, skew=1200, tuned=True, gpu=False),
    fm(512 * 64, 2047, "LM", "Stream", tuned=True, gpu=False), fm(512 * 64, 2032, "LM", "WavesLmTail", body=2016, tail=16, tuned=True, gpu=False),
    fm(512 * 64, 8192, "LM", "WavesLm", body=8192, skew=1200, tuned=True, gpu=False),
    fm(512 * 64, 8208, "LM", "WavesLmTail", body=8192, tail=16, tuned=True, gpu=False),
    fm(512 * 64, 2064, "LM", "WavesLmTail", body=2048, tail=16, skew=1200, tuned=True, gpu=False),
    fm(512 * 64, 2048, "LM", "WavesLm", body=2048, gpu=False), fm(512 * 64, 8192, "LM", "WavesLm", body=8192, gpu=False),
    # (the FrameMajor kernel has no stagger argument)
    fm(512 * 64, 2048, "FM", "WavesFm", waves=4, tuned=True, gpu=False),
]

# ---- the five switches, with IDSP_DIAG=1 and without
for diag in (True, False):
    d = DIAG if diag else {}

    def sw(d=d, **kv):
        return dict(d, **kv)

    for n in ("0", "3", "4", "5"):
        # IDSP_FM_DISC_WAVES (dds.hip:621-625): 0 is the stream kernel, 3 three front waves, anything else four — beyond 81920 lanes too, but never
        # below 8 frames, and for FrameMajor only (the LaneMajor condition of :642 does not read it)
        forced = {"0": ("Stream", 0), "3": ("WavesFm", 3)}.get(n, ("WavesFm", 4)) if diag else ("WavesFm", 4)
        FM_DISC_CASES += [
            fm(200, 8, "FM", forced[0], waves=forced[1], sw=sw(IDSP_FM_DISC_WAVES=n), gpu=diag),
            fm(64, 2064, "FM", forced[0], waves=forced[1], sw=sw(IDSP_FM_DISC_WAVES=n), gpu=diag),
            fm(200, 7, "FM", "Stream", sw=sw(IDSP_FM_DISC_WAVES=n), gpu=diag),
            fm(65, 64, "LM", "WavesLm", body=64, sw=sw(IDSP_FM_DISC_WAVES=n), gpu=diag),
            fm(70, 33, "LM", "Stream", sw=sw(IDSP_FM_DISC_WAVES=n), gpu=diag),
        ]
        beyond = forced if diag and n != "0" else ("Stream", 0)
        FM_DISC_CASES.append(fm(81921, 8, "FM", beyond[0], waves=beyond[1], sw=sw(IDSP_FM_DISC_WAVES=n), gpu=diag and n == "4"))
    # IDSP_FM_DISC_LM_WAVES (dds.hip:637): off only when it parses to 0
    FM_DISC_CASES += [
        fm(65, 64, "LM", "Stream" if diag else "WavesLm", body=0 if diag else 64, sw=sw(IDSP_FM_DISC_LM_WAVES="0"), gpu=diag),
        fm(64, 48, "LM", "Stream" if diag else "WavesLmTail", body=0 if diag else 32, tail=0 if diag else 16, sw=sw(IDSP_FM_DISC_LM_WAVES="0"), gpu=diag),
        fm(200, 8, "FM", "WavesFm", waves=4, sw=sw(IDSP_FM_DISC_LM_WAVES="0"), gpu=diag),
        fm(65, 64, "LM", "WavesLm", body=64, sw=sw(IDSP_FM_DISC_LM_WAVES="1"), gpu=False),
    ]
    # IDSP_FMD_SKEW / _SHIFT / _MOD (dds.hip:650-655): the forced ticks whatever the shape and the device (0 switches the stagger off), the shift
    # masked with 31, a modulus of 0 made 1; defaults 4 and 4
    FM_DISC_CASES += [
        fm(130, 64, "LM", "WavesLm", body=64, skew=700 if diag else 0, shift=3 if diag else 4, mod=1 if diag else 4,
           sw=sw(IDSP_FMD_SKEW="700", IDSP_FMD_SKEW_SHIFT="35", IDSP_FMD_SKEW_MOD="0"), gpu=diag),
        fm(64, 48, "LM", "WavesLmTail", body=32, tail=16, skew=700 if diag else 0, shift=3 if diag else 4, mod=1 if diag else 4,
           sw=sw(IDSP_FMD_SKEW="700", IDSP_FMD_SKEW_SHIFT="35", IDSP_FMD_SKEW_MOD="0"), gpu=diag),
        fm(130, 64, "LM", "WavesLm", body=64, skew=700 if diag else 0, sw=sw(IDSP_FMD_SKEW="700"), gpu=False),
        fm(512 * 64, 2048, "LM", "WavesLm", body=2048, skew=0 if diag else 1200, tuned=True, sw=sw(IDSP_FMD_SKEW="0"), gpu=False),
        fm(512 * 64, 2048, "LM", "WavesLm", body=2048, skew=1200, shift=0 if diag else 4, tuned=True, sw=sw(IDSP_FMD_SKEW_SHIFT="0"), gpu=False),
        fm(512 * 64, 2048, "LM", "WavesLm", body=2048, skew=1200, shift=31 if diag else 4, tuned=True, sw=sw(IDSP_FMD_SKEW_SHIFT="31"), gpu=False),
        fm(512 * 64, 2048, "LM", "WavesLm", body=2048, skew=1200, mod=8 if diag else 4, tuned=True, sw=sw(IDSP_FMD_SKEW_MOD="8"), gpu=False),
        fm(512 * 64, 2048, "LM", "WavesLm", body=2048, skew=1200, mod=1 if diag else 4, tuned=True, sw=sw(IDSP_FMD_SKEW_MOD="0"), gpu=False),
        # ... read by the LaneMajor role kernel's launch only
        fm(200, 8, "FM", "WavesFm", waves=4, sw=sw(IDSP_FMD_SKEW="700"), gpu=False),
        fm(70, 33, "LM", "Stream", sw=sw(IDSP_FMD_SKEW="700"), gpu=False),
    ]


# ------------------------------------------------------------------------------------------------------------------------- DDS
def dds(lanes, frames, layout, split, circle, sw=None, gpu=True):
    """a row; the processor of the stream launch (dds.hip:567-580): two threads per lane with the full-circle table, with the 512-byte
    table, or one thread per lane (which never takes the full-circle table)"""
    proc = "DdsSplitProcT<true>" if circle else "DdsSplitProcT<false>" if split else "DdsProcT<false>"
    return Dds(lanes, frames, layout, dict(sw or {}), proc, "split=%d circle=%d" % (split, circle), gpu)


DDS_CASES = [
    # the full-circle table for FrameMajor calls of 256 frames or more (dds.hip:566) ...
    dds(5, 255, "FM", 1, 0), dds(5, 256, "FM", 1, 1), dds(5, 255, "LM", 1, 0), dds(5, 256, "LM", 1, 0), dds(67, 300, "FM", 1, 1), dds(67, 300, "LM", 1, 0),
    # ... on the two-threads-per-lane form, which ends at 40960 lanes (:567, :576-580)
    dds(40960, 256, "FM", 1, 1), dds(40961, 256, "FM", 0, 0), dds(40960, 256, "LM", 1, 0), dds(40961, 256, "LM", 0, 0),
    dds(40960, 255, "FM", 1, 0, gpu=False), dds(40961, 255, "FM", 0, 0, gpu=False),
    # (no frames: the entry returns for lanes == 0 only, and the stream launcher launches nothing)
    dds(5, 0, "FM", 1, 0, gpu=False),
]
for diag in (True, False):
    d = DIAG if diag else {}
    DDS_CASES += [
        # IDSP_DDS_NO_CIRCLE (dds.hip:565)
        dds(5, 256, "FM", 1, 0 if diag else 1, sw=dict(d, IDSP_DDS_NO_CIRCLE="1"), gpu=diag),
        dds(5, 256, "LM", 1, 0, sw=dict(d, IDSP_DDS_NO_CIRCLE="1"), gpu=diag),
        dds(40961, 256, "FM", 0, 0, sw=dict(d, IDSP_DDS_NO_CIRCLE="1"), gpu=False),
        # IDSP_SPLIT_MAX_LANES (:567, through the lock-in family's switches)
        dds(100, 256, "FM", 1, 1, sw=dict(d, IDSP_SPLIT_MAX_LANES="100"), gpu=diag),
        dds(101, 256, "FM", 0 if diag else 1, 0 if diag else 1, sw=dict(d, IDSP_SPLIT_MAX_LANES="100"), gpu=diag),
        dds(101, 256, "LM", 0 if diag else 1, 0, sw=dict(d, IDSP_SPLIT_MAX_LANES="100"), gpu=diag),
        dds(40961, 256, "FM", 1 if diag else 0, 1 if diag else 0, sw=dict(d, IDSP_SPLIT_MAX_LANES="50000"), gpu=False),
    ]


def _switches(sw):
    return " ".join("%s=%s" % kv for kv in sorted(sw.items()))


def fm_disc_line(c):
    return "fm_disc %d %d %s %d %d %s%s" % (c.lanes, c.frames, c.layout, c.off[0], c.off[1], "tuned " if c.tuned else "", _switches(c.sw))


def dds_line(c):
    return "dds %d %d %s %s" % (c.lanes, c.frames, c.layout, _switches(c.sw))
