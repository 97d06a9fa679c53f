"""Which kernel a call of idsp_hbf_{dec,int}_f32 and of idsp_cic_{dec,int}_{i32,i64} takes, and with which launch parameters: one table,
shared by tests/test_resample_plan.py (no GPU: `plan_hbf` / `plan_cic` of idsp_amd/csrc/resample_plan.h through build/stream_plan_cli) and
tests/test_gpu_resample_plan.py (the real entries, through `idsp_last_kernel()`, values against the oracle).

Every expectation was written by hand from the dispatch as it stood before the choice moved into resample_plan.h (the parent of the
commit that added this file): `launch_hbf` of hbf.hip and the conditions of `hbfb::launch_blk` (hbf_blk.h), `hbfr::launch_ring`
(hbf_ring.h) and `hbfw::launch_wave` (hbf_wave.h) behind its "0 = launched, 1 = not mine" protocol; `cic::run_orders` of cic_kernels.h,
`ring_pieces` of cic_ring_host.h and `dispatch` of cic_ring_{dec,int}.hip.  None was produced by running the new functions.

Half-band row: kind, tap set (-1: custom taps), stages, lanes, frames (low rate), layout, byte offset of the wide buffer (x of a
decimator, y of an interpolator) from a 16-byte boundary, switches (honoured with IDSP_DIAG=1 only), the start of what
idsp_last_kernel() reports, the launch parameters, and whether the row also runs on the GPU.  Cic row: kind, bits, order, rate (a chunk
is rate + 1 samples), lanes, frames, layout, (x, y) byte offsets, switches, name, parameters, gpu.  Not on the GPU: 2^31 lanes and a
switch without IDSP_DIAG (the library reads the environment once per process).  Imports neither torch nor the library."""
import collections

Hbf = collections.namedtuple("Hbf", "kind tap_set stages lanes frames layout off sw name params gpu")
Cic = collections.namedtuple("Cic", "kind bits order rate lanes frames layout off sw name params gpu")

DIAG = {"IDSP_DIAG": "1"}


def xcd(n):
    """grid of the kernels that deal contiguous runs of n lanes / lane groups to the 8 XCDs: a multiple of 8"""
    return 8 * ((n + 7) // 8)


# ------------------------------------------------------------------------------------------------------------------- half-band
GENERIC = {"dec": "hbf_dec_kernel (generic taps)", "int": "hbf_int_kernel (generic taps)"}
BLK, RING, INT_LM = "hbf_dec_blk[LaneMajor]", "hbf_dec_ring[FrameMajor]", "hbf_int_wave[LaneMajor]"


def hbf(kind, tap_set, stages, lanes, frames, layout, form, grid, off=0, sw=None, gpu=True):
    name = {"Generic": GENERIC[kind], "BlkLm": BLK, "RingFm": RING, "BlockFm": "hbf_%s_block_fm" % kind, "WaveFm": "hbf_%s_wave[FrameMajor]" % kind,
            "WaveLm": INT_LM}[form]
    return Hbf(kind, tap_set, stages, lanes, frames, layout, off, dict(sw or {}), name, "form=%s grid=%d" % (form, grid), gpu)


def rnd(stages):
    """low-rate frames of one round of 1024 high-rate samples; + 3: one full round and a ragged one (test_gpu_parity.py hbf_shapes)"""
    return 1024 >> stages


HBF_CASES = []
for ts in (0, 1):
    # LaneMajor decimators: the blocked kernel, a workgroup per lane, every cascade (hbf_blk.h:446-464) ...
    HBF_CASES += [hbf("dec", ts, s, 3, rnd(s) + 4, "LM", "BlkLm", 3) for s in (1, 2, 3, 4, 5)]
    # ... interpolators: the wave kernel, a workgroup per lane (hbf_wave.h:672-678)
    HBF_CASES += [hbf("int", ts, s, 29, rnd(s) + 4, "LM", "WaveLm", 29) for s in (1, 2, 3, 4, 5)]
    # FrameMajor /16 decimator: the ring on whole 16-lane groups (hbf_ring.h:583-584: 9 and 11 groups), else block_fm on whole 4-lane
    # groups (152 = 16 k + 8), else a wave per lane
    HBF_CASES += [hbf("dec", ts, 4, 144, 67, "FM", "RingFm", 16), hbf("dec", ts, 4, 176, 67, "FM", "RingFm", 16),
                  hbf("dec", ts, 4, 152, 67, "FM", "BlockFm", xcd(38)), hbf("dec", ts, 4, 150, 67, "FM", "WaveFm", xcd(150))]
    # ... the ring for 4 stages only (hbf_ring_dec.hip:9): 3 and 5 stages on 16 lanes; interpolators have none
    HBF_CASES += [hbf("dec", ts, 3, 16, 131, "FM", "BlockFm", 8), hbf("dec", ts, 5, 16, 35, "FM", "BlockFm", 8),
                  hbf("int", ts, 4, 144, 67, "FM", "BlockFm", xcd(36))]
    # block_fm on whole 4-lane groups (hbf_wave.h:684,698: 9 and 13 groups), 4 k + 2 lanes a wave per lane, for both kinds
    for kind in ("dec", "int"):
        HBF_CASES += [hbf(kind, ts, 2, 36, 259, "FM", "BlockFm", 16), hbf(kind, ts, 2, 52, 259, "FM", "BlockFm", 16),
                      hbf(kind, ts, 2, 38, 259, "FM", "WaveFm", 40), hbf(kind, ts, 5, 38, 35, "FM", "WaveFm", 40),
                      # one stage FrameMajor: a frame is 8 bytes (hbf.hip:581 `R >= 4`, hbf_wave.h:709): the generic kernel, 8 * ceil(lanes / 8) workgroups
                      hbf(kind, ts, 1, 20, 515, "FM", "Generic", 24)]

HBF_CASES += [
    # LaneMajor rows of whole 16-byte pieces, `frames * R % 4 == 0` (hbf.hip:581): one stage and an odd frame count is the only way to miss
    hbf("dec", 0, 1, 5, 515, "LM", "Generic", 5), hbf("dec", 0, 1, 5, 516, "LM", "BlkLm", 5),
    hbf("int", 1, 1, 5, 515, "LM", "Generic", 5), hbf("int", 1, 1, 5, 516, "LM", "WaveLm", 5),
    hbf("dec", 1, 2, 5, 259, "LM", "BlkLm", 5), hbf("int", 0, 2, 5, 259, "LM", "WaveLm", 5),
    # the wide buffer one element off the 16-byte grid (hbf.hip:581): generic, whatever else holds
    hbf("dec", 0, 4, 3, 67, "LM", "Generic", 3, off=4), hbf("int", 0, 4, 3, 67, "LM", "Generic", 3, off=4),
    hbf("dec", 0, 4, 144, 67, "FM", "Generic", 144, off=4), hbf("int", 1, 3, 36, 131, "FM", "Generic", 40, off=4),
    hbf("dec", 1, 2, 38, 259, "FM", "Generic", 40, off=8),
    # custom taps (hbf.hip:577 builtin_tap_set = -1)
    hbf("dec", -1, 3, 5, 131, "LM", "Generic", 5), hbf("dec", -1, 4, 16, 67, "FM", "Generic", 16),
    hbf("int", -1, 3, 5, 131, "LM", "Generic", 5), hbf("int", -1, 2, 36, 259, "FM", "Generic", 40),
    # the 31-bit grid: 2^31 - 1 lanes is the entry's own limit, and the blocked kernel's (hbf_blk.h:449); the interpolator's wave kernel has none
    hbf("dec", 0, 4, (1 << 31) - 1, 64, "LM", "BlkLm", (1 << 31) - 1, gpu=False), hbf("dec", 0, 4, 1 << 31, 64, "LM", "Generic", 1 << 31, gpu=False),
    hbf("int", 0, 4, (1 << 31) - 1, 64, "LM", "WaveLm", (1 << 31) - 1, gpu=False), hbf("int", 0, 4, 1 << 31, 64, "LM", "WaveLm", 1 << 31, gpu=False),
]

# ---- the four switches, with IDSP_DIAG=1 and without
for diag in (True, False):
    d = DIAG if diag else {}

    def sw(name, d=d):
        return dict(d, **{name: "1"})

    HBF_CASES += [
        # IDSP_HBF_GENERIC (hbf.hip:576-577): every built-in cascade on the generic kernels
        hbf("dec", 0, 4, 3, 67, "LM", "Generic" if diag else "BlkLm", 3, sw=sw("IDSP_HBF_GENERIC"), gpu=diag),
        hbf("dec", 0, 4, 144, 67, "FM", "Generic" if diag else "RingFm", 144 if diag else 16, sw=sw("IDSP_HBF_GENERIC"), gpu=diag),
        hbf("int", 1, 3, 5, 131, "LM", "Generic" if diag else "WaveLm", 5, sw=sw("IDSP_HBF_GENERIC"), gpu=diag),
        hbf("int", 1, 3, 36, 131, "FM", "Generic" if diag else "BlockFm", 40 if diag else 16, sw=sw("IDSP_HBF_GENERIC"), gpu=diag),
        # IDSP_HBF_NO_BLK (hbf.hip:585): a LaneMajor decimator then asks the ring (hbf_ring.h:582 `if (lm) return 1`) and the wave launcher
        # (hbf_wave.h:673-674 `return 1`), and ends on the GENERIC kernel; nothing else reads it
        hbf("dec", 0, 4, 3, 67, "LM", "Generic" if diag else "BlkLm", 3, sw=sw("IDSP_HBF_NO_BLK"), gpu=diag),
        hbf("dec", 1, 1, 5, 516, "LM", "Generic" if diag else "BlkLm", 5, sw=sw("IDSP_HBF_NO_BLK"), gpu=diag),
        hbf("dec", 0, 4, 144, 67, "FM", "RingFm", 16, sw=sw("IDSP_HBF_NO_BLK"), gpu=diag),
        hbf("int", 0, 4, 3, 67, "LM", "WaveLm", 3, sw=sw("IDSP_HBF_NO_BLK"), gpu=diag),
        # IDSP_HBF_NO_RING (hbf.hip:590): the /16 FrameMajor decimator on block_fm; the LaneMajor one stays on the blocked kernel
        hbf("dec", 0, 4, 144, 67, "FM", "BlockFm" if diag else "RingFm", xcd(36) if diag else 16, sw=sw("IDSP_HBF_NO_RING"), gpu=diag),
        hbf("dec", 1, 4, 3, 67, "LM", "BlkLm", 3, sw=sw("IDSP_HBF_NO_RING"), gpu=diag),
        # IDSP_HBF_NO_BLOCK_FM (hbf_wave.h:683,697): a wave per lane; the ring is ahead of it
        hbf("dec", 0, 3, 36, 131, "FM", "WaveFm" if diag else "BlockFm", 40 if diag else 16, sw=sw("IDSP_HBF_NO_BLOCK_FM"), gpu=diag),
        hbf("int", 1, 2, 36, 259, "FM", "WaveFm" if diag else "BlockFm", 40 if diag else 16, sw=sw("IDSP_HBF_NO_BLOCK_FM"), gpu=diag),
        hbf("dec", 0, 4, 144, 67, "FM", "RingFm", 16, sw=sw("IDSP_HBF_NO_BLOCK_FM"), gpu=diag),
    ]
    # no ring and no block kernel: the wave-per-lane decimator
    HBF_CASES.append(hbf("dec", 1, 4, 144, 67, "FM", "WaveFm" if diag else "RingFm", 144 if diag else 16,
                         sw=dict(d, IDSP_HBF_NO_RING="1", IDSP_HBF_NO_BLOCK_FM="1"), gpu=diag))


# ------------------------------------------------------------------------------------------------------------------------- Cic
def cic(kind, bits, order, rate, lanes, frames, layout, form, ppt=0, vpc=0, grid=None, off=(0, 0), sw=None, gpu=True):
    name = {"RingLm": "cic_%s_ring[LaneMajor]" % kind, "RingFm": "cic_int_ring[FrameMajor]"}.get(form, "cic_%s_kernel" % kind)
    if grid is None:
        grid = lanes if form == "RingLm" else xcd(lanes // 16) if form == "RingFm" else (lanes + 63) // 64
    return Cic(kind, bits, order, rate, lanes, frames, layout, off, dict(sw or {}), name, "form=%s ppt=%d vpc=%d grid=%d" % (form, ppt, vpc, grid), gpu)


def rate_for(bits, chunk_bytes):
    return chunk_bytes // (bits // 8) - 1


CIC_CASES = []
for bits in (32, 64):
    e = bits // 8  # one element, in bytes
    for kind in ("dec", "int"):
        hi, lo = ((e, 0), (0, e)) if kind == "dec" else ((0, e), (e, 0))  # (x, y) offsets that put the high-rate / the low-rate tensor off the grid
        CIC_CASES += [
            # LaneMajor, a chunk of 1, 2, 4, 8 whole pieces and 64 frames or more: a wave per lane (cic_ring_host.h:57-65), every order
            cic(kind, bits, 1, rate_for(bits, 16), 5, 64, "LM", "RingLm", ppt=1), cic(kind, bits, 2, rate_for(bits, 32), 3, 65, "LM", "RingLm", ppt=2),
            cic(kind, bits, 3, rate_for(bits, 64), 7, 127, "LM", "RingLm", ppt=4), cic(kind, bits, 4, rate_for(bits, 128), 2, 128, "LM", "RingLm", ppt=8),
            cic(kind, bits, 5, rate_for(bits, 64), 1, 449, "LM", "RingLm", ppt=4), cic(kind, bits, 6, rate_for(bits, 32), 9, 200, "LM", "RingLm", ppt=2),
            # 63 frames: a lane per thread, the chunk as one vector (cic_kernels.h:499-505); 5 lanes are no whole block
            cic(kind, bits, 1, rate_for(bits, 16), 5, 63, "LM", "Lane", vpc=1),
            # a chunk of 256 bytes: no ring (`fb > 128`), 16 vectors; 512 bytes: no vectors either (cic_kernels.h:504); 48 bytes: whole pieces
            # but no power of two — no ring, no vectors; 8 bytes: no whole piece
            cic(kind, bits, 2, rate_for(bits, 256), 64, 64, "LM", "LaneTiles", vpc=16), cic(kind, bits, 2, rate_for(bits, 256), 3, 64, "LM", "Lane", vpc=16),
            cic(kind, bits, 2, rate_for(bits, 512), 64, 64, "LM", "Lane"), cic(kind, bits, 3, rate_for(bits, 48), 64, 64, "LM", "Lane"),
            cic(kind, bits, 3, rate_for(bits, 8), 64, 64, "LM", "Lane"),
            # the LaneMajor tiles (cic_kernels.h:508-510): whole blocks of 64 lanes, at least one tile of 16 vectors = 16 / vpc frames
            cic(kind, bits, 3, rate_for(bits, 64), 64, 3, "LM", "Lane", vpc=4), cic(kind, bits, 3, rate_for(bits, 64), 64, 4, "LM", "LaneTiles", vpc=4),
            cic(kind, bits, 4, rate_for(bits, 16), 128, 15, "LM", "Lane", vpc=1), cic(kind, bits, 4, rate_for(bits, 16), 128, 16, "LM", "LaneTiles", vpc=1),
            cic(kind, bits, 2, rate_for(bits, 32), 128, 37, "LM", "LaneTiles", vpc=2), cic(kind, bits, 2, rate_for(bits, 32), 129, 37, "LM", "Lane", vpc=2),
            cic(kind, bits, 5, rate_for(bits, 128), 192, 19, "LM", "LaneTiles", vpc=8), cic(kind, bits, 5, rate_for(bits, 128), 1024, 2, "LM", "LaneTiles", vpc=8),
            # ... and BOTH tensors on the 16-byte grid: the low-rate one off it keeps the vectors, the high-rate one off it loses them too
            cic(kind, bits, 3, rate_for(bits, 64), 64, 8, "LM", "LaneTiles", vpc=4), cic(kind, bits, 3, rate_for(bits, 64), 64, 8, "LM", "Lane", vpc=4, off=lo), cic(kind, bits, 3, rate_for(bits, 64), 64, 8, "LM", "Lane", off=hi),
            # the ring reads the high-rate tensor's address only (cic_ring_host.h:60)
            cic(kind, bits, 3, rate_for(bits, 64), 7, 127, "LM", "RingLm", ppt=4, off=lo), cic(kind, bits, 3, rate_for(bits, 64), 7, 127, "LM", "Lane", off=hi),
            # the 31-bit grid (cic_ring_host.h:61): 2^31 lanes are whole blocks, on the tiles
            cic(kind, bits, 1, rate_for(bits, 16), (1 << 31) - 1, 64, "LM", "RingLm", ppt=1, gpu=False),
            cic(kind, bits, 1, rate_for(bits, 16), 1 << 31, 64, "LM", "LaneTiles", vpc=1, gpu=False),
        ]
    # FrameMajor: the interpolator's ring on whole groups of 16 lanes (cic_ring_int.hip:64), the decimator has none (cic_kernels.h:490)
    CIC_CASES += [
        cic("int", bits, 1, rate_for(bits, 16), 16, 64, "FM", "RingFm", ppt=1), cic("int", bits, 2, rate_for(bits, 32), 48, 65, "FM", "RingFm", ppt=2),
        cic("int", bits, 6, rate_for(bits, 128), 16, 199, "FM", "RingFm", ppt=8), cic("int", bits, 3, rate_for(bits, 64), 160, 256, "FM", "RingFm", ppt=4),
        cic("int", bits, 3, rate_for(bits, 64), 144, 100, "FM", "RingFm", ppt=4), cic("int", bits, 3, rate_for(bits, 64), 152, 100, "FM", "Lane", vpc=4),
        cic("int", bits, 3, rate_for(bits, 64), 32, 63, "FM", "Lane", vpc=4), cic("int", bits, 3, rate_for(bits, 256), 32, 64, "FM", "Lane", vpc=16),
        cic("int", bits, 3, rate_for(bits, 48), 32, 64, "FM", "Lane"),
        cic("int", bits, 3, rate_for(bits, 64), 32, 64, "FM", "RingFm", ppt=4, off=(e, 0)), cic("int", bits, 3, rate_for(bits, 64), 32, 64, "FM", "Lane", off=(0, e)),
        cic("int", bits, 1, rate_for(bits, 16), (1 << 31) - 16, 64, "FM", "RingFm", ppt=1, gpu=False), cic("int", bits, 1, rate_for(bits, 16), 1 << 31, 64, "FM", "Lane", vpc=1, gpu=False),
        cic("dec", bits, 3, rate_for(bits, 64), 32, 64, "FM", "Lane", vpc=4), cic("dec", bits, 4, rate_for(bits, 16), 65, 70, "FM", "Lane", vpc=1),
        cic("dec", bits, 2, rate_for(bits, 48), 300, 40, "FM", "Lane"), cic("dec", bits, 3, rate_for(bits, 64), 32, 64, "FM", "Lane", off=(e, 0)),
        cic("dec", bits, 3, rate_for(bits, 64), 32, 64, "FM", "Lane", vpc=4, off=(0, e)),
    ]

# a chunk that is no whole number of elements' worth of pieces at all: rate 11 at i32 is 48 bytes (above), rate 2 is 12
CIC_CASES += [cic("dec", 32, 5, 2, 257, 5, "LM", "Lane"), cic("int", 32, 5, 2, 257, 5, "FM", "Lane")]

# ---- the two switches, with IDSP_DIAG=1 and without
for diag in (True, False):
    d = DIAG if diag else {}
    ring, tiles, both = dict(d, IDSP_CIC_NO_RING="1"), dict(d, IDSP_CIC_NO_LM_TILES="1"), dict(d, IDSP_CIC_NO_RING="1", IDSP_CIC_NO_LM_TILES="1")
    for kind in ("dec", "int"):
        CIC_CASES += [
            # IDSP_CIC_NO_RING (cic_ring_host.h:33-37,60): what the lane-per-thread kernels make of the same call
            cic(kind, 32, 3, 15, 64, 64, "LM", "LaneTiles" if diag else "RingLm", ppt=0 if diag else 4, vpc=4 if diag else 0, sw=ring, gpu=diag),
            cic(kind, 64, 2, 3, 7, 127, "LM", "Lane" if diag else "RingLm", ppt=0 if diag else 2, vpc=2 if diag else 0, sw=ring, gpu=diag),
            # IDSP_CIC_NO_LM_TILES (cic_kernels.h:447-451,510)
            cic(kind, 32, 3, 15, 64, 4, "LM", "Lane" if diag else "LaneTiles", vpc=4, sw=tiles, gpu=diag),
            cic(kind, 64, 2, 3, 7, 127, "LM", "RingLm", ppt=2, sw=tiles, gpu=diag),
            cic(kind, 32, 3, 15, 64, 64, "LM", "Lane" if diag else "RingLm", ppt=0 if diag else 4, vpc=4 if diag else 0, sw=both, gpu=diag),
        ]
    CIC_CASES += [cic("int", 32, 3, 15, 32, 64, "FM", "Lane" if diag else "RingFm", ppt=0 if diag else 4, vpc=4 if diag else 0, sw=ring, gpu=diag)]


def hbf_line(c):
    return "hbf %s %d %d %d %d %s %d %s" % (c.kind, c.tap_set, c.stages, c.lanes, c.frames, c.layout, c.off, " ".join("%s=%s" % kv for kv in sorted(c.sw.items())))


def cic_line(c):
    return "cic %s %d %d %d %d %d %s %d %d %s" % (c.kind, c.bits, c.order, c.rate, c.lanes, c.frames, c.layout, c.off[0], c.off[1],
                                                 " ".join("%s=%s" % kv for kv in sorted(c.sw.items())))
