// pfb.h — geometry of the polyphase channelizer kernels (pfb.hip), shared with whoever places shapes around their tiles.
#pragma once

#include "common.h"

namespace idsp {

// FRAME_MAJOR: one thread per lane, one wave per (64-lane group, time segment).  A segment re-reads the `taps - 1` frames in front
// of it from x (the first one takes them from state), so the re-read share is (taps - 1) / kPfbFmSegFrames: 2.7 % at taps = 8.
constexpr int kPfbFmSegFrames = 256;
#define IDSP_PFB_FM_SEG_STR "256"
// LANE_MAJOR: one 256-thread workgroup per (lane, time tile), one output frame per thread and tile; a tile re-reads the `taps`
// frames in front of it the same way.
constexpr int kPfbLmTileFrames = 256;
#define IDSP_PFB_LM_TILE_STR "256"

static_assert(kPfbFmSegFrames >= IDSP_PFB_MAX_TAPS && kPfbLmTileFrames >= IDSP_PFB_MAX_TAPS,
              "a segment's halo must lie inside the segment in front of it, and the tail of a split call inside x");

}  // namespace idsp
