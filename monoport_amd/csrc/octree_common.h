// What the octree housekeeping kernels of octree.hip and topk.hip share: the per-frame buffer descriptors that travel
// to the kernels by value, the bitset geometry (one 64-bit word per 64 consecutive x) and the bit spread that maps a
// coarse level's evaluated word onto the even positions of the next level's.
#pragma once
#include "mp_internal.h"

namespace mp {

typedef unsigned long long u64;

static inline size_t align256(size_t x) { return (x + 255) & ~size_t(255); }
static inline int words64(int r) { return (r + 63) / 64; }

// The housekeeping kernels of a level serve ALL frames of a batch in one launch (blockIdx.z = frame; round 5: per
// frame they were 40-odd launches of 3-25 us between two query launches, each too small to fill the chip): the
// per-frame pointers travel by value.
struct FrameBufs {
  const float *prev[kMaxFrames];   // previous level's volume
  float *cur[kMaxFrames];          // this level's volume
  u64 *bnd[kMaxFrames];            // boundary flags of this level
  const u64 *ev_prev[kMaxFrames];  // evaluated bits of the previous level
  u64 *ev[kMaxFrames];             // evaluated bits of this level
  uint32_t *packed[kMaxFrames];    // point list
  int32_t *count[kMaxFrames];      // its length (device side)
  int32_t *flag[kMaxFrames];       // level 0: "anything above the threshold" (status[0])
};
static_assert(sizeof(FrameBufs) <= 2048 + 64, "kernel argument");

__device__ __forceinline__ u64 spread32(u64 x) {  // bit i -> bit 2i
  x &= 0xffffffffull;
  x = (x | (x << 16)) & 0x0000ffff0000ffffull;
  x = (x | (x << 8)) & 0x00ff00ff00ff00ffull;
  x = (x | (x << 4)) & 0x0f0f0f0f0f0f0f0full;
  x = (x | (x << 2)) & 0x3333333333333333ull;
  x = (x | (x << 1)) & 0x5555555555555555ull;
  return x;
}

// point_order.hip: a level's point lists sorted in place by the texel cell each point samples (counting sort per frame,
// blockIdx.z = frame).  A frame's list is packed[f][0 .. *count[f]); calib[f] / proj[f] as in QueryItem; tmp[f]: `cap`
// entries, hist[f]: h * w + 1 words (point_order_carve lays both out in point_order_scratch_bytes(cap, h, w) bytes).
// A frame with more than `cap` points keeps its order.  `lattice`: stride, res_final, half_step, bmin, blen of the level.
struct OrderFrames {
  uint32_t *packed[kMaxFrames];
  const int32_t *count[kMaxFrames];
  const float *calib[kMaxFrames];
  uint32_t *tmp[kMaxFrames];
  int32_t *hist[kMaxFrames];
  int proj[kMaxFrames];
};
size_t point_order_scratch_bytes(long long cap, int h, int w);
void point_order_carve(void *scratch, long long cap, OrderFrames &of, int f);
int launch_point_order(mp_ctx *ctx, const OrderFrames &of, int n_frames, const PointSrc &lattice, int h, int w,
                       long long cap, hipStream_t st);

// topk.hip: the fixed-budget selection of one level for n_frames frames (blockIdx.z = frame).  fb.cur holds the
// upsampled volume, fb.count is zeroed; fb.flag[f] (NULL = frame on) gates frame f on the device.  `scratch`:
// topk_scratch_bytes(n_frames, r) bytes.
int launch_topk_select(mp_ctx *ctx, void *scratch, const FrameBufs &fb, int n_frames, int rp, int r, long long k,
                       float max_dist, float balance, hipStream_t st);

}  // namespace mp
