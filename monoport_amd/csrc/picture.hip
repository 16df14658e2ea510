// The piece between a rendered G-buffer and a per-pixel netC query (mp_picture_points / mp_picture_paint,
// include/monoport_hip.h): the covered pixels of a frame's pictures become a counted point list in ascending pixel
// order, and the predictions go back into the picture.
//
// The list is defined bit for bit, so its order may not depend on which thread arrives first: no atomic cursor.
//   picture_count   one thread per pixel: covered = face_id >= 0; the block's number of covered pixels -> blk[block]
//   picture_scan    one workgroup per frame: in-place exclusive scan of blk; count = {min(K, capacity), K}
//   picture_emit    one thread per pixel: k = blk[block] + the block scan of the flags; pixel k of the list
//   picture_paint   one thread per list entry: the scatter, mp_paint's expression
// All four are streaming integer / copy kernels: 4 B of face id read twice and 12 B of position read once per pixel,
// 16 B per covered pixel written.  Positions travel as their 32-bit patterns.
//
// blockIdx.y is the frame; the per-frame pointers travel by value (PictureFrames).  blk comes from the stream's
// scratch arena and is written whole by picture_count before anything reads it: no memset, whatever the arena held.
#include "mesh_common.h"

#include <cstring>

#pragma clang fp contract(off)

namespace mp {

constexpr int kPicBlock = kScanBlock;  // block_exclusive_scan (mesh_common.h)
constexpr int kPaintBlock = 256;
constexpr int kPaintBlocks = 1024;  // workgroups of picture_paint per frame; they stride over the list

struct PictureFrames {
  const int32_t *face[kMaxFrames];
  const uint32_t *position[kMaxFrames];  // [L,3]
  uint32_t *points[kMaxFrames];          // [3,capacity]
  int32_t *pixels[kMaxFrames];
  int32_t *count[kMaxFrames];
};
struct PicturePaintFrames {
  const float *values[kMaxFrames];  // [3,capacity]
  const int32_t *pixels[kMaxFrames];
  const int32_t *count[kMaxFrames];
  float *image[kMaxFrames];  // [L,3]
};
static_assert(sizeof(PictureFrames) + 256 <= 4096 && sizeof(PicturePaintFrames) + 256 <= 4096, "picture: kernel arguments");

__global__ __launch_bounds__(kPicBlock) void picture_count(PictureFrames fr, int n_pixels, int *__restrict__ blk,
                                                           int n_blocks) {
  const int32_t *__restrict__ face = fr.face[blockIdx.y];
  const long long p = (long long)blockIdx.x * kPicBlock + threadIdx.x;
  int n = (p < n_pixels && face[p] >= 0) ? 1 : 0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) n += __shfl_down(n, o);
  __shared__ int wsum[kPicBlock / 64];
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = n;
  __syncthreads();
  if (threadIdx.x == 0) {
    int tot = 0;
#pragma unroll
    for (int k = 0; k < kPicBlock / 64; ++k) tot += wsum[k];
    blk[(long long)blockIdx.y * n_blocks + blockIdx.x] = tot;
  }
}

__global__ __launch_bounds__(kPicBlock) void picture_scan(PictureFrames fr, int *__restrict__ blk_all, int n_blocks,
                                                          long long capacity) {
  int *__restrict__ blk = blk_all + (long long)blockIdx.x * n_blocks;
  __shared__ int carry;
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  for (int b0 = 0; b0 < n_blocks; b0 += kPicBlock) {
    const int b = b0 + threadIdx.x;
    int tot;
    const int ex = block_exclusive_scan(b < n_blocks ? blk[b] : 0, &tot);
    if (b < n_blocks) blk[b] = carry + ex;
    __syncthreads();
    if (threadIdx.x == 0) carry += tot;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    int32_t *__restrict__ count = fr.count[blockIdx.x];
    count[0] = mesh_min(carry, capacity);
    count[1] = carry;
  }
}

__global__ __launch_bounds__(kPicBlock) void picture_emit(PictureFrames fr, int n_pixels, const int *__restrict__ blk,
                                                          int n_blocks, long long capacity) {
  const int32_t *__restrict__ face = fr.face[blockIdx.y];
  const int base = blk[(long long)blockIdx.y * n_blocks + blockIdx.x];
  if (base >= capacity) return;  // the whole block lies beyond the list (uniform: before the block scan's barriers)
  const long long p = (long long)blockIdx.x * kPicBlock + threadIdx.x;
  const int covered = (p < n_pixels && face[p] >= 0) ? 1 : 0;
  int tot;
  const long long k = (long long)base + block_exclusive_scan(covered, &tot);
  if (!covered || k >= capacity) return;
  const uint32_t *__restrict__ pos = fr.position[blockIdx.y];
  uint32_t *__restrict__ points = fr.points[blockIdx.y];
  fr.pixels[blockIdx.y][k] = (int32_t)p;
#pragma unroll
  for (int c = 0; c < 3; ++c) points[c * capacity + k] = pos[3 * p + c];
}

__global__ __launch_bounds__(kPaintBlock) void picture_paint(PicturePaintFrames fr, long long capacity, int n_pixels,
                                                             float scale, float bias, float lo, float hi) {
  const float *__restrict__ values = fr.values[blockIdx.y];
  const int32_t *__restrict__ pixels = fr.pixels[blockIdx.y];
  float *__restrict__ image = fr.image[blockIdx.y];
  const long long n = mesh_min(fr.count[blockIdx.y][0], capacity);
  for (long long k = (long long)blockIdx.x * kPaintBlock + threadIdx.x; k < n; k += (long long)gridDim.x * kPaintBlock) {
    const int p = pixels[k];
    if (p < 0 || p >= n_pixels) continue;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float o = values[c * capacity + k] * scale + bias;  // two operations: the file is built without contraction
      o = o < lo ? lo : (o > hi ? hi : o);
      image[3 * (long long)p + c] = o;
    }
  }
}

static long long picture_blocks(long long n_pixels) { return (n_pixels + kPicBlock - 1) / kPicBlock; }

// per frame: one int per 1024 pixels (the block sums, then their prefixes)
size_t picture_points_scratch_bytes(int n_frames, long long n_pixels) {
  return (size_t)n_frames * (size_t)picture_blocks(n_pixels) * sizeof(int) + 256;
}

int launch_picture_points_batch(mp_ctx *ctx, void *scratch, int n_frames, const int32_t *const *face_id,
                                const float *const *position, long long n_pixels, long long capacity,
                                float *const *points, int32_t *const *pixels, int32_t *const *count, hipStream_t st) {
  PictureFrames fr;
  std::memset(&fr, 0, sizeof(fr));
  for (int f = 0; f < n_frames; ++f) {
    fr.face[f] = face_id[f];
    fr.position[f] = reinterpret_cast<const uint32_t *>(position[f]);
    fr.points[f] = reinterpret_cast<uint32_t *>(points[f]);
    fr.pixels[f] = pixels[f];
    fr.count[f] = count[f];
  }
  const int nb = (int)picture_blocks(n_pixels);  // n_pixels <= 2^31 / 3: at most 699051 blocks
  int *blk = static_cast<int *>(scratch);
  const dim3 grid((unsigned)nb, n_frames);
  hipLaunchKernelGGL(picture_count, grid, dim3(kPicBlock), 0, st, fr, (int)n_pixels, blk, nb);
  hipLaunchKernelGGL(picture_scan, dim3(n_frames), dim3(kPicBlock), 0, st, fr, blk, nb, capacity);
  hipLaunchKernelGGL(picture_emit, grid, dim3(kPicBlock), 0, st, fr, (int)n_pixels, blk, nb, capacity);
  MP_HIP(ctx, hipGetLastError());
  return MP_OK;
}

int launch_picture_paint_batch(mp_ctx *ctx, int n_frames, const float *const *values, const int32_t *const *pixels,
                               const int32_t *const *count, long long capacity, long long n_pixels, float scale,
                               float bias, float lo, float hi, float *const *image, hipStream_t st) {
  PicturePaintFrames fr;
  std::memset(&fr, 0, sizeof(fr));
  for (int f = 0; f < n_frames; ++f) {
    fr.values[f] = values[f];
    fr.pixels[f] = pixels[f];
    fr.count[f] = count[f];
    fr.image[f] = image[f];
  }
  // a list of mp_picture_points is never longer than the pixels; the workgroups stride over a longer one
  const long long most = capacity < n_pixels ? capacity : n_pixels;
  long long blocks = (most + kPaintBlock - 1) / kPaintBlock;
  if (blocks > kPaintBlocks) blocks = kPaintBlocks;
  hipLaunchKernelGGL(picture_paint, dim3((unsigned)blocks, n_frames), dim3(kPaintBlock), 0, st, fr, capacity,
                     (int)n_pixels, scale, bias, lo, hi);
  MP_HIP(ctx, hipGetLastError());
  return MP_OK;
}

}  // namespace mp
