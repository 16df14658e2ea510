// Self-occluded SH lighting: precomputed radiance transfer traced in the occupancy volume (mp_volume_bits,
// mp_mesh_transfer, mp_mesh_transfer_shade; include/monoport_hip.h).
//   volume_bits_fine    one wavefront per 64 voxels of a row: v > level, a ballot, two words
//   volume_bits_blocks  one thread per 8^3 block: the OR of its 64 row bytes, a ballot, two words
//   mesh_transfer       one thread per vertex, the directions in ascending order: a ray per direction that faces away
//                       from the surface, marched sample by sample through the bits; the 64-bit visibility words and
//                       the nine coefficients, summed in the one order the header writes
//   transfer_shade      one thread per vertex: the nine coefficients times the lighting's [9][3]
// Lanes are consecutive vertices under ONE direction: marching cubes emits neighbours next to each other, so a
// wavefront's rays start close, run parallel, read the same few words of bits and leave the box after a similar number
// of samples; direction, step and basis row are wave-uniform (scalar loads), each lane keeps its own mask word and
// its nine sums in registers, and no cross-lane step, atomic or scratch is needed.  (Lanes = the directions of one
// vertex would give the mask by a ballot, but 64 rays that fan out gather 64 different words per sample and the
// ordered float sum would need a serial pass over the lanes.)
// Empty space: a workgroup holds the frame's block bits in LDS.  A sample in an empty block looks ahead: m more
// samples are skipped only after sample j + m itself was computed BY THE DEFINITION's expression and found inside the
// volume and in the same block.  o + fl(j * delta) is monotone in j on every axis, so the samples between lie in that
// block too: the skip is exact whatever the estimate of m was.
// Every float operation of the definition is one IEEE f32 +, -, *, / , sqrtf or floorf in the order the header writes
// (-ffp-contract=off); the look-ahead's estimate is free to be anything.  No float atomics, no scratch.
#include "mp_internal.h"

#include <cstring>

namespace mp {

constexpr int kBitsBlock = 256;
constexpr int kTransferBlock = 64;  // one wavefront: many small workgroups spread one mesh over the CUs

static inline int bits_wx(int r) { return (r + 31) >> 5; }
static inline int bits_nb(int r) { return (r + 7) >> 3; }
static inline long long bits_fine_words(int r) { return (long long)r * r * bits_wx(r); }
static inline int bits_block_words(int r) {
  const long long nb = bits_nb(r);
  return (int)((nb * nb * nb + 31) >> 5);
}
long long volume_bits_words(int r) { return bits_fine_words(r) + bits_block_words(r); }

struct BitsFrames {
  const float *vol[kMaxFrames];
  uint32_t *bits[kMaxFrames];
  const int32_t *gate[kMaxFrames];  // NULL = frame on; else the frame is served only if *gate != 0
};

__device__ __forceinline__ bool bits_gated_off(const BitsFrames &fr, int f) {
  const int32_t *gate = fr.gate[f];
  return gate != nullptr && *gate == 0;
}

// item = (row, chunk of 64 voxels); kBitsBlock / 64 items per workgroup.  A NaN is not > level; x >= r: 0
__global__ __launch_bounds__(kBitsBlock) void volume_bits_fine(BitsFrames fr, int r, int wx, int chunks,
                                                                long long n_items, float level) {
  const int f = blockIdx.y;
  if (bits_gated_off(fr, f)) return;
  const long long item = (long long)blockIdx.x * (kBitsBlock / 64) + (threadIdx.x >> 6);
  if (item >= n_items) return;  // wave-uniform
  const int lane = threadIdx.x & 63;
  const long long row = item / chunks;
  const int chunk = (int)(item - row * chunks);
  const int x = chunk * 64 + lane;
  bool set = false;
  if (x < r) set = fr.vol[f][row * r + x] > level;
  const unsigned long long m = __ballot(set);
  if (lane == 0) {
    uint32_t *w = fr.bits[f] + row * wx + chunk * 2;
    w[0] = (uint32_t)m;
    if (chunk * 2 + 1 < wx) w[1] = (uint32_t)(m >> 32);
  }
}

// block bi = (bz * nb + by) * nb + bx at bit bi & 31 of word fine_words + (bi >> 5); the grid covers whole wavefronts
__global__ __launch_bounds__(kBitsBlock) void volume_bits_blocks(BitsFrames fr, int r, int wx, int nb,
                                                                  long long fine_words, int block_words) {
  const int f = blockIdx.y;
  if (bits_gated_off(fr, f)) return;
  const int bi = blockIdx.x * kBitsBlock + threadIdx.x;
  const uint8_t *fine = reinterpret_cast<const uint8_t *>(fr.bits[f]);
  uint32_t any = 0;
  if (bi < nb * nb * nb) {
    const int bx = bi % nb, by = (bi / nb) % nb, bz = bi / (nb * nb);
    const int z1 = min(8 * bz + 8, r), y1 = min(8 * by + 8, r);
    for (int z = 8 * bz; z < z1; ++z)
      for (int y = 8 * by; y < y1; ++y) any |= fine[((long long)z * r + y) * wx * 4 + bx];
  }
  const unsigned long long m = __ballot(any != 0);
  if ((threadIdx.x & 63) == 0) {
    const int w0 = bi >> 5;
    uint32_t *w = fr.bits[f] + fine_words;
    if (w0 < block_words) w[w0] = (uint32_t)m;
    if (w0 + 1 < block_words) w[w0 + 1] = (uint32_t)(m >> 32);
  }
}

int launch_volume_bits_batch(mp_ctx *ctx, int n_frames, const float *const *vol, int r, float level,
                             uint32_t *const *bits, const int32_t *const *gate, hipStream_t st) {
  BitsFrames fr;
  std::memset(&fr, 0, sizeof(fr));
  for (int f = 0; f < n_frames; ++f) {
    fr.vol[f] = vol[f];
    fr.bits[f] = bits[f];
    fr.gate[f] = gate ? gate[f] : nullptr;
  }
  const int wx = bits_wx(r), nb = bits_nb(r), chunks = (r + 63) >> 6;
  const long long n_items = (long long)r * r * chunks;
  const int per = kBitsBlock / 64;
  hipLaunchKernelGGL(volume_bits_fine, dim3((unsigned)((n_items + per - 1) / per), n_frames), dim3(kBitsBlock), 0, st,
                     fr, r, wx, chunks, n_items, level);
  MP_HIP(ctx, hipGetLastError());
  hipLaunchKernelGGL(volume_bits_blocks, dim3((unsigned)((nb * nb * nb + kBitsBlock - 1) / kBitsBlock), n_frames),
                     dim3(kBitsBlock), 0, st, fr, r, wx, nb, bits_fine_words(r), bits_block_words(r));
  MP_HIP(ctx, hipGetLastError());
  return MP_OK;
}

struct TransferFrames {
  const float *verts[kMaxFrames], *normals[kMaxFrames];
  const int32_t *counts[kMaxFrames];
  const uint32_t *bits[kMaxFrames];
  unsigned long long *mask[kMaxFrames];  // nullptr: not wanted
  float *prt[kMaxFrames];                // nullptr: not wanted
};
struct TransferParams {
  float bmin[3], len[3], vox[3];  // len = bmax - bmin, vox = R / len (f32, on the host: the same IEEE operations)
  float rf, weight, bias_w, step_w;
  int r, wx, nb, block_words, n_dirs, max_steps;
  long long fine_words, max_v;
  const float *dirs, *basis;
};
static_assert(sizeof(TransferFrames) + sizeof(TransferParams) + 256 <= 4096, "mesh_transfer: kernel arguments");

// the vertex count a frame's kernels serve: counts[0] clamped to 0..max_v
__device__ __forceinline__ long long transfer_count(const int32_t *counts, long long max_v) {
  const long long n = counts[0];
  return n < 0 ? 0 : (n > max_v ? max_v : n);
}

__global__ __launch_bounds__(kTransferBlock) void mesh_transfer(TransferFrames fr, TransferParams pa) {
  extern __shared__ uint32_t block_bits[];
  const int f = blockIdx.y;
  const long long count = transfer_count(fr.counts[f], pa.max_v);
  if ((long long)blockIdx.x * kTransferBlock >= count) return;  // workgroup-uniform
  const uint32_t *__restrict__ bits = fr.bits[f];
  for (int i = threadIdx.x; i < pa.block_words; i += kTransferBlock) block_bits[i] = bits[pa.fine_words + i];
  __syncthreads();
  const long long v = (long long)blockIdx.x * kTransferBlock + threadIdx.x;
  if (v >= count) return;
  const float *__restrict__ vp = fr.verts[f] + 3 * v;
  const float *__restrict__ np = fr.normals[f] + 3 * v;
  float u[3], o[3];
  light_normalise(np[0], np[1], np[2], u[0], u[1], u[2]);
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float g = ((vp[a] - pa.bmin[a]) / pa.len[a]) * pa.rf;
    o[a] = g + (pa.bias_w * u[a]) * pa.vox[a];
  }
  unsigned long long *mask = fr.mask[f];
  float *prt = fr.prt[f];
  const int words = pa.n_dirs >> 6;
  const int r = pa.r, wx = pa.wx, nb = pa.nb, last = pa.max_steps - 1;
  const float rf = pa.rf;
  float acc[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) acc[k] = 0.0f;
  unsigned long long word = 0;
  for (int d = 0; d < pa.n_dirs; ++d) {
    const float *__restrict__ w = pa.dirs + 3 * d;
    const float kd = (w[0] * u[0] + w[1] * u[1]) + w[2] * u[2];
    if (kd > 0.0f) {
      float delta[3], inv[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        delta[a] = (pa.step_w * w[a]) * pa.vox[a];
        inv[a] = 1.0f / delta[a];  // the look-ahead's estimate only
      }
      bool open = true;
      int j = 0;
      while (j <= last) {
        const float fj = (float)j;
        const float sx = o[0] + (fj * delta[0]), sy = o[1] + (fj * delta[1]), sz = o[2] + (fj * delta[2]);
        if (!(sx >= 0.0f && sx < rf && sy >= 0.0f && sy < rf && sz >= 0.0f && sz < rf)) break;  // left: unoccluded
        const int ix = (int)floorf(sx), iy = (int)floorf(sy), iz = (int)floorf(sz);
        const int bx = ix >> 3, by = iy >> 3, bz = iz >> 3;
        const int bi = (bz * nb + by) * nb + bx;
        if ((block_bits[bi >> 5] >> (bi & 31)) & 1u) {
          if ((bits[((long long)iz * r + iy) * wx + (ix >> 5)] >> (ix & 31)) & 1u) {
            open = false;
            break;
          }
          ++j;
          continue;
        }
        // an empty block: how many samples more stay in it?  The estimate: the nearest face along the ray
        float t = (float)(last - j);
        {
          const float s[3] = {sx, sy, sz};
          const int b[3] = {bx, by, bz};
#pragma unroll
          for (int a = 0; a < 3; ++a) {
            const float face = (float)(8 * b[a] + (delta[a] > 0.0f ? 8 : 0));
            const float ta = (face - s[a]) * inv[a];
            if (delta[a] != 0.0f && ta < t) t = ta;
          }
        }
        int m = t >= 1.0f ? (int)t : 0;  // a NaN: 0
        while (m > 0) {  // the proof: sample j + m by the definition's own expression
          const float fm = (float)(j + m);
          const float qx = o[0] + (fm * delta[0]), qy = o[1] + (fm * delta[1]), qz = o[2] + (fm * delta[2]);
          if (qx >= 0.0f && qx < rf && qy >= 0.0f && qy < rf && qz >= 0.0f && qz < rf &&
              ((int)floorf(qx) >> 3) == bx && ((int)floorf(qy) >> 3) == by && ((int)floorf(qz) >> 3) == bz)
            break;
          m >>= 1;
        }
        j += m + 1;
      }
      if (open) {
        word |= 1ull << (d & 63);
        const float *__restrict__ b = pa.basis + 9 * d;
#pragma unroll
        for (int k = 0; k < 9; ++k) acc[k] = acc[k] + (kd * b[k]);
      }
    }
    if ((d & 63) == 63) {
      if (mask) mask[v * words + (d >> 6)] = word;
      word = 0;
    }
  }
  if (prt) {
#pragma unroll
    for (int k = 0; k < 9; ++k) prt[9 * v + k] = acc[k] * pa.weight;
  }
}

int launch_mesh_transfer_batch(mp_ctx *ctx, int n_frames, const float *const *verts, const float *const *normals,
                               long long max_v, const int32_t *const *counts, const uint32_t *const *bits,
                               const TransferRays &rays, uint64_t *const *mask, float *const *prt, hipStream_t st) {
  TransferFrames fr;
  TransferParams pa;
  std::memset(&fr, 0, sizeof(fr));
  std::memset(&pa, 0, sizeof(pa));
  for (int f = 0; f < n_frames; ++f) {
    fr.verts[f] = verts[f];
    fr.normals[f] = normals[f];
    fr.counts[f] = counts[f];
    fr.bits[f] = bits[f];
    fr.mask[f] = mask ? reinterpret_cast<unsigned long long *>(mask[f]) : nullptr;
    fr.prt[f] = prt ? prt[f] : nullptr;
  }
  pa.rf = (float)rays.r;
  for (int a = 0; a < 3; ++a) {
    pa.bmin[a] = rays.bmin[a];
    pa.len[a] = rays.bmax[a] - rays.bmin[a];
    pa.vox[a] = pa.rf / pa.len[a];
  }
  pa.weight = rays.weight;
  pa.bias_w = rays.bias_w;
  pa.step_w = rays.step_w;
  pa.r = rays.r;
  pa.wx = bits_wx(rays.r);
  pa.nb = bits_nb(rays.r);
  pa.block_words = bits_block_words(rays.r);
  pa.fine_words = bits_fine_words(rays.r);
  pa.n_dirs = rays.n_dirs;
  pa.max_steps = rays.max_steps;
  pa.max_v = max_v;
  pa.dirs = rays.dirs;
  pa.basis = rays.basis;
  hipLaunchKernelGGL(mesh_transfer, dim3((unsigned)((max_v + kTransferBlock - 1) / kTransferBlock), n_frames),
                     dim3(kTransferBlock), (size_t)pa.block_words * sizeof(uint32_t), st, fr, pa);
  MP_HIP(ctx, hipGetLastError());
  return MP_OK;
}

struct ShadeFrames {
  const float *prt[kMaxFrames];
  const int32_t *counts[kMaxFrames];
  float *out[kMaxFrames];
};
struct ShadeParams {
  float sh[27];  // [9][3]
};

__global__ __launch_bounds__(kBitsBlock) void transfer_shade(ShadeFrames fr, ShadeParams pa, long long max_v) {
  const int f = blockIdx.y;
  const long long v = (long long)blockIdx.x * kBitsBlock + threadIdx.x;
  if (v >= transfer_count(fr.counts[f], max_v)) return;
  const float *__restrict__ p = fr.prt[f] + 9 * v;
  float t[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    const float pk = p[k];
#pragma unroll
    for (int c = 0; c < 3; ++c) t[c] = t[c] + pk * pa.sh[3 * k + c];
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) fr.out[f][3 * v + c] = t[c];
}

int launch_mesh_transfer_shade_batch(mp_ctx *ctx, int n_frames, const float *const *prt, long long max_v,
                                     const int32_t *const *counts, const float *sh, float *const *out, hipStream_t st) {
  ShadeFrames fr;
  ShadeParams pa;
  std::memset(&fr, 0, sizeof(fr));
  for (int f = 0; f < n_frames; ++f) {
    fr.prt[f] = prt[f];
    fr.counts[f] = counts[f];
    fr.out[f] = out[f];
  }
  std::memcpy(pa.sh, sh, sizeof(pa.sh));
  hipLaunchKernelGGL(transfer_shade, dim3((unsigned)((max_v + kBitsBlock - 1) / kBitsBlock), n_frames),
                     dim3(kBitsBlock), 0, st, fr, pa, max_v);
  MP_HIP(ctx, hipGetLastError());
  return MP_OK;
}

}  // namespace mp
