// The resolve of a supersampled picture (mp_picture_resolve, include/monoport_hip.h): every output pixel is the box of
// its s x s samples -- the mean of the image, the subject's coverage, the nearest showing sample's depth and face id,
// the largest mask.
//   picture_resolve<S, Wide>  one thread per output pixel, adjacent lanes adjacent j: a wavefront reads each of its S
//                             input rows as ONE contiguous span (64 S pixels) and writes one contiguous span
// A streaming kernel, defined bit for bit: the image sum is S*S - 1 sequential IEEE f32 additions in row-major sample
// order and one IEEE division (no FMA: there is no product); no atomics, no scratch, no LDS.  S is a template
// parameter, so the sample loops unroll and the samples stay in registers.  Wide (S = 2, 4 with every input 16-byte
// aligned): a lane's S samples of a row are one 8 / 16-byte load per plane (three per image row) instead of S dwords;
// the same values in the same order.  blockIdx.y is the picture (frame x view); the per-picture pointers travel by
// value (ResolveFrames), as picture_composite's do.
#include "mp_internal.h"

#include <cstring>

#pragma clang fp contract(off)

namespace mp {

constexpr int kResolveBlock = 256;

struct ResolveFrames {  // per picture = (frame, view); a plane nobody gave or wants is nullptr in every entry
  const float *image[kMaxFrames];   // [S h, S w, 3]
  const float *depth[kMaxFrames];   // [S h, S w]
  const int32_t *face[kMaxFrames];  // [S h, S w]
  const uint8_t *mask[kMaxFrames];  // [S h, S w]
  float *image_out[kMaxFrames];     // [h, w, 3]
  uint32_t *depth_out[kMaxFrames];  // [h, w]
  int32_t *face_out[kMaxFrames];
  uint8_t *mask_out[kMaxFrames];
  float *coverage[kMaxFrames];
};
static_assert(sizeof(ResolveFrames) + 256 <= 4096, "picture_resolve: kernel arguments");

// the rasteriser's orderable key of a depth's bits (raster.hip): unsigned order = float order, -0 below +0
__device__ __forceinline__ uint32_t resolve_key(uint32_t b) { return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u); }

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// N consecutive 32-bit words from p; Wide: p is 8-byte (N even) / 16-byte (N a multiple of 4) aligned
template <int N, bool Wide>
__device__ __forceinline__ void load_words(const void *p, uint32_t (&v)[N]) {
  if constexpr (Wide && N % 4 == 0) {
#pragma unroll
    for (int k = 0; k < N / 4; ++k) {
      const u32x4 t = reinterpret_cast<const u32x4 *>(p)[k];
      v[4 * k] = t.x, v[4 * k + 1] = t.y, v[4 * k + 2] = t.z, v[4 * k + 3] = t.w;
    }
  } else if constexpr (Wide && N % 2 == 0) {
#pragma unroll
    for (int k = 0; k < N / 2; ++k) {
      const u32x2 t = reinterpret_cast<const u32x2 *>(p)[k];
      v[2 * k] = t.x, v[2 * k + 1] = t.y;
    }
  } else {
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = reinterpret_cast<const uint32_t *>(p)[k];
  }
}

// N consecutive bytes from p; Wide: p is N-byte aligned (N = 2, 4)
template <int N, bool Wide>
__device__ __forceinline__ void load_bytes(const uint8_t *p, uint32_t (&v)[N]) {
  if constexpr (Wide && N == 4) {
    const uint32_t t = *reinterpret_cast<const uint32_t *>(p);
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = (t >> (8 * k)) & 0xFFu;
  } else if constexpr (Wide && N == 2) {
    const uint32_t t = *reinterpret_cast<const uint16_t *>(p);
    v[0] = t & 0xFFu, v[1] = t >> 8;
  } else {
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = p[k];
  }
}

template <int S, bool Wide>
__global__ __launch_bounds__(kResolveBlock) void picture_resolve(ResolveFrames fr, int h, int w, int nearest) {
  const int p = blockIdx.x * kResolveBlock + threadIdx.x;  // h w <= 2048^2
  if (p >= h * w) return;
  const int f = blockIdx.y;
  const int i = p / w, j = p - i * w;
  const size_t row = (size_t)S * w;                    // samples of an input row
  const size_t first = (size_t)S * i * row + S * j;    // sample (0, 0) of the pixel
  const float *__restrict__ image = fr.image[f];
  const float *__restrict__ depth = fr.depth[f];
  const int32_t *__restrict__ face = fr.face[f];
  const uint8_t *__restrict__ mask = fr.mask[f];
  const bool want_image = fr.image_out[f] != nullptr;
  const bool want_near = fr.depth_out[f] != nullptr || fr.face_out[f] != nullptr;
  const bool want_flags = fr.coverage[f] != nullptr || fr.mask_out[f] != nullptr || want_near;
  const uint32_t flip = nearest == MP_NEAREST_MIN_Z ? 0x80000000u : 0u;  // the key of -depth

  float acc[3] = {0.0f, 0.0f, 0.0f};
  int count = 0;
  uint32_t most = 0, best_key = 0, best_depth = 0;  // +0.0
  int32_t best_face = -1;
  bool found = false;
#pragma unroll
  for (int a = 0; a < S; ++a) {
    const size_t q = first + a * row;
    if (want_image) {
      uint32_t v[3 * S];
      load_words<3 * S, Wide>(image + 3 * q, v);
#pragma unroll
      for (int b = 0; b < S; ++b)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float x = __uint_as_float(v[3 * b + c]);
          acc[c] = (a == 0 && b == 0) ? x : acc[c] + x;
        }
    }
    if (!want_flags) continue;
    uint32_t m[S], fc[S], d[S];
    if (mask) load_bytes<S, Wide>(mask + q, m);
    if (face && (!mask || want_near)) load_words<S, Wide>(face + q, fc);
    if (want_near) load_words<S, Wide>(depth + q, d);
#pragma unroll
    for (int b = 0; b < S; ++b) {
      const bool subject = mask ? m[b] == 2u : (int32_t)fc[b] >= 0;
      const bool shows = mask ? m[b] != 0u : (int32_t)fc[b] >= 0;
      count += subject ? 1 : 0;
      if (mask) most = m[b] > most ? m[b] : most;
      if (want_near && shows) {
        const uint32_t key = resolve_key(d[b] ^ flip);
        if (!found || key > best_key) best_key = key, best_depth = d[b], best_face = (int32_t)fc[b];
        found = true;
      }
    }
  }
  constexpr float kSamples = (float)(S * S);
  if (want_image) {
    float *__restrict__ out = fr.image_out[f];
#pragma unroll
    for (int c = 0; c < 3; ++c) out[3 * (size_t)p + c] = acc[c] / kSamples;
  }
  if (fr.depth_out[f]) fr.depth_out[f][p] = best_depth;
  if (fr.face_out[f]) fr.face_out[f][p] = best_face;
  if (fr.mask_out[f]) fr.mask_out[f][p] = (uint8_t)most;
  if (fr.coverage[f]) fr.coverage[f][p] = (float)count / kSamples;
}

template <int S>
static void resolve_launch(const ResolveFrames &fr, int n_pictures, int h, int w, int nearest, bool wide,
                           hipStream_t st) {
  const dim3 grid((unsigned)(((long long)h * w + kResolveBlock - 1) / kResolveBlock), n_pictures);
  if (wide)
    hipLaunchKernelGGL((picture_resolve<S, true>), grid, dim3(kResolveBlock), 0, st, fr, h, w, nearest);
  else
    hipLaunchKernelGGL((picture_resolve<S, false>), grid, dim3(kResolveBlock), 0, st, fr, h, w, nearest);
}

int launch_picture_resolve_batch(mp_ctx *ctx, int n_frames, int n_views, const float *const *image,
                                 const float *const *depth, const int32_t *const *face_id, const uint8_t *const *mask,
                                 int h, int w, int samples, int nearest, float *const *image_out,
                                 float *const *depth_out, int32_t *const *face_out, uint8_t *const *mask_out,
                                 float *const *coverage, hipStream_t st) {
  ResolveFrames fr;
  std::memset(&fr, 0, sizeof(fr));
  const size_t fine = (size_t)samples * h * samples * w, coarse = (size_t)h * w;  // pixels of a view
  uintptr_t bits = 0;  // the union of every input address: its low bits are the alignment all of them share
  for (int f = 0; f < n_frames; ++f)
    for (int v = 0; v < n_views; ++v) {
      const int k = f * n_views + v;
      if (image) fr.image[k] = image[f] + 3 * fine * v;
      if (depth) fr.depth[k] = depth[f] + fine * v;
      if (face_id) fr.face[k] = face_id[f] + fine * v;
      if (mask) fr.mask[k] = mask[f] + fine * v;
      if (image_out) fr.image_out[k] = image_out[f] + 3 * coarse * v;
      if (depth_out) fr.depth_out[k] = reinterpret_cast<uint32_t *>(depth_out[f]) + coarse * v;
      if (face_out) fr.face_out[k] = face_out[f] + coarse * v;
      if (mask_out) fr.mask_out[k] = mask_out[f] + coarse * v;
      if (coverage) fr.coverage[k] = coverage[f] + coarse * v;
      bits |= (uintptr_t)fr.image[k] | (uintptr_t)fr.depth[k] | (uintptr_t)fr.face[k] | (uintptr_t)fr.mask[k];
    }
  const bool wide = samples != 3 && !(bits & 15);
  const int n = n_frames * n_views;
  if (samples == 2)
    resolve_launch<2>(fr, n, h, w, nearest, wide, st);
  else if (samples == 3)
    resolve_launch<3>(fr, n, h, w, nearest, false, st);
  else
    resolve_launch<4>(fr, n, h, w, nearest, wide, st);
  MP_HIP(ctx, hipGetLastError());
  return MP_OK;
}

}  // namespace mp
