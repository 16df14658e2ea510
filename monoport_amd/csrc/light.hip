// Lighting the subject per pixel (mp_picture_light, include/monoport_hip.h): second-order spherical harmonics at the
// pixel's normal, one directional light with an optional visibility picture, a gamma, and albedo * shading.
//   picture_light      one thread per pixel: the normal picture the rasteriser wrote, normalised; nine basis values; the
//                      27 coefficients; the direct term; the clamped product
// A streaming kernel, defined bit for bit: every float operation is one IEEE f32 +, -, *, / or sqrtf in the order the
// header writes (the library is built with -ffp-contract=off: no FMA), except powf under a gamma != 1.  No atomics, no
// scratch.  blockIdx.y is the frame; the per-frame pointers and the per-(frame, view) matrices travel by value
// (LightFrames), the coefficients and the light per call (LightParams).
#include "mp_internal.h"

#include <cstring>

namespace mp {

constexpr int kLightBlock = 256;

struct LightFrames {
  const float *normal[kMaxFrames];     // [L,3]
  const int32_t *face[kMaxFrames];     // [L]
  const uint32_t *albedo[kMaxFrames];  // [L,3]; nullptr: the constant albedo
  const float *vis[kMaxFrames];        // [L]; nullptr: nothing occludes the light
  uint32_t *image[kMaxFrames];         // nullptr: not wanted; may be albedo
  float *shading[kMaxFrames];          // nullptr: not wanted
  const float *ambient[kMaxFrames];    // [L,3]; picture_light<true> only: the SH term, given per pixel
  float mats[kLightMaxMats][9];        // frame-major, then view; unused without has_mats
};
struct LightParams {
  float sh[27];  // [9][3]
  float dir[3], rgb[3], albedo_rgb[3];
  float gamma, inv_gamma, background;
  int has_mats, has_direct, n_views, view_pixels;
};
static_assert(sizeof(LightFrames) + sizeof(LightParams) + 256 <= 4096, "picture_light: kernel arguments");

// no __restrict__ on albedo / image: image may be albedo; a thread reads its pixel, then writes it
// kAmbient (mp_picture_light_transfer): res starts from ambient[p] instead of the basis at the normal; the normal
// picture may then be nullptr where there is no direct term
template <bool kAmbient>
__global__ __launch_bounds__(kLightBlock) void picture_light(LightFrames fr, LightParams pa, int n_pixels) {
  const long long p = (long long)blockIdx.x * kLightBlock + threadIdx.x;
  if (p >= n_pixels) return;
  const int f = blockIdx.y;
  const uint32_t *alb = fr.albedo[f];
  uint32_t *out = fr.image[f];
  float *shading = fr.shading[f];
  if (fr.face[f][p] < 0) {  // an uncovered span costs a wavefront its face ids only
    if (shading) {
#pragma unroll
      for (int c = 0; c < 3; ++c) shading[3 * p + c] = 0.0f;
    }
    if (out) {
      if (!alb) {
#pragma unroll
        for (int c = 0; c < 3; ++c) out[3 * p + c] = __float_as_uint(pa.background);
      } else if (out != alb) {
#pragma unroll
        for (int c = 0; c < 3; ++c) out[3 * p + c] = alb[3 * p + c];
      }
    }
    return;
  }
  const float *__restrict__ nrm = fr.normal[f];
  float nx = 0.0f, ny = 0.0f, nz = 0.0f;
  if (!kAmbient || nrm) light_normalise(nrm[3 * p], nrm[3 * p + 1], nrm[3 * p + 2], nx, ny, nz);
  float res[3] = {0.0f, 0.0f, 0.0f};
  if constexpr (kAmbient) {
#pragma unroll
    for (int c = 0; c < 3; ++c) res[c] = fr.ambient[f][3 * p + c];
  } else {
    float mx = nx, my = ny, mz = nz;  // the SH normal
    if (pa.has_mats) {
      const float *m = fr.mats[f * pa.n_views + (int)(p / pa.view_pixels)];
      const float tx = (m[0] * nx + m[1] * ny) + m[2] * nz;
      const float ty = (m[3] * nx + m[4] * ny) + m[5] * nz;
      const float tz = (m[6] * nx + m[7] * ny) + m[8] * nz;
      light_normalise(tx, ty, tz, mx, my, mz);
    }
    const float c1 = 0.429043f, c2 = 0.511664f, c3 = 0.743125f, c4 = 0.886227f, c5 = 0.247708f;
    float h[9];
    h[0] = c4;
    h[1] = (2.0f * c2) * my;
    h[2] = (2.0f * c2) * mz;
    h[3] = (2.0f * c2) * mx;
    h[4] = ((2.0f * c1) * mx) * my;
    h[5] = ((2.0f * c1) * my) * mz;
    h[6] = ((c3 * mz) * mz) - c5;
    h[7] = ((2.0f * c1) * mz) * mx;
    h[8] = c1 * ((mx * mx) - (my * my));
#pragma unroll
    for (int i = 0; i < 9; ++i) {
#pragma unroll
      for (int c = 0; c < 3; ++c) res[c] = res[c] + h[i] * pa.sh[3 * i + c];
    }
  }
  if (pa.has_direct) {  // on the world normal, whatever the SH frame
    const float t = -((pa.dir[0] * nx + pa.dir[1] * ny) + pa.dir[2] * nz);
    const float k = t > 0.0f ? t : 0.0f;  // facing away, a NaN: +0.0
    const float vis = fr.vis[f] ? 1.0f - fr.vis[f][p] : 1.0f;
    const float kv = k * vis;
#pragma unroll
    for (int c = 0; c < 3; ++c) res[c] = res[c] + kv * pa.rgb[c];
  }
  if (pa.gamma != 1.0f) {
#pragma unroll
    for (int c = 0; c < 3; ++c) res[c] = powf(res[c] > 0.0f ? res[c] : 0.0f, pa.inv_gamma);
  }
  if (out) {
    float a[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) a[c] = alb ? __uint_as_float(alb[3 * p + c]) : pa.albedo_rgb[c];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float v = a[c] * res[c];
      out[3 * p + c] = __float_as_uint(v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v));  // mp_paint's clamp: keeps a NaN
    }
  }
  if (shading) {
#pragma unroll
    for (int c = 0; c < 3; ++c) shading[3 * p + c] = res[c];
  }
}

int launch_picture_light_batch(mp_ctx *ctx, int n_frames, const float *const *normal, const int32_t *const *face_id,
                               const float *const *albedo, const float *albedo_rgb, const float *const *visibility,
                               const float *const *ambient, long long n_pixels, int n_views, const float *sh,
                               const float *direct_dir,
                               const float *direct_rgb, float gamma, const float *normal_mats, float background,
                               float *const *image_out, float *const *shading, hipStream_t st) {
  LightFrames fr;
  LightParams pa;
  std::memset(&fr, 0, sizeof(fr));
  std::memset(&pa, 0, sizeof(pa));
  for (int f = 0; f < n_frames; ++f) {
    fr.normal[f] = normal ? normal[f] : nullptr;
    fr.ambient[f] = ambient ? ambient[f] : nullptr;
    fr.face[f] = face_id[f];
    fr.albedo[f] = albedo ? reinterpret_cast<const uint32_t *>(albedo[f]) : nullptr;
    fr.vis[f] = visibility ? visibility[f] : nullptr;
    fr.image[f] = image_out ? reinterpret_cast<uint32_t *>(image_out[f]) : nullptr;
    fr.shading[f] = shading ? shading[f] : nullptr;
  }
  if (normal_mats) std::memcpy(fr.mats, normal_mats, sizeof(float) * 9 * (size_t)n_frames * n_views);
  if (sh) std::memcpy(pa.sh, sh, sizeof(pa.sh));
  for (int c = 0; c < 3; ++c) {
    pa.dir[c] = direct_dir[c];
    pa.rgb[c] = direct_rgb[c];
    pa.albedo_rgb[c] = albedo_rgb ? albedo_rgb[c] : 0.0f;
  }
  pa.gamma = gamma;
  pa.inv_gamma = 1.0f / gamma;
  pa.background = background;
  pa.has_mats = normal_mats != nullptr;
  pa.has_direct = direct_rgb[0] != 0.0f || direct_rgb[1] != 0.0f || direct_rgb[2] != 0.0f;
  pa.n_views = n_views;
  pa.view_pixels = (int)(n_pixels / n_views);
  const dim3 grid((unsigned)((n_pixels + kLightBlock - 1) / kLightBlock), n_frames);
  if (ambient)
    hipLaunchKernelGGL(picture_light<true>, grid, dim3(kLightBlock), 0, st, fr, pa, (int)n_pixels);
  else
    hipLaunchKernelGGL(picture_light<false>, grid, dim3(kLightBlock), 0, st, fr, pa, (int)n_pixels);
  MP_HIP(ctx, hipGetLastError());
  return MP_OK;
}

}  // namespace mp
