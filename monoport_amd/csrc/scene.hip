// The scene behind the subject (mp_texture_mips / mp_picture_texture / mp_picture_composite / mp_picture_shadow,
// include/monoport_hip.h): a mip pyramid of a texture, the texture looked up per pixel of a UV picture the rasteriser
// wrote, the composite of two pictures by coverage or by depth, and the shadow a shadow map casts on a picture.
//   texture_mip        one thread per texel of a level: the 2x2 box of the level below (level 0: the copy)
//   picture_texture    one thread per pixel: covered?, the level from the uv steps to its four neighbours, four texels
//                      of that level, the paint
//   picture_composite  one thread per pixel: which of the two pictures shows; its values as 32-bit patterns
//   picture_shadow     one thread per pixel: its position under the light, (2r+2)^2 taps of the light's depth map, the
//                      darkened pixel (the projection is the rasteriser's own: query_common.h, FMA and division there)
// All four are streaming kernels and defined bit for bit: every float operation is one IEEE f32 +, - or * in the order
// the header writes (no sqrt, log or division, whose rounding could differ from numpy's), no atomics, no scratch.
// blockIdx.y is the frame; the per-frame pointers travel by value (TextureFrames, CompositeFrames, ShadowFrames).
#include "mp_internal.h"
#include "query_common.h"

#include <cstring>

#pragma clang fp contract(off)

namespace mp {

constexpr int kSceneBlock = 256;
constexpr float kUvMost = 65536.0f;  // a covered pixel has |u|, |v| <= this: texel indices stay inside int32

struct TextureFrames {
  const float *uv[kMaxFrames];      // [L,3]
  const int32_t *face[kMaxFrames];  // [L]
  float *image[kMaxFrames];         // [L,3]
};
struct CompositeFrames {
  const uint32_t *front_image[kMaxFrames];  // [L,3]
  const float *front_depth[kMaxFrames];     // [L]
  const int32_t *front_face[kMaxFrames];
  const uint32_t *back_image[kMaxFrames];
  const float *back_depth[kMaxFrames];
  const int32_t *back_face[kMaxFrames];
  uint32_t *image[kMaxFrames];
  uint32_t *depth[kMaxFrames];  // nullptr: not wanted
  uint8_t *mask[kMaxFrames];    // nullptr: not wanted
};
struct ShadowFrames {
  const uint32_t *image_in[kMaxFrames];  // [L,3]; nullptr: no image
  const float *position[kMaxFrames];     // [L,3]
  const int32_t *face[kMaxFrames];       // [L]
  const float *map_depth[kMaxFrames];    // [hs,ws]
  const int32_t *map_face[kMaxFrames];   // [hs,ws]
  uint32_t *image_out[kMaxFrames];       // nullptr: no image; may be image_in
  float *shade[kMaxFrames];              // nullptr: not wanted
  float cal[kMaxFrames][12];             // the light's [R|t]
};
static_assert(sizeof(TextureFrames) + 256 <= 4096 && sizeof(CompositeFrames) + 256 <= 4096, "scene: kernel arguments");
static_assert(sizeof(ShadowFrames) + 256 <= 4096, "picture_shadow: kernel arguments");

static int mip_size(int n) { return n > 1 ? n >> 1 : 1; }

// the most levels a ht x wt texture has: down to 1 x 1
static int texture_max_levels(int ht, int wt) {
  int n = 1;
  for (int m = ht > wt ? ht : wt; m > 1; m >>= 1) ++n;
  return n;
}

bool texture_sizes_ok(int ht, int wt, int levels) {
  return ht >= 1 && ht <= 8192 && wt >= 1 && wt <= 8192 && levels >= 1 && levels <= 14 &&
         levels <= texture_max_levels(ht, wt);
}

long long texture_pyramid_floats(int ht, int wt, int levels) {
  long long n = 0;
  for (int l = 0; l < levels; ++l) {
    n += 3LL * ht * wt;
    ht = mip_size(ht), wt = mip_size(wt);
  }
  return n;
}

// dst [h,w,3] from src [hs,ws,3]; copy: dst = src (level 0)
__global__ __launch_bounds__(kSceneBlock) void texture_mip(const float *__restrict__ src, int hs, int ws,
                                                           float *__restrict__ dst, int h, int w, int copy) {
  const long long k = (long long)blockIdx.x * kSceneBlock + threadIdx.x;  // the float of dst
  if (k >= 3LL * h * w) return;
  if (copy) {
    dst[k] = src[k];
    return;
  }
  const int c = (int)(k % 3);
  const long long t = k / 3;
  const int j = (int)(t % w), i = (int)(t / w);
  const int i0 = min(2 * i, hs - 1), i1 = min(2 * i + 1, hs - 1);
  const int j0 = min(2 * j, ws - 1), j1 = min(2 * j + 1, ws - 1);
  const float a = src[((long long)i0 * ws + j0) * 3 + c], b = src[((long long)i0 * ws + j1) * 3 + c];
  const float cc = src[((long long)i1 * ws + j0) * 3 + c], d = src[((long long)i1 * ws + j1) * 3 + c];
  dst[k] = ((a + b) + (cc + d)) * 0.25f;
}

__device__ __forceinline__ bool uv_covered(int32_t face, float u, float v) {
  // a NaN fails both comparisons; an infinity fails one
  return face >= 0 && fabsf(u) <= kUvMost && fabsf(v) <= kUvMost;
}

// d2 of pixel q against (s, t) if q is covered, folded into the smaller of the axis: `best` < 0 = none yet
__device__ __forceinline__ float uv_step(const float *__restrict__ uv, const int32_t *__restrict__ face, long long q,
                                         float s, float t, float fw, float fh, float best) {
  const float u = uv[3 * q], v = uv[3 * q + 1];
  if (!uv_covered(face[q], u, v)) return best;
  const float ds = u * fw - s, dt = v * fh - t;
  const float d2 = (ds * ds) + (dt * dt);
  return (best < 0.0f || d2 < best) ? d2 : best;
}

__device__ __forceinline__ int wrap_index(int i, int n, int wrap) {
  if (wrap == MP_WRAP_REPEAT) return ((i % n) + n) % n;
  return i < 0 ? 0 : (i > n - 1 ? n - 1 : i);
}

__global__ __launch_bounds__(kSceneBlock) void picture_texture(TextureFrames fr, int n_pixels, int h, int w,
                                                               const float *__restrict__ pyramid, int ht, int wt,
                                                               int levels, int wrap, float scale, float bias, float lo,
                                                               float hi, float background) {
  const long long p = (long long)blockIdx.x * kSceneBlock + threadIdx.x;
  if (p >= n_pixels) return;
  const float *__restrict__ uv = fr.uv[blockIdx.y];
  const int32_t *__restrict__ face = fr.face[blockIdx.y];
  float *__restrict__ image = fr.image[blockIdx.y];
  const float u = uv[3 * p], v = uv[3 * p + 1];
  if (!uv_covered(face[p], u, v)) {
#pragma unroll
    for (int c = 0; c < 3; ++c) image[3 * p + c] = background;
    return;
  }
  const int j = (int)(p % w), i = (int)((p / w) % h);  // the view is p / (h w): neighbours stay inside it
  const float fw = (float)wt, fh = (float)ht;
  const float s = u * fw, t = v * fh;
  float ri = -1.0f, rj = -1.0f;
  if (i + 1 < h) ri = uv_step(uv, face, p + w, s, t, fw, fh, ri);
  if (i > 0) ri = uv_step(uv, face, p - w, s, t, fw, fh, ri);
  if (j + 1 < w) rj = uv_step(uv, face, p + 1, s, t, fw, fh, rj);
  if (j > 0) rj = uv_step(uv, face, p - 1, s, t, fw, fh, rj);
  if (ri < 0.0f) ri = 0.0f;
  if (rj < 0.0f) rj = 0.0f;
  const float rho2 = ri > rj ? ri : rj;
  // nearest mip: the number of l in 0..levels-2 with rho2 > 2^(2l+1); the thresholds ascend, so the first miss ends it
  long long off = 0;
  int hl = ht, wl = wt;
  float thr = 2.0f;
  for (int l = 0; l + 1 < levels && rho2 > thr; ++l) {
    off += 3LL * hl * wl;
    hl = hl > 1 ? hl >> 1 : 1;
    wl = wl > 1 ? wl >> 1 : 1;
    thr = thr * 4.0f;  // exact
  }
  const float *__restrict__ tex = pyramid + off;
  const float sl = u * (float)wl - 0.5f, tl = v * (float)hl - 0.5f;
  const float s0 = floorf(sl), t0 = floorf(tl);
  const float fs = sl - s0, ft = tl - t0;
  const int x0 = wrap_index((int)s0, wl, wrap), x1 = wrap_index((int)s0 + 1, wl, wrap);
  const int y0 = wrap_index((int)t0, hl, wrap), y1 = wrap_index((int)t0 + 1, hl, wrap);
  const float gs = 1.0f - fs, gt = 1.0f - ft;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float c00 = tex[((long long)y0 * wl + x0) * 3 + c], c10 = tex[((long long)y0 * wl + x1) * 3 + c];
    const float c01 = tex[((long long)y1 * wl + x0) * 3 + c], c11 = tex[((long long)y1 * wl + x1) * 3 + c];
    const float value = (c00 * gs + c10 * fs) * gt + (c01 * gs + c11 * fs) * ft;
    float o = value * scale + bias;
    o = o < lo ? lo : (o > hi ? hi : o);
    image[3 * p + c] = o;
  }
}

// no __restrict__: the outputs may be the front's (or the back's) own buffers; a thread reads its pixel, then writes it
__global__ __launch_bounds__(kSceneBlock) void picture_composite(CompositeFrames fr, int n_pixels, int mode, int nearest,
                                                                 uint32_t background) {
  const long long p = (long long)blockIdx.x * kSceneBlock + threadIdx.x;
  if (p >= n_pixels) return;
  const int f = blockIdx.y;
  const bool fc = fr.front_face[f][p] >= 0, bc = fr.back_face[f][p] >= 0;
  const float df = fr.front_depth[f][p], db = fr.back_depth[f][p];
  const bool back_nearer = nearest == MP_NEAREST_MIN_Z ? db < df : db > df;  // a NaN: not nearer
  const bool front = fc && (!bc || mode == MP_COMPOSITE_OVER || !back_nearer);
  uint32_t px[3] = {background, background, background};
  uint32_t d = 0;  // +0.0
  uint8_t m = 0;
  if (front) {
#pragma unroll
    for (int c = 0; c < 3; ++c) px[c] = fr.front_image[f][3 * p + c];
    d = __float_as_uint(df), m = 2;
  } else if (bc) {
#pragma unroll
    for (int c = 0; c < 3; ++c) px[c] = fr.back_image[f][3 * p + c];
    d = __float_as_uint(db), m = 1;
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) fr.image[f][3 * p + c] = px[c];
  if (fr.depth[f]) fr.depth[f][p] = d;
  if (fr.mask[f]) fr.mask[f][p] = m;
}

constexpr float kShadowMost = 4194304.0f;  // 2^22: map coordinates beyond it are outside every map (and stay inside int32)

// shade of one point under the light: 0 for a point that fails steps 2-3 of the definition, touching no map memory
__device__ __forceinline__ float shadow_shade(const float *__restrict__ cal, int proj, int nearest, float px, float py,
                                              float pz, const float *__restrict__ map_depth,
                                              const int32_t *__restrict__ map_face, int hs, int ws, float bias, int radius,
                                              float k_r) {
  float x, y, z;
  project_mode(cal, proj, px, py, pz, x, y, z);
  if (!(__builtin_isfinite(x) && __builtin_isfinite(y) && __builtin_isfinite(z))) return 0.0f;
  if (proj == MP_PROJ_PERSPECTIVE && !(z > 0.0f)) return 0.0f;
  const float a = (x + 1.0f) * (0.5f * (float)hs) - 0.5f;
  const float b = (y + 1.0f) * (0.5f * (float)ws) - 0.5f;
  if (fabsf(a) > kShadowMost || fabsf(b) > kShadowMost) return 0.0f;
  const float af = floorf(a), bf = floorf(b);
  const float fa = a - af, fb = b - bf;
  const int i0 = (int)af, j0 = (int)bf;
  // no tap inside the map: nothing occludes
  if (i0 + radius + 1 < 0 || i0 - radius >= hs || j0 + radius + 1 < 0 || j0 - radius >= ws) return 0.0f;
  const float ga = 1.0f - fa, gb = 1.0f - fb;
  float total = 0.0f;
  for (int di = -radius; di <= radius + 1; ++di) {
    const int i = i0 + di;
    const bool row_in = i >= 0 && i < hs;
    float row = 0.0f;
    for (int dj = -radius; dj <= radius + 1; ++dj) {
      const int j = j0 + dj;
      float occ = 0.0f;
      if (row_in && j >= 0 && j < ws) {
        const long long t = (long long)i * ws + j;
        if (map_face[t] >= 0) {
          const float d = map_depth[t];
          const bool nearer = nearest == MP_NEAREST_MIN_Z ? (d + bias < z) : (d - bias > z);  // a tie, a NaN: not
          occ = nearer ? 1.0f : 0.0f;
        }
      }
      const float wj = dj == -radius ? gb : (dj == radius + 1 ? fb : 1.0f);
      row = row + wj * occ;
    }
    const float wi = di == -radius ? ga : (di == radius + 1 ? fa : 1.0f);
    total = total + wi * row;
  }
  const float s = total * k_r;
  return s < 1.0f ? s : 1.0f;
}

// no __restrict__ on the images: image_out may be image_in; a thread reads its pixel, then writes it
__global__ __launch_bounds__(kSceneBlock) void picture_shadow(ShadowFrames fr, int n_pixels, int hs, int ws, int proj,
                                                              int nearest, float bias, int radius, float k_r,
                                                              float strength) {
  const long long p = (long long)blockIdx.x * kSceneBlock + threadIdx.x;
  if (p >= n_pixels) return;
  const int f = blockIdx.y;
  float s = 0.0f;
  if (fr.face[f][p] >= 0) {  // an uncovered span costs a wavefront its face ids only
    const float *__restrict__ pos = fr.position[f];
    s = shadow_shade(fr.cal[f], proj, nearest, pos[3 * p], pos[3 * p + 1], pos[3 * p + 2], fr.map_depth[f],
                     fr.map_face[f], hs, ws, bias, radius, k_r);
  }
  if (fr.shade[f]) fr.shade[f][p] = s;
  uint32_t *out = fr.image_out[f];
  if (!out) return;
  const uint32_t *in = fr.image_in[f];
  if (s == 0.0f) {
    if (out != in) {
#pragma unroll
      for (int c = 0; c < 3; ++c) out[3 * p + c] = in[3 * p + c];
    }
    return;
  }
  const float factor = 1.0f - strength * s;
#pragma unroll
  for (int c = 0; c < 3; ++c) out[3 * p + c] = __float_as_uint(__uint_as_float(in[3 * p + c]) * factor);
}

static unsigned scene_blocks(long long n) { return (unsigned)((n + kSceneBlock - 1) / kSceneBlock); }

int launch_texture_mips(mp_ctx *ctx, const float *tex, int ht, int wt, int levels, float *pyramid, hipStream_t st) {
  const float *src = tex;
  float *dst = pyramid;
  int hs = ht, ws = wt;
  for (int l = 0; l < levels; ++l) {
    const int h = l ? mip_size(hs) : hs, w = l ? mip_size(ws) : ws;
    hipLaunchKernelGGL(texture_mip, dim3(scene_blocks(3LL * h * w)), dim3(kSceneBlock), 0, st, src, hs, ws, dst, h, w,
                       l == 0 ? 1 : 0);
    src = dst, dst += 3LL * h * w, hs = h, ws = w;
  }
  MP_HIP(ctx, hipGetLastError());
  return MP_OK;
}

int launch_picture_texture_batch(mp_ctx *ctx, int n_frames, const float *const *uv, const int32_t *const *face_id,
                                 long long n_pixels, int h, int w, const float *pyramid, int ht, int wt, int levels,
                                 int wrap, float scale, float bias, float lo, float hi, float background,
                                 float *const *image, hipStream_t st) {
  TextureFrames fr;
  std::memset(&fr, 0, sizeof(fr));
  for (int f = 0; f < n_frames; ++f) fr.uv[f] = uv[f], fr.face[f] = face_id[f], fr.image[f] = image[f];
  hipLaunchKernelGGL(picture_texture, dim3(scene_blocks(n_pixels), n_frames), dim3(kSceneBlock), 0, st, fr,
                     (int)n_pixels, h, w, pyramid, ht, wt, levels, wrap, scale, bias, lo, hi, background);
  MP_HIP(ctx, hipGetLastError());
  return MP_OK;
}

int launch_picture_composite_batch(mp_ctx *ctx, int n_frames, const float *const *front_image,
                                   const float *const *front_depth, const int32_t *const *front_face,
                                   const float *const *back_image, const float *const *back_depth,
                                   const int32_t *const *back_face, long long n_pixels, int mode, int nearest,
                                   float background, float *const *image, float *const *depth, uint8_t *const *mask,
                                   hipStream_t st) {
  CompositeFrames fr;
  std::memset(&fr, 0, sizeof(fr));
  for (int f = 0; f < n_frames; ++f) {
    fr.front_image[f] = reinterpret_cast<const uint32_t *>(front_image[f]);
    fr.front_depth[f] = front_depth[f];
    fr.front_face[f] = front_face[f];
    fr.back_image[f] = reinterpret_cast<const uint32_t *>(back_image[f]);
    fr.back_depth[f] = back_depth[f];
    fr.back_face[f] = back_face[f];
    fr.image[f] = reinterpret_cast<uint32_t *>(image[f]);
    fr.depth[f] = depth ? reinterpret_cast<uint32_t *>(depth[f]) : nullptr;
    fr.mask[f] = mask ? mask[f] : nullptr;
  }
  uint32_t bg;
  std::memcpy(&bg, &background, 4);
  hipLaunchKernelGGL(picture_composite, dim3(scene_blocks(n_pixels), n_frames), dim3(kSceneBlock), 0, st, fr,
                     (int)n_pixels, mode, nearest, bg);
  MP_HIP(ctx, hipGetLastError());
  return MP_OK;
}

int launch_picture_shadow_batch(mp_ctx *ctx, int n_frames, const float *const *image_in, const float *const *position,
                                const int32_t *const *face_id, long long n_pixels, const float *const *map_depth,
                                const int32_t *const *map_face, int hs, int ws, const float *light_calibs, int proj,
                                int nearest, float bias, int radius, float strength, float *const *image_out,
                                float *const *shade, hipStream_t st) {
  static const float k_r[4] = {1.0f, 1.0f / 9.0f, 1.0f / 25.0f, 1.0f / 49.0f};  // the f32 nearest to 1 / (2r+1)^2
  ShadowFrames fr;
  std::memset(&fr, 0, sizeof(fr));
  for (int f = 0; f < n_frames; ++f) {
    fr.image_in[f] = image_in ? reinterpret_cast<const uint32_t *>(image_in[f]) : nullptr;
    fr.position[f] = position[f];
    fr.face[f] = face_id[f];
    fr.map_depth[f] = map_depth[f];
    fr.map_face[f] = map_face[f];
    fr.image_out[f] = image_out ? reinterpret_cast<uint32_t *>(image_out[f]) : nullptr;
    fr.shade[f] = shade ? shade[f] : nullptr;
    std::memcpy(fr.cal[f], light_calibs + 12 * (size_t)f, 12 * sizeof(float));
  }
  hipLaunchKernelGGL(picture_shadow, dim3(scene_blocks(n_pixels), n_frames), dim3(kSceneBlock), 0, st, fr,
                     (int)n_pixels, hs, ws, proj, nearest, bias, radius, k_r[radius], strength);
  MP_HIP(ctx, hipGetLastError());
  return MP_OK;
}

}  // namespace mp
