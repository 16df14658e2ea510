// Z-buffered triangle rasteriser of the device's own meshes (mp_mesh_render, include/monoport_hip.h): any camera,
// any image size, frames x views in one set of launches.
//
// The picture is defined bit for bit, so nothing here may depend on the order in which threads arrive: integer
// atomics only.  Every float operation is one IEEE f32 operation in the order the header gives it (the library is built
// with -ffp-contract=off; / is the correctly rounded one); coverage is exact integer arithmetic on coordinates snapped
// to 1/256 pixel.
//   raster_setup    one thread per (image, vertex): project (query_common.h: the device function of mp_orthogonal /
//                   mp_perspective), snap, validity -> (X, Y, z, valid) in scratch
//   raster_faces    one thread per (image, face): a face whose clamped box holds at most kSmallBox pixel centres is
//                   walked by its thread; a larger one is appended to the image's list (one integer atomic; where a
//                   face lands in the list does not matter)
//   raster_large    one workgroup per listed face, lanes over the pixels of its box
//   raster_resolve  one thread per pixel: decodes the winning key, recomputes the winner's barycentrics with the same
//                   expressions (raster_weights) and writes the requested outputs
// A fragment is ONE 64-bit atomicMax of orderable(depth) << 32 | (0xFFFFFFFF - face) on the pixel's key; 0 = no
// fragment.  A plain load of the key in front of it skips a fragment that has already lost (keys only grow, so a stale
// value can only let a loser through to the atomic, which then changes nothing).
//
// The clipped form (mp_mesh_render_clip: near-plane clipping, perspective-correct interpolation) is four sibling kernels
// further down, raster_*_clip; the four above are not touched by it.
//
// blockIdx.y is the image slot = frame * n_views + view (at most kMaxFrames of them); the per-slot pointers and cameras
// travel by value (RasterMeshes / RasterCams / RasterOut).  Every per-frame size comes from that frame's device counts.
#include "mp_internal.h"
#include "query_common.h"

#include <cstring>

#pragma clang fp contract(off)

namespace mp {

constexpr int kRasterBlock = 256;
constexpr int kSmallBox = 64;          // pixel centres one thread walks at most
constexpr int kLargeBlocks = 1024;     // workgroups of raster_large per image; they stride over the list
constexpr float kSnapGuard = 4194304.0f;  // 2^22: |u|, |v| beyond it make a vertex invalid

__device__ __forceinline__ int raster_min(int count, long long cap) {
  if (count < 0) return 0;
  return (long long)count < cap ? count : (int)cap;
}

struct RasterMeshes {  // per image slot (the views of a frame repeat the frame's pointers)
  const float *verts[kMaxFrames];
  const int32_t *faces[kMaxFrames];
  const int32_t *counts[kMaxFrames];
};
struct RasterCams {
  float cal[kMaxFrames][12];
};
struct RasterOut {  // per image slot; each table is all NULL when the output is not requested
  const float *attr[kMaxFrames];
  float *image[kMaxFrames];
  float *depth[kMaxFrames];
  int32_t *face[kMaxFrames];
};
static_assert(sizeof(RasterMeshes) + sizeof(RasterCams) + 256 <= 4096, "raster_setup: kernel arguments");
static_assert(sizeof(RasterMeshes) + sizeof(RasterOut) + 256 <= 4096, "raster_resolve: kernel arguments");

// Scratch of n images: keys n x [H W] u64 (padded to 256 B) | list counters [n] int (256 B) | snapped vertices n x [max_v] int4 |
// lists n x [max_f] int.  Keys and counters are cleared by ONE memset.
struct RasterScratch {
  unsigned long long *keys;
  int *n_large;
  int4 *snapped;
  int *list;
  long long max_v, max_f, hw;
  int h, w;
  __host__ __device__ unsigned long long *image_keys(int s) const { return keys + hw * s; }
  __host__ __device__ int4 *image_verts(int s) const { return snapped + max_v * s; }
  __host__ __device__ int *image_list(int s) const { return list + max_f * s; }
};

// b -> an unsigned that orders as the float does (-0 < +0)
__device__ __forceinline__ uint32_t orderable(uint32_t b) { return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u); }

__global__ __launch_bounds__(kRasterBlock) void raster_setup(RasterMeshes fr, RasterCams cams, RasterScratch sc,
                                                             int proj) {
  const int s = blockIdx.y;
  const int nv = raster_min(fr.counts[s][0], sc.max_v);
  const long long v = (long long)blockIdx.x * kRasterBlock + threadIdx.x;
  if (v >= nv) return;
  const float *__restrict__ verts = fr.verts[s];
  float x, y, z;
  project_mode(cams.cal[s], proj, verts[3 * v + 0], verts[3 * v + 1], verts[3 * v + 2], x, y, z);
  const float u = ((x + 1.0f) * (0.5f * (float)sc.h)) * 256.0f;
  const float t = ((y + 1.0f) * (0.5f * (float)sc.w)) * 256.0f;
  const bool ok = __builtin_isfinite(u) && __builtin_isfinite(t) && __builtin_isfinite(z) &&
                  !(fabsf(u) > kSnapGuard) && !(fabsf(t) > kSnapGuard);
  int4 o;
  o.x = ok ? (int)rintf(u) : 0;
  o.y = ok ? (int)rintf(t) : 0;
  o.z = __float_as_int(z);
  o.w = ok ? 1 : 0;
  sc.image_verts(s)[v] = o;
}

// One face ready to be covered: counter-clockwise in (X, Y) (area2 > 0), its box of pixel centres clamped to the image.
struct RasterTri {
  long long x[3], y[3];
  float z[3];
  int idx[3];
  long long area2;
  int i0, i1, j0, j1;  // inclusive; empty when i0 > i1 or j0 > j1
};

// false: the face is skipped (an index outside [0, nv), an invalid vertex, zero area)
__device__ __forceinline__ bool raster_load_tri(const int32_t *__restrict__ faces, const int4 *__restrict__ snapped,
                                                long long f, int nv, int h, int w, RasterTri &t) {
  int4 p[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    t.idx[c] = faces[3 * f + c];
    if (t.idx[c] < 0 || t.idx[c] >= nv) return false;
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) p[c] = snapped[t.idx[c]];
  if (!(p[0].w && p[1].w && p[2].w)) return false;
  long long area2 = (long long)(p[1].x - p[0].x) * (long long)(p[2].y - p[0].y) -
                    (long long)(p[1].y - p[0].y) * (long long)(p[2].x - p[0].x);
  if (area2 == 0) return false;
  if (area2 < 0) {  // exchange the second and third vertex with everything attached to them
    const int4 q = p[1];
    p[1] = p[2];
    p[2] = q;
    const int k = t.idx[1];
    t.idx[1] = t.idx[2];
    t.idx[2] = k;
    area2 = -area2;
  }
  t.area2 = area2;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    t.x[c] = p[c].x;
    t.y[c] = p[c].y;
    t.z[c] = __int_as_float(p[c].z);
  }
  // pixel i has its centre at 256 i + 128: i in [ceil((min - 128) / 256), floor((max - 128) / 256)]
  const int xmin = min(p[0].x, min(p[1].x, p[2].x)), xmax = max(p[0].x, max(p[1].x, p[2].x));
  const int ymin = min(p[0].y, min(p[1].y, p[2].y)), ymax = max(p[0].y, max(p[1].y, p[2].y));
  t.i0 = max((xmin - 128 + 255) >> 8, 0);
  t.i1 = min((xmax - 128) >> 8, h - 1);
  t.j0 = max((ymin - 128 + 255) >> 8, 0);
  t.j1 = min((ymax - 128) >> 8, w - 1);
  return true;
}

// edge(A, B, P) and whether a centre ON the edge A -> B belongs to the face (top-left rule)
__device__ __forceinline__ bool raster_edge(long long ax, long long ay, long long bx, long long by, long long px,
                                            long long py, long long &e) {
  const long long dx = bx - ax, dy = by - ay;
  e = dx * (py - ay) - dy * (px - ax);
  return e > 0 || (e == 0 && (dy < 0 || (dy == 0 && dx > 0)));
}

// coverage of the centre of pixel (i, j) and its edge values
__device__ __forceinline__ bool raster_cover(const RasterTri &t, int i, int j, long long e[3]) {
  const long long px = 256LL * i + 128, py = 256LL * j + 128;
  const bool c0 = raster_edge(t.x[1], t.y[1], t.x[2], t.y[2], px, py, e[0]);
  const bool c1 = raster_edge(t.x[2], t.y[2], t.x[0], t.y[0], px, py, e[1]);
  const bool c2 = raster_edge(t.x[0], t.y[0], t.x[1], t.y[1], px, py, e[2]);
  return c0 && c1 && c2;
}

// the barycentrics of the fragment and its depth: the one place both the face kernels and the resolve take them from
__device__ __forceinline__ float raster_weights(const RasterTri &t, const long long e[3], float w[3]) {
  const float a = (float)t.area2;
#pragma unroll
  for (int k = 0; k < 3; ++k) w[k] = (float)e[k] / a;
  return (w[0] * t.z[0] + w[1] * t.z[1]) + w[2] * t.z[2];
}

// step 5's key maximum of one fragment
__device__ __forceinline__ void raster_emit(float depth, int i, int j, uint32_t face, int nearest,
                                            unsigned long long *__restrict__ keys, int w) {
  if (!__builtin_isfinite(depth)) return;
  const float d = nearest == MP_NEAREST_MIN_Z ? -depth : depth;
  const unsigned long long key =
      ((unsigned long long)orderable(__float_as_uint(d)) << 32) | (unsigned long long)(0xFFFFFFFFu - face);
  unsigned long long *p = keys + (long long)i * w + j;
  if (*p >= key) return;  // early z: keys only grow
  atomicMax(p, key);
}

__device__ __forceinline__ void raster_fragment(const RasterTri &t, int i, int j, uint32_t face, int nearest,
                                                unsigned long long *__restrict__ keys, int w) {
  long long e[3];
  if (!raster_cover(t, i, j, e)) return;
  float wt[3];
  raster_emit(raster_weights(t, e, wt), i, j, face, nearest, keys, w);
}

__global__ __launch_bounds__(kRasterBlock) void raster_faces(RasterMeshes fr, RasterScratch sc, int nearest) {
  const int s = blockIdx.y;
  const int32_t *__restrict__ counts = fr.counts[s];
  const int nf = raster_min(counts[1], sc.max_f);
  const long long f = (long long)blockIdx.x * kRasterBlock + threadIdx.x;
  if (f >= nf) return;
  const int nv = raster_min(counts[0], sc.max_v);
  RasterTri t;
  if (!raster_load_tri(fr.faces[s], sc.image_verts(s), f, nv, sc.h, sc.w, t)) return;
  if (t.i0 > t.i1 || t.j0 > t.j1) return;
  const long long box = (long long)(t.i1 - t.i0 + 1) * (t.j1 - t.j0 + 1);
  if (box > kSmallBox) {
    sc.image_list(s)[atomicAdd(&sc.n_large[s], 1)] = (int)f;  // at most once per face: the list holds max_f
    return;
  }
  unsigned long long *__restrict__ keys = sc.image_keys(s);
  for (int i = t.i0; i <= t.i1; ++i)
    for (int j = t.j0; j <= t.j1; ++j) raster_fragment(t, i, j, (uint32_t)f, nearest, keys, sc.w);
}

__global__ __launch_bounds__(kRasterBlock) void raster_large(RasterMeshes fr, RasterScratch sc, int nearest) {
  const int s = blockIdx.y;
  const int n = min(sc.n_large[s], (int)min(sc.max_f, (long long)0x7fffffff));
  if ((int)blockIdx.x >= n) return;
  const int32_t *__restrict__ counts = fr.counts[s];
  const int nv = raster_min(counts[0], sc.max_v);
  const int *__restrict__ list = sc.image_list(s);
  unsigned long long *__restrict__ keys = sc.image_keys(s);
  for (int k = blockIdx.x; k < n; k += gridDim.x) {
    const int f = list[k];
    RasterTri t;
    if (!raster_load_tri(fr.faces[s], sc.image_verts(s), f, nv, sc.h, sc.w, t)) continue;  // listed faces pass
    const int nj = t.j1 - t.j0 + 1;
    const long long box = (long long)(t.i1 - t.i0 + 1) * nj;
    for (long long p = threadIdx.x; p < box; p += kRasterBlock)
      raster_fragment(t, t.i0 + (int)(p / nj), t.j0 + (int)(p % nj), (uint32_t)f, nearest, keys, sc.w);
  }
}

__global__ __launch_bounds__(kRasterBlock) void raster_resolve(RasterMeshes fr, RasterOut out, RasterScratch sc,
                                                               int ch_major, float scale, float bias, float lo,
                                                               float hi, float background) {
  const int s = blockIdx.y;
  const long long p = (long long)blockIdx.x * kRasterBlock + threadIdx.x;
  if (p >= sc.hw) return;
  float *__restrict__ image = out.image[s];
  float *__restrict__ depth = out.depth[s];
  int32_t *__restrict__ face = out.face[s];
  const unsigned long long key = sc.image_keys(s)[p];
  RasterTri t;
  bool hit = key != 0;
  const long long f = (long long)(0xFFFFFFFFu - (uint32_t)key);
  if (hit) {  // a key names a face that passed every test in raster_faces; the same tests, never a read out of bounds
    const int32_t *__restrict__ counts = fr.counts[s];
    hit = f < raster_min(counts[1], sc.max_f) &&
          raster_load_tri(fr.faces[s], sc.image_verts(s), f, raster_min(counts[0], sc.max_v), sc.h, sc.w, t);
  }
  if (!hit) {
    if (image) image[3 * p + 0] = background, image[3 * p + 1] = background, image[3 * p + 2] = background;
    if (depth) depth[p] = 0.0f;
    if (face) face[p] = -1;
    return;
  }
  long long e[3];
  float wt[3];
  raster_cover(t, (int)(p / sc.w), (int)(p % sc.w), e);
  const float d = raster_weights(t, e, wt);
  if (depth) depth[p] = d;
  if (face) face[p] = (int32_t)f;
  if (image) {
    const float *__restrict__ attr = out.attr[s];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float a[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) a[k] = ch_major ? attr[c * sc.max_v + t.idx[k]] : attr[3 * (long long)t.idx[k] + c];
      float o = (wt[0] * a[0] + wt[1] * a[1]) + wt[2] * a[2];
      o = o * scale + bias;
      o = o < lo ? lo : (o > hi ? hi : o);
      image[3 * p + c] = o;
    }
  }
}

// ---- the clipped form (mp_mesh_render_clip): near-plane clipping and perspective-correct interpolation -----------------
// Stateless: no clipped geometry is stored.  A face thread clips its own face in registers (raster_clip_face) and the
// resolve re-derives the same sub-triangles from the face index in the key, with the same device functions.  What the
// clipped kernels take on top of the unclipped ones travels in a RasterClip of their own, so the four kernels above
// keep their argument blocks.
struct RasterClip {
  float4 *cam;        // n x [max_v] camera-space vertices (xc, yc, zc, -): the rows of project() before the divide
  long long max_v;
  float near;
  int pc;  // MP_RENDER_PERSPECTIVE_CORRECT
  __device__ float4 *image_cam(int s) const { return cam + max_v * s; }
};
static_assert(sizeof(RasterMeshes) + sizeof(RasterCams) + sizeof(RasterClip) + 256 <= 4096,
              "raster_setup_clip: kernel arguments");
static_assert(sizeof(RasterMeshes) + sizeof(RasterOut) + sizeof(RasterClip) + 256 <= 4096,
              "raster_resolve_clip: kernel arguments");

// step 2 of a cut vertex (raster_setup's expressions)
__device__ __forceinline__ bool raster_snap(float x, float y, float z, int h, int w, int &X, int &Y) {
  const float u = ((x + 1.0f) * (0.5f * (float)h)) * 256.0f;
  const float t = ((y + 1.0f) * (0.5f * (float)w)) * 256.0f;
  const bool ok = __builtin_isfinite(u) && __builtin_isfinite(t) && __builtin_isfinite(z) &&
                  !(fabsf(u) > kSnapGuard) && !(fabsf(t) > kSnapGuard);
  X = ok ? (int)rintf(u) : 0;
  Y = ok ? (int)rintf(t) : 0;
  return ok;
}

__global__ __launch_bounds__(kRasterBlock) void raster_setup_clip(RasterMeshes fr, RasterCams cams, RasterScratch sc,
                                                                  RasterClip cl) {
  const int s = blockIdx.y;
  const int nv = raster_min(fr.counts[s][0], sc.max_v);
  const long long v = (long long)blockIdx.x * kRasterBlock + threadIdx.x;
  if (v >= nv) return;
  const float *__restrict__ verts = fr.verts[s];
  float4 c;
  project(cams.cal[s], verts[3 * v + 0], verts[3 * v + 1], verts[3 * v + 2], c.x, c.y, c.z);
  c.w = 0.0f;
  cl.image_cam(s)[v] = c;
  int4 o;
  o.w = raster_snap(__fdiv_rn(c.x, c.z), __fdiv_rn(c.y, c.z), c.z, sc.h, sc.w, o.x, o.y) ? 1 : 0;  // project_mode
  o.z = __float_as_int(c.z);
  sc.image_verts(s)[v] = o;
}

// A vertex of a sub-triangle: the mesh's vertex `in` itself (out < 0), or cut(in, out) at parameter t
struct ClipVert {
  int x, y;
  float z;
  int in, out;
  float t;
};
// A sub-triangle ready to be covered; tri.idx[k] is the `in` of its vertex k
struct ClipTri {
  RasterTri tri;
  int out[3];
  float t[3];
};

__device__ __forceinline__ bool clip_own(const int4 *__restrict__ snapped, int idx, ClipVert &v) {
  const int4 p = snapped[idx];
  v.x = p.x, v.y = p.y, v.z = __int_as_float(p.z), v.in = idx, v.out = -1, v.t = 0.0f;
  return p.w != 0;
}

// cut(I, O): from the inside vertex to the outside one, so that two faces sharing the edge compute the same bits
__device__ __forceinline__ bool clip_cut(const float4 &I, int i, const float4 &O, int o, float near, int h, int w,
                                         ClipVert &v) {
  const float t = (near - I.z) / (O.z - I.z);
  const float xc = I.x + t * (O.x - I.x);
  const float yc = I.y + t * (O.y - I.y);
  v.z = near, v.in = i, v.out = o, v.t = t;
  return raster_snap(xc / near, yc / near, near, h, w, v.x, v.y);
}

// step 3's area2, orientation exchange and box of one sub-triangle; false: zero area
__device__ __forceinline__ bool clip_tri(const ClipVert &a, ClipVert b, ClipVert c, int h, int w, ClipTri &o) {
  long long area2 = (long long)(b.x - a.x) * (long long)(c.y - a.y) - (long long)(b.y - a.y) * (long long)(c.x - a.x);
  if (area2 == 0) return false;
  if (area2 < 0) {
    const ClipVert q = b;
    b = c;
    c = q;
    area2 = -area2;
  }
  RasterTri &t = o.tri;
  t.area2 = area2;
  t.x[0] = a.x, t.y[0] = a.y, t.z[0] = a.z, t.idx[0] = a.in, o.out[0] = a.out, o.t[0] = a.t;
  t.x[1] = b.x, t.y[1] = b.y, t.z[1] = b.z, t.idx[1] = b.in, o.out[1] = b.out, o.t[1] = b.t;
  t.x[2] = c.x, t.y[2] = c.y, t.z[2] = c.z, t.idx[2] = c.in, o.out[2] = c.out, o.t[2] = c.t;
  const int xmin = min(a.x, min(b.x, c.x)), xmax = max(a.x, max(b.x, c.x));
  const int ymin = min(a.y, min(b.y, c.y)), ymax = max(a.y, max(b.y, c.y));
  t.i0 = max((xmin - 128 + 255) >> 8, 0);
  t.i1 = min((xmax - 128) >> 8, h - 1);
  t.j0 = max((ymin - 128 + 255) >> 8, 0);
  t.j1 = min((ymax - 128) >> 8, w - 1);
  return true;
}

// The sub-triangles of face f in front of the near plane: bit k of the result says that sub[k] is to be covered; 0: the
// face is skipped (an index outside [0, nv), a non-finite camera coordinate, no vertex inside, an invalid inside or cut
// vertex, zero area).
__device__ __forceinline__ int raster_clip_face(const int32_t *__restrict__ faces, const int4 *__restrict__ snapped,
                                                const float4 *__restrict__ cam, long long f, int nv, int h, int w,
                                                float near, ClipTri sub[2]) {
  int i0 = faces[3 * f + 0], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
  if (i0 < 0 || i0 >= nv || i1 < 0 || i1 >= nv || i2 < 0 || i2 >= nv) return 0;
  float4 p0 = cam[i0], p1 = cam[i1], p2 = cam[i2];
  auto finite = [](const float4 &p) {
    return __builtin_isfinite(p.x) && __builtin_isfinite(p.y) && __builtin_isfinite(p.z);
  };
  if (!(finite(p0) && finite(p1) && finite(p2))) return 0;
  const bool in0 = p0.z >= near, in1 = p1.z >= near, in2 = p2.z >= near;
  const int n_in = (int)in0 + (int)in1 + (int)in2;
  if (n_in == 0) return 0;
  ClipVert a, b, c;
  if (n_in == 3) {
    if (!clip_own(snapped, i0, a) || !clip_own(snapped, i1, b) || !clip_own(snapped, i2, c)) return 0;
    return clip_tri(a, b, c, h, w, sub[0]) ? 1 : 0;
  }
  // rotate cyclically: one inside -> it comes first; two inside -> the outside one comes last
  const int r = n_in == 1 ? (in0 ? 0 : (in1 ? 1 : 2)) : (!in2 ? 0 : (!in0 ? 1 : 2));
  for (int k = 0; k < 2; ++k)
    if (r > k) {
      const float4 q = p0;
      p0 = p1, p1 = p2, p2 = q;
      const int j = i0;
      i0 = i1, i1 = i2, i2 = j;
    }
  if (!clip_own(snapped, i0, a)) return 0;
  if (n_in == 1) {  // (A, P, Q), P = cut(A, B), Q = cut(A, C)
    if (!clip_cut(p0, i0, p1, i1, near, h, w, b) || !clip_cut(p0, i0, p2, i2, near, h, w, c)) return 0;
    return clip_tri(a, b, c, h, w, sub[0]) ? 1 : 0;
  }
  ClipVert q;  // (A, B, P) and (A, P, Q), P = cut(B, C), Q = cut(A, C)
  if (!clip_own(snapped, i1, b)) return 0;
  if (!clip_cut(p1, i1, p2, i2, near, h, w, c) || !clip_cut(p0, i0, p2, i2, near, h, w, q)) return 0;
  return (clip_tri(a, b, c, h, w, sub[0]) ? 1 : 0) | (clip_tri(a, c, q, h, w, sub[1]) ? 2 : 0);
}

// step 4 of the clipped form: the factors q_k an attribute is summed with, what the sum is divided by under
// MP_RENDER_PERSPECTIVE_CORRECT (s), and the depth
__device__ __forceinline__ float raster_weights_clip(const RasterTri &t, const long long e[3], int pc, float q[3],
                                                     float &s) {
  const float depth = raster_weights(t, e, q);
  s = 1.0f;
  if (!pc) return depth;
#pragma unroll
  for (int k = 0; k < 3; ++k) q[k] = q[k] / t.z[k];
  s = (q[0] + q[1]) + q[2];
  return 1.0f / s;
}

__device__ __forceinline__ void raster_fragment_clip(const RasterTri &t, int i, int j, uint32_t face, int nearest,
                                                     int pc, unsigned long long *__restrict__ keys, int w) {
  long long e[3];
  if (!raster_cover(t, i, j, e)) return;
  float q[3], s;
  const float depth = raster_weights_clip(t, e, pc, q, s);
  raster_emit(depth, i, j, face, nearest, keys, w);
}

__global__ __launch_bounds__(kRasterBlock) void raster_faces_clip(RasterMeshes fr, RasterScratch sc, RasterClip cl,
                                                                  int nearest) {
  const int s = blockIdx.y;
  const int32_t *__restrict__ counts = fr.counts[s];
  const int nf = raster_min(counts[1], sc.max_f);
  const long long f = (long long)blockIdx.x * kRasterBlock + threadIdx.x;
  if (f >= nf) return;
  const int nv = raster_min(counts[0], sc.max_v);
  ClipTri sub[2];
  const int live = raster_clip_face(fr.faces[s], sc.image_verts(s), cl.image_cam(s), f, nv, sc.h, sc.w, cl.near, sub);
  long long largest = 0;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const RasterTri &t = sub[k].tri;
    if (((live >> k) & 1) && t.i0 <= t.i1 && t.j0 <= t.j1)
      largest = max(largest, (long long)(t.i1 - t.i0 + 1) * (t.j1 - t.j0 + 1));
  }
  if (largest == 0) return;
  if (largest > kSmallBox) {  // the face as a whole, at most once: raster_large_clip walks every sub-triangle of it
    sc.image_list(s)[atomicAdd(&sc.n_large[s], 1)] = (int)f;
    return;
  }
  unsigned long long *__restrict__ keys = sc.image_keys(s);
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    if (!((live >> k) & 1)) continue;
    const RasterTri &t = sub[k].tri;
    for (int i = t.i0; i <= t.i1; ++i)
      for (int j = t.j0; j <= t.j1; ++j) raster_fragment_clip(t, i, j, (uint32_t)f, nearest, cl.pc, keys, sc.w);
  }
}

__global__ __launch_bounds__(kRasterBlock) void raster_large_clip(RasterMeshes fr, RasterScratch sc, RasterClip cl,
                                                                  int nearest) {
  const int s = blockIdx.y;
  const int n = min(sc.n_large[s], (int)min(sc.max_f, (long long)0x7fffffff));
  if ((int)blockIdx.x >= n) return;
  const int32_t *__restrict__ counts = fr.counts[s];
  const int nv = raster_min(counts[0], sc.max_v);
  const int *__restrict__ list = sc.image_list(s);
  unsigned long long *__restrict__ keys = sc.image_keys(s);
  // the per-image pointers once, in front of the loop: the argument blocks need not stay live across it
  const int32_t *__restrict__ faces = fr.faces[s];
  const int4 *__restrict__ snapped = sc.image_verts(s);
  const float4 *__restrict__ cam = cl.image_cam(s);
  const int h = sc.h, w = sc.w, pc = cl.pc;
  const float near = cl.near;
  for (int k = blockIdx.x; k < n; k += gridDim.x) {
    const int f = list[k];
    ClipTri sub[2];
    const int live = raster_clip_face(faces, snapped, cam, f, nv, h, w, near, sub);
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      if (!((live >> c) & 1)) continue;
      const RasterTri &t = sub[c].tri;
      const int nj = t.j1 - t.j0 + 1;
      if (t.i0 > t.i1 || nj <= 0) continue;
      const int box = (t.i1 - t.i0 + 1) * nj;  // at most 4096 x 4096 centres
      for (int p = threadIdx.x; p < box; p += kRasterBlock)
        raster_fragment_clip(t, t.i0 + p / nj, t.j0 + p % nj, (uint32_t)f, nearest, pc, keys, w);
    }
  }
}

__global__ __launch_bounds__(kRasterBlock) void raster_resolve_clip(RasterMeshes fr, RasterOut out, RasterScratch sc,
                                                                    RasterClip cl, int ch_major, float scale,
                                                                    float bias, float lo, float hi, float background) {
  const int s = blockIdx.y;
  const long long p = (long long)blockIdx.x * kRasterBlock + threadIdx.x;
  if (p >= sc.hw) return;
  float *__restrict__ image = out.image[s];
  float *__restrict__ depth = out.depth[s];
  int32_t *__restrict__ face = out.face[s];
  const unsigned long long key = sc.image_keys(s)[p];
  const long long f = (long long)(0xFFFFFFFFu - (uint32_t)key);
  ClipTri sub[2];
  long long e[3];
  int pick = -1;  // the lowest-numbered sub-triangle of the winning face that covers this centre
  if (key != 0) {
    const int32_t *__restrict__ counts = fr.counts[s];
    int live = 0;
    if (f < raster_min(counts[1], sc.max_f))
      live = raster_clip_face(fr.faces[s], sc.image_verts(s), cl.image_cam(s), f, raster_min(counts[0], sc.max_v), sc.h,
                              sc.w, cl.near, sub);
    const int i = (int)(p / sc.w), j = (int)(p % sc.w);
    if ((live & 1) && raster_cover(sub[0].tri, i, j, e)) pick = 0;
    else if ((live & 2) && raster_cover(sub[1].tri, i, j, e)) pick = 1;
  }
  if (pick < 0) {
    if (image) image[3 * p + 0] = background, image[3 * p + 1] = background, image[3 * p + 2] = background;
    if (depth) depth[p] = 0.0f;
    if (face) face[p] = -1;
    return;
  }
  const ClipTri &t = pick ? sub[1] : sub[0];
  float q[3], sum;
  const float d = raster_weights_clip(t.tri, e, cl.pc, q, sum);
  if (depth) depth[p] = d;
  if (face) face[p] = (int32_t)f;
  if (image) {
    const float *__restrict__ attr = out.attr[s];
    auto value = [&](int v, int c) { return ch_major ? attr[c * sc.max_v + v] : attr[3 * (long long)v + c]; };
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float a[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        a[k] = value(t.tri.idx[k], c);
        if (t.out[k] >= 0) a[k] = a[k] + t.t[k] * (value(t.out[k], c) - a[k]);  // a cut vertex: aI + t (aO - aI)
      }
      float o = (q[0] * a[0] + q[1] * a[1]) + q[2] * a[2];
      if (cl.pc) o = o / sum;
      o = o * scale + bias;
      o = o < lo ? lo : (o > hi ? hi : o);
      image[3 * p + c] = o;
    }
  }
}

// the keys of n images, padded to 256 bytes so that what follows them stays aligned
static size_t raster_key_bytes(int n_images, long long hw) { return ((size_t)8 * hw * n_images + 255) & ~(size_t)255; }

// n images: keys 8 H W | snapped vertices 16 max_v [| camera-space vertices 16 max_v: the clipped form] | list 4 max_f
// each, + 256 for the list counters + the padding
size_t mesh_render_scratch_bytes(int n_images, long long max_v, long long max_f, int h, int w, bool clip) {
  return raster_key_bytes(n_images, (long long)h * w) + 256 +
         (size_t)n_images * ((size_t)(clip ? 32 : 16) * max_v + (size_t)4 * max_f);
}

int launch_mesh_render_batch(mp_ctx *ctx, void *scratch, int n_frames, int n_views, const float *const *verts,
                             long long max_v, const int32_t *const *faces, long long max_f,
                             const int32_t *const *counts, const float *const *attr, int ch_major, const float *calibs,
                             int proj, int nearest, int h, int w, float scale, float bias, float lo, float hi,
                             float background, float *const *image, float *const *depth, int32_t *const *face_id,
                             const MeshRenderClip *clip, hipStream_t st) {
  const int n = n_frames * n_views;
  const long long hw = (long long)h * w;
  RasterMeshes fr;
  RasterCams cams;
  RasterOut out;
  std::memset(&fr, 0, sizeof(fr));
  std::memset(&cams, 0, sizeof(cams));
  std::memset(&out, 0, sizeof(out));
  for (int f = 0; f < n_frames; ++f)
    for (int v = 0; v < n_views; ++v) {
      const int s = f * n_views + v;
      fr.verts[s] = verts ? verts[f] : nullptr;
      fr.faces[s] = faces ? faces[f] : nullptr;
      fr.counts[s] = counts[f];
      out.attr[s] = attr ? attr[f] : nullptr;
      out.image[s] = image ? image[f] + 3 * hw * v : nullptr;
      out.depth[s] = depth ? depth[f] + hw * v : nullptr;
      out.face[s] = face_id ? face_id[f] + hw * v : nullptr;
      std::memcpy(cams.cal[s], calibs + 12 * (size_t)s, 12 * sizeof(float));
    }
  RasterScratch sc;
  sc.keys = static_cast<unsigned long long *>(scratch);
  sc.n_large = reinterpret_cast<int *>(static_cast<unsigned char *>(scratch) + raster_key_bytes(n, hw));
  sc.snapped = reinterpret_cast<int4 *>(reinterpret_cast<unsigned char *>(sc.n_large) + 256);
  RasterClip cl;  // the clipped form keeps its camera-space vertices between the snapped ones and the lists
  cl.cam = reinterpret_cast<float4 *>(sc.snapped + max_v * n);
  cl.max_v = max_v;
  cl.near = clip ? clip->near : 0.0f;
  cl.pc = clip ? (clip->flags & MP_RENDER_PERSPECTIVE_CORRECT) : 0;
  sc.list = clip ? reinterpret_cast<int *>(cl.cam + max_v * n) : reinterpret_cast<int *>(sc.snapped + max_v * n);
  sc.max_v = max_v;
  sc.max_f = max_f;
  sc.hw = hw;
  sc.h = h;
  sc.w = w;
  MP_HIP(ctx, hipMemsetAsync(sc.keys, 0, raster_key_bytes(n, hw) + 256, st));  // the keys and the list counters
  if (max_v > 0 && max_f > 0) {
    const dim3 vb((unsigned)((max_v + kRasterBlock - 1) / kRasterBlock), n);
    const dim3 fb((unsigned)((max_f + kRasterBlock - 1) / kRasterBlock), n);
    const dim3 lb((unsigned)(max_f < kLargeBlocks ? max_f : kLargeBlocks), n);
    if (clip) {
      hipLaunchKernelGGL(raster_setup_clip, vb, dim3(kRasterBlock), 0, st, fr, cams, sc, cl);
      hipLaunchKernelGGL(raster_faces_clip, fb, dim3(kRasterBlock), 0, st, fr, sc, cl, nearest);
      hipLaunchKernelGGL(raster_large_clip, lb, dim3(kRasterBlock), 0, st, fr, sc, cl, nearest);
    } else {
      hipLaunchKernelGGL(raster_setup, vb, dim3(kRasterBlock), 0, st, fr, cams, sc, proj);
      hipLaunchKernelGGL(raster_faces, fb, dim3(kRasterBlock), 0, st, fr, sc, nearest);
      hipLaunchKernelGGL(raster_large, lb, dim3(kRasterBlock), 0, st, fr, sc, nearest);
    }
  }
  const dim3 pb((unsigned)((hw + kRasterBlock - 1) / kRasterBlock), n);
  if (clip)
    hipLaunchKernelGGL(raster_resolve_clip, pb, dim3(kRasterBlock), 0, st, fr, out, sc, cl, ch_major, scale, bias, lo,
                       hi, background);
  else
    hipLaunchKernelGGL(raster_resolve, pb, dim3(kRasterBlock), 0, st, fr, out, sc, ch_major, scale, bias, lo, hi,
                       background);
  MP_HIP(ctx, hipGetLastError());
  return MP_OK;
}

}  // namespace mp
