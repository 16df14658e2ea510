// Binary glTF on the device (mp_mesh_glb[_batch], include/monoport_hip.h): the meshes of up to kMaxFrames frames as the
// chain leaves them -> one quantised .glb file per frame at out + f * capacity, info [f] = {bytes, overflowed}.  No
// entropy coder: the file's size is a closed form of (nv, nf, attribute set), so every kernel derives the whole layout
// from the frame's counts and nothing but the positions' extremes passes between them.
//   glb_layout_kernel   one wave per frame: info, and the extremes reset to (65535, 0) in each of the frame's kGlbSlots
//                       slots -- the only scratch of the call, written here before anything reads it
//   glb_pack_kernel     blockIdx.y = frame, thread i: vertex i -> one 8-byte position, one dword per normal and per
//                       colour; the extremes of the wave by shuffles, then integer atomicMin / atomicMax of lane 0 into
//                       the wave's slot (its number modulo kGlbSlots) where the wave improves on what it reads (a stale
//                       read is never below the minimum: skipping is safe).  Marching cubes emits vertices in z order,
//                       so along one axis EVERY wave improves on the one before it: on one word per frame those
//                       atomics are a chain of 1,344 at 257^3 and were the whole run time; over 64 slots, each on a
//                       cache line of its own, they are 21.  Then faces 2 i and 2 i + 1 -> three dwords of 16-bit
//                       indices, or face i -> three dwords of 32-bit ones
//   glb_header_kernel   one workgroup per frame: the slots joined by one wave, the header, the JSON text from the
//                       host's template with its numbers formatted in LDS, the BIN chunk's header; or the fixed empty
//                       file
// A frame whose file exceeds the capacity is left by the last two kernels before their first store.  A row of `out`
// that is not 4-byte aligned in memory (an odd capacity) is written byte by byte.
// Every float operation is one IEEE f32 operation in the order the header states.
// The textured file (mp_mesh_glb_textured[_batch]) is the same three kernels over another layout: the second half of
// this file.
#include "mp_internal.h"
#include "mesh_common.h"

#include <cstdio>
#include <cstring>
#include <string>

#pragma clang fp contract(off)

namespace mp {

constexpr int kGlbBlock = 256;
constexpr int kGlbJsonMax = 1792;  // the padded text of the largest attribute set (launch_mesh_glb_batch checks)
constexpr int kGlbHolesMax = 24;
constexpr int kGlbPrefix = 20;     // file header + JSON chunk header
constexpr int kGlbEmptyWords = MP_GLB_MIN_BYTES / 4;
constexpr int kGlbSlots = 64;      // partial extremes per frame, joined by the header kernel's first wave
constexpr int kGlbSlotInts = 32;   // a slot is a 128-byte line: min x y z, max x y z, the rest spare
static_assert(MP_GLB_MIN_BYTES % 4 == 0, "the empty file is copied in dwords");

// the numbers the device fills in
enum GlbHole { kHoleNv, kHoleNi, kHoleCt, kHoleMin, kHoleMax = kHoleMin + 3, kHolePosOff = kHoleMax + 3, kHolePosLen,
               kHoleNrmOff, kHoleNrmLen, kHoleColOff, kHoleColLen, kHoleIdxOff, kHoleIdxLen, kHoleBin };

struct GlbFrames {
  const float *verts[kMaxFrames];
  const int32_t *faces[kMaxFrames];
  const int32_t *counts[kMaxFrames];
  const float *normals[kMaxFrames];  // all nullptr without MP_GLB_NORMALS
  const float *colors[kMaxFrames];   // all nullptr without MP_GLB_COLORS
};
struct GlbGeom {
  long long max_v, max_f, capacity;
  int flags, color_planes, json_len;  // json_len: the padded text, % 8 == 4
  float color_scale, color_bias, b_min[3], inv[3];
  uint8_t *out;
  int32_t *info;
  int *state;  // [n_frames][kGlbSlots][kGlbSlotInts]: min x y z, max x y z in front of every slot
};
struct GlbHoleAt {
  uint16_t at;  // offset in the text
  uint8_t width, kind;
};
struct GlbTemplate {
  uint32_t json[kGlbJsonMax / 4];
  uint32_t empty[kGlbEmptyWords];
  GlbHoleAt holes[kGlbHolesMax];
  int n_holes;
};
static_assert(sizeof(GlbFrames) + sizeof(GlbGeom) + sizeof(GlbTemplate) + 64 <= 4096, "mp_mesh_glb: kernel arguments");

// where everything lies in the file of a mesh of nv vertices and nf faces
struct GlbLayout {
  int nv, nf, wide, empty;
  long long off_n, off_c, off_i, idx_bytes, bin, total;
};
__host__ __device__ inline GlbLayout glb_layout(long long nv, long long nf, int flags, int json_len) {
  GlbLayout l;
  l.nv = (int)nv, l.nf = (int)nf;
  l.empty = nv == 0 || nf == 0;
  l.wide = nv > 65535;
  l.off_n = 8 * nv;
  l.off_c = l.off_n + ((flags & MP_GLB_NORMALS) ? 4 * nv : 0);
  l.off_i = l.off_c + ((flags & MP_GLB_COLORS) ? 4 * nv : 0);
  l.idx_bytes = (l.wide ? 12 : 6) * nf;
  l.bin = (l.off_i + l.idx_bytes + 3) & ~3LL;
  l.total = l.empty ? MP_GLB_MIN_BYTES : kGlbPrefix + json_len + 8 + l.bin;
  return l;
}

__device__ __forceinline__ GlbLayout glb_frame_layout(const GlbFrames &fr, const GlbGeom &g, int f) {
  const int32_t *__restrict__ counts = fr.counts[f];
  return glb_layout(mesh_min(counts[0], g.max_v), mesh_min(counts[1], g.max_f), g.flags, g.json_len);
}

struct __attribute__((packed, aligned(4))) GlbPair {
  uint32_t lo, hi;
};
__device__ __forceinline__ void put32(uint8_t *p, uint32_t v, bool dwords) {
  if (dwords) {
    *reinterpret_cast<uint32_t *>(p) = v;
  } else {
    p[0] = (uint8_t)v, p[1] = (uint8_t)(v >> 8), p[2] = (uint8_t)(v >> 16), p[3] = (uint8_t)(v >> 24);
  }
}
__device__ __forceinline__ void put64(uint8_t *p, uint32_t lo, uint32_t hi, bool dwords) {
  if (dwords) {
    *reinterpret_cast<GlbPair *>(p) = GlbPair{lo, hi};
  } else {
    put32(p, lo, false);
    put32(p + 4, hi, false);
  }
}

__device__ __forceinline__ int glb_position(float x, float b_min, float inv) {
  const float d = x - b_min;
  const float t = d * inv;
  return t > 0.0f ? (t < 65535.0f ? (int)(t + 0.5f) : 65535) : 0;
}
__device__ __forceinline__ uint32_t glb_normal(float n) {
  const float t = n != n ? 0.0f : (n > -1.0f ? (n < 1.0f ? n : 1.0f) : -1.0f);
  const float m = t * 127.0f;
  return (uint32_t)(int)(m + (t < 0.0f ? -0.5f : 0.5f)) & 0xffu;
}
__device__ __forceinline__ uint32_t glb_colour(float p, float scale, float bias) {
  const float s = p * scale;
  const float c = s + bias;
  const float t = c > 0.0f ? (c < 1.0f ? c : 1.0f) : 0.0f;  // step 1 of the JPEG definition
  const float m = t * 255.0f;
  return (uint32_t)(int)(m + 0.5f);
}
__device__ __forceinline__ uint32_t glb_index(int i, int nv) { return (uint32_t)(i < 0 ? 0 : (i >= nv ? nv - 1 : i)); }

__global__ __launch_bounds__(kGlbSlots) void glb_layout_kernel(GlbFrames fr, GlbGeom g) {
  const int f = blockIdx.x;
  if (threadIdx.x == 0) {
    const GlbLayout l = glb_frame_layout(fr, g, f);
    g.info[2 * f + 0] = (int32_t)l.total;
    g.info[2 * f + 1] = l.total > g.capacity;
  }
  int *__restrict__ st = g.state + ((long long)f * kGlbSlots + threadIdx.x) * kGlbSlotInts;
#pragma unroll
  for (int k = 0; k < 3; ++k) st[k] = 65535, st[3 + k] = 0;
}

__global__ __launch_bounds__(kGlbBlock) void glb_pack_kernel(GlbFrames fr, GlbGeom g) {
  const int f = blockIdx.y;
  const GlbLayout l = glb_frame_layout(fr, g, f);
  if (l.empty || l.total > g.capacity) return;
  const long long i = (long long)blockIdx.x * kGlbBlock + threadIdx.x;
  const long long first = (long long)blockIdx.x * kGlbBlock;
  const int nv = l.nv, nf = l.nf;
  const int face_items = l.wide ? nf : (nf + 1) >> 1;
  if (first >= nv && first >= face_items) return;
  uint8_t *row = g.out + (long long)f * g.capacity;
  const bool dwords = ((uintptr_t)row & 3u) == 0;
  uint8_t *bin = row + kGlbPrefix + g.json_len + 8;

  if (first + (threadIdx.x & ~63u) < nv) {  // the wave holds vertices
    int lo[3] = {65535, 65535, 65535}, hi[3] = {0, 0, 0};
    if (i < nv) {
      const float *__restrict__ verts = fr.verts[f];
      int q[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) lo[k] = hi[k] = q[k] = glb_position(verts[3 * i + k], g.b_min[k], g.inv[k]);
      put64(bin + 8 * i, (uint32_t)q[0] | ((uint32_t)q[1] << 16), (uint32_t)q[2], dwords);
      if (g.flags & MP_GLB_NORMALS) {
        const float *__restrict__ nrm = fr.normals[f];
        put32(bin + l.off_n + 4 * i,
              glb_normal(nrm[3 * i + 0]) | (glb_normal(nrm[3 * i + 1]) << 8) | (glb_normal(nrm[3 * i + 2]) << 16),
              dwords);
      }
      if (g.flags & MP_GLB_COLORS) {
        const float *__restrict__ col = fr.colors[f];
        const long long s = g.color_planes ? g.max_v : 1, e = g.color_planes ? 1 : 3;
        put32(bin + l.off_c + 4 * i,
              glb_colour(col[e * i], g.color_scale, g.color_bias) |
                  (glb_colour(col[e * i + s], g.color_scale, g.color_bias) << 8) |
                  (glb_colour(col[e * i + 2 * s], g.color_scale, g.color_bias) << 16),
              dwords);
      }
    }
    // the wave's extremes (lanes beyond nv hold the neutral values), then one lane's integer atomics
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const int a = __shfl_xor(lo[k], o), b = __shfl_xor(hi[k], o);
        lo[k] = a < lo[k] ? a : lo[k];
        hi[k] = b > hi[k] ? b : hi[k];
      }
    }
    if ((threadIdx.x & 63) == 0) {
      const int wave = blockIdx.x * (kGlbBlock / 64) + (threadIdx.x >> 6);
      int *st = g.state + ((long long)f * kGlbSlots + (wave & (kGlbSlots - 1))) * kGlbSlotInts;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        if (lo[k] < __atomic_load_n(&st[k], __ATOMIC_RELAXED)) atomicMin(&st[k], lo[k]);
        if (hi[k] > __atomic_load_n(&st[3 + k], __ATOMIC_RELAXED)) atomicMax(&st[3 + k], hi[k]);
      }
    }
  }

  if (i >= face_items) return;
  const int32_t *__restrict__ faces = fr.faces[f];
  if (l.wide) {
    uint8_t *p = bin + l.off_i + 12 * i;
#pragma unroll
    for (int k = 0; k < 3; ++k) put32(p + 4 * k, glb_index(faces[3 * i + k], nv), dwords);
    return;
  }
  const bool two = 2 * i + 1 < nf;  // an odd nf: the last lane has one face and the two bytes of padding
  uint32_t c[6];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    c[k] = glb_index(faces[6 * i + k], nv);
    c[3 + k] = two ? glb_index(faces[6 * i + 3 + k], nv) : 0u;
  }
  uint8_t *p = bin + l.off_i + 12 * i;
  put32(p, c[0] | (c[1] << 16), dwords);
  put32(p + 4, c[2] | (c[3] << 16), dwords);
  if (two) put32(p + 8, c[4] | (c[5] << 16), dwords);
}

__device__ __forceinline__ long long glb_hole_value(int kind, const GlbLayout &l, const int *ext) {
  switch (kind) {
    case kHoleNv: return l.nv;
    case kHoleNi: return 3LL * l.nf;
    case kHoleCt: return l.wide ? 5125 : 5123;
    case kHolePosOff: return 0;
    case kHolePosLen: return l.off_n;
    case kHoleNrmOff: return l.off_n;
    case kHoleNrmLen: return 4LL * l.nv;
    case kHoleColOff: return l.off_c;
    case kHoleColLen: return 4LL * l.nv;
    case kHoleIdxOff: return l.off_i;
    case kHoleIdxLen: return l.idx_bytes;
    case kHoleBin: return l.bin;
    default: return ext[kind - kHoleMin];  // kHoleMin .. kHoleMax + 2
  }
}

__global__ __launch_bounds__(kGlbBlock) void glb_header_kernel(GlbFrames fr, GlbGeom g, GlbTemplate tp) {
  __shared__ uint32_t file[(kGlbPrefix + kGlbJsonMax + 8) / 4];
  __shared__ int ext[6];  // min x y z, max x y z over the frame's slots
  const int f = blockIdx.x;
  const GlbLayout l = glb_frame_layout(fr, g, f);
  if (l.total > g.capacity) return;
  uint8_t *row = g.out + (long long)f * g.capacity;
  const bool dwords = ((uintptr_t)row & 3u) == 0;
  if (l.empty) {
    for (int i = threadIdx.x; i < kGlbEmptyWords; i += kGlbBlock) put32(row + 4 * i, tp.empty[i], dwords);
    return;
  }
  if (threadIdx.x < kGlbSlots) {  // the first wave joins the slots
    const int *__restrict__ st = g.state + ((long long)f * kGlbSlots + threadIdx.x) * kGlbSlotInts;
    int lo[3], hi[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) lo[k] = st[k], hi[k] = st[3 + k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const int a = __shfl_xor(lo[k], o), b = __shfl_xor(hi[k], o);
        lo[k] = a < lo[k] ? a : lo[k];
        hi[k] = b > hi[k] ? b : hi[k];
      }
    }
    if (threadIdx.x == 0) {
#pragma unroll
      for (int k = 0; k < 3; ++k) ext[k] = lo[k], ext[3 + k] = hi[k];
    }
  }
  const int json_words = g.json_len / 4;
  for (int i = threadIdx.x; i < json_words; i += kGlbBlock) file[kGlbPrefix / 4 + i] = tp.json[i];
  if (threadIdx.x == 0) {
    file[0] = 0x46546C67u;  // "glTF"
    file[1] = 2u;
    file[2] = (uint32_t)l.total;
    file[3] = (uint32_t)g.json_len;
    file[4] = 0x4E4F534Au;  // "JSON"
    file[kGlbPrefix / 4 + json_words] = (uint32_t)l.bin;
    file[kGlbPrefix / 4 + json_words + 1] = 0x004E4942u;  // "BIN\0"
  }
  __syncthreads();
  if ((int)threadIdx.x < tp.n_holes) {
    const GlbHoleAt h = tp.holes[threadIdx.x];
    long long v = glb_hole_value(h.kind, l, ext);
    uint8_t *text = reinterpret_cast<uint8_t *>(file) + kGlbPrefix + h.at;
    for (int j = h.width - 1; j >= 0; --j) {  // right-aligned, leading spaces
      text[j] = (v > 0 || j == h.width - 1) ? (uint8_t)('0' + v % 10) : (uint8_t)' ';
      v /= 10;
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kGlbPrefix / 4 + json_words + 2; i += kGlbBlock) put32(row + 4 * i, file[i], dwords);
}

// ---- host: the text of one call -------------------------------------------------------------------------------------
namespace {

struct GlbText {
  std::string s;
  GlbHoleAt holes[kGlbHolesMax];
  int n_holes = 0;
  void put(const char *t) { s += t; }
  void hole(int kind, int width) {
    holes[n_holes++] = GlbHoleAt{(uint16_t)s.size(), (uint8_t)width, (uint8_t)kind};
    s.append((size_t)width, ' ');
  }
  void real(double v) {
    char buf[64];
    snprintf(buf, sizeof(buf), "%24.17g", v);
    s += buf;
  }
  void integer(int v) { s += std::to_string(v); }
};

const char *const kGlbAsset = "{\"asset\":{\"version\":\"2.0\",\"generator\":\"monoport_amd\"}";

// the JSON text of a mesh under `flags` with its holes, padded to a length % 8 == 4
GlbText glb_text(int flags, const float *b_min, const float *b_max) {
  const bool nrm = flags & MP_GLB_NORMALS, col = flags & MP_GLB_COLORS;
  const int k = 1 + nrm + col;
  GlbText t;
  t.put(kGlbAsset);
  t.put(",\"extensionsUsed\":[\"KHR_mesh_quantization\"],\"extensionsRequired\":[\"KHR_mesh_quantization\"]");
  t.put(",\"scene\":0,\"scenes\":[{\"nodes\":[0]}],\"nodes\":[{\"mesh\":0,\"translation\":[");
  for (int a = 0; a < 3; ++a) t.put(a ? "," : ""), t.real((double)b_min[a]);
  t.put("],\"scale\":[");
  for (int a = 0; a < 3; ++a) t.put(a ? "," : ""), t.real(((double)b_max[a] - (double)b_min[a]) / 65535.0);
  t.put("]}],\"materials\":[{\"doubleSided\":true}],\"meshes\":[{\"primitives\":[{\"attributes\":{\"POSITION\":0");
  if (nrm) t.put(",\"NORMAL\":1");
  if (col) t.put(",\"COLOR_0\":"), t.integer(k - 1);
  t.put("},\"indices\":"), t.integer(k);
  t.put(",\"material\":0,\"mode\":4}]}],\"accessors\":[{\"bufferView\":0,\"componentType\":5123,\"count\":");
  t.hole(kHoleNv, 10);
  t.put(",\"type\":\"VEC3\",\"min\":[");
  for (int a = 0; a < 3; ++a) t.put(a ? "," : ""), t.hole(kHoleMin + a, 5);
  t.put("],\"max\":[");
  for (int a = 0; a < 3; ++a) t.put(a ? "," : ""), t.hole(kHoleMax + a, 5);
  t.put("]}");
  if (nrm) {
    t.put(",{\"bufferView\":1,\"componentType\":5120,\"normalized\":true,\"count\":");
    t.hole(kHoleNv, 10);
    t.put(",\"type\":\"VEC3\"}");
  }
  if (col) {
    t.put(",{\"bufferView\":"), t.integer(k - 1);
    t.put(",\"componentType\":5121,\"normalized\":true,\"count\":");
    t.hole(kHoleNv, 10);
    t.put(",\"type\":\"VEC3\"}");
  }
  t.put(",{\"bufferView\":"), t.integer(k);
  t.put(",\"componentType\":"), t.hole(kHoleCt, 4);
  t.put(",\"count\":"), t.hole(kHoleNi, 10);
  t.put(",\"type\":\"SCALAR\"}],\"bufferViews\":[");
  const int views[4][2] = {{kHolePosOff, kHolePosLen}, {kHoleNrmOff, kHoleNrmLen}, {kHoleColOff, kHoleColLen},
                           {kHoleIdxOff, kHoleIdxLen}};
  const bool present[4] = {true, nrm, col, true};
  for (int v = 0; v < 4; ++v) {
    if (!present[v]) continue;
    t.put(v ? ",{\"buffer\":0,\"byteOffset\":" : "{\"buffer\":0,\"byteOffset\":");
    t.hole(views[v][0], 10);
    t.put(",\"byteLength\":"), t.hole(views[v][1], 10);
    t.put(v == 0 ? ",\"byteStride\":8,\"target\":34962}" : v < 3 ? ",\"byteStride\":4,\"target\":34962}" : ",\"target\":34963}");
  }
  t.put("],\"buffers\":[{\"byteLength\":"), t.hole(kHoleBin, 10);
  t.put("}]}");
  t.s.append((size_t)((12 - t.s.size() % 8) % 8), ' ');
  return t;
}

// the text's length depends on the attribute set alone: every number in it has a fixed width
int glb_json_len(int flags) {
  const float lo[3] = {0, 0, 0}, hi[3] = {1, 1, 1};
  return (int)glb_text(flags, lo, hi).s.size();
}

}  // namespace

long long glb_bytes(long long nv, long long nf, int flags) { return glb_layout(nv, nf, flags, glb_json_len(flags)).total; }

size_t glb_scratch_bytes(int n_frames) { return (size_t)n_frames * kGlbSlots * kGlbSlotInts * sizeof(int); }

int launch_mesh_glb_batch(mp_ctx *ctx, void *scratch, const GlbCall &c, const float *const *verts,
                          const int32_t *const *faces, const int32_t *const *counts, const float *const *normals,
                          const float *const *colors, uint8_t *out, int32_t *info, hipStream_t st) {
  GlbFrames fr;
  std::memset(&fr, 0, sizeof(fr));
  for (int f = 0; f < c.n_frames; ++f) {
    fr.verts[f] = verts ? verts[f] : nullptr;
    fr.faces[f] = faces ? faces[f] : nullptr;
    fr.counts[f] = counts[f];
    fr.normals[f] = normals ? normals[f] : nullptr;
    fr.colors[f] = colors ? colors[f] : nullptr;
  }
  GlbGeom g;
  std::memset(&g, 0, sizeof(g));
  g.max_v = c.max_v, g.max_f = c.max_f, g.capacity = c.capacity;
  g.flags = (normals ? MP_GLB_NORMALS : 0) | (colors ? MP_GLB_COLORS : 0);
  g.color_planes = c.color_planes, g.color_scale = c.color_scale, g.color_bias = c.color_bias;
  for (int a = 0; a < 3; ++a) g.b_min[a] = c.b_min[a], g.inv[a] = c.inv[a];
  g.out = out, g.info = info, g.state = static_cast<int *>(scratch);
  const GlbText text = glb_text(g.flags, c.b_min, c.b_max);
  const std::string empty = std::string(kGlbAsset) + ",\"scene\":0,\"scenes\":[{}]}  ";
  if (text.s.size() > (size_t)kGlbJsonMax || text.s.size() % 8 != 4 || (int)text.s.size() != glb_json_len(g.flags) ||
      empty.size() != MP_GLB_MIN_BYTES - kGlbPrefix)
    return fail(ctx, MP_ERR_STATE, "mp_mesh_glb: a JSON text of %zu bytes", text.s.size());
  g.json_len = (int)text.s.size();
  GlbTemplate tp;
  std::memset(&tp, 0, sizeof(tp));
  std::memcpy(tp.json, text.s.data(), text.s.size());
  std::memcpy(tp.holes, text.holes, sizeof(text.holes));
  tp.n_holes = text.n_holes;
  const uint32_t head[5] = {0x46546C67u, 2u, MP_GLB_MIN_BYTES, MP_GLB_MIN_BYTES - kGlbPrefix, 0x4E4F534Au};
  std::memcpy(tp.empty, head, sizeof(head));
  std::memcpy(tp.empty + 5, empty.data(), empty.size());

  static_assert(kGlbSlots == 64, "one wave resets and joins a frame's slots");
  hipLaunchKernelGGL(glb_layout_kernel, dim3(c.n_frames), dim3(kGlbSlots), 0, st, fr, g);
  const long long items = c.max_v > c.max_f ? c.max_v : c.max_f;
  const dim3 grid((unsigned)((items + kGlbBlock - 1) / kGlbBlock), c.n_frames);
  if (grid.x) hipLaunchKernelGGL(glb_pack_kernel, grid, dim3(kGlbBlock), 0, st, fr, g);
  hipLaunchKernelGGL(glb_header_kernel, dim3(c.n_frames), dim3(kGlbBlock), 0, st, fr, g, tp);
  MP_HIP(ctx, hipGetLastError());
  return MP_OK;
}

// ---- the textured file (mp_mesh_glb_textured[_batch]) ---------------------------------------------------------------
// The same three kernels over another layout: 3 nf corner vertices instead of nv indexed ones, TEXCOORD_0 as the
// closed form of the atlas, and the PNG of the atlas as the last buffer view, copied by the pack kernel four bytes per
// thread.  Only the image's length, and with it the BIN chunk's, the buffer's and the file's, come from the device.
//   glb_tex_layout_kernel   info (code 2: too many faces for the atlas, or no usable image) and the extremes' reset
//   glb_tex_pack_kernel     thread i: corner i -> position, normal, UV, the extremes as above; image word i
//   glb_tex_header_kernel   the slots joined, header, JSON, BIN chunk header; or the fixed empty file
constexpr int kGlbTexJsonMax = 2048;
constexpr int kPngMinBytes = 57;  // MP_PNG_MIN_BYTES

enum GlbTexHole { kTexHoleNc, kTexHoleMin, kTexHoleMax = kTexHoleMin + 3, kTexHolePosOff = kTexHoleMax + 3,
                  kTexHolePosLen, kTexHoleNrmOff, kTexHoleNrmLen, kTexHoleUvOff, kTexHoleUvLen, kTexHoleImgOff,
                  kTexHoleImgLen, kTexHoleBin };

struct GlbTexFrames {
  const float *verts[kMaxFrames];
  const int32_t *faces[kMaxFrames];
  const int32_t *counts[kMaxFrames];
  const float *normals[kMaxFrames];  // all nullptr without MP_GLB_NORMALS
};
struct GlbTexGeom {
  long long max_v, max_f, capacity, png_capacity;
  int flags, json_len, size, cell, grid;
  float b_min[3], inv[3];
  const uint8_t *png;
  const int32_t *png_info;
  uint8_t *out;
  int32_t *info;
  int *state;
};
struct GlbTexTemplate {
  uint32_t json[kGlbTexJsonMax / 4];
  uint32_t empty[kGlbEmptyWords];
  GlbHoleAt holes[kGlbHolesMax];
  int n_holes;
};
static_assert(sizeof(GlbTexFrames) + sizeof(GlbTexGeom) + sizeof(GlbTexTemplate) + 64 <= 4096,
              "mp_mesh_glb_textured: kernel arguments");

struct GlbTexLayout {
  int nv, nf, empty, code;  // code: 0, or 2 = no file at all
  long long off_n, off_t, off_img, img, bin, total;
};
__host__ __device__ inline GlbTexLayout glb_tex_layout(long long nv, long long nf, int flags, int json_len,
                                                       long long png_bytes) {
  GlbTexLayout l;
  l.nv = (int)nv, l.nf = (int)nf;
  l.empty = nv == 0 || nf == 0;
  l.code = 0;
  l.off_n = 24 * nf;
  l.off_t = l.off_n + ((flags & MP_GLB_NORMALS) ? 12 * nf : 0);
  l.off_img = l.off_t + 24 * nf;
  l.img = png_bytes;
  l.bin = (l.off_img + l.img + 3) & ~3LL;
  l.total = l.empty ? MP_GLB_MIN_BYTES : kGlbPrefix + json_len + 8 + l.bin;
  return l;
}

__device__ __forceinline__ GlbTexLayout glb_tex_frame_layout(const GlbTexFrames &fr, const GlbTexGeom &g, int f) {
  const int32_t *__restrict__ counts = fr.counts[f];
  const int32_t *__restrict__ pi = g.png_info + 2 * f;
  const long long png_bytes = pi[0];
  GlbTexLayout l = glb_tex_layout(mesh_min(counts[0], g.max_v), mesh_min(counts[1], g.max_f), g.flags, g.json_len,
                                  png_bytes);
  if (!l.empty && (l.nf > 2LL * g.grid * g.grid || pi[1] != 0 || png_bytes < kPngMinBytes || png_bytes > g.png_capacity))
    l.code = 2, l.total = 0;
  return l;
}

__global__ __launch_bounds__(kGlbSlots) void glb_tex_layout_kernel(GlbTexFrames fr, GlbTexGeom g) {
  const int f = blockIdx.x;
  if (threadIdx.x == 0) {
    const GlbTexLayout l = glb_tex_frame_layout(fr, g, f);
    g.info[2 * f + 0] = (int32_t)l.total;
    g.info[2 * f + 1] = l.code ? l.code : (l.total > g.capacity);
  }
  int *__restrict__ st = g.state + ((long long)f * kGlbSlots + threadIdx.x) * kGlbSlotInts;
#pragma unroll
  for (int k = 0; k < 3; ++k) st[k] = 65535, st[3 + k] = 0;
}

__global__ __launch_bounds__(kGlbBlock) void glb_tex_pack_kernel(GlbTexFrames fr, GlbTexGeom g) {
  const int f = blockIdx.y;
  const GlbTexLayout l = glb_tex_frame_layout(fr, g, f);
  if (l.empty || l.code || l.total > g.capacity) return;
  const long long i = (long long)blockIdx.x * kGlbBlock + threadIdx.x;
  const long long first = (long long)blockIdx.x * kGlbBlock;
  const long long nc = 3LL * l.nf, words = (l.img + 3) >> 2;
  if (first >= nc && first >= words) return;
  uint8_t *row = g.out + (long long)f * g.capacity;
  const bool dwords = ((uintptr_t)row & 3u) == 0;
  uint8_t *bin = row + kGlbPrefix + g.json_len + 8;

  if (first + (threadIdx.x & ~63u) < nc) {  // the wave holds corners
    int lo[3] = {65535, 65535, 65535}, hi[3] = {0, 0, 0};
    if (i < nc) {
      const int face = (int)(i / 3), k = (int)(i - 3LL * face);
      const int v = (int)glb_index(fr.faces[f][i], l.nv);
      const float *__restrict__ verts = fr.verts[f];
      int q[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) lo[a] = hi[a] = q[a] = glb_position(verts[3LL * v + a], g.b_min[a], g.inv[a]);
      put64(bin + 8 * i, (uint32_t)q[0] | ((uint32_t)q[1] << 16), (uint32_t)q[2], dwords);
      if (g.flags & MP_GLB_NORMALS) {
        const float *__restrict__ nrm = fr.normals[f];
        put32(bin + l.off_n + 4 * i,
              glb_normal(nrm[3LL * v + 0]) | (glb_normal(nrm[3LL * v + 1]) << 8) | (glb_normal(nrm[3LL * v + 2]) << 16),
              dwords);
      }
      // the corner's texel: the cell's origin plus (0,0), (l,0), (0,l), mirrored in the upper half
      const int cellq = face >> 1, h = face & 1, leg = g.cell - 2 - h;
      const int ci = k == 1 ? leg : 0, cj = k == 2 ? leg : 0;
      const int x = (cellq % g.grid) * g.cell + (h ? g.cell - 1 - ci : ci);
      const int y = (cellq / g.grid) * g.cell + (h ? g.cell - 1 - cj : cj);
      const float u = ((float)x + 0.5f) / (float)g.size, w = ((float)y + 0.5f) / (float)g.size;  // exact
      put64(bin + l.off_t + 8 * i, __float_as_uint(u), __float_as_uint(w), dwords);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const int a = __shfl_xor(lo[k], o), b = __shfl_xor(hi[k], o);
        lo[k] = a < lo[k] ? a : lo[k];
        hi[k] = b > hi[k] ? b : hi[k];
      }
    }
    if ((threadIdx.x & 63) == 0) {
      const int wave = blockIdx.x * (kGlbBlock / 64) + (threadIdx.x >> 6);
      int *st = g.state + ((long long)f * kGlbSlots + (wave & (kGlbSlots - 1))) * kGlbSlotInts;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        if (lo[k] < __atomic_load_n(&st[k], __ATOMIC_RELAXED)) atomicMin(&st[k], lo[k]);
        if (hi[k] > __atomic_load_n(&st[3 + k], __ATOMIC_RELAXED)) atomicMax(&st[3 + k], hi[k]);
      }
    }
  }

  if (i >= words) return;  // image word i: four bytes of the PNG, zeros beyond its end
  const uint8_t *__restrict__ src = g.png + (long long)f * g.png_capacity + 4 * i;
  uint32_t v = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (4 * i + k < l.img) v |= (uint32_t)src[k] << (8 * k);
  put32(bin + l.off_img + 4 * i, v, dwords);
}

__device__ __forceinline__ long long glb_tex_hole_value(int kind, const GlbTexLayout &l, const int *ext) {
  switch (kind) {
    case kTexHoleNc: return 3LL * l.nf;
    case kTexHolePosOff: return 0;
    case kTexHolePosLen: return l.off_n;
    case kTexHoleNrmOff: return l.off_n;
    case kTexHoleNrmLen: return 12LL * l.nf;
    case kTexHoleUvOff: return l.off_t;
    case kTexHoleUvLen: return 24LL * l.nf;
    case kTexHoleImgOff: return l.off_img;
    case kTexHoleImgLen: return l.img;
    case kTexHoleBin: return l.bin;
    default: return ext[kind - kTexHoleMin];  // kTexHoleMin .. kTexHoleMax + 2
  }
}

__global__ __launch_bounds__(kGlbBlock) void glb_tex_header_kernel(GlbTexFrames fr, GlbTexGeom g, GlbTexTemplate tp) {
  __shared__ uint32_t file[(kGlbPrefix + kGlbTexJsonMax + 8) / 4];
  __shared__ int ext[6];
  const int f = blockIdx.x;
  const GlbTexLayout l = glb_tex_frame_layout(fr, g, f);
  if (l.code || l.total > g.capacity) return;
  uint8_t *row = g.out + (long long)f * g.capacity;
  const bool dwords = ((uintptr_t)row & 3u) == 0;
  if (l.empty) {
    for (int i = threadIdx.x; i < kGlbEmptyWords; i += kGlbBlock) put32(row + 4 * i, tp.empty[i], dwords);
    return;
  }
  if (threadIdx.x < kGlbSlots) {
    const int *__restrict__ st = g.state + ((long long)f * kGlbSlots + threadIdx.x) * kGlbSlotInts;
    int lo[3], hi[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) lo[k] = st[k], hi[k] = st[3 + k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const int a = __shfl_xor(lo[k], o), b = __shfl_xor(hi[k], o);
        lo[k] = a < lo[k] ? a : lo[k];
        hi[k] = b > hi[k] ? b : hi[k];
      }
    }
    if (threadIdx.x == 0) {
#pragma unroll
      for (int k = 0; k < 3; ++k) ext[k] = lo[k], ext[3 + k] = hi[k];
    }
  }
  const int json_words = g.json_len / 4;
  for (int i = threadIdx.x; i < json_words; i += kGlbBlock) file[kGlbPrefix / 4 + i] = tp.json[i];
  if (threadIdx.x == 0) {
    file[0] = 0x46546C67u;  // "glTF"
    file[1] = 2u;
    file[2] = (uint32_t)l.total;
    file[3] = (uint32_t)g.json_len;
    file[4] = 0x4E4F534Au;  // "JSON"
    file[kGlbPrefix / 4 + json_words] = (uint32_t)l.bin;
    file[kGlbPrefix / 4 + json_words + 1] = 0x004E4942u;  // "BIN\0"
  }
  __syncthreads();
  if ((int)threadIdx.x < tp.n_holes) {
    const GlbHoleAt h = tp.holes[threadIdx.x];
    long long v = glb_tex_hole_value(h.kind, l, ext);
    uint8_t *text = reinterpret_cast<uint8_t *>(file) + kGlbPrefix + h.at;
    for (int j = h.width - 1; j >= 0; --j) {
      text[j] = (v > 0 || j == h.width - 1) ? (uint8_t)('0' + v % 10) : (uint8_t)' ';
      v /= 10;
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kGlbPrefix / 4 + json_words + 2; i += kGlbBlock) put32(row + 4 * i, file[i], dwords);
}

namespace {

// the JSON text of a textured mesh under `flags` (MP_GLB_NORMALS or 0) with its holes, padded to a length % 8 == 4
GlbText glb_tex_text(int flags, const float *b_min, const float *b_max) {
  const bool nrm = flags & MP_GLB_NORMALS;
  const int c = 1 + nrm, k = c + 1;
  GlbText t;
  t.put(kGlbAsset);
  t.put(",\"extensionsUsed\":[\"KHR_mesh_quantization\"],\"extensionsRequired\":[\"KHR_mesh_quantization\"]");
  t.put(",\"scene\":0,\"scenes\":[{\"nodes\":[0]}],\"nodes\":[{\"mesh\":0,\"translation\":[");
  for (int a = 0; a < 3; ++a) t.put(a ? "," : ""), t.real((double)b_min[a]);
  t.put("],\"scale\":[");
  for (int a = 0; a < 3; ++a) t.put(a ? "," : ""), t.real(((double)b_max[a] - (double)b_min[a]) / 65535.0);
  t.put("]}],\"materials\":[{\"doubleSided\":true,\"pbrMetallicRoughness\":{\"baseColorTexture\":{\"index\":0},"
        "\"metallicFactor\":0,\"roughnessFactor\":1}}],\"textures\":[{\"sampler\":0,\"source\":0}],"
        "\"samplers\":[{\"magFilter\":9729,\"minFilter\":9729,\"wrapS\":33071,\"wrapT\":33071}],"
        "\"images\":[{\"bufferView\":");
  t.integer(k);
  t.put(",\"mimeType\":\"image/png\"}],\"meshes\":[{\"primitives\":[{\"attributes\":{\"POSITION\":0");
  if (nrm) t.put(",\"NORMAL\":1");
  t.put(",\"TEXCOORD_0\":"), t.integer(c);
  t.put("},\"material\":0,\"mode\":4}]}],\"accessors\":[{\"bufferView\":0,\"componentType\":5123,\"count\":");
  t.hole(kTexHoleNc, 10);
  t.put(",\"type\":\"VEC3\",\"min\":[");
  for (int a = 0; a < 3; ++a) t.put(a ? "," : ""), t.hole(kTexHoleMin + a, 5);
  t.put("],\"max\":[");
  for (int a = 0; a < 3; ++a) t.put(a ? "," : ""), t.hole(kTexHoleMax + a, 5);
  t.put("]}");
  if (nrm) {
    t.put(",{\"bufferView\":1,\"componentType\":5120,\"normalized\":true,\"count\":");
    t.hole(kTexHoleNc, 10);
    t.put(",\"type\":\"VEC3\"}");
  }
  t.put(",{\"bufferView\":"), t.integer(c);
  t.put(",\"componentType\":5126,\"count\":"), t.hole(kTexHoleNc, 10);
  t.put(",\"type\":\"VEC2\"}],\"bufferViews\":[");
  const int views[4][2] = {{kTexHolePosOff, kTexHolePosLen}, {kTexHoleNrmOff, kTexHoleNrmLen},
                           {kTexHoleUvOff, kTexHoleUvLen}, {kTexHoleImgOff, kTexHoleImgLen}};
  const bool present[4] = {true, nrm, true, true};
  const char *const tails[4] = {",\"byteStride\":8,\"target\":34962}", ",\"byteStride\":4,\"target\":34962}",
                                ",\"byteStride\":8,\"target\":34962}", "}"};
  for (int v = 0; v < 4; ++v) {
    if (!present[v]) continue;
    t.put(v ? ",{\"buffer\":0,\"byteOffset\":" : "{\"buffer\":0,\"byteOffset\":");
    t.hole(views[v][0], 10);
    t.put(",\"byteLength\":"), t.hole(views[v][1], 10);
    t.put(tails[v]);
  }
  t.put("],\"buffers\":[{\"byteLength\":"), t.hole(kTexHoleBin, 10);
  t.put("}]}");
  t.s.append((size_t)((12 - t.s.size() % 8) % 8), ' ');
  return t;
}

int glb_tex_json_len(int flags) {
  const float lo[3] = {0, 0, 0}, hi[3] = {1, 1, 1};
  return (int)glb_tex_text(flags, lo, hi).s.size();
}

}  // namespace

long long glb_textured_bytes(long long nf, int flags, long long png_bytes) {
  return glb_tex_layout(nf ? 1 : 0, nf, flags, glb_tex_json_len(flags), png_bytes).total;
}

int launch_mesh_glb_textured_batch(mp_ctx *ctx, void *scratch, const GlbCall &c, const GlbTextureCall &tc,
                                   const float *const *verts, const int32_t *const *faces,
                                   const int32_t *const *counts, const float *const *normals, uint8_t *out,
                                   int32_t *info, hipStream_t st) {
  GlbTexFrames fr;
  std::memset(&fr, 0, sizeof(fr));
  for (int f = 0; f < c.n_frames; ++f) {
    fr.verts[f] = verts ? verts[f] : nullptr;
    fr.faces[f] = faces ? faces[f] : nullptr;
    fr.counts[f] = counts[f];
    fr.normals[f] = normals ? normals[f] : nullptr;
  }
  GlbTexGeom g;
  std::memset(&g, 0, sizeof(g));
  g.max_v = c.max_v, g.max_f = c.max_f, g.capacity = c.capacity, g.png_capacity = tc.png_capacity;
  g.flags = normals ? MP_GLB_NORMALS : 0;
  g.size = tc.size, g.cell = tc.cell, g.grid = tc.size / tc.cell;
  for (int a = 0; a < 3; ++a) g.b_min[a] = c.b_min[a], g.inv[a] = c.inv[a];
  g.png = tc.png, g.png_info = tc.png_info;
  g.out = out, g.info = info, g.state = static_cast<int *>(scratch);
  const GlbText text = glb_tex_text(g.flags, c.b_min, c.b_max);
  const std::string empty = std::string(kGlbAsset) + ",\"scene\":0,\"scenes\":[{}]}  ";
  if (text.s.size() > (size_t)kGlbTexJsonMax || text.s.size() % 8 != 4 ||
      (int)text.s.size() != glb_tex_json_len(g.flags) || text.n_holes > kGlbHolesMax ||
      empty.size() != MP_GLB_MIN_BYTES - kGlbPrefix)
    return fail(ctx, MP_ERR_STATE, "mp_mesh_glb_textured: a JSON text of %zu bytes", text.s.size());
  g.json_len = (int)text.s.size();
  GlbTexTemplate tp;
  std::memset(&tp, 0, sizeof(tp));
  std::memcpy(tp.json, text.s.data(), text.s.size());
  std::memcpy(tp.holes, text.holes, sizeof(text.holes));
  tp.n_holes = text.n_holes;
  const uint32_t head[5] = {0x46546C67u, 2u, MP_GLB_MIN_BYTES, MP_GLB_MIN_BYTES - kGlbPrefix, 0x4E4F534Au};
  std::memcpy(tp.empty, head, sizeof(head));
  std::memcpy(tp.empty + 5, empty.data(), empty.size());

  hipLaunchKernelGGL(glb_tex_layout_kernel, dim3(c.n_frames), dim3(kGlbSlots), 0, st, fr, g);
  const long long words = (tc.png_capacity + 3) / 4, corners = 3 * c.max_f;
  const long long items = corners > words ? corners : words;
  const dim3 grid((unsigned)((items + kGlbBlock - 1) / kGlbBlock), c.n_frames);
  hipLaunchKernelGGL(glb_tex_pack_kernel, grid, dim3(kGlbBlock), 0, st, fr, g);
  hipLaunchKernelGGL(glb_tex_header_kernel, dim3(c.n_frames), dim3(kGlbBlock), 0, st, fr, g, tp);
  MP_HIP(ctx, hipGetLastError());
  return MP_OK;
}

}  // namespace mp
