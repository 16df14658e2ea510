// Per-vertex normals of a triangle mesh (compute_normal, monoport/lib/mesh_util.py:201-220) and the
// [V,3] -> [3,V] hand-over of the vertices to the counted colour query.
//
// Both modes are defined bit for bit (include/monoport_hip.h), so nothing here may depend on the order
// in which threads arrive: no float atomics.  Every float operation is one IEEE f32 operation in the
// order numpy performs it (the library is built with -ffp-contract=off; sqrtf and / are the correctly
// rounded ones, hipcc's default -fhip-fp32-correctly-rounded-divide-sqrt).
//   face pass   : one thread per face: unit normal -> scratch; per corner either atomicMax of the face
//                 index (reference mode: the LAST face wins, as numpy's a[idx] += b leaves it) or an
//                 integer count of the vertex's corners (accumulate mode)
//   reference   : one thread per vertex adds the three claimed faces' normals in corner order
//   accumulate  : store-and-sum: every vertex gets a segment of one list (segments are handed out with an
//                 integer atomic per wave: where a segment lies does not matter), the corners are
//                 filled in as keys 3 * face + corner in arrival order, and one thread per vertex adds its
//                 faces' normals in ascending key order by picking the next-larger key each step: O(valence^2)
//                 reads, exact for any valence.
// The sizes come from device memory (counts of mp_marching_cubes); the grids are sized from the
// capacities and blocks beyond the counts leave at once.
//
// Every kernel serves up to kMaxFrames meshes of one capacity per launch (blockIdx.y = frame: mp_mesh_normals_batch /
// mp_mesh_points_batch; the per-mesh calls are the one-frame case).  Each frame reads its own counts and has its own
// part of the scratch (MeshScratch), the running total of the segment allocation included.
#include "mp_internal.h"
#include "mesh_common.h"

#include <cstring>

#pragma clang fp contract(off)

namespace mp {

constexpr int kMeshBlock = 256;

// normalize_v3 (mesh_util.py:190-198): sqrt(x**2 + y**2 + z**2) left to right, eps = 1e-8 in f32
__device__ __forceinline__ void normalize_v3(float &x, float &y, float &z) {
  float len = sqrtf(x * x + y * y + z * z);
  if (len < 1e-8f) len = 1e-8f;
  x = x / len;
  y = y / len;
  z = z / len;
}

// the face's three indices if all of them name a vertex present, else false (the face is skipped)
__device__ __forceinline__ bool face_indices(const int32_t *__restrict__ faces, int f, int nv, int idx[3]) {
  idx[0] = faces[3 * (long long)f + 0];
  idx[1] = faces[3 * (long long)f + 1];
  idx[2] = faces[3 * (long long)f + 2];
  return idx[0] >= 0 && idx[0] < nv && idx[1] >= 0 && idx[1] < nv && idx[2] >= 0 && idx[2] < nv;
}

struct MeshFrames {
  const float *verts[kMaxFrames];
  const int32_t *faces[kMaxFrames];
  const int32_t *counts[kMaxFrames];
  float *normals[kMaxFrames];
};

// Scratch of n frames: face normals n x [max_f,3] f32 | keys n x [3 max_f] int | per-vertex ints n x [3 max_v] |
// totals [n].  The per-vertex part is last[v][corner] per frame in reference mode; in accumulate mode it is the
// valences of ALL frames (n x [max_v], cleared by one memset) followed by their cursors (n x [max_v]).
struct MeshScratch {
  float *fn;
  int *keys, *per_vertex, *total;
  long long max_v, max_f;
  int n_frames;
  __host__ __device__ float *face_normals(int f) const { return fn + 3 * max_f * f; }
  __host__ __device__ int *key_list(int f) const { return keys + 3 * max_f * f; }
  __host__ __device__ int *last(int f) const { return per_vertex + 3 * max_v * f; }
  __host__ __device__ int *valence(int f) const { return per_vertex + max_v * f; }
  __host__ __device__ int *cursor(int f) const { return per_vertex + max_v * (n_frames + f); }
};

__global__ __launch_bounds__(kMeshBlock) void mesh_face_kernel(MeshFrames fr, MeshScratch sc, int mode) {
  const int32_t *__restrict__ counts = fr.counts[blockIdx.y];
  const long long max_v = sc.max_v, max_f = sc.max_f;
  const int nf = mesh_min(counts[1], max_f);
  const long long f = (long long)blockIdx.x * kMeshBlock + threadIdx.x;
  if (f >= nf) return;
  const int nv = mesh_min(counts[0], max_v);
  int idx[3];
  const float *__restrict__ verts = fr.verts[blockIdx.y];
  const int32_t *__restrict__ faces = fr.faces[blockIdx.y];
  float *__restrict__ fn = sc.face_normals(blockIdx.y);
  int *__restrict__ per_vertex = mode == MP_NORMALS_REFERENCE ? sc.last(blockIdx.y) : sc.valence(blockIdx.y);
  if (!face_indices(faces, (int)f, nv, idx)) return;
  float p[3][3];
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int k = 0; k < 3; ++k) p[c][k] = verts[3 * (long long)idx[c] + k];
  // np.cross(t1 - t0, t2 - t0): multiply, multiply, subtract per component
  const float a0 = p[1][0] - p[0][0], a1 = p[1][1] - p[0][1], a2 = p[1][2] - p[0][2];
  const float b0 = p[2][0] - p[0][0], b1 = p[2][1] - p[0][1], b2 = p[2][2] - p[0][2];
  float nx = a1 * b2 - a2 * b1;
  float ny = a2 * b0 - a0 * b2;
  float nz = a0 * b1 - a1 * b0;
  normalize_v3(nx, ny, nz);
  fn[3 * f + 0] = nx;
  fn[3 * f + 1] = ny;
  fn[3 * f + 2] = nz;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    if (mode == MP_NORMALS_REFERENCE)
      atomicMax(&per_vertex[3 * (long long)idx[c] + c], (int)f);  // last[v][corner], cleared to -1
    else
      atomicAdd(&per_vertex[idx[c]], 1);  // valence[v], cleared to 0
  }
}

__global__ __launch_bounds__(kMeshBlock) void mesh_reference_kernel(MeshFrames fr, MeshScratch sc) {
  const int nv = mesh_min(fr.counts[blockIdx.y][0], sc.max_v);
  const long long v = (long long)blockIdx.x * kMeshBlock + threadIdx.x;
  if (v >= nv) return;
  const float *__restrict__ fn = sc.face_normals(blockIdx.y);
  const int *__restrict__ last = sc.last(blockIdx.y);
  float *__restrict__ normals = fr.normals[blockIdx.y];
  float x = 0.0f, y = 0.0f, z = 0.0f;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int f = last[3 * v + c];
    if (f < 0) continue;
    x = x + fn[3 * (long long)f + 0];
    y = y + fn[3 * (long long)f + 1];
    z = z + fn[3 * (long long)f + 2];
  }
  normalize_v3(x, y, z);
  normals[3 * v + 0] = x;
  normals[3 * v + 1] = y;
  normals[3 * v + 2] = z;
}

// cursor[v] = start of vertex v's segment of the frame's corner list; the frame's total counts the entries handed out
__global__ __launch_bounds__(kMeshBlock) void mesh_segments_kernel(MeshFrames fr, MeshScratch sc) {
  const int nv = mesh_min(fr.counts[blockIdx.y][0], sc.max_v);
  if ((long long)blockIdx.x * kMeshBlock >= nv) return;
  const int *__restrict__ valence = sc.valence(blockIdx.y);
  int *__restrict__ cursor = sc.cursor(blockIdx.y);
  int *__restrict__ total = sc.total + blockIdx.y;
  const long long v = (long long)blockIdx.x * kMeshBlock + threadIdx.x;
  const int n = v < nv ? valence[v] : 0;
  const int lane = threadIdx.x & 63;
  int incl = n;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(incl, o);
    if (lane >= o) incl += t;
  }
  int base = 0;
  if (lane == 63) base = atomicAdd(total, incl);
  base = __shfl(base, 63);
  if (v < nv) cursor[v] = base + incl - n;
}

__global__ __launch_bounds__(kMeshBlock) void mesh_fill_kernel(MeshFrames fr, MeshScratch sc) {
  const int32_t *__restrict__ counts = fr.counts[blockIdx.y];
  const int nf = mesh_min(counts[1], sc.max_f);
  const long long f = (long long)blockIdx.x * kMeshBlock + threadIdx.x;
  if (f >= nf) return;
  const int nv = mesh_min(counts[0], sc.max_v);
  const int32_t *__restrict__ faces = fr.faces[blockIdx.y];
  int *__restrict__ cursor = sc.cursor(blockIdx.y);
  int *__restrict__ keys = sc.key_list(blockIdx.y);
  int idx[3];
  if (!face_indices(faces, (int)f, nv, idx)) return;
#pragma unroll
  for (int c = 0; c < 3; ++c) keys[atomicAdd(&cursor[idx[c]], 1)] = 3 * (int)f + c;
}

// after the fill cursor[v] is the END of the segment; the keys of a segment are distinct
__global__ __launch_bounds__(kMeshBlock) void mesh_accumulate_kernel(MeshFrames fr, MeshScratch sc) {
  const int nv = mesh_min(fr.counts[blockIdx.y][0], sc.max_v);
  const long long v = (long long)blockIdx.x * kMeshBlock + threadIdx.x;
  if (v >= nv) return;
  const float *__restrict__ fn = sc.face_normals(blockIdx.y);
  const int *__restrict__ valence = sc.valence(blockIdx.y);
  const int *__restrict__ cursor = sc.cursor(blockIdx.y);
  const int *__restrict__ keys = sc.key_list(blockIdx.y);
  float *__restrict__ normals = fr.normals[blockIdx.y];
  const int n = valence[v];
  const int *seg = keys + (cursor[v] - n);
  float x = 0.0f, y = 0.0f, z = 0.0f;
  int prev = -1;
  for (int step = 0; step < n; ++step) {
    int next = 0x7fffffff;
    for (int j = 0; j < n; ++j) {
      const int k = seg[j];
      if (k > prev && k < next) next = k;
    }
    if (next == 0x7fffffff) break;  // cannot happen for distinct keys; never index with it
    const long long f = next / 3;
    x = x + fn[3 * f + 0];
    y = y + fn[3 * f + 1];
    z = z + fn[3 * f + 2];
    prev = next;
  }
  normalize_v3(x, y, z);
  normals[3 * v + 0] = x;
  normals[3 * v + 1] = y;
  normals[3 * v + 2] = z;
}

struct PointFrames {
  const float *verts[kMaxFrames];
  const int32_t *counts[kMaxFrames];
  float *points[kMaxFrames];
  int32_t *count_out[kMaxFrames];
};

__global__ __launch_bounds__(kMeshBlock) void mesh_points_kernel(PointFrames fr, long long max_v) {
  const float *__restrict__ verts = fr.verts[blockIdx.y];
  float *__restrict__ points = fr.points[blockIdx.y];
  const int nv = mesh_min(fr.counts[blockIdx.y][0], max_v);
  const long long v = (long long)blockIdx.x * kMeshBlock + threadIdx.x;
  if (v == 0) fr.count_out[blockIdx.y][0] = nv;
  if (v >= nv) return;
#pragma unroll
  for (int k = 0; k < 3; ++k) points[k * max_v + v] = verts[3 * v + k];
}

// per frame: face normals [max_f,3] f32 | keys [3 max_f] int | per-vertex ints [3 max_v] | total [1] (MeshScratch)
size_t mesh_normals_scratch_bytes(int n_frames, long long max_v, long long max_f) {
  return (size_t)n_frames * (size_t)(6 * max_f + 3 * max_v + 1) * 4 + 256;
}

int launch_mesh_normals_batch(mp_ctx *ctx, void *scratch, int n_frames, const float *const *verts, long long max_v,
                              const int32_t *const *faces, long long max_f, const int32_t *const *counts, int mode,
                              float *const *normals, hipStream_t st) {
  // keys are 3 * face + corner in an int
  if (max_f > 0x7fffffffLL / 3 || max_v > 0x7fffffffLL / 3)
    return fail(ctx, MP_ERR_UNSUPPORTED, "mesh normals: %lld vertices / %lld faces need 64-bit indices", max_v, max_f);
  if (max_v == 0) return MP_OK;
  MeshFrames fr;
  std::memset(&fr, 0, sizeof(fr));
  for (int f = 0; f < n_frames; ++f) {
    fr.verts[f] = verts[f];
    fr.faces[f] = faces[f];
    fr.counts[f] = counts[f];
    fr.normals[f] = normals[f];
  }
  MeshScratch sc;
  sc.fn = static_cast<float *>(scratch);
  sc.keys = reinterpret_cast<int *>(sc.fn + 3 * max_f * n_frames);
  sc.per_vertex = sc.keys + 3 * max_f * n_frames;
  sc.total = sc.per_vertex + 3 * max_v * n_frames;
  sc.max_v = max_v;
  sc.max_f = max_f;
  sc.n_frames = n_frames;
  const dim3 fb((unsigned)((max_f + kMeshBlock - 1) / kMeshBlock), n_frames);
  const dim3 vb((unsigned)((max_v + kMeshBlock - 1) / kMeshBlock), n_frames);
  if (mode == MP_NORMALS_REFERENCE) {
    // last[v][corner] = -1, all frames
    MP_HIP(ctx, hipMemsetAsync(sc.per_vertex, 0xff, (size_t)3 * max_v * n_frames * sizeof(int), st));
    if (fb.x) hipLaunchKernelGGL(mesh_face_kernel, fb, dim3(kMeshBlock), 0, st, fr, sc, mode);
    hipLaunchKernelGGL(mesh_reference_kernel, vb, dim3(kMeshBlock), 0, st, fr, sc);
  } else {
    MP_HIP(ctx, hipMemsetAsync(sc.per_vertex, 0, (size_t)max_v * n_frames * sizeof(int), st));  // the valences
    MP_HIP(ctx, hipMemsetAsync(sc.total, 0, (size_t)n_frames * sizeof(int), st));
    if (fb.x) hipLaunchKernelGGL(mesh_face_kernel, fb, dim3(kMeshBlock), 0, st, fr, sc, mode);
    hipLaunchKernelGGL(mesh_segments_kernel, vb, dim3(kMeshBlock), 0, st, fr, sc);
    if (fb.x) hipLaunchKernelGGL(mesh_fill_kernel, fb, dim3(kMeshBlock), 0, st, fr, sc);
    hipLaunchKernelGGL(mesh_accumulate_kernel, vb, dim3(kMeshBlock), 0, st, fr, sc);
  }
  MP_HIP(ctx, hipGetLastError());
  return MP_OK;
}

int launch_mesh_points_batch(mp_ctx *ctx, int n_frames, const float *const *verts, long long max_v,
                             const int32_t *const *counts, float *const *points, int32_t *const *count_out,
                             hipStream_t st) {
  PointFrames fr;
  std::memset(&fr, 0, sizeof(fr));
  for (int f = 0; f < n_frames; ++f) {
    fr.verts[f] = verts[f];
    fr.counts[f] = counts[f];
    fr.points[f] = points[f];
    fr.count_out[f] = count_out[f];
  }
  const unsigned vb = (unsigned)((max_v + kMeshBlock - 1) / kMeshBlock);
  hipLaunchKernelGGL(mesh_points_kernel, dim3(vb ? vb : 1, n_frames), dim3(kMeshBlock), 0, st, fr, max_v);
  MP_HIP(ctx, hipGetLastError());
  return MP_OK;
}

}  // namespace mp
