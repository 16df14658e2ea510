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
#include "mp_internal.h"

#pragma clang fp contract(off)

namespace mp {

constexpr int kMeshBlock = 256;

__device__ __forceinline__ int mesh_min(int count, long long cap) {
  if (count < 0) return 0;
  return (long long)count < cap ? count : (int)cap;
}

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

__global__ __launch_bounds__(kMeshBlock) void mesh_face_kernel(
    const float *__restrict__ verts, long long max_v, const int32_t *__restrict__ faces, long long max_f,
    const int32_t *__restrict__ counts, int mode, float *__restrict__ fn, int *__restrict__ per_vertex) {
  const int nf = mesh_min(counts[1], max_f);
  const long long f = (long long)blockIdx.x * kMeshBlock + threadIdx.x;
  if (f >= nf) return;
  const int nv = mesh_min(counts[0], max_v);
  int idx[3];
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

__global__ __launch_bounds__(kMeshBlock) void mesh_reference_kernel(
    long long max_v, const int32_t *__restrict__ counts, const float *__restrict__ fn,
    const int *__restrict__ last, float *__restrict__ normals) {
  const int nv = mesh_min(counts[0], max_v);
  const long long v = (long long)blockIdx.x * kMeshBlock + threadIdx.x;
  if (v >= nv) return;
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

// cursor[v] = start of vertex v's segment of the corner list; *total counts the entries handed out
__global__ __launch_bounds__(kMeshBlock) void mesh_segments_kernel(long long max_v,
                                                                   const int32_t *__restrict__ counts,
                                                                   const int *__restrict__ valence,
                                                                   int *__restrict__ cursor,
                                                                   int *__restrict__ total) {
  const int nv = mesh_min(counts[0], max_v);
  if ((long long)blockIdx.x * kMeshBlock >= nv) return;
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

__global__ __launch_bounds__(kMeshBlock) void mesh_fill_kernel(long long max_v,
                                                               const int32_t *__restrict__ faces,
                                                               long long max_f,
                                                               const int32_t *__restrict__ counts,
                                                               int *__restrict__ cursor,
                                                               int *__restrict__ keys) {
  const int nf = mesh_min(counts[1], max_f);
  const long long f = (long long)blockIdx.x * kMeshBlock + threadIdx.x;
  if (f >= nf) return;
  const int nv = mesh_min(counts[0], max_v);
  int idx[3];
  if (!face_indices(faces, (int)f, nv, idx)) return;
#pragma unroll
  for (int c = 0; c < 3; ++c) keys[atomicAdd(&cursor[idx[c]], 1)] = 3 * (int)f + c;
}

// after the fill cursor[v] is the END of the segment; the keys of a segment are distinct
__global__ __launch_bounds__(kMeshBlock) void mesh_accumulate_kernel(
    long long max_v, const int32_t *__restrict__ counts, const float *__restrict__ fn,
    const int *__restrict__ valence, const int *__restrict__ cursor, const int *__restrict__ keys,
    float *__restrict__ normals) {
  const int nv = mesh_min(counts[0], max_v);
  const long long v = (long long)blockIdx.x * kMeshBlock + threadIdx.x;
  if (v >= nv) return;
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

__global__ __launch_bounds__(kMeshBlock) void mesh_points_kernel(const float *__restrict__ verts, long long max_v,
                                                                 const int32_t *__restrict__ counts,
                                                                 float *__restrict__ points,
                                                                 int32_t *__restrict__ count_out) {
  const int nv = mesh_min(counts[0], max_v);
  const long long v = (long long)blockIdx.x * kMeshBlock + threadIdx.x;
  if (v == 0) count_out[0] = nv;
  if (v >= nv) return;
#pragma unroll
  for (int k = 0; k < 3; ++k) points[k * max_v + v] = verts[3 * v + k];
}

// face normals [max_f,3] f32 | keys [3 max_f] int | per-vertex ints [3 max_v] | total [1]
size_t mesh_normals_scratch_bytes(long long max_v, long long max_f) {
  return (size_t)(6 * max_f + 3 * max_v + 1) * 4 + 256;
}

int launch_mesh_normals(mp_ctx *ctx, void *scratch, const float *verts, long long max_v, const int32_t *faces,
                        long long max_f, const int32_t *counts, int mode, float *normals, hipStream_t st) {
  // keys are 3 * face + corner in an int
  if (max_f > 0x7fffffffLL / 3 || max_v > 0x7fffffffLL / 3)
    return fail(ctx, MP_ERR_UNSUPPORTED, "mesh normals: %lld vertices / %lld faces need 64-bit indices", max_v, max_f);
  if (max_v == 0) return MP_OK;
  float *fn = static_cast<float *>(scratch);
  int *keys = reinterpret_cast<int *>(fn + 3 * max_f);
  int *per_vertex = keys + 3 * max_f;
  int *total = per_vertex + 3 * max_v;
  const unsigned fb = (unsigned)((max_f + kMeshBlock - 1) / kMeshBlock);
  const unsigned vb = (unsigned)((max_v + kMeshBlock - 1) / kMeshBlock);
  if (mode == MP_NORMALS_REFERENCE) {
    MP_HIP(ctx, hipMemsetAsync(per_vertex, 0xff, (size_t)3 * max_v * sizeof(int), st));  // last[v][corner] = -1
    if (fb)
      hipLaunchKernelGGL(mesh_face_kernel, dim3(fb), dim3(kMeshBlock), 0, st, verts, max_v, faces, max_f, counts,
                         mode, fn, per_vertex);
    hipLaunchKernelGGL(mesh_reference_kernel, dim3(vb), dim3(kMeshBlock), 0, st, max_v, counts, fn, per_vertex,
                       normals);
  } else {
    int *valence = per_vertex, *cursor = per_vertex + max_v;
    MP_HIP(ctx, hipMemsetAsync(valence, 0, (size_t)max_v * sizeof(int), st));
    MP_HIP(ctx, hipMemsetAsync(total, 0, sizeof(int), st));
    if (fb)
      hipLaunchKernelGGL(mesh_face_kernel, dim3(fb), dim3(kMeshBlock), 0, st, verts, max_v, faces, max_f, counts,
                         mode, fn, valence);
    hipLaunchKernelGGL(mesh_segments_kernel, dim3(vb), dim3(kMeshBlock), 0, st, max_v, counts, valence, cursor,
                       total);
    if (fb)
      hipLaunchKernelGGL(mesh_fill_kernel, dim3(fb), dim3(kMeshBlock), 0, st, max_v, faces, max_f, counts, cursor,
                         keys);
    hipLaunchKernelGGL(mesh_accumulate_kernel, dim3(vb), dim3(kMeshBlock), 0, st, max_v, counts, fn, valence,
                       cursor, keys, normals);
  }
  MP_HIP(ctx, hipGetLastError());
  return MP_OK;
}

int launch_mesh_points(mp_ctx *ctx, const float *verts, long long max_v, const int32_t *counts, float *points,
                       int32_t *count_out, hipStream_t st) {
  const unsigned vb = (unsigned)((max_v + kMeshBlock - 1) / kMeshBlock);
  hipLaunchKernelGGL(mesh_points_kernel, dim3(vb ? vb : 1), dim3(kMeshBlock), 0, st, verts, max_v, counts, points,
                     count_out);
  MP_HIP(ctx, hipGetLastError());
  return MP_OK;
}

}  // namespace mp
