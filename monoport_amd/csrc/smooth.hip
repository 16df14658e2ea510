// Taubin smoothing of a triangle mesh as mp_marching_cubes / mp_mesh_simplify leave it (mp_mesh_smooth[_batch]; no
// counterpart in the reference): lambda | mu passes of the umbrella operator over the one-ring, between the mesh and
// its normals.
//
// Defined bit for bit (include/monoport_hip.h), so nothing here may depend on the order in which threads arrive: the
// only atomics are INTEGER ones, no float is ever added atomically.  Store-and-sum: every vertex owns a segment of one
// list of neighbour indices, and one thread per vertex adds its neighbours' positions in ascending index order.
//   count     : one thread per face: cnt[a] += 1 per directed entry (a -> b and b -> a of every edge with a != b of a
//               valid face: up to six per face)
//   segments  : cursor[v] = start of v's segment (wave prefix + one integer atomic per wave: where a segment lies is
//               arrival dependent and does not matter)
//   fill      : one thread per face: the neighbour indices through the cursors, in arrival order
//   ring      : one thread per vertex: sorts its segment in place (selection sort: valence <= 13 on marching-cubes
//               meshes; a fan of any size is slow and exact), compacts it to the distinct neighbours ascending, takes
//               the parity of every multiplicity on the way -> deg[v], fixed[v], the caller's ring[v]
//   pass      : one thread per vertex, 2 x iterations launches (lambda, mu, lambda, ...): all of a pass read the
//               previous pass's positions and write the next buffer, every row [0, nv) (a fixed vertex is copied), so
//               the ping-pong between verts_out and one scratch buffer needs no copy: pass 0 reads the input, even
//               passes write the scratch, odd ones verts_out, and the last one is odd.
// Every kernel serves up to kMaxFrames meshes of one capacity per launch (blockIdx.y = frame).  The sizes come from
// device memory (counts of mp_marching_cubes); the grids are sized from the capacities and blocks beyond the counts
// leave at once.  Every float operation is one IEEE f32 operation in the order the header states.
#include "mp_internal.h"
#include "mesh_common.h"

#include <cstring>

#pragma clang fp contract(off)

namespace mp {

constexpr int kSmoothBlock = 256;

struct SmoothFrames {
  const float *verts[kMaxFrames];
  const int32_t *faces[kMaxFrames];
  const int32_t *counts[kMaxFrames];
  float *verts_out[kMaxFrames];
  int32_t *ring[kMaxFrames];  // entries may be nullptr
};

// Scratch of n frames: cnt n x [max_v] | total [32] | cursor n x [max_v] | deg n x [max_v] | fixed n x [max_v] |
// pong n x [max_v,3] f32 | nbr n x [6 max_f]  (ints unless stated; cnt and total first: one memset)
struct SmoothScratch {
  int *cnt, *total, *cursor, *deg, *fixed, *nbr;
  float *pong;
  long long max_v, max_f;
};

// the face's three indices if all of them name a vertex present, else false (the face is skipped)
__device__ __forceinline__ bool smooth_face(const int32_t *__restrict__ faces, long long f, int nv, int idx[3]) {
  idx[0] = faces[3 * f + 0];
  idx[1] = faces[3 * f + 1];
  idx[2] = faces[3 * f + 2];
  return idx[0] >= 0 && idx[0] < nv && idx[1] >= 0 && idx[1] < nv && idx[2] >= 0 && idx[2] < nv;
}

__global__ __launch_bounds__(kSmoothBlock) void smooth_count_kernel(SmoothFrames fr, SmoothScratch sc) {
  const int32_t *__restrict__ counts = fr.counts[blockIdx.y];
  const int nf = mesh_min(counts[1], sc.max_f);
  const long long f = (long long)blockIdx.x * kSmoothBlock + threadIdx.x;
  if (f >= nf) return;
  const int nv = mesh_min(counts[0], sc.max_v);
  int idx[3];
  if (!smooth_face(fr.faces[blockIdx.y], f, nv, idx)) return;
  int *__restrict__ cnt = sc.cnt + sc.max_v * blockIdx.y;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int a = idx[c], b = idx[c == 2 ? 0 : c + 1];
    if (a == b) continue;
    atomicAdd(&cnt[a], 1);
    atomicAdd(&cnt[b], 1);
  }
}

// cursor[v] = start of vertex v's segment of the frame's neighbour list (at most 6 nf entries in all)
__global__ __launch_bounds__(kSmoothBlock) void smooth_segments_kernel(SmoothFrames fr, SmoothScratch sc) {
  const int nv = mesh_min(fr.counts[blockIdx.y][0], sc.max_v);
  if ((long long)blockIdx.x * kSmoothBlock >= nv) return;
  const int *__restrict__ cnt = sc.cnt + sc.max_v * blockIdx.y;
  int *__restrict__ cursor = sc.cursor + sc.max_v * blockIdx.y;
  const long long v = (long long)blockIdx.x * kSmoothBlock + threadIdx.x;
  const int n = v < nv ? cnt[v] : 0;
  const int lane = threadIdx.x & 63;
  int incl = n;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(incl, o);
    if (lane >= o) incl += t;
  }
  int base = 0;
  if (lane == 63) base = atomicAdd(sc.total + blockIdx.y, incl);
  base = __shfl(base, 63);
  if (v < nv) cursor[v] = base + incl - n;
}

__global__ __launch_bounds__(kSmoothBlock) void smooth_fill_kernel(SmoothFrames fr, SmoothScratch sc) {
  const int32_t *__restrict__ counts = fr.counts[blockIdx.y];
  const int nf = mesh_min(counts[1], sc.max_f);
  const long long f = (long long)blockIdx.x * kSmoothBlock + threadIdx.x;
  if (f >= nf) return;
  const int nv = mesh_min(counts[0], sc.max_v);
  int idx[3];
  if (!smooth_face(fr.faces[blockIdx.y], f, nv, idx)) return;
  int *__restrict__ cursor = sc.cursor + sc.max_v * blockIdx.y;
  int *__restrict__ nbr = sc.nbr + 6 * sc.max_f * blockIdx.y;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int a = idx[c], b = idx[c == 2 ? 0 : c + 1];
    if (a == b) continue;
    nbr[atomicAdd(&cursor[a], 1)] = b;  // < the frame's total <= 6 nf
    nbr[atomicAdd(&cursor[b], 1)] = a;
  }
}

// after the fill cursor[v] is the END of the segment of cnt[v] entries; they are sorted and made distinct in place
__global__ __launch_bounds__(kSmoothBlock) void smooth_ring_kernel(SmoothFrames fr, SmoothScratch sc, int pin) {
  const int nv = mesh_min(fr.counts[blockIdx.y][0], sc.max_v);
  const long long v = (long long)blockIdx.x * kSmoothBlock + threadIdx.x;
  if (v >= nv) return;
  const long long row = sc.max_v * blockIdx.y + v;
  const int n = sc.cnt[row];
  int *seg = sc.nbr + 6 * sc.max_f * blockIdx.y + (sc.cursor[row] - n);
  for (int i = 0; i + 1 < n; ++i) {
    int best = i, key = seg[i];
    for (int j = i + 1; j < n; ++j) {
      const int k = seg[j];
      if (k < key) best = j, key = k;
    }
    seg[best] = seg[i];
    seg[i] = key;
  }
  int d = 0, border = 0;
  for (int i = 0; i < n;) {
    const int b = seg[i];
    int m = 0;
    while (i < n && seg[i] == b) ++i, ++m;
    border |= m & 1;
    seg[d++] = b;  // d <= i: behind the reader
  }
  sc.deg[row] = d;
  sc.fixed[row] = d == 0 || (pin && border);
  int32_t *__restrict__ ring = fr.ring[blockIdx.y];
  if (ring) ring[v] = border ? -d : d;
}

// src_all / dst_all: the scratch buffer [n_frames, max_v, 3], or nullptr = the frames' own fr.verts / fr.verts_out
__global__ __launch_bounds__(kSmoothBlock) void smooth_pass_kernel(SmoothFrames fr, SmoothScratch sc,
                                                                   const float *src_all, float *dst_all, float phi) {
  const int nv = mesh_min(fr.counts[blockIdx.y][0], sc.max_v);
  const long long v = (long long)blockIdx.x * kSmoothBlock + threadIdx.x;
  if (v >= nv) return;
  const long long row0 = sc.max_v * blockIdx.y;
  const float *__restrict__ src = src_all ? src_all + 3 * row0 : fr.verts[blockIdx.y];
  float *__restrict__ dst = dst_all ? dst_all + 3 * row0 : fr.verts_out[blockIdx.y];
  const float px = src[3 * v + 0], py = src[3 * v + 1], pz = src[3 * v + 2];
  float qx = px, qy = py, qz = pz;
  if (!sc.fixed[row0 + v]) {
    const int d = sc.deg[row0 + v];  // >= 1
    const int *__restrict__ seg = sc.nbr + 6 * sc.max_f * blockIdx.y + (sc.cursor[row0 + v] - sc.cnt[row0 + v]);
    float sx = 0.0f, sy = 0.0f, sz = 0.0f;
    for (int i = 0; i < d; ++i) {
      const long long b = seg[i];  // in [0, nv)
      sx = sx + src[3 * b + 0];
      sy = sy + src[3 * b + 1];
      sz = sz + src[3 * b + 2];
    }
    const float fd = (float)d;
    const float mx = sx / fd, my = sy / fd, mz = sz / fd;
    qx = px + phi * (mx - px);
    qy = py + phi * (my - py);
    qz = pz + phi * (mz - pz);
  }
  dst[3 * v + 0] = qx;
  dst[3 * v + 1] = qy;
  dst[3 * v + 2] = qz;
}

// n_frames * (24 max_f + 28 max_v) + 256: the frames' totals (kMaxFrames ints) lie in the 256
size_t mesh_smooth_scratch_bytes(int n_frames, long long max_v, long long max_f) {
  return (size_t)n_frames * ((size_t)max_f * 24 + (size_t)max_v * 28) + 256;
}

int launch_mesh_smooth_batch(mp_ctx *ctx, void *scratch, int n_frames, const float *const *verts, long long max_v,
                             const int32_t *const *faces, long long max_f, const int32_t *const *counts,
                             int iterations, float lambda, float mu, int pin, float *const *verts_out,
                             int32_t *const *ring, hipStream_t st) {
  static_assert(kMaxFrames * sizeof(int) <= 256, "the totals live in the scratch's 256 spare bytes");
  SmoothFrames fr;
  std::memset(&fr, 0, sizeof(fr));
  for (int f = 0; f < n_frames; ++f) {
    fr.verts[f] = verts[f];
    fr.faces[f] = faces[f];
    fr.counts[f] = counts[f];
    fr.verts_out[f] = verts_out[f];
    fr.ring[f] = ring ? ring[f] : nullptr;
  }
  SmoothScratch sc;
  sc.max_v = max_v;
  sc.max_f = max_f;
  sc.cnt = static_cast<int *>(scratch);
  sc.total = sc.cnt + max_v * n_frames;
  sc.cursor = sc.total + kMaxFrames;
  sc.deg = sc.cursor + max_v * n_frames;
  sc.fixed = sc.deg + max_v * n_frames;
  sc.pong = reinterpret_cast<float *>(sc.fixed + max_v * n_frames);
  sc.nbr = reinterpret_cast<int *>(sc.pong + 3 * max_v * n_frames);
  const dim3 fb((unsigned)((max_f + kSmoothBlock - 1) / kSmoothBlock), n_frames);
  const dim3 vb((unsigned)((max_v + kSmoothBlock - 1) / kSmoothBlock), n_frames);
  // the valences of all frames and their totals
  MP_HIP(ctx, hipMemsetAsync(sc.cnt, 0, ((size_t)max_v * n_frames + kMaxFrames) * sizeof(int), st));
  if (fb.x) hipLaunchKernelGGL(smooth_count_kernel, fb, dim3(kSmoothBlock), 0, st, fr, sc);
  hipLaunchKernelGGL(smooth_segments_kernel, vb, dim3(kSmoothBlock), 0, st, fr, sc);
  if (fb.x) hipLaunchKernelGGL(smooth_fill_kernel, fb, dim3(kSmoothBlock), 0, st, fr, sc);
  hipLaunchKernelGGL(smooth_ring_kernel, vb, dim3(kSmoothBlock), 0, st, fr, sc, pin);
  SmoothFrames back = fr;  // the lambda passes after the first read what the mu pass before them wrote: verts_out
  for (int f = 0; f < n_frames; ++f) back.verts[f] = verts_out[f];
  for (int k = 0; k < iterations; ++k) {
    hipLaunchKernelGGL(smooth_pass_kernel, vb, dim3(kSmoothBlock), 0, st, k == 0 ? fr : back, sc,
                       (const float *)nullptr, sc.pong, lambda);
    hipLaunchKernelGGL(smooth_pass_kernel, vb, dim3(kSmoothBlock), 0, st, fr, sc, (const float *)sc.pong,
                       (float *)nullptr, mu);
  }
  MP_HIP(ctx, hipGetLastError());
  return MP_OK;
}

}  // namespace mp
