// Vertex-clustering simplification of a triangle mesh as mp_marching_cubes leaves it (mp_mesh_simplify[_batch];
// no counterpart in the reference): the level-of-detail dial between marching cubes and the normals / colours.
//
// Defined bit for bit (include/monoport_hip.h), so nothing here may depend on the order in which threads arrive:
// the only atomics are INTEGER additions (64-bit fixed-point coordinate sums, 32-bit member counts), which commute.
//   mark        : one thread per vertex: its cell key (or -1 = invalid) -> scratch, the cell's flag in an n^3 table
//                 (cleared by one memset for all frames); clears the sums of row v (there are never more new
//                 vertices than old ones, so no second memset)
//   cells       : count -> block sums -> one-block-per-frame scan -> index (the shape of mcubes.hip): the table
//                 becomes the exclusive prefix of the flags = the cell's new vertex, ascending in key by
//                 construction; counts_out[0] = occupied cells.  Blocks of 1024 empty cells leave at once.
//   accumulate  : one thread per vertex: vmap, three 64-bit adds and one 32-bit add into its new vertex
//   finish      : one thread per new vertex: the mean, one IEEE division in double
//   faces       : flag (remapped, no index out of range / invalid / collapsed) + block sums -> the same scan ->
//                 stable compaction in input order; counts_out[1] = survivors
// Every kernel serves up to kMaxFrames meshes of one capacity per launch (blockIdx.y = frame; the scan: blockIdx.x).
// The sizes come from device memory (counts of mp_marching_cubes); the grids are sized from the capacities and blocks
// beyond the counts leave at once.  Every float operation is one IEEE operation in the order the header states.
#include "mp_internal.h"
#include "mesh_common.h"

#include <cstring>

#pragma clang fp contract(off)

namespace mp {

constexpr int kSimBlock = 256;  // the per-vertex kernels

struct SimplifyFrames {
  const float *verts[kMaxFrames];
  const int32_t *faces[kMaxFrames];
  const int32_t *counts[kMaxFrames];
  float *verts_out[kMaxFrames];
  int32_t *faces_out[kMaxFrames];
  int32_t *counts_out[kMaxFrames];
  int32_t *vmap[kMaxFrames];  // entries may be nullptr
};

struct SimplifyGeom {
  int n;
  float bmin[3], inv[3];
};

// Scratch of n frames: sums n x [max_v,3] int64 | table n x [n_cells] | blk_c n x [nb_c] | members n x [max_v] |
// index n x [max_v] | flags n x [max_f] | blk_f n x [nb_f]  (ints unless stated; the table first among them: one memset)
struct SimplifyScratch {
  long long *sums;
  int *table, *blk_c, *members, *index, *flags, *blk_f;
  long long n_cells, max_v, max_f;
  int nb_c, nb_f;
};

__device__ __forceinline__ bool simplify_valid(float x) { return fabsf(x) < 32768.0f; }  // false for NaN / inf too

// clamp((int)floorf(t), 0, n - 1), the clamp taken before the conversion so that every finite or infinite t is defined
__device__ __forceinline__ int simplify_cell(float v, float bmin, float inv, int n) {
  const float t = (v - bmin) * inv;
  if (t < 0.0f) return 0;
  if (t >= (float)n) return n - 1;
  return (int)floorf(t);
}

__global__ __launch_bounds__(kSimBlock) void simplify_mark_kernel(SimplifyFrames fr, SimplifyGeom g,
                                                                  SimplifyScratch sc) {
  const int nv = mesh_min(fr.counts[blockIdx.y][0], sc.max_v);
  const long long v = (long long)blockIdx.x * kSimBlock + threadIdx.x;
  if (v >= nv) return;
  const float *__restrict__ verts = fr.verts[blockIdx.y];
  const long long row = sc.max_v * blockIdx.y + v;
  const float x = verts[3 * v + 0], y = verts[3 * v + 1], z = verts[3 * v + 2];
  int key = -1;
  if (simplify_valid(x) && simplify_valid(y) && simplify_valid(z)) {
    const int cx = simplify_cell(x, g.bmin[0], g.inv[0], g.n);
    const int cy = simplify_cell(y, g.bmin[1], g.inv[1], g.n);
    const int cz = simplify_cell(z, g.bmin[2], g.inv[2], g.n);
    key = (cz * g.n + cy) * g.n + cx;  // < n^3 <= 2^27
    sc.table[sc.n_cells * blockIdx.y + key] = 1;  // every writer stores the same value
  }
  sc.index[row] = key;
  sc.sums[3 * row + 0] = 0;
  sc.sums[3 * row + 1] = 0;
  sc.sums[3 * row + 2] = 0;
  sc.members[row] = 0;
}

__global__ __launch_bounds__(kScanBlock) void simplify_cell_count_kernel(SimplifyScratch sc) {
  const int *__restrict__ table = sc.table + sc.n_cells * blockIdx.y;
  const long long c = (long long)blockIdx.x * kScanBlock + threadIdx.x;
  int tot;
  block_exclusive_scan(c < sc.n_cells ? table[c] : 0, &tot);
  if (threadIdx.x == 0) sc.blk_c[(long long)sc.nb_c * blockIdx.y + blockIdx.x] = tot;
}

// one block per frame: in-place exclusive scan of n_blocks block sums (any number of them: 1024 per step with a
// carry); counts_out[which] = their total
__global__ __launch_bounds__(kScanBlock) void simplify_scan_kernel(SimplifyFrames fr, int *__restrict__ blk_all,
                                                                   int n_blocks, int which) {
  int *__restrict__ blk = blk_all + (long long)n_blocks * blockIdx.x;
  __shared__ int carry;
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  for (int b0 = 0; b0 < n_blocks; b0 += kScanBlock) {
    const int b = b0 + threadIdx.x;
    int tot;
    const int e = block_exclusive_scan(b < n_blocks ? blk[b] : 0, &tot);
    if (b < n_blocks) blk[b] = carry + e;
    __syncthreads();
    if (threadIdx.x == 0) carry += tot;
    __syncthreads();
  }
  if (threadIdx.x == 0) fr.counts_out[blockIdx.x][which] = carry;
}

// table[c] = number of occupied cells in front of c (read for occupied cells only)
__global__ __launch_bounds__(kScanBlock) void simplify_cell_index_kernel(SimplifyFrames fr, SimplifyScratch sc) {
  const int *__restrict__ blk = sc.blk_c + (long long)sc.nb_c * blockIdx.y;
  const int next = blockIdx.x + 1 < gridDim.x ? blk[blockIdx.x + 1] : fr.counts_out[blockIdx.y][0];
  if (next == blk[blockIdx.x]) return;  // no occupied cell in this block: no vertex reads its entries
  int *__restrict__ table = sc.table + sc.n_cells * blockIdx.y;
  const long long c = (long long)blockIdx.x * kScanBlock + threadIdx.x;
  int tot;
  const int e = block_exclusive_scan(c < sc.n_cells ? table[c] : 0, &tot);
  if (c < sc.n_cells) table[c] = blk[blockIdx.x] + e;
}

__global__ __launch_bounds__(kSimBlock) void simplify_accumulate_kernel(SimplifyFrames fr, SimplifyScratch sc) {
  const int nv = mesh_min(fr.counts[blockIdx.y][0], sc.max_v);
  const long long v = (long long)blockIdx.x * kSimBlock + threadIdx.x;
  if (v >= nv) return;
  const float *__restrict__ verts = fr.verts[blockIdx.y];
  int32_t *__restrict__ vmap = fr.vmap[blockIdx.y];
  const long long row0 = sc.max_v * blockIdx.y;
  const int key = sc.index[row0 + v];
  int idx = -1;
  if (key >= 0) {
    idx = sc.table[sc.n_cells * blockIdx.y + key];  // < occupied cells <= nv
    unsigned long long *sums = reinterpret_cast<unsigned long long *>(sc.sums + 3 * (row0 + idx));
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const long long q = llrint((double)verts[3 * v + a] * 1048576.0);  // |q| < 2^35: exact, then ties to even
      atomicAdd(&sums[a], (unsigned long long)q);  // two's complement: the signed sum
    }
    atomicAdd(&sc.members[row0 + idx], 1);
  }
  sc.index[row0 + v] = idx;  // what the face kernels read, with or without a caller's vmap
  if (vmap) vmap[v] = idx;
}

__global__ __launch_bounds__(kSimBlock) void simplify_finish_kernel(SimplifyFrames fr, SimplifyScratch sc) {
  const int n_new = mesh_min(fr.counts_out[blockIdx.y][0], sc.max_v);
  const long long i = (long long)blockIdx.x * kSimBlock + threadIdx.x;
  if (i >= n_new) return;
  float *__restrict__ out = fr.verts_out[blockIdx.y];
  const long long row = sc.max_v * blockIdx.y + i;
  const double den = (double)sc.members[row] * 1048576.0;  // >= 2^20: an occupied cell has a member
#pragma unroll
  for (int a = 0; a < 3; ++a) out[3 * i + a] = (float)((double)sc.sums[3 * row + a] / den);
}

__global__ __launch_bounds__(kScanBlock) void simplify_face_flag_kernel(SimplifyFrames fr, SimplifyScratch sc) {
  const int32_t *__restrict__ counts = fr.counts[blockIdx.y];
  const int nf = mesh_min(counts[1], sc.max_f);
  const long long f = (long long)blockIdx.x * kScanBlock + threadIdx.x;
  int keep = 0;
  if (f < nf) {
    const int nv = mesh_min(counts[0], sc.max_v);
    const int32_t *__restrict__ faces = fr.faces[blockIdx.y];
    const int *__restrict__ index = sc.index + sc.max_v * blockIdx.y;
    const int i0 = faces[3 * f + 0], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
    if (i0 >= 0 && i0 < nv && i1 >= 0 && i1 < nv && i2 >= 0 && i2 < nv) {
      const int a = index[i0], b = index[i1], c = index[i2];
      keep = a >= 0 && b >= 0 && c >= 0 && a != b && b != c && a != c;
    }
    sc.flags[sc.max_f * blockIdx.y + f] = keep;
  }
  int tot;
  block_exclusive_scan(keep, &tot);  // every block stores its sum, also beyond the faces present
  if (threadIdx.x == 0) sc.blk_f[(long long)sc.nb_f * blockIdx.y + blockIdx.x] = tot;
}

__global__ __launch_bounds__(kScanBlock) void simplify_face_compact_kernel(SimplifyFrames fr, SimplifyScratch sc) {
  const int nf = mesh_min(fr.counts[blockIdx.y][1], sc.max_f);
  if ((long long)blockIdx.x * kScanBlock >= nf) return;
  const long long f = (long long)blockIdx.x * kScanBlock + threadIdx.x;
  const int keep = f < nf ? sc.flags[sc.max_f * blockIdx.y + f] : 0;
  int tot;
  const int e = block_exclusive_scan(keep, &tot);
  if (!keep) return;
  const long long pos = sc.blk_f[(long long)sc.nb_f * blockIdx.y + blockIdx.x] + e;  // < survivors <= nf
  const int32_t *__restrict__ faces = fr.faces[blockIdx.y];
  const int *__restrict__ index = sc.index + sc.max_v * blockIdx.y;
  int32_t *__restrict__ out = fr.faces_out[blockIdx.y];
#pragma unroll
  for (int c = 0; c < 3; ++c) out[3 * pos + c] = index[faces[3 * f + c]];
}

static long long simplify_blocks(long long n) { return (n + kScanBlock - 1) / kScanBlock; }

// n_frames * (4 n^3 + 4 ceil(n^3 / 1024) + 32 max_v + 4 max_f + 4 ceil(max_f / 1024)) + 256
size_t mesh_simplify_scratch_bytes(int n_frames, int n, long long max_v, long long max_f) {
  const long long cells = (long long)n * n * n;
  const size_t ints = (size_t)(cells + simplify_blocks(cells) + 2 * max_v + max_f + simplify_blocks(max_f));
  return (size_t)n_frames * (ints * 4 + (size_t)max_v * 24) + 256;
}

int launch_mesh_simplify_batch(mp_ctx *ctx, void *scratch, int n_frames, const float *const *verts, long long max_v,
                               const int32_t *const *faces, long long max_f, const int32_t *const *counts,
                               const float *bmin, const float *inv, int n, float *const *verts_out,
                               int32_t *const *faces_out, int32_t *const *counts_out, int32_t *const *vmap,
                               hipStream_t st) {
  SimplifyFrames fr;
  std::memset(&fr, 0, sizeof(fr));
  for (int f = 0; f < n_frames; ++f) {
    fr.verts[f] = verts[f];
    fr.faces[f] = faces[f];
    fr.counts[f] = counts[f];
    fr.verts_out[f] = verts_out[f];
    fr.faces_out[f] = faces_out[f];
    fr.counts_out[f] = counts_out[f];
    fr.vmap[f] = vmap ? vmap[f] : nullptr;
  }
  SimplifyGeom g;
  g.n = n;
  for (int a = 0; a < 3; ++a) {
    g.bmin[a] = bmin[a];
    g.inv[a] = inv[a];
  }
  SimplifyScratch sc;
  sc.n_cells = (long long)n * n * n;
  sc.max_v = max_v;
  sc.max_f = max_f;
  sc.nb_c = (int)simplify_blocks(sc.n_cells);
  sc.nb_f = (int)simplify_blocks(max_f);
  sc.sums = static_cast<long long *>(scratch);  // the arena's blocks are aligned for any type
  sc.table = reinterpret_cast<int *>(sc.sums + 3 * max_v * n_frames);
  sc.blk_c = sc.table + sc.n_cells * n_frames;
  sc.members = sc.blk_c + (long long)sc.nb_c * n_frames;
  sc.index = sc.members + max_v * n_frames;
  sc.flags = sc.index + max_v * n_frames;
  sc.blk_f = sc.flags + max_f * n_frames;
  const dim3 vb((unsigned)((max_v + kSimBlock - 1) / kSimBlock), n_frames);
  const dim3 cb((unsigned)sc.nb_c, n_frames);
  const dim3 fb((unsigned)sc.nb_f, n_frames);
  MP_HIP(ctx, hipMemsetAsync(sc.table, 0, (size_t)sc.n_cells * n_frames * sizeof(int), st));  // all frames' flags
  hipLaunchKernelGGL(simplify_mark_kernel, vb, dim3(kSimBlock), 0, st, fr, g, sc);
  hipLaunchKernelGGL(simplify_cell_count_kernel, cb, dim3(kScanBlock), 0, st, sc);
  hipLaunchKernelGGL(simplify_scan_kernel, dim3(n_frames), dim3(kScanBlock), 0, st, fr, sc.blk_c, sc.nb_c, 0);
  hipLaunchKernelGGL(simplify_cell_index_kernel, cb, dim3(kScanBlock), 0, st, fr, sc);
  hipLaunchKernelGGL(simplify_accumulate_kernel, vb, dim3(kSimBlock), 0, st, fr, sc);
  hipLaunchKernelGGL(simplify_finish_kernel, vb, dim3(kSimBlock), 0, st, fr, sc);
  if (fb.x) hipLaunchKernelGGL(simplify_face_flag_kernel, fb, dim3(kScanBlock), 0, st, fr, sc);
  hipLaunchKernelGGL(simplify_scan_kernel, dim3(n_frames), dim3(kScanBlock), 0, st, fr, sc.blk_f, sc.nb_f, 1);
  if (fb.x) hipLaunchKernelGGL(simplify_face_compact_kernel, fb, dim3(kScanBlock), 0, st, fr, sc);
  MP_HIP(ctx, hipGetLastError());
  return MP_OK;
}

}  // namespace mp
