// Largest connected body of an occupancy volume: union-find labelling of the voxels with value > level, the largest
// component kept, every other inside voxel replaced by `fill` (mp_volume_keep_largest).
//
// Not present in the reference (it renders straight from the volume); the clean-up step in front of marching cubes.
// The definition is the header's: 6 or 26 connectivity, a component's id = its smallest linear voxel index, the
// largest component wins and the smaller id breaks a tie.
//   init      label[v] = v for foreground, kBackground else; the frame's header zeroed
//   merge     every foreground voxel unions itself with its forward foreground neighbours (atomicMin on roots)
//   compress  label[v] = find(v) for non-roots, -1 (= minus a size of 1) for roots
//   count     label[root] -= voxels pointing at it: added per wave, then per block, before the global atomic
//   select    one 64-bit atomicMax of (size << 32 | ~id) over the roots; roots and foreground voxels counted
//   apply     out[v] = in[v] or fill; stats written
// The phases are separated by launch boundaries only: no workgroup waits on another, and every loop ends because a
// parent label only ever decreases (a root is hooked under a SMALLER root, so a component's final root is its
// smallest index).  Integer atomics only (min, add, max commute exactly), so the result is a pure function of the
// input whatever order they land in.
#include "mp_internal.h"

#include <climits>
#include <cstring>

namespace mp {

constexpr int kCcMergeBlock = 256;   // one voxel per thread
constexpr int kCcBlock = 1024;       // the streaming passes: kCcVec consecutive voxels per thread
constexpr int kCcVec = 4;
constexpr int kCcHeaderInts = 256;   // per frame behind the labels: best (u64) | foreground | roots
constexpr int kBackground = INT_MIN; // no size reaches 2^31, so -size never collides

struct CcFrames {
  const float *vol[kMaxFrames];
  float *out[kMaxFrames];
  int32_t *stats[kMaxFrames];
  const int32_t *gate[kMaxFrames];  // NULL = frame on; else the frame is served only if *gate != 0
};

__device__ __forceinline__ bool cc_gated_off(const CcFrames &fr, int f) {
  const int32_t *gate = fr.gate[f];
  return gate != nullptr && *gate == 0;
}

// relaxed agent-scope accesses of labels that other workgroups change while this kernel runs
__device__ __forceinline__ int label_load(const int *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void label_store(int *p, int v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// root of x: ends because label[x] <= x along the path (a negative label is a root that compress has marked)
__device__ __forceinline__ int cc_find(const int *label, int x) {
  for (;;) {
    const int p = label_load(label + x);
    if (p == x || p < 0) return x;
    x = p;
  }
}

__device__ __forceinline__ void cc_union(int *label, int a, int b) {
  for (;;) {
    a = cc_find(label, a);
    b = cc_find(label, b);
    if (a == b) return;
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    // a > b: hook a under b if a is still a root; else go on from what it was hooked under meanwhile
    const int old = atomicMin(label + a, b);
    if (old == a) return;
    a = old;
  }
}

__global__ __launch_bounds__(kCcBlock) void cc_init_kernel(CcFrames fr, int n, float level, int *__restrict__ scratch,
                                                           long long stride) {
  if (cc_gated_off(fr, blockIdx.y)) return;
  const float *__restrict__ v = fr.vol[blockIdx.y];
  int *__restrict__ label = scratch + blockIdx.y * stride;
  if (blockIdx.x == 0 && threadIdx.x < 4) label[stride - kCcHeaderInts + threadIdx.x] = 0;
  const long long i0 = ((long long)blockIdx.x * kCcBlock + threadIdx.x) * kCcVec;
  if (i0 >= n) return;
  if (i0 + kCcVec <= n) {
    int4 l;
    if (((uintptr_t)v & 15) == 0) {
      const float4 q = *reinterpret_cast<const float4 *>(v + i0);
      l.x = q.x > level ? (int)i0 : kBackground;
      l.y = q.y > level ? (int)i0 + 1 : kBackground;
      l.z = q.z > level ? (int)i0 + 2 : kBackground;
      l.w = q.w > level ? (int)i0 + 3 : kBackground;
    } else {
      l.x = v[i0] > level ? (int)i0 : kBackground;
      l.y = v[i0 + 1] > level ? (int)i0 + 1 : kBackground;
      l.z = v[i0 + 2] > level ? (int)i0 + 2 : kBackground;
      l.w = v[i0 + 3] > level ? (int)i0 + 3 : kBackground;
    }
    *reinterpret_cast<int4 *>(label + i0) = l;
  } else {
    for (long long i = i0; i < n; ++i) label[i] = v[i] > level ? (int)i : kBackground;
  }
}

template <int CONN>
__global__ __launch_bounds__(kCcMergeBlock) void cc_merge_kernel(CcFrames fr, int n, int r, int *__restrict__ scratch,
                                                                 long long stride) {
  if (cc_gated_off(fr, blockIdx.y)) return;
  int *label = scratch + blockIdx.y * stride;
  const long long i = (long long)blockIdx.x * kCcMergeBlock + threadIdx.x;
  if (i >= n) return;
  const int v = (int)i;
  if (label_load(label + v) == kBackground) return;
  const unsigned uv = (unsigned)v, ur = (unsigned)r;
  const unsigned row = uv / ur;
  const int x = (int)(uv - row * ur);
  const int z = (int)(row / ur);
  const int y = (int)(row - (unsigned)z * ur);
  const int rr = r * r;
  if (CONN == 6) {
    if (x + 1 < r && label_load(label + v + 1) != kBackground) cc_union(label, v, v + 1);
    if (y + 1 < r && label_load(label + v + r) != kBackground) cc_union(label, v, v + r);
    if (z + 1 < r && label_load(label + v + rr) != kBackground) cc_union(label, v, v + rr);
  } else {
    // the 13 neighbours whose linear index is larger: (1,0,0), (-1..1,1,0) and (-1..1,-1..1,1)
#pragma unroll
    for (int dz = 0; dz <= 1; ++dz)
#pragma unroll
      for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
          if (dz * 9 + dy * 3 + dx <= 0) continue;
          const int xx = x + dx, yy = y + dy, zz = z + dz;
          if (xx < 0 || xx >= r || yy < 0 || yy >= r || zz >= r) continue;
          const int w = v + dz * rr + dy * r + dx;
          if (label_load(label + w) != kBackground) cc_union(label, v, w);
        }
  }
}

__global__ __launch_bounds__(kCcBlock) void cc_compress_kernel(CcFrames fr, int n, int *__restrict__ scratch,
                                                               long long stride) {
  if (cc_gated_off(fr, blockIdx.y)) return;
  int *label = scratch + blockIdx.y * stride;
  const long long i0 = ((long long)blockIdx.x * kCcBlock + threadIdx.x) * kCcVec;
#pragma unroll
  for (int k = 0; k < kCcVec; ++k) {
    const long long i = i0 + k;
    if (i >= n) break;
    const int p = label_load(label + i);
    if (p == kBackground) continue;
    // another thread may read this voxel on its own way up: the old parent, the root and the root's mark all lead
    // it to the same root
    const int root = cc_find(label, (int)i);
    label_store(label + i, root == (int)i ? -1 : root);
  }
}

// label[root] -= cnt (0 = lane idle) with one addition per distinct root of the wave.  While *slot_open (wave-uniform),
// the first root's total is parked in (*slot_root, *slot_cnt) instead, for the block's sum.
__device__ __forceinline__ void cc_wave_add(int *label, int root, int cnt, bool *slot_open, int *slot_root,
                                            int *slot_cnt) {
  const int lane = threadIdx.x & 63;
  bool active = cnt > 0;
  for (;;) {
    const unsigned long long m = __ballot(active);
    if (!m) break;
    const int leader = __ffsll((long long)m) - 1;
    const int r0 = __shfl(root, leader);
    const bool same = active && root == r0;
    int c = same ? cnt : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
    if (lane == leader) {
      if (*slot_open) {
        *slot_root = r0;
        *slot_cnt = c;
      } else {
        atomicAdd(label + r0, -c);
      }
    }
    *slot_open = false;
    if (same) active = false;
  }
}

__global__ __launch_bounds__(kCcBlock) void cc_count_kernel(CcFrames fr, int n, int *__restrict__ scratch,
                                                            long long stride) {
  if (cc_gated_off(fr, blockIdx.y)) return;
  int *label = scratch + blockIdx.y * stride;
  const long long i0 = ((long long)blockIdx.x * kCcBlock + threadIdx.x) * kCcVec;
  // the thread's voxels that point at a root (a root's own label is negative and only ever added to here; the
  // labels of the others are not changed by this kernel), equal roots combined
  int root[kCcVec], cnt[kCcVec];
  if (i0 + kCcVec <= n) {
    const int4 l = *reinterpret_cast<const int4 *>(label + i0);
    root[0] = l.x, root[1] = l.y, root[2] = l.z, root[3] = l.w;
  } else {
#pragma unroll
    for (int k = 0; k < kCcVec; ++k) root[k] = i0 + k < n ? label[i0 + k] : kBackground;
  }
#pragma unroll
  for (int k = 0; k < kCcVec; ++k) {
    cnt[k] = root[k] >= 0 ? 1 : 0;
#pragma unroll
    for (int j = 0; j < k; ++j)
      if (cnt[k] && cnt[j] && root[j] == root[k]) {
        cnt[j] += cnt[k];
        cnt[k] = 0;
      }
  }
  // almost all voxels of a body share ONE root: a wave's first root goes through LDS to one addition per block
  __shared__ int wroot[kCcBlock / 64], wcnt[kCcBlock / 64];
  const int wv = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) wroot[wv] = wcnt[wv] = 0;
  bool slot_open = true;
#pragma unroll
  for (int k = 0; k < kCcVec; ++k) cc_wave_add(label, root[k], cnt[k], &slot_open, &wroot[wv], &wcnt[wv]);
  __syncthreads();
  if (wv == 0) {
    const bool on = threadIdx.x < kCcBlock / 64;
    slot_open = false;
    cc_wave_add(label, on ? wroot[threadIdx.x] : 0, on ? wcnt[threadIdx.x] : 0, &slot_open, nullptr, nullptr);
  }
}

__global__ __launch_bounds__(kCcBlock) void cc_select_kernel(CcFrames fr, int n, int *__restrict__ scratch,
                                                             long long stride) {
  if (cc_gated_off(fr, blockIdx.y)) return;
  int *label = scratch + blockIdx.y * stride;
  int *head = label + stride - kCcHeaderInts;
  const long long i0 = ((long long)blockIdx.x * kCcBlock + threadIdx.x) * kCcVec;
  unsigned long long best = 0;
  int roots = 0, fg = 0;
#pragma unroll
  for (int k = 0; k < kCcVec; ++k) {
    const long long i = i0 + k;
    if (i >= n) break;
    const int l = label[i];
    if (l >= 0 || l == kBackground) continue;
    const unsigned long long key = ((unsigned long long)(unsigned)(-l) << 32) | (unsigned)~(unsigned)i;
    best = key > best ? key : best;
    ++roots;
    fg += -l;  // the sizes of a frame's roots add up to its foreground: < 2^31
  }
  if (!__syncthreads_or(roots)) return;  // most blocks hold no root
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long t = __shfl_xor(best, o);
    best = t > best ? t : best;
    roots += __shfl_xor(roots, o);
    fg += __shfl_xor(fg, o);
  }
  __shared__ unsigned long long wbest[kCcBlock / 64];
  __shared__ int wroots[kCcBlock / 64], wfg[kCcBlock / 64];
  if ((threadIdx.x & 63) == 0) {
    wbest[threadIdx.x >> 6] = best;
    wroots[threadIdx.x >> 6] = roots;
    wfg[threadIdx.x >> 6] = fg;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < kCcBlock / 64; ++k) {
      best = wbest[k] > best ? wbest[k] : best;
      roots += wroots[k];
      fg += wfg[k];
    }
    atomicMax(reinterpret_cast<unsigned long long *>(head), best);
    atomicAdd(head + 2, fg);
    atomicAdd(head + 3, roots);
  }
}

__global__ __launch_bounds__(kCcBlock) void cc_apply_kernel(CcFrames fr, int n, float fill,
                                                            const int *__restrict__ scratch, long long stride) {
  int32_t *stats = fr.stats[blockIdx.y];
  if (cc_gated_off(fr, blockIdx.y)) {
    if (blockIdx.x == 0 && threadIdx.x < 4) stats[threadIdx.x] = threadIdx.x == 3 ? -1 : 0;
    return;
  }
  const int *__restrict__ label = scratch + blockIdx.y * stride;
  const int *head = label + stride - kCcHeaderInts;
  const unsigned long long best = *reinterpret_cast<const unsigned long long *>(head);
  const int kept = best ? (int)~(unsigned)(best & 0xffffffffu) : -1;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    stats[0] = head[2];
    stats[1] = head[3];
    stats[2] = (int)(best >> 32);
    stats[3] = kept;
  }
  // `out` may be `in`: each voxel is read and written by one thread, and a voxel that keeps its value is then
  // not written at all
  const float *v = fr.vol[blockIdx.y];
  float *out = fr.out[blockIdx.y];
  const bool in_place = out == v;
  const long long i0 = ((long long)blockIdx.x * kCcBlock + threadIdx.x) * kCcVec;
  if (i0 >= n) return;
  if (i0 + kCcVec <= n) {
    const int4 l = *reinterpret_cast<const int4 *>(label + i0);
    const int lv[4] = {l.x, l.y, l.z, l.w};
    bool drop[4], any = false;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      drop[k] = lv[k] != kBackground && (lv[k] < 0 ? (int)i0 + k : lv[k]) != kept;
      any = any || drop[k];
    }
    if (in_place) {
      if (any) {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (drop[k]) out[i0 + k] = fill;
      }
    } else if ((((uintptr_t)v | (uintptr_t)out) & 15) == 0) {
      float4 q = *reinterpret_cast<const float4 *>(v + i0);
      q.x = drop[0] ? fill : q.x;
      q.y = drop[1] ? fill : q.y;
      q.z = drop[2] ? fill : q.z;
      q.w = drop[3] ? fill : q.w;
      *reinterpret_cast<float4 *>(out + i0) = q;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) out[i0 + k] = drop[k] ? fill : v[i0 + k];
    }
  } else {
    for (long long i = i0; i < n; ++i) {
      const int l = label[i];
      const bool drop = l != kBackground && (l < 0 ? (int)i : l) != kept;
      if (drop)
        out[i] = fill;
      else if (!in_place)
        out[i] = v[i];
    }
  }
}

size_t cc_scratch_bytes(int r) {
  const size_t n = (size_t)r * r * r;
  return ((n + 3) / 4 * 4 + kCcHeaderInts) * sizeof(int);
}

int launch_keep_largest_batch(mp_ctx *ctx, void *scratch, int n_frames, const float *const *vol, int r, float level,
                              int connectivity, float fill, float *const *out, int32_t *const *stats,
                              const int32_t *const *gate, hipStream_t st) {
  const long long n = (long long)r * r * r;
  if (n >= (1LL << 31)) return fail(ctx, MP_ERR_UNSUPPORTED, "keep largest: resolution %d needs 64-bit voxel indices", r);
  CcFrames fr;
  std::memset(&fr, 0, sizeof(fr));
  for (int f = 0; f < n_frames; ++f) {
    fr.vol[f] = vol[f];
    fr.out[f] = out[f];
    fr.stats[f] = stats[f];
    fr.gate[f] = gate ? gate[f] : nullptr;
  }
  int *base = static_cast<int *>(scratch);
  const long long stride = (long long)(cc_scratch_bytes(r) / sizeof(int));  // per frame: labels | header
  const long long per_block = (long long)kCcBlock * kCcVec;
  const dim3 grid((unsigned)((n + per_block - 1) / per_block), n_frames);
  const dim3 mgrid((unsigned)((n + kCcMergeBlock - 1) / kCcMergeBlock), n_frames);
  hipLaunchKernelGGL(cc_init_kernel, grid, dim3(kCcBlock), 0, st, fr, (int)n, level, base, stride);
  if (connectivity == MP_CONN_6)
    hipLaunchKernelGGL(cc_merge_kernel<6>, mgrid, dim3(kCcMergeBlock), 0, st, fr, (int)n, r, base, stride);
  else
    hipLaunchKernelGGL(cc_merge_kernel<26>, mgrid, dim3(kCcMergeBlock), 0, st, fr, (int)n, r, base, stride);
  hipLaunchKernelGGL(cc_compress_kernel, grid, dim3(kCcBlock), 0, st, fr, (int)n, base, stride);
  hipLaunchKernelGGL(cc_count_kernel, grid, dim3(kCcBlock), 0, st, fr, (int)n, base, stride);
  hipLaunchKernelGGL(cc_select_kernel, grid, dim3(kCcBlock), 0, st, fr, (int)n, base, stride);
  hipLaunchKernelGGL(cc_apply_kernel, grid, dim3(kCcBlock), 0, st, fr, (int)n, fill, base, stride);
  MP_HIP(ctx, hipGetLastError());
  return MP_OK;
}

}  // namespace mp
