// What the mesh stages share on the device: the 1024-thread block scan of the count -> block sums -> scan -> emit
// passes (mcubes.hip, simplify.hip) and the clamp of a device count to its capacity (mesh.hip, simplify.hip).
#pragma once
#include "mp_internal.h"

namespace mp {

constexpr int kScanBlock = 1024;

// exclusive prefix of `val` over the 1024 threads of the block; *total = block sum
__device__ __forceinline__ int block_exclusive_scan(int val, int *total) {
  __shared__ int wsum[kScanBlock / 64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int incl = val;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(incl, o);
    if (lane >= o) incl += t;
  }
  __syncthreads();  // protects wsum across consecutive calls
  if (lane == 63) wsum[wv] = incl;
  __syncthreads();
  int base = 0, tot = 0;
#pragma unroll
  for (int k = 0; k < kScanBlock / 64; ++k) {
    const int s = wsum[k];
    if (k < wv) base += s;
    tot += s;
  }
  *total = tot;
  return base + incl - val;
}

// a device count (vertices / faces present) cut to the capacity of its buffer
__device__ __forceinline__ int mesh_min(int count, long long cap) {
  if (count < 0) return 0;
  return (long long)count < cap ? count : (int)cap;
}

}  // namespace mp
