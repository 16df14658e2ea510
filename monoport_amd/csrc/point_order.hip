// Order an octree level's point list by the texels its points sample (mp_octree_order_points; launch_recon calls it
// between select_compact and the level's query launch).
//
// The table query kernel (query_table.hip) gathers four table rows per point; how many DISTINCT rows the 32 points of
// a tile touch is decided by the order of the list alone, and the kernel's fraction of the MFMA roof follows that count
// (profiles/point_order_probe.txt: the same launches run 5-13 % faster on a list sorted by texel cell).  The order of
// the list is free: results are scattered by node code, and a point's value does not depend on its tile-mates.
//
// A counting sort per frame (blockIdx.z = frame, like the housekeeping kernels of octree.hip), key = y0 * W + x0 of
// bilinear tap 0, computed with the query kernels' own inline functions (lattice_coord, project_mode, in_image,
// make_taps), so that it names the rows the kernel will really load; points outside the image (NaN and +-inf
// projections included) share one last bin H * W:
//   1. order_zero_kernel       histogram [H*W + 1] int32 per frame := 0 (zeroed on the stream in EVERY call)
//   2. order_hist_kernel       key of every listed point, global atomicAdd on the frame's histogram
//   3. order_scan_kernel       exclusive scan of the histogram in place, one workgroup per frame
//   4. order_scatter_kernel    key again, slot = atomicAdd(cursor[key], 1), code -> temporary list
//   5. order_copy_kernel       temporary list -> the frame's `packed` buffer (the query launch reads the pointer and the
//                              device-side count it always read)
// No host synchronisation: counts stay on the device.  THE ORDER INSIDE A BIN IS UNSPECIFIED (slots are handed out by
// atomics), so the list may differ from run to run; volumes, status and every other output may not.
// The temporary list holds `cap` entries per frame (launch_recon: r^3 / 8; a boundary shell is ~1 % of the lattice).  A
// frame whose count exceeds `cap` is left in selection order -- every kernel takes that decision on the device from the
// same count -- which is slower in the query but stays correct.
#include "octree_common.h"
#include "query_common.h"

#pragma clang fp contract(off)

namespace mp {

__device__ __forceinline__ int texel_key(uint32_t code, const PointSrc &s, const float *__restrict__ cal, int proj,
                                         int h, int w) {
  const float px = lattice_coord(code & 1023u, s, 0);
  const float py = lattice_coord((code >> 10) & 1023u, s, 1);
  const float pz = lattice_coord(code >> 20, s, 2);
  float x, y, z;
  project_mode(cal, proj, px, py, pz, x, y, z);
  if (!in_image(x, y)) return h * w;  // NaN compares false: non-finite projections land here too
  return (int)make_taps(x, y, h, w, 1, true).o[0];  // rows of one float: the offset of tap 0 is y0 * w + x0
}

// the frame's count if it is to be sorted, else 0
__device__ __forceinline__ long long order_count(const OrderFrames &of, int f, long long cap) {
  const long long n = *of.count[f];
  return n <= cap ? n : 0;
}

__global__ __launch_bounds__(256) void order_zero_kernel(OrderFrames of, int bins) {
  int32_t *__restrict__ hist = of.hist[blockIdx.z];
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < bins) hist[t] = 0;
}

__global__ __launch_bounds__(256) void order_hist_kernel(OrderFrames of, PointSrc src, int h, int w, long long cap) {
  const int f = blockIdx.z;
  const long long n = order_count(of, f, cap);
  const uint32_t *__restrict__ packed = of.packed[f];
  int32_t *__restrict__ hist = of.hist[f];
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
    atomicAdd(hist + texel_key(packed[i], src, of.calib[f], of.proj[f], h, w), 1);
}

// in place: hist[b] := sum of hist[0 .. b - 1].  Thread t owns the bins [t * per, (t + 1) * per).
__global__ __launch_bounds__(1024) void order_scan_kernel(OrderFrames of, int bins, long long cap) {
  __shared__ int wave_sum[16];
  const int f = blockIdx.z;
  if (order_count(of, f, cap) == 0) return;  // uniform over the workgroup
  int32_t *__restrict__ hist = of.hist[f];
  const int per = (bins + 1023) / 1024;
  const int b0 = min((int)threadIdx.x * per, bins), b1 = min(b0 + per, bins);
  int mine = 0;
  for (int b = b0; b < b1; ++b) mine += hist[b];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int incl = mine;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int v = __shfl_up(incl, o);
    if (lane >= o) incl += v;
  }
  if (lane == 63) wave_sum[wave] = incl;
  __syncthreads();
  int base = incl - mine;
  for (int k = 0; k < wave; ++k) base += wave_sum[k];
  for (int b = b0; b < b1; ++b) {
    const int c = hist[b];
    hist[b] = base;
    base += c;
  }
}

__global__ __launch_bounds__(256) void order_scatter_kernel(OrderFrames of, PointSrc src, int h, int w, long long cap) {
  const int f = blockIdx.z;
  const long long n = order_count(of, f, cap);
  const uint32_t *__restrict__ packed = of.packed[f];
  uint32_t *__restrict__ tmp = of.tmp[f];
  int32_t *__restrict__ cursor = of.hist[f];
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const uint32_t code = packed[i];
    tmp[atomicAdd(cursor + texel_key(code, src, of.calib[f], of.proj[f], h, w), 1)] = code;
  }
}

__global__ __launch_bounds__(256) void order_copy_kernel(OrderFrames of, long long cap) {
  const int f = blockIdx.z;
  const long long n = order_count(of, f, cap);
  const uint32_t *__restrict__ tmp = of.tmp[f];
  uint32_t *__restrict__ packed = of.packed[f];
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
    packed[i] = tmp[i];
}

size_t point_order_scratch_bytes(long long cap, int h, int w) {
  return align256((size_t)cap * sizeof(uint32_t)) + align256(((size_t)h * w + 1) * sizeof(int32_t));
}

void point_order_carve(void *scratch, long long cap, OrderFrames &of, int f) {
  of.tmp[f] = static_cast<uint32_t *>(scratch);
  of.hist[f] = reinterpret_cast<int32_t *>(static_cast<unsigned char *>(scratch) + align256((size_t)cap * sizeof(uint32_t)));
}

int launch_point_order(mp_ctx *ctx, const OrderFrames &of, int n_frames, const PointSrc &lattice, int h, int w,
                       long long cap, hipStream_t st) {
  if (cap <= 0 || n_frames <= 0) return MP_OK;
  const int bins = h * w + 1;
  long long blocks = (cap + 255) / 256;
  if (blocks > 256) blocks = 256;  // grid-stride: 256 workgroups per frame keep the chip busy from 4 frames on
  const dim3 grid((unsigned)blocks, 1, (unsigned)n_frames);
  hipLaunchKernelGGL(order_zero_kernel, dim3((unsigned)((bins + 255) / 256), 1, (unsigned)n_frames), dim3(256), 0, st, of,
                     bins);
  hipLaunchKernelGGL(order_hist_kernel, grid, dim3(256), 0, st, of, lattice, h, w, cap);
  hipLaunchKernelGGL(order_scan_kernel, dim3(1, 1, (unsigned)n_frames), dim3(1024), 0, st, of, bins, cap);
  hipLaunchKernelGGL(order_scatter_kernel, grid, dim3(256), 0, st, of, lattice, h, w, cap);
  hipLaunchKernelGGL(order_copy_kernel, grid, dim3(256), 0, st, of, cap);
  MP_HIP(ctx, hipGetLastError());
  return MP_OK;
}

}  // namespace mp
