// Fixed-budget octree refinement: the k most uncertain nodes of a level, chosen on the device (mp_octree_select_topk,
// mp_recon_topk_batch; the definition is the header's, restated in numpy in tests/topk_ref.py).
//
// Per level, after the upsample (octree.hip): u(v) = fabsf(cur[v] - balance); a node is a CANDIDATE if it is not in
// the evaluated set (the even-coordinate image of the previous level's), u is not NaN and u <= max_dist; selected are
// the min(k, #candidates) candidates smallest under (u, z r^2 + y r + x).  u >= 0, so its bit pattern orders like an
// unsigned integer: a radix select on the 32 key bits, 11 + 11 + 10 from the top.
//   hist p     per-frame histogram of digit p over the candidates that match the prefix found so far: LDS histogram
//              per workgroup, flushed with integer atomics                                        (p = 0, 1, 2)
//   scan p     one workgroup per frame: the bin that holds the k-th key, the keys strictly below it; after p = 2 the
//              threshold key T, `below`, the number of keys equal to T and how many of those are still wanted
//   tie count  candidates with key == T per block (64 consecutive items), blocks taken in linear index order
//   tie scan   exclusive scan of those counts, one workgroup per frame
//   emit       key < T: selected; key == T: selected if its rank among the ties (scan + position in the block) is
//              below k - below.  Writes the packed list (one block-aggregated atomic on the count per block), the
//              evaluated bits and the count.
// tie count and tie scan do nothing when every tie or none is wanted (the state says so).  The phases are separated by
// launch boundaries only: no workgroup waits on another.  Integer atomics only, so the histograms, T and the
// selected SET are a pure function of the inputs; only the ORDER of the list depends on the order the waves' atomics
// land in (as in select_compact_kernel).  The host enqueues everything and knows neither T nor the counts.
//
// Work item = one 64-bit word of the bitsets = 64 consecutive x of one (z, y) row, one wave per item, items in
// (z, y, word) order: (item, lane) order is linear index order, a wave's loads are one contiguous 256 bytes, and the
// ballot of a predicate is the word.
#include <cstring>

#include "mp_internal.h"
#include "octree_common.h"

#pragma clang fp contract(off)

namespace mp {

constexpr int kTkBins = 2048;            // 11-bit digits (the last one has 10)
constexpr int kTkState = 16;             // ints of state in front of the three histograms
constexpr int kTkHeader = kTkState + 3 * kTkBins;  // per frame, zeroed per level
// tie count / emit: fixed block -> index mapping, every wave takes kTkPer consecutive items, so the barriers and the
// global atomic of a block are paid once for 64 items (with one item per wave a block lived for little more than the
// round trip of its atomic)
constexpr int kTkBlock = 1024;
constexpr int kTkWaves = kTkBlock / 64;
constexpr int kTkPer = 4;
constexpr int kTkItems = kTkWaves * kTkPer;
constexpr int kTkHistBlock = 256;        // histogram passes: grid-stride over items
constexpr int kTkHistGrid = 1024;        // workgroups per frame at most
constexpr int kTkScanBlock = 256;

// state words
enum { kT = 0, kBelow = 1, kWant = 2, kNeed = 3, kEq = 4, kAll = 5 };
// kT: the key prefix found so far, then the threshold; kBelow: candidates with a key below it; kWant: how many of the
// prefix's candidates are still wanted (k - below); kNeed / kEq (after the last scan): ties wanted / ties there;
// kAll: there are at most k candidates, every one is selected (T = 0xffffffff, which no candidate's key reaches).
// All zero (k == 0, or a gated-off frame that never gets there): nothing is selected.

__device__ __forceinline__ int digit_shift(int p) { return p == 0 ? 21 : p == 1 ? 10 : 0; }

struct TkNode {
  bool live;      // the item exists (uniform over the wave)
  bool cand;
  uint32_t key;
  u64 done;       // evaluated one level up
  int x, y, z;
  long long item;
};

// the node of (item, lane) and whether it is a candidate
__device__ __forceinline__ TkNode tk_node(const FrameBufs &fb, int f, long long item, long long n_items, int lane,
                                          int rp, int w64p, int r, int w64, float balance, float max_dist) {
  TkNode n;
  n.item = item;
  n.live = item < n_items;
  n.cand = false;
  n.key = 0;
  n.done = 0;
  n.x = n.y = n.z = 0;
  if (!n.live) return n;
  const unsigned row = (unsigned)(item / w64);
  const int w = (int)(item - (long long)row * w64);
  n.z = (int)(row / (unsigned)r);
  n.y = (int)(row - (unsigned)n.z * (unsigned)r);
  n.x = 64 * w + lane;
  if (!(n.z & 1) && !(n.y & 1)) {
    const u64 pw = fb.ev_prev[f][((long long)(n.z >> 1) * rp + (n.y >> 1)) * w64p + (w >> 1)];
    n.done = spread32(pw >> (32 * (w & 1)));
  }
  if (n.x < r) {
    const float u = fabsf(fb.cur[f][(long long)row * r + n.x] - balance);
    n.key = __float_as_uint(u);
    n.cand = !((n.done >> lane) & 1ull) && u == u && u <= max_dist;
  }
  return n;
}

__device__ __forceinline__ bool tk_gated_off(const FrameBufs &fb, int f) {
  const int32_t *g = fb.flag[f];
  return g != nullptr && *g == 0;
}

// ---- histogram of digit p -------------------------------------------------------------------------
// Real volumes hold millions of nodes with one key (out-of-image nodes are exactly 0.0, u == balance): lanes that
// share the first active lane's bin are counted with a ballot and added once; two such rounds take the dominant
// bins, whatever is left goes to the LDS histogram lane by lane.
template <int P>
__global__ __launch_bounds__(kTkHistBlock) void topk_hist_kernel(FrameBufs fb, int rp, int w64p, int r, int w64,
                                                                 float balance, float max_dist,
                                                                 int32_t *__restrict__ header) {
  const int f = blockIdx.z;
  if (tk_gated_off(fb, f)) return;
  int32_t *st = header + (long long)f * kTkHeader;
  uint32_t prefix = 0;
  if (P > 0) {
    if (st[kAll]) return;
    prefix = (uint32_t)st[kT];
  }
  int32_t *hist = st + kTkState + P * kTkBins;
  __shared__ int lds[kTkBins];
  for (int i = threadIdx.x; i < kTkBins; i += kTkHistBlock) lds[i] = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const long long n_items = (long long)r * r * w64;
  const long long wave0 = (long long)blockIdx.x * (kTkHistBlock / 64) + (threadIdx.x >> 6);
  const long long stride = (long long)gridDim.x * (kTkHistBlock / 64);
  for (long long item = wave0; item < n_items; item += stride) {
    const TkNode n = tk_node(fb, f, item, n_items, lane, rp, w64p, r, w64, balance, max_dist);
    bool in = n.cand;
    if (P == 1) in = in && (n.key >> 21) == (prefix >> 21);
    if (P == 2) in = in && (n.key >> 10) == (prefix >> 10);
    const int bin = P == 0 ? (int)(n.key >> 21) : P == 1 ? (int)((n.key >> 10) & 2047u) : (int)(n.key & 1023u);
    u64 active = __ballot(in);
#pragma unroll
    for (int round = 0; round < 2; ++round) {
      if (!active) break;
      const int leader = __ffsll((long long)active) - 1;
      const int lb = __shfl(bin, leader);
      const u64 same = __ballot(((active >> lane) & 1ull) && bin == lb);
      if (lane == leader) atomicAdd(&lds[lb], __popcll(same));
      active &= ~same;
    }
    if ((active >> lane) & 1ull) atomicAdd(&lds[bin], 1);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kTkBins; i += kTkHistBlock) {
    const int c = lds[i];
    if (c) atomicAdd(hist + i, c);
  }
}

// ---- block-wide exclusive scan of one int per thread (blockDim.x a multiple of 64, <= 1024) ------
__device__ __forceinline__ int block_exclusive_scan(int v, int *wave_sums, int *total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n_waves = blockDim.x >> 6;
  int incl = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(incl, o);
    if (lane >= o) incl += t;
  }
  __syncthreads();  // wave_sums may still be read from the previous call
  if (lane == 63) wave_sums[wave] = incl;
  __syncthreads();
  int base = 0, all = 0;
  for (int i = 0; i < n_waves; ++i) {
    const int s = wave_sums[i];
    if (i < wave) base += s;
    all += s;
  }
  *total = all;
  return base + incl - v;
}

// ---- narrow the prefix by digit p: one workgroup per frame -----------------------------------------
template <int P>
__global__ __launch_bounds__(kTkScanBlock) void topk_scan_kernel(FrameBufs fb, long long k,
                                                                 int32_t *__restrict__ header) {
  const int f = blockIdx.x;
  if (tk_gated_off(fb, f)) return;
  int32_t *st = header + (long long)f * kTkHeader;
  if (P > 0 && st[kAll]) return;
  const int32_t *hist = st + kTkState + P * kTkBins;
  __shared__ int wave_sums[kTkScanBlock / 64];
  constexpr int kPer = kTkBins / kTkScanBlock;
  const long long want = P == 0 ? k : (long long)st[kWant];  // >= 1
  int c[kPer], sum = 0;
#pragma unroll
  for (int i = 0; i < kPer; ++i) {
    c[i] = hist[threadIdx.x * kPer + i];
    sum += c[i];
  }
  int total;
  int excl = block_exclusive_scan(sum, wave_sums, &total);
  if (P == 0 && (long long)total <= want) {  // at most k candidates: all of them
    if (threadIdx.x == 0) {
      st[kT] = (int32_t)0xffffffffu;
      st[kBelow] = total;
      st[kAll] = 1;
    }
    return;
  }
  // the one thread whose bins hold the want-th key of this prefix
  if ((long long)excl < want && want <= (long long)excl + sum) {
    int b = 0;
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
      if ((long long)excl + c[i] >= want) {
        b = i;
        break;
      }
      excl += c[i];
    }
    const uint32_t digit = (uint32_t)(threadIdx.x * kPer + b);
    st[kT] = (int32_t)((uint32_t)st[kT] | (digit << digit_shift(P)));
    st[kBelow] += excl;
    st[kWant] = (int32_t)(want - excl);
    if (P == 2) {
      st[kNeed] = (int32_t)(want - excl);
      st[kEq] = c[b];
    }
  }
}

// ties are ranked only when some but not all of them are wanted
__device__ __forceinline__ bool tk_ranked(const int32_t *st) { return st[kNeed] > 0 && st[kNeed] < st[kEq]; }

// ---- ties per block ---------------------------------------------------------------------------------
__global__ __launch_bounds__(kTkBlock) void topk_tie_count_kernel(FrameBufs fb, int rp, int w64p, int r, int w64,
                                                                  float balance, float max_dist,
                                                                  const int32_t *__restrict__ header,
                                                                  int32_t *__restrict__ tie_count, int n_blocks) {
  const int f = blockIdx.z;
  if (tk_gated_off(fb, f)) return;
  const int32_t *st = header + (long long)f * kTkHeader;
  if (!tk_ranked(st)) return;
  const uint32_t T = (uint32_t)st[kT];
  __shared__ int wave_ties[kTkWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long n_items = (long long)r * r * w64;
  const long long item0 = (long long)blockIdx.x * kTkItems + wave * kTkPer;
  int ties = 0;
#pragma unroll
  for (int j = 0; j < kTkPer; ++j) {
    const TkNode n = tk_node(fb, f, item0 + j, n_items, lane, rp, w64p, r, w64, balance, max_dist);
    ties += __popcll(__ballot(n.cand && n.key == T));
  }
  if (lane == 0) wave_ties[wave] = ties;
  __syncthreads();
  if (threadIdx.x == 0) {
    int s = 0;
    for (int i = 0; i < kTkWaves; ++i) s += wave_ties[i];
    tie_count[(long long)f * n_blocks + blockIdx.x] = s;
  }
}

// ---- exclusive scan of the tie counts: one workgroup per frame -----------------------------------------
__global__ __launch_bounds__(kTkBlock) void topk_tie_scan_kernel(FrameBufs fb, const int32_t *__restrict__ header,
                                                                 const int32_t *__restrict__ tie_count,
                                                                 int32_t *__restrict__ tie_base, int n_blocks) {
  const int f = blockIdx.x;
  if (tk_gated_off(fb, f)) return;
  if (!tk_ranked(header + (long long)f * kTkHeader)) return;
  __shared__ int wave_sums[kTkBlock / 64];
  const int32_t *in = tie_count + (long long)f * n_blocks;
  int32_t *out = tie_base + (long long)f * n_blocks;
  int carry = 0;
  for (int i0 = 0; i0 < n_blocks; i0 += kTkBlock) {  // uniform trip count
    const int i = i0 + threadIdx.x;
    const int v = i < n_blocks ? in[i] : 0;
    int total;
    const int excl = block_exclusive_scan(v, wave_sums, &total);
    if (i < n_blocks) out[i] = carry + excl;
    carry += total;
  }
}

// ---- emit ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kTkBlock) void topk_emit_kernel(FrameBufs fb, int rp, int w64p, int r, int w64,
                                                             float balance, float max_dist,
                                                             const int32_t *__restrict__ header,
                                                             const int32_t *__restrict__ tie_base, int n_blocks) {
  const int f = blockIdx.z;
  if (tk_gated_off(fb, f)) return;
  const int32_t *st = header + (long long)f * kTkHeader;
  const uint32_t T = (uint32_t)st[kT];
  const int need = st[kNeed];
  const bool ranked = tk_ranked(st);  // uniform over the frame
  __shared__ int wave_ties[kTkWaves];
  __shared__ int wave_sel[kTkWaves];
  __shared__ int block_base;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const u64 below_lane = (1ull << lane) - 1ull;
  const long long n_items = (long long)r * r * w64;
  const long long item0 = (long long)blockIdx.x * kTkItems + wave * kTkPer;
  // the wave's kTkPer consecutive items, in linear index order
  bool live[kTkPer], lt[kTkPer], eq[kTkPer];
  u64 done[kTkPer], beq[kTkPer];
  uint32_t code[kTkPer];
  int ties = 0;
#pragma unroll
  for (int j = 0; j < kTkPer; ++j) {
    const TkNode n = tk_node(fb, f, item0 + j, n_items, lane, rp, w64p, r, w64, balance, max_dist);
    live[j] = n.live;
    lt[j] = n.cand && n.key < T;
    eq[j] = n.cand && n.key == T;
    done[j] = n.done;
    code[j] = (uint32_t)n.x | ((uint32_t)n.y << 10) | ((uint32_t)n.z << 20);
    beq[j] = __ballot(eq[j]);
    ties += __popcll(beq[j]);
  }
  int rank = 0;
  if (ranked) {
    if (lane == 0) wave_ties[wave] = ties;
    __syncthreads();
    rank = tie_base[(long long)f * n_blocks + blockIdx.x];
    for (int i = 0; i < wave; ++i) rank += wave_ties[i];
  }
  u64 sel[kTkPer];
  bool s[kTkPer];
  int n_sel = 0;
#pragma unroll
  for (int j = 0; j < kTkPer; ++j) {
    // not ranked: every tie (need == eq count) or none (need == 0)
    const bool take = eq[j] && (ranked ? rank + __popcll(beq[j] & below_lane) < need : need > 0);
    rank += __popcll(beq[j]);
    s[j] = lt[j] || take;
    sel[j] = __ballot(s[j]);
    n_sel += __popcll(sel[j]);
  }
  // one atomic on the count per block: the waves' popcounts meet in LDS (with one atomic per wave the 100 k waves
  // of a 257^3 level that select something queued up on the one address: 0.45 ms of a 0.57 ms selection)
  if (lane == 0) wave_sel[wave] = n_sel;
  __syncthreads();
  if (threadIdx.x == 0) {
    int total = 0;
    for (int i = 0; i < kTkWaves; ++i) total += wave_sel[i];
    block_base = total ? atomicAdd(fb.count[f], total) : 0;
  }
  __syncthreads();
  int base = block_base;
  for (int i = 0; i < wave; ++i) base += wave_sel[i];
#pragma unroll
  for (int j = 0; j < kTkPer; ++j) {
    if (!live[j]) break;
    if (lane == 0) fb.ev[f][item0 + j] = done[j] | sel[j];
    if (s[j]) fb.packed[f][base + __popcll(sel[j] & below_lane)] = code[j];
    base += __popcll(sel[j]);
  }
}

// ---- host ---------------------------------------------------------------------------------------------
static inline int tk_blocks(int r) {
  const long long n_items = (long long)r * r * words64(r);
  return (int)((n_items + kTkItems - 1) / kTkItems);
}

size_t topk_scratch_bytes(int n_frames, int r) {
  return align256((size_t)n_frames * kTkHeader * sizeof(int32_t)) +
         2 * align256((size_t)n_frames * tk_blocks(r) * sizeof(int32_t)) + 256;
}

int launch_topk_select(mp_ctx *ctx, void *scratch, const FrameBufs &fb, int n_frames, int rp, int r, long long k,
                       float max_dist, float balance, hipStream_t st) {
  const int w64 = words64(r), w64p = words64(rp), n_blocks = tk_blocks(r);
  unsigned char *p = static_cast<unsigned char *>(scratch);
  int32_t *header = reinterpret_cast<int32_t *>(p);
  p += align256((size_t)n_frames * kTkHeader * sizeof(int32_t));
  int32_t *tie_count = reinterpret_cast<int32_t *>(p);
  p += align256((size_t)n_frames * n_blocks * sizeof(int32_t));
  int32_t *tie_base = reinterpret_cast<int32_t *>(p);
  MP_HIP(ctx, hipMemsetAsync(header, 0, (size_t)n_frames * kTkHeader * sizeof(int32_t), st));
  const dim3 per_block(n_blocks, 1, n_frames);
  if (k > 0) {  // k == 0: the zeroed state selects nothing, emit only writes the evaluated bits
    const long long waves = (long long)r * r * w64;
    const long long hb = (waves + kTkHistBlock / 64 - 1) / (kTkHistBlock / 64);
    const dim3 hist_grid((unsigned)(hb < kTkHistGrid ? hb : kTkHistGrid), 1, n_frames);
#define MP_TOPK_DIGIT(P)                                                                                          \
  hipLaunchKernelGGL((topk_hist_kernel<P>), hist_grid, dim3(kTkHistBlock), 0, st, fb, rp, w64p, r, w64, balance, \
                     max_dist, header);                                                                           \
  hipLaunchKernelGGL((topk_scan_kernel<P>), dim3(n_frames), dim3(kTkScanBlock), 0, st, fb, k, header)
    MP_TOPK_DIGIT(0);
    MP_TOPK_DIGIT(1);
    MP_TOPK_DIGIT(2);
#undef MP_TOPK_DIGIT
    hipLaunchKernelGGL(topk_tie_count_kernel, per_block, dim3(kTkBlock), 0, st, fb, rp, w64p, r, w64, balance,
                       max_dist, header, tie_count, n_blocks);
    hipLaunchKernelGGL(topk_tie_scan_kernel, dim3(n_frames), dim3(kTkBlock), 0, st, fb, header, tie_count, tie_base,
                       n_blocks);
  }
  hipLaunchKernelGGL(topk_emit_kernel, per_block, dim3(kTkBlock), 0, st, fb, rp, w64p, r, w64, balance, max_dist,
                     header, tie_base, n_blocks);
  MP_HIP(ctx, hipGetLastError());
  return MP_OK;
}

}  // namespace mp
