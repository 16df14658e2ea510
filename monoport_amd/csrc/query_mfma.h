// MFMA building blocks of the fused f32 query kernels (query.hip: 64-point tiles, query_small.hip:
// 32-point tiles for launches that cannot fill the chip): fragment-stream segments, the z column,
// bias initialisation, leaky ReLU, the point-major hidden-chunk store and the 64-point tile's layers.
#pragma once
#include "mp_internal.h"
#include "query_common.h"

// Reference parity is op-order parity: keep every a*b+c exactly as written (the HIP headers
// define __fmul_rn & co. as plain operators, which hipcc would otherwise contract into FMAs).
// Fused multiply-adds are requested explicitly (fmaf / MFMA) where they are wanted.
#pragma clang fp contract(off)

constexpr int kPrefetch1 = 1;  // A-fragment prefetch distance (k-groups) of the MR = 4 / MR = 2 segments
constexpr int kPrefetch0 = 3;  // same for layer 0's MR = 1 segment

namespace mp {

// ---- MFMA building blocks ----------------------------------------------------------------------
template <int MR, int NR>
__device__ __forceinline__ void mma_group(f32x16 (&acc)[MR][NR], const f32x4 (&a)[MR],
                                          const f32x4 (&b)[NR]) {
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int m = 0; m < MR; ++m)
#pragma unroll
      for (int n = 0; n < NR; ++n)
        acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[m][i], b[n][i], acc[m][n], 0, 0, 0);
}

// acc[MR][NR] += A[rows of this wave][K segment] * B[K segment][points], in two calls:
//   seg_prefetch : issue the first PF groups of A into the ring -- placed EARLY by the caller
//                  (before the previous segment's epilogue / barrier) so L2 latency is hidden;
//   seg_main     : the K loop.  Every iteration issues the A fragment PF groups ahead and the B
//                  operand one group ahead, then the 4*MR*NR MFMAs of the current group.
//   a: fragment stream of row block 0 at group 0 as a wave-uniform index into the weight buffer
//      (16-byte units; the lane's slot is added by the buffer load); row block m is
//      a + m * rb_stride; group g is + g * 64.
//   b: LDS byte address of this lane's point row for column block 0; column block n is
//      + n * 32 * ROWB; group g lives in 16-byte slot (2g + h) ^ (p & 15) = (2g) ^ swz.
// The loop is deliberately NOT unrolled beyond the ring size: hipcc clusters every load of a
// big unrolled block at its top and spills the accumulators.
template <int MR, int PF>
__device__ __forceinline__ void seg_prefetch(f32x4 (&ring)[PF + 1][MR], const WStream &ws, int a,
                                             int rb_stride, int n_groups) {
#pragma unroll
  for (int d = 0; d < PF; ++d)
#pragma unroll
    for (int m = 0; m < MR; ++m)
      ring[d][m] = wload128(ws, a + m * rb_stride + min(d, n_groups - 1) * 64);
}

template <int MR, int NR, int PF, int ROWB>
__device__ __forceinline__ void seg_main(f32x16 (&acc)[MR][NR], f32x4 (&ring)[PF + 1][MR],
                                         const WStream &ws, int a, int rb_stride, int n_groups,
                                         const unsigned char *b, int swz) {
  constexpr int RS = PF + 1;
  f32x4 bcur[NR];
#pragma unroll
  for (int n = 0; n < NR; ++n)
    bcur[n] = *reinterpret_cast<const f32x4 *>(b + n * 32 * ROWB + (swz << 4));
#pragma unroll 1
  for (int g0 = 0; g0 < n_groups; g0 += RS) {
#pragma unroll
    for (int r = 0; r < RS; ++r) {
      const int g = g0 + r;
      const int gp = min(g + PF, n_groups - 1);
#pragma unroll
      for (int m = 0; m < MR; ++m)
        ring[(r + PF) % RS][m] = wload128(ws, a + m * rb_stride + gp * 64);
      const int boff = ((2 * min(g + 1, n_groups - 1)) ^ swz) << 4;
      f32x4 bnxt[NR];
#pragma unroll
      for (int n = 0; n < NR; ++n)
        bnxt[n] = *reinterpret_cast<const f32x4 *>(b + n * 32 * ROWB + boff);
      // keep the prefetches ABOVE this group's MFMAs: left alone, hipcc sinks them to the end of
      // the group (to recycle registers) and every group then starts with a full L2 round trip
      __builtin_amdgcn_sched_barrier(0);
      mma_group<MR, NR>(acc, ring[r % RS], bcur);
#pragma unroll
      for (int n = 0; n < NR; ++n) bcur[n] = bnxt[n];
    }
  }
}

// seg_main for ONE row block x ONE column block (layer 3 of the wave-specialised table kernel: 32 rows per consumer
// wave) with the k-steps alternating between TWO accumulators: a wave whose MFMAs chain through a single accumulator
// runs at 2/3 of the matrix rate when another wave shares its SIMD (profiles/r03y_mfma_peak_probe.txt); two
// independent chains restore it.  The caller adds the two accumulators at the end (addition order is free).
template <int PF, int ROWB>
__device__ __forceinline__ void seg_main_split(f32x16 &acc_e, f32x16 &acc_o, f32x4 (&ring)[PF + 1][1], const WStream &ws,
                                               int a, int n_groups, const unsigned char *b, int swz) {
  constexpr int RS = PF + 1;
  f32x4 bcur = *reinterpret_cast<const f32x4 *>(b + (swz << 4));
#pragma unroll 1
  for (int g0 = 0; g0 < n_groups; g0 += RS) {
#pragma unroll
    for (int r = 0; r < RS; ++r) {
      const int g = g0 + r;
      const int gp = min(g + PF, n_groups - 1);
      ring[(r + PF) % RS][0] = wload128(ws, a + gp * 64);
      const int boff = ((2 * min(g + 1, n_groups - 1)) ^ swz) << 4;
      const f32x4 bnxt = *reinterpret_cast<const f32x4 *>(b + boff);
      __builtin_amdgcn_sched_barrier(0);
      const f32x4 af = ring[r % RS][0];
      acc_e = __builtin_amdgcn_mfma_f32_32x32x2f32(af[0], bcur[0], acc_e, 0, 0, 0);
      acc_o = __builtin_amdgcn_mfma_f32_32x32x2f32(af[1], bcur[1], acc_o, 0, 0, 0);
      acc_e = __builtin_amdgcn_mfma_f32_32x32x2f32(af[2], bcur[2], acc_e, 0, 0, 0);
      acc_o = __builtin_amdgcn_mfma_f32_32x32x2f32(af[3], bcur[3], acc_o, 0, 0, 0);
      bcur = bnxt;
    }
  }
}

// The z column: one k-step whose B operand is z_feat in lanes 0-31 and 0 in lanes 32-63.
template <int MR, int NR>
__device__ __forceinline__ void gemm_z(f32x16 (&acc)[MR][NR], const float (&az)[MR],
                                       const float (&zb)[NR]) {
#pragma unroll
  for (int m = 0; m < MR; ++m)
#pragma unroll
    for (int n = 0; n < NR; ++n)
      acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(az[m], zb[n], acc[m][n], 0, 0, 0);
}

// Accumulators start from the bias: register t of lane (j, h) of a C-layout tile holds row
// (t & 3) + 8 (t >> 2) + 4 h of the 32-row block (cdna_hip_programming.md section 3), so the 16
// registers are four 16-byte pieces of the bias vector.
__device__ __forceinline__ void init_from_bias(f32x16 &v, const WStream &ws, int bias32) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const f32x4 bq = wload_bias4(ws, bias32 + 8 * q);
#pragma unroll
    for (int i = 0; i < 4; ++i) v[4 * q + i] = bq[i];
  }
}

__device__ __forceinline__ void lrelu(f32x16 &v) {
#pragma unroll
  for (int t = 0; t < 16; ++t)
    v[t] = fmaxf(v[t], v[t] * 0.01f);  // = v > 0 ? v : 0.01 v (F.leaky_relu, SurfaceClassifier.py:58), bit for bit
}

// Store a C-layout 32x32 tile into the hidden-chunk buffer, point-major: rows 8q+4h..+3 of a
// point are 4 consecutive floats = one 16-byte slot.
template <int ROWBYTES = kHbRowBytes>
__device__ __forceinline__ void store_hidden(unsigned char *hb, const f32x16 &v, int rb_local,
                                             int cb, int j, int h) {
  const int p = 32 * cb + j;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int slot = 8 * rb_local + 2 * q + h;
    f32x4 o = {v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]};
    *reinterpret_cast<f32x4 *>(hb + p * ROWBYTES + ((slot ^ (p & 15)) << 4)) = o;
  }
}

// ---- the 64-point tile's layer chain (query.hip, query_views.hip) ------------------------------
// Four waves, one tile of 64 columns: xs = the feature tile [64][C] and hb = the hidden-chunk buffer
// [64][64 rows] (both f32, point-major, swizzled 16-byte slots), zb = z_feat of the two column blocks
// as B operands (lanes 0-31).  Layer 0 (1024 x (C + 1)) is never materialised: it is produced in
// 64-row chunks that go through hb straight into layer 1's K loop, whose 512 x 64 accumulator tile
// is spread over the 4 waves' registers (128 VGPRs each); layer 2 consumes layer 1 the same way,
// chunk by chunk from the owning wave's registers.  The skip-concat (SurfaceClassifier.py:55) is a
// second K segment read from xs.  Leaves layer 2's rows [64 wv, +64) after the leaky ReLU in acc2.
template <int C>
__device__ __forceinline__ void mlp64_layers012(f32x16 (&acc2)[2][2], const MlpPack &mlp, const WStream &ws,
                                                const unsigned char *xs, unsigned char *hb, const float (&zb)[2],
                                                int wv, int j, int h, int swz) {
  constexpr int ROWB = C * 4;
  constexpr int NGX = C / 8;  // K groups of the feature segment
  const unsigned char *xrow = xs + j * ROWB;       // this lane's point row, column block 0
  const unsigned char *hrow = hb + j * kHbRowBytes;

  // ---------------- layers 0 + 1, fused over 64-row chunks of layer 0 ----------------
  f32x16 acc1[4][2];
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    init_from_bias(acc1[m][0], ws, mlp.bias[1] + 32 * (4 * wv + m));
    acc1[m][1] = acc1[m][0];
  }
  {
    const int rb0 = wv >> 1, cb0 = wv & 1;  // this wave's tile inside a layer-0 chunk
    const int a0 = mlp.ax[0] / 4;           // 16-byte units (segments are 256-byte aligned)
    const int a1 = mlp.ah[1] / 4 + (4 * wv) * (kHidden[0] / 8) * 64;
    const float zz[1] = {zb[cb0]};
    f32x4 ring0[kPrefetch0 + 1][1];
    f32x16 acc0[1][1];
    float az0[1];
    seg_prefetch<1, kPrefetch0>(ring0, ws, a0 + rb0 * NGX * 64, 0, NGX);
    init_from_bias(acc0[0][0], ws, mlp.bias[0] + 32 * rb0);
    az0[0] = wload32(ws, mlp.az[0] + rb0 * 64);
#pragma unroll 1
    for (int ck = 0; ck < kHidden[0] / 64; ++ck) {
      // layer-0 rows [64 ck + 32 rb0, +32) x points [32 cb0, +32)
      const int rb = 2 * ck + rb0;
      seg_main<1, 1, kPrefetch0, ROWB>(acc0, ring0, ws, a0 + rb * NGX * 64, 0, NGX, xrow + cb0 * 32 * ROWB, swz);
      // layer-1 weights of this chunk start streaming before the chunk is even stored
      f32x4 ring1[kPrefetch1 + 1][4];
      seg_prefetch<4, kPrefetch1>(ring1, ws, a1 + ck * 8 * 64, (kHidden[0] / 8) * 64, 8);
      gemm_z<1, 1>(acc0, az0, zz);
      lrelu(acc0[0][0]);
      store_hidden(hb, acc0[0][0], rb0, cb0, j, h);
      // next chunk's layer-0 operands
      const int rbn = min(rb + 2, kHidden[0] / 32 - 2 + rb0);
      seg_prefetch<1, kPrefetch0>(ring0, ws, a0 + rbn * NGX * 64, 0, NGX);
      init_from_bias(acc0[0][0], ws, mlp.bias[0] + 32 * rbn);
      az0[0] = wload32(ws, mlp.az[0] + rbn * 64);
      __syncthreads();
      // layer-1 rows [128 wv, +128) += W1[:, 64 ck .. +64) * chunk
      seg_main<4, 2, kPrefetch1, kHbRowBytes>(acc1, ring1, ws, a1 + ck * 8 * 64, (kHidden[0] / 8) * 64, 8,
                                              hrow, swz);
      __syncthreads();
    }
    // skip segment of layer 1: W1[:, 1024 .. 1024 + C] * x, then the z column
    const int a1x = mlp.ax[1] / 4 + (4 * wv) * NGX * 64;
    f32x4 ring1[kPrefetch1 + 1][4];
    float az1[4];
    seg_prefetch<4, kPrefetch1>(ring1, ws, a1x, NGX * 64, NGX);
#pragma unroll
    for (int m = 0; m < 4; ++m) az1[m] = wload32(ws, mlp.az[1] + (4 * wv + m) * 64);
    seg_main<4, 2, kPrefetch1, ROWB>(acc1, ring1, ws, a1x, NGX * 64, NGX, xrow, swz);
    gemm_z<4, 2>(acc1, az1, zb);
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int n = 0; n < 2; ++n) lrelu(acc1[m][n]);
  }

  // ---------------- layer 2: rows [64 wv, +64), K = 512 hidden (8 chunks) + skip ----------------
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    init_from_bias(acc2[m][0], ws, mlp.bias[2] + 32 * (2 * wv + m));
    acc2[m][1] = acc2[m][0];
  }
  {
    const int a2 = mlp.ah[2] / 4 + (2 * wv) * (kHidden[1] / 8) * 64;
    f32x4 ring2[2][2];
    seg_prefetch<2, 1>(ring2, ws, a2, (kHidden[1] / 8) * 64, 8);
#pragma unroll
    for (int ck = 0; ck < 8; ++ck) {
      if (wv == (ck >> 1)) {  // owner of hidden rows [64 ck, +64): row blocks 2(ck&1), +1
#pragma unroll
        for (int mm = 0; mm < 2; ++mm)
#pragma unroll
          for (int n = 0; n < 2; ++n) store_hidden(hb, acc1[2 * (ck & 1) + mm][n], mm, n, j, h);
      }
      __syncthreads();
      seg_main<2, 2, 1, kHbRowBytes>(acc2, ring2, ws, a2 + ck * 8 * 64, (kHidden[1] / 8) * 64, 8,
                                     hrow, swz);
      if (ck < 7) seg_prefetch<2, 1>(ring2, ws, a2 + (ck + 1) * 8 * 64, (kHidden[1] / 8) * 64, 8);
      __syncthreads();
    }
    const int a2x = mlp.ax[2] / 4 + (2 * wv) * NGX * 64;
    float az2[2];
    seg_prefetch<2, 1>(ring2, ws, a2x, NGX * 64, NGX);
#pragma unroll
    for (int m = 0; m < 2; ++m) az2[m] = wload32(ws, mlp.az[2] + (2 * wv + m) * 64);
    seg_main<2, 2, 1, ROWB>(acc2, ring2, ws, a2x, NGX * 64, NGX, xrow, swz);
    gemm_z<2, 2>(acc2, az2, zb);
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int n = 0; n < 2; ++n) lrelu(acc2[m][n]);
  }
}

// Layer 4 (Cout x (128 + C + 1)) on the VALU, without bias and z term: partial sums of the 64 columns
// into red[part][o][p], parts 0-3 = hidden rows of wave `part` (acc3 = layer 3's rows [32 wv, +32)),
// parts 4-7 = feature quarter of wave `part - 4`.  K4 = padded row stride of the last layer (pack.hip).
template <int C, int COUT>
__device__ __forceinline__ void mlp64_layer4_partials(float *red, const f32x16 (&acc3)[1][2], const MlpPack &mlp,
                                                      const unsigned char *xs, int wv, int lane, int j,
                                                      int h) {
  constexpr int ROWB = C * 4;
  constexpr int K4 = (kHidden[3] + C + 1 + 3) & ~3;
  // hidden part: this lane holds rows 32 wv + 8q + 4h + i of points 32 cb + j
#pragma unroll
  for (int o = 0; o < COUT; ++o) {
    const float *w4 = (mlp.base + mlp.w4) + o * K4 + 32 * wv + 4 * h;
    float s0 = 0.0f, s1 = 0.0f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const f32x4 wq = *reinterpret_cast<const f32x4 *>(w4 + 8 * q);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        s0 = fmaf(wq[i], acc3[0][0][4 * q + i], s0);
        s1 = fmaf(wq[i], acc3[0][1][4 * q + i], s1);
      }
    }
    s0 += __shfl_xor(s0, 32);
    s1 += __shfl_xor(s1, 32);
    if (h == 0) {
      red[(wv * COUT + o) * kTilePts + j] = s0;
      red[(wv * COUT + o) * kTilePts + 32 + j] = s1;
    }
  }
  // feature part: lane = point, wave = quarter of the C channels
  const int p = lane;
  float sx[COUT];
#pragma unroll
  for (int o = 0; o < COUT; ++o) sx[o] = 0.0f;
  constexpr int SLOTS = C / 16;  // 16-byte slots per quarter
#pragma unroll 4
  for (int s = 0; s < SLOTS; ++s) {
    const int slot = wv * SLOTS + s;
    const f32x4 xv = *reinterpret_cast<const f32x4 *>(xs + p * ROWB + ((slot ^ (p & 15)) << 4));
#pragma unroll
    for (int o = 0; o < COUT; ++o) {
      const f32x4 wq =
          *reinterpret_cast<const f32x4 *>((mlp.base + mlp.w4) + o * K4 + kHidden[3] + 4 * slot);
#pragma unroll
      for (int i = 0; i < 4; ++i) sx[o] = fmaf(wq[i], xv[i], sx[o]);
    }
  }
#pragma unroll
  for (int o = 0; o < COUT; ++o) red[((4 + wv) * COUT + o) * kTilePts + p] = sx[o];
}

}  // namespace mp
