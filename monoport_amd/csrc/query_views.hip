// Multi-view PIFu query for gfx950 (MI355X): SurfaceClassifier(num_views = V > 1) in eval mode
// (heads/SurfaceClassifier.py:39-71 with the view mean of :60-66) behind MonoPortNet.query
// (MonoPortNet.py:48-91), fused like pifu_query_kernel (query.hip).
//
// Tile mapping: a tile's 64 MFMA columns are (point, view) pairs, column p = V g + v for the
// G = floor(64 / V) points g of the tile and the V views v; a point's views never split across
// tiles, columns >= G V stay dead.  Per column the kernel is the plain kernel:
//   * gather: column p samples view v's map at view v's projection of point g.  Unlike the plain
//     kernel a finite point OUTSIDE the image is sampled too (grid_sample's zero padding, partial
//     taps at the border): its features feed the view mean.  Non-finite projections sample 0 and
//     poison the whole point at the end (NaN in every row, as the reference's NaN samples do).
//   * layers 0-2 unchanged, each column on its own features and z.
//   * after layer 2's leaky ReLU (i == len(filters) // 2) every column of a group is replaced by
//     the group mean IN PLACE, once per 64-row chunk of layer 2's output as it passes through the
//     hidden-chunk buffer `hb` on its way into layer 3, and once for the feature tile `xs` (which
//     layer 3's and layer 4's skip segments read): tmpy = feature.view(-1,V,C+1,N).mean(1).  The
//     mean sums in view order and divides by V with one IEEE division -- torch's CPU mean over the
//     view axis bit for bit -- so it adds no rounding of its own.  No LDS beyond the plain kernel's.
//   * layers 3-4 run per column (redundantly within a group, ~6 % of the FLOPs); column (g, v)
//     writes row v of the result with view v's in-image mask: preds = in_img[:, None] * pred
//     ([V,1,N] * [1,Cout,N], MonoPortNet.py:89).
// With V = 1 every column is its own group and the result equals pifu_query_kernel's bit for bit.
//
// LATTICE = true (mp_recon_views, one octree level): the points are the level's packed node list
// (x | y<<10 | z<<20, shared by all views) turned into world coordinates by lattice_coord, their number is read
// from device memory, and only the columns of ONE view write: row `view` of the result, scattered to
// volume[z,y,x].  Gather, layers, view mean and tile mapping are those of the explicit-point kernel.
//
// LATTICE and BATCH (mp_recon_views_batch, one octree level of n frames): the tiles of the frames form one index
// space as in query_common.h ("tiles of a launch") with P = G: frame f owns the next ceil(count_f / G) global tiles,
// so a tile never spans two frames, a frame without nodes owns none, and the coarse levels of several frames fill
// the machine together.  The owner is looked up from the device-side counts at the top of every tile iteration and
// made wave-uniform there; from then on the tile is a tile of the one-frame lattice kernel on that frame's node
// list, volume, maps and calibrations (ViewLatticeFrame), line for line.
//
// BATCH without LATTICE (mp_query_views_counted_batch, explicit points of n frames counted on the device): the same
// tile ownership over the frames' clamped counts; a frame's tile is a tile of the explicit-point kernel on that
// frame's [3, capacity] points, shared by its views as a lattice's nodes are (ViewPointsFrame: load_point reads
// them), and only the columns of ONE view write: row `view`, to out[f][o * capacity + i] for i < count_f.
#include <cstring>

#include "mp_internal.h"
#include "query_common.h"

#include "query_mfma.h"

#pragma clang fp contract(off)

namespace mp {

// group mean of V consecutive point rows of a swizzled point-major LDS tile, in place: the point's
// view sum in view order, then one IEEE division by V (SurfaceClassifier.py:61-66, torch CPU mean)
template <int ROWBYTES>
__device__ __forceinline__ void group_mean_inplace(unsigned char *buf, int nv, int groups, int tid) {
  constexpr int SLOTS = ROWBYTES / 16;
  const float fv = (float)nv;
  for (int u = tid; u < groups * SLOTS; u += kQueryThreads) {
    const int g = u / SLOTS, s = u - g * SLOTS;
    const int p0 = g * nv;
    f32x4 sum = *reinterpret_cast<const f32x4 *>(buf + p0 * ROWBYTES + ((s ^ (p0 & 15)) << 4));
    for (int v = 1; v < nv; ++v) {
      const int p = p0 + v;
      sum += *reinterpret_cast<const f32x4 *>(buf + p * ROWBYTES + ((s ^ (p & 15)) << 4));
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) sum[i] = __fdiv_rn(sum[i], fv);
    for (int v = 0; v < nv; ++v) {
      const int p = p0 + v;
      *reinterpret_cast<f32x4 *>(buf + p * ROWBYTES + ((s ^ (p & 15)) << 4)) = sum;
    }
  }
}

// column p (< 64) of a tile -> (point g, view v) = (p / V, p % V) with one multiply and shift: magic =
// ceil(65536 / V) is exact for p < 64, V <= 8, and keeps the per-lane integer division out of the kernel
__device__ __forceinline__ void column_view(int p, int nv, int magic, int &g, int &v) {
  g = (p * magic) >> 16;
  v = p - g * nv;
}

// z_feat of point n in view u: the view's projection z times z_scale (MonoPortNet.py:72, :78);
// DIRECT: row C of view u's explicit feature columns
// LATTICE: point n of set.src, shared by the views (a level's node list, or a counted frame's explicit points),
// instead of view u's own explicit point
template <int C, bool DIRECT, bool LATTICE, typename SET>
__device__ __forceinline__ float view_z(const SET &set, int u, long long n, float z_scale,
                                        float &x, float &y) {
  if constexpr (DIRECT) {
    x = 0.0f;
    y = 0.0f;
    return set.pts[u][(long long)C * set.sc + n];
  } else if constexpr (LATTICE) {
    float px, py, pz, z;
    uint32_t code;
    load_point(set.src, n, px, py, pz, code);
    project_mode(set.calib[u], set.proj, px, py, pz, x, y, z);
    return __fmul_rn(z, z_scale);
  } else {
    const float *__restrict__ cal = set.calib[u];
    const float *__restrict__ q = set.pts[u] + n * set.sn;
    float z;
    project_mode(cal, set.proj, q[0], q[set.sc], q[2 * set.sc], x, y, z);
    return __fmul_rn(z, z_scale);
  }
}

// z_feat of column p of the tile starting at point n0: its own view's, or (mean) the group mean over the
// views, summed in view order and divided by V like the feature means; 0 for dead columns
template <int C, bool DIRECT, bool LATTICE, typename SET>
__device__ __forceinline__ float column_z(const SET &set, int p, int magic, long long n0, long long n_pts,
                                          int ncol, float z_scale, bool mean) {
  const int nv = set.nv;
  int g, v;
  column_view(p, nv, magic, g, v);
  const long long n = n0 + g;
  if (p >= ncol || n >= n_pts) return 0.0f;
  if (!mean) {
    float x, y;
    return view_z<C, DIRECT, LATTICE>(set, v, n, z_scale, x, y);
  }
  float sum = 0.0f;
  for (int u = 0; u < nv; ++u) {
    float x, y;
    const float zf = view_z<C, DIRECT, LATTICE>(set, u, n, z_scale, x, y);
    sum = u == 0 ? zf : sum + zf;
  }
  return __fdiv_rn(sum, (float)nv);
}

// DIRECT = true: SurfaceClassifier.forward on explicit features [V][C+1][N] (set.pts[v], row
// stride set.sc), one output [Cout, N] written by the view-0 columns.
// LATTICE = true: one octree level (see the head of this file); `set` is then a ViewLatticeDev.
// BATCH (with LATTICE): the same level of n frames; `set` is then a ViewLatticeBatchDev.
// BATCH (without LATTICE): counted explicit points of n frames; `set` is then a ViewPointsBatchDev.
template <bool LATTICE, bool BATCH = false>
struct ViewSetArg {
  typedef ViewSetDev type;
};
template <>
struct ViewSetArg<true, false> {
  typedef ViewLatticeDev type;
};
template <>
struct ViewSetArg<true, true> {
  typedef ViewLatticeBatchDev type;
};
template <>
struct ViewSetArg<false, true> {
  typedef ViewPointsBatchDev type;
};

// Frame f of a ViewLatticeBatchDev under the member names of ViewLatticeDev, so that the tile body reads either.
// feat / calib point at the frame's nv entries INSIDE the kernel arguments: indexing them stays a scalar load.
struct ViewLatticeFrame {
  int nv, proj, view;
  const float *const *feat;
  const float *const *calib;
  PointSrc src;
  float *vol;
};
__device__ __forceinline__ ViewLatticeFrame lattice_frame(const ViewLatticeBatchDev &set, int f) {
  ViewLatticeFrame fr;
  fr.nv = set.nv;
  fr.proj = set.proj;
  fr.view = set.view;
  fr.feat = set.feat + f * set.nv;
  fr.calib = set.calib + f * set.nv;
  fr.src.pts = nullptr;
  fr.src.sn = fr.src.sc = fr.src.out_stride = 0;
  fr.src.packed = set.it[f].packed;
  fr.src.stride = set.stride;
  fr.src.level_res = set.level_res;
  fr.src.res_final = set.res_final;
  fr.src.half_step = set.half_step;
  for (int i = 0; i < 3; ++i) {
    fr.src.bmin[i] = set.bmin[i];
    fr.src.blen[i] = set.blen[i];
  }
  fr.src.n_dev = set.it[f].n_dev;
  fr.src.n = set.it[f].n;
  fr.vol = set.it[f].vol;
  return fr;
}
// Frame f of a ViewPointsBatchDev: explicit points [3, capacity] behind load_point (packed == nullptr), one output
struct ViewPointsFrame {
  int nv, proj, view;
  const float *const *feat;
  const float *const *calib;
  PointSrc src;
  float *out;
  long long out_stride;
};
__device__ __forceinline__ ViewPointsFrame lattice_frame(const ViewPointsBatchDev &set, int f) {
  ViewPointsFrame fr;
  fr.nv = set.nv;
  fr.proj = set.proj;
  fr.view = set.view;
  fr.feat = set.feat + f * set.nv;
  fr.calib = set.calib + f * set.nv;
  fr.src.pts = set.it[f].pts;
  fr.src.sn = 1;
  fr.src.sc = set.capacity;
  fr.src.out_stride = set.capacity;
  fr.src.packed = nullptr;
  fr.src.stride = fr.src.level_res = 0;
  fr.src.res_final = fr.src.half_step = 0.0f;
  for (int i = 0; i < 3; ++i) fr.src.bmin[i] = fr.src.blen[i] = 0.0f;
  fr.src.n_dev = set.it[f].n_dev;
  fr.src.n = 0;
  fr.out = set.it[f].out;
  fr.out_stride = set.capacity;
  return fr;
}
__device__ __forceinline__ const ViewSetDev &lattice_frame(const ViewSetDev &set, int) { return set; }
__device__ __forceinline__ const ViewLatticeDev &lattice_frame(const ViewLatticeDev &set, int) { return set; }

// ceil(n / gpts) for a level's count n (<= 1023^3 < 2^30 - 64) and gpts = floor(64 / V) points per tile, V <= 8:
// m35 = ceil(2^35 / gpts) <= 2^32 and q = ((n + gpts - 1) m35) >> 35 is the exact quotient, because the excess
// e = m35 gpts - 2^35 is 0 for a power of two and < gpts <= 21 < 2^5 otherwise, so (n + gpts - 1) e < 2^35; the
// product stays below 2^62.  Keeps 32 integer divisions out of every tile's lookup.
__device__ __forceinline__ long long view_tiles(long long n, int gpts, unsigned long long m35) {
  return (long long)(((unsigned long long)(n + gpts - 1) * m35) >> 35);
}

// tile_owner (query_common.h) for the frames of a ViewLatticeBatchDev / ViewPointsBatchDev and tiles of gpts points:
// fi = the frame that owns `gtile` (-1: past the last tile of the last frame), tile0 = its first tile, n = its count
// (set.count: a ViewPointsBatchDev's is clamped to [0, capacity]).  Every
// thread reads the same counts, so the result is the same in every lane; the caller makes that known to the
// compiler (readfirstlane), which keeps the frame's pointers in SGPRs.
template <typename SET>
__device__ __forceinline__ void view_tile_owner(const SET &set, long long gtile, int gpts,
                                                unsigned long long m35, int &fi_out, long long &tile0_out,
                                                long long &n_out) {
  int fi = -1;
  long long tile0 = 0, n_owner = 0, acc = 0;
  for (int f0 = 0; f0 < set.n; f0 += 8)  // groups of 8 loads in flight, as in tile_owner
#pragma unroll
    for (int fk = 0; fk < 8; ++fk) {
      const int f = f0 + fk;
      if (f < set.n) {
        const long long nf = set.count(f);
        const long long t = view_tiles(nf, gpts, m35);
        if (fi < 0 && gtile < acc + t) {
          fi = f;
          tile0 = acc;
          n_owner = nf;
        }
        acc += t;
      }
    }
  fi_out = fi;
  tile0_out = tile0;
  n_out = n_owner;
}
__device__ __forceinline__ long long uniform64(long long v) {
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)(unsigned long long)v);
  const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)((unsigned long long)v >> 32));
  return (long long)(((unsigned long long)hi << 32) | lo);
}

template <int C, int COUT, int WPS, bool DIRECT, bool LATTICE = false, bool BATCH = false>
__global__ __launch_bounds__(kQueryThreads, WPS) void pifu_query_views_kernel(
    MlpPack mlp, int fh, int fw, float z_scale, int act, typename ViewSetArg<LATTICE, BATCH>::type aset) {
  static_assert(!(DIRECT && LATTICE), "explicit features have no lattice");
  static_assert(!(DIRECT && BATCH), "explicit features are not batched");
  constexpr bool SHARED = LATTICE || BATCH;  // one point set for all views, behind load_point
  constexpr int ROWB = C * 4;
  constexpr int NGX = C / 8;  // K groups of the feature segment
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char *xs = smem;                    // [64 columns][C] f32, swizzled 16-byte slots
  unsigned char *hb = smem + kTilePts * ROWB;  // [64 columns][64 rows] f32, swizzled

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j = lane & 31, h = lane >> 5;
  const int nv = aset.nv;
  const int gpts = kTilePts / nv;  // points per tile
  const int ncol = gpts * nv;      // live columns
  const int magic = (65536 + nv - 1) / nv;  // column_view
  long long n_pts = 0, tiles = 0;
  unsigned long long m35 = 0;  // view_tiles
  if constexpr (BATCH) {
    m35 = ((1ull << 35) + (unsigned)gpts - 1) / (unsigned)gpts;
  } else {
    if constexpr (LATTICE)
      n_pts = aset.src.n_dev ? (long long)*aset.src.n_dev : aset.src.n;  // a level's count lives on the device
    else
      n_pts = aset.n;
    tiles = (n_pts + gpts - 1) / gpts;
  }

  const int swz = h ^ (j & 15);
  const WStream ws = make_wstream(mlp.base, mlp.n_floats, lane);

  for (long long gtile = blockIdx.x; BATCH || gtile < tiles; gtile += gridDim.x) {
    long long tile = gtile;
    int fi = 0;
    if constexpr (BATCH) {
      // the tile's frame: gtile and the counts are the same for every thread of the workgroup, so all of them
      // leave the loop in the same trip and take the same number of barriers
      long long tile0;
      view_tile_owner(aset, gtile, gpts, m35, fi, tile0, n_pts);
      fi = __builtin_amdgcn_readfirstlane(fi);
      if (fi < 0) break;  // past the last tile of the last frame
      tile = gtile - uniform64(tile0);
      n_pts = uniform64(n_pts);
    }
    const auto &set = lattice_frame(aset, fi);
    const long long n0 = tile * gpts;

    // ---------------- gather ----------------
    if constexpr (DIRECT) {
      // lane = column; each wave moves C/16 four-channel slots
      int g, v;
      column_view(lane, nv, magic, g, v);
      const long long n = n0 + g;
      const bool live = lane < ncol && n < n_pts;
      const float *__restrict__ fp = set.pts[0];
      for (int u = 1; u < nv; ++u)
        if (u == v) fp = set.pts[u];
      for (int s0 = wv; s0 < C / 4; s0 += 4) {
        f32x4 r = {0.0f, 0.0f, 0.0f, 0.0f};
        if (live) {
#pragma unroll
          for (int k = 0; k < 4; ++k) r[k] = fp[(long long)(4 * s0 + k) * set.sc + n];
        }
        *reinterpret_cast<f32x4 *>(xs + lane * ROWB + ((s0 ^ (lane & 15)) << 4)) = r;
      }
    } else {
      // 16 columns per wave, one column at a time across the wave (lane = 16-byte channel slot):
      // the column, hence its view, is wave-uniform
      constexpr int GB = 4;
#pragma unroll 1
      for (int i0 = 0; i0 < 16; i0 += GB) {
        Taps t[GB];
        const float *fmap[GB];
#pragma unroll
        for (int u = 0; u < GB; ++u) {
          const int p = 16 * wv + i0 + u;
          int g, v;
          column_view(p, nv, magic, g, v);
          const long long n = n0 + g;
          const bool live_n = p < ncol && n < n_pts;
          fmap[u] = set.feat[v];
          float x = 0.0f, y = 0.0f;
          if (live_n) (void)view_z<C, false, SHARED>(set, v, n, z_scale, x, y);
          // grid_sample on every finite projection, in the image or not (zero padding)
          t[u] = make_taps(x, y, fh, fw, C, live_n && !non_finite(x, y));
        }
        f32x4 val[GB][C / 256][4];
#pragma unroll
        for (int u = 0; u < GB; ++u)
#pragma unroll
          for (int part = 0; part < C / 256; ++part)
#pragma unroll
            for (int k = 0; k < 4; ++k)
              val[u][part][k] =
                  *reinterpret_cast<const f32x4 *>(fmap[u] + t[u].o[k] + 4 * (lane + 64 * part));
#pragma unroll
        for (int u = 0; u < GB; ++u) {
          const int p = 16 * wv + i0 + u;
#pragma unroll
          for (int part = 0; part < C / 256; ++part) {
            const int slot = lane + 64 * part;
            const f32x4 r = blend(val[u][part][0], val[u][part][1], val[u][part][2], val[u][part][3], t[u]);
            *reinterpret_cast<f32x4 *>(xs + p * ROWB + ((slot ^ (p & 15)) << 4)) = r;
          }
        }
      }
    }
    // z_feat of this wave's two column blocks for the z k-steps of layers 0-2 (lanes 0-31 carry it, 32-63 supply 0)
    float zb[2];
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) zb[cb] = h == 0 ? column_z<C, DIRECT, SHARED>(set, 32 * cb + j, magic, n0, n_pts, ncol, z_scale, false) : 0.0f;
    __syncthreads();

    // ---------------- layers 0-2, each column on its own features and z (query_mfma.h) ----------------
    f32x16 acc2[2][2];
    mlp64_layers012<C>(acc2, mlp, ws, xs, hb, zb, wv, j, h, swz);

    const unsigned char *xrow = xs + j * ROWB;  // this lane's column row, column block 0
    const unsigned char *hrow = hb + j * kHbRowBytes;

    // ---------------- layer 3 on the view means: rows [32 wv, +32), K = 256 hidden (4 chunks) + skip ----------------
    f32x16 acc3[1][2];
    init_from_bias(acc3[0][0], ws, mlp.bias[3] + 32 * wv);
    acc3[0][1] = acc3[0][0];
    {
      const int a3 = mlp.ah[3] / 4 + wv * (kHidden[2] / 8) * 64;
      f32x4 ring3[4][1];
      seg_prefetch<1, 3>(ring3, ws, a3, 0, 8);
#pragma unroll
      for (int ck = 0; ck < 4; ++ck) {
        if (wv == ck) {
#pragma unroll
          for (int mm = 0; mm < 2; ++mm)
#pragma unroll
            for (int n = 0; n < 2; ++n) store_hidden(hb, acc2[mm][n], mm, n, j, h);
        }
        __syncthreads();
        if (nv > 1) {
          // y = y.view(-1,V,256,N).mean(1), this chunk's 64 rows; the first chunk also takes
          // tmpy = feature.view(-1,V,C+1,N).mean(1) -- every wave is past layer 2's reads of xs
          group_mean_inplace<kHbRowBytes>(hb, nv, gpts, tid);
          if (ck == 0) group_mean_inplace<ROWB>(xs, nv, gpts, tid);
          __syncthreads();
        }
        seg_main<1, 2, 3, kHbRowBytes>(acc3, ring3, ws, a3 + ck * 8 * 64, 0, 8, hrow, swz);
        if (ck < 3) seg_prefetch<1, 3>(ring3, ws, a3 + (ck + 1) * 8 * 64, 0, 8);
        __syncthreads();
      }
      const int a3x = mlp.ax[3] / 4 + wv * NGX * 64;
      float az3[1];
      seg_prefetch<1, 3>(ring3, ws, a3x, 0, NGX);
      az3[0] = wload32(ws, mlp.az[3] + wv * 64);
      seg_main<1, 2, 3, ROWB>(acc3, ring3, ws, a3x, 0, NGX, xrow, swz);
      // the z row of tmpy: the group mean of z_feat (made here rather than kept live through layers 0-2)
      float zm[2];
#pragma unroll
      for (int cb = 0; cb < 2; ++cb) zm[cb] = h == 0 ? column_z<C, DIRECT, SHARED>(set, 32 * cb + j, magic, n0, n_pts, ncol, z_scale, true) : 0.0f;
      gemm_z<1, 2>(acc3, az3, zm);
#pragma unroll
      for (int n = 0; n < 2; ++n) lrelu(acc3[0][n]);
    }

    // ---------------- layer 4 (Cout x (128 + C + 1)) on the VALU ----------------
    float *red = reinterpret_cast<float *>(hb);  // red[part][o][column], see mlp64_layer4_partials
    constexpr int K4 = (kHidden[3] + C + 1 + 3) & ~3;
    mlp64_layer4_partials<C, COUT>(red, acc3, mlp, xs, wv, lane, j, h);
    __syncthreads();
    if (tid < COUT * kTilePts) {
      const int o = tid / kTilePts, p = tid % kTilePts;
      int g, v;
      column_view(p, nv, magic, g, v);
      const long long n = n0 + g;
      if (p < ncol && n < n_pts) {
        float val = (mlp.base + mlp.bias[4])[o];
#pragma unroll
        for (int part = 0; part < 8; ++part) val += red[(part * COUT + o) * kTilePts + p];
        const float wz = (mlp.base + mlp.w4)[o * K4 + kHidden[3] + C];
        // the group's z mean, this column's own projection and whether any view is non-finite
        float zsum = 0.0f, xo = 0.0f, yo = 0.0f;
        bool poisoned = false;
        float *__restrict__ out = nullptr;
        if constexpr (!SHARED) out = set.out[0];
        for (int u = 0; u < nv; ++u) {
          float x, y;
          const float zf = view_z<C, DIRECT, SHARED>(set, u, n, z_scale, x, y);
          zsum = u == 0 ? zf : zsum + zf;
          poisoned = poisoned || (set.proj == MP_PROJ_PERSPECTIVE && non_finite(x, y));
          if (u == v) {
            xo = x;
            yo = y;
            if constexpr (!DIRECT && !SHARED) out = set.out[u];
          }
        }
        val = fmaf(wz, __fdiv_rn(zsum, (float)nv), val);
        if constexpr (DIRECT) {
          if (v == 0) out[o * set.out_stride + n] = activate(val, act);
        } else if constexpr (LATTICE) {
          // row `view` only, straight into the level's volume (COUT = 1: o == 0)
          if (v == set.view) {
            const float r = poisoned ? __builtin_nanf("") : in_image(xo, yo) ? activate(val, act) : 0.0f;
            const uint32_t code = set.src.packed[n];
            const long long lr = set.src.level_res;
            set.vol[((long long)(code >> 20) * lr + ((code >> 10) & 1023u)) * lr + (code & 1023u)] = r;
          }
        } else if constexpr (BATCH) {
          // row `view` only, to the frame's [Cout, capacity] output; n < n_pts <= capacity
          if (v == set.view) {
            const float r = poisoned ? __builtin_nanf("") : in_image(xo, yo) ? activate(val, act) : 0.0f;
            set.out[o * set.out_stride + n] = r;
          }
        } else {
          // MonoPortNet.py:89 per view; a non-finite view's NaN samples reach every row through the mean
          const float r = poisoned ? __builtin_nanf("") : in_image(xo, yo) ? activate(val, act) : 0.0f;
          out[o * set.out_stride + n] = r;
        }
      }
    }
    __syncthreads();  // red / xs are rewritten by the next tile
  }
}

// ---- host side -----------------------------------------------------------------------------------
template <int C, int COUT, int WPS, bool DIRECT>
static int launch_views_t(mp_ctx *ctx, const Mlp &m, const ViewSetDev &set, int h, int w, float z_scale,
                          hipStream_t st) {
  constexpr int lds = kTilePts * C * 4 + kHbBytes;
  auto kern = pifu_query_views_kernel<C, COUT, WPS, DIRECT>;
  if (const int rc = raise_lds_limit(ctx, reinterpret_cast<const void *>(kern), lds)) return rc;
  const long long gpts = kTilePts / set.nv;
  const long long tiles = (set.n + gpts - 1) / gpts;
  if (tiles <= 0) return MP_OK;
  const long long grid = query_grid(tiles, (long long)ctx->n_cu * WPS, false);
  if (const int rc = prof_begin(ctx, st)) return rc;
  hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(kQueryThreads), lds, st, m.pack(), h, w, z_scale, m.act,
                     set);
  if (const int rc = prof_end(ctx, st)) return rc;
  MP_HIP(ctx, hipGetLastError());
  return MP_OK;
}

// One octree level.  The level's count is on the device (set.src.n_dev) except at level 0: the grid is the
// stream's resident share striding over the tiles, and a count of 0 leaves every workgroup at its loop test.
int launch_query_views_lattice(mp_ctx *ctx, const Mlp &m, const ViewLatticeDev &set, int h, int w, float z_scale,
                               long long max_points, hipStream_t st) {
  if (set.nv < 1 || set.nv > kMaxViews)
    return fail(ctx, MP_ERR_UNSUPPORTED, "multi-view octree: 1..%d views, got %d", kMaxViews, set.nv);
  if (m.c != 256 || m.cout != 1 || m.precision != MP_PREC_F32)
    return fail(ctx, MP_ERR_UNSUPPORTED, "multi-view octree: f32 netG heads (C=256, Cout=1); got C=%d Cout=%d precision %d",
                m.c, m.cout, m.precision);
  if (set.view < 0 || set.view >= set.nv)
    return fail(ctx, MP_ERR_ARG, "multi-view octree: view %d of %d", set.view, set.nv);
  constexpr int C = 256, WPS = 2;
  constexpr int lds = kTilePts * C * 4 + kHbBytes;
  auto kern = pifu_query_views_kernel<C, 1, WPS, false, true>;
  if (const int rc = raise_lds_limit(ctx, reinterpret_cast<const void *>(kern), lds)) return rc;
  const long long gpts = kTilePts / set.nv;
  const long long tiles = (max_points + gpts - 1) / gpts;
  if (tiles <= 0) return MP_OK;
  const long long grid = query_grid(tiles, (long long)ctx->n_cu * WPS, set.src.n_dev != nullptr);
  if (const int rc = prof_begin(ctx, st)) return rc;
  hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(kQueryThreads), lds, st, m.pack(), h, w, z_scale, m.act,
                     set);
  if (const int rc = prof_end(ctx, st)) return rc;
  MP_HIP(ctx, hipGetLastError());
  return MP_OK;
}

// The same level of set.n frames in one launch: the grid covers the frames' tiles together (each frame's rounded
// up on its own, as view_tile_owner counts them), so what one frame leaves of the machine the next one fills.
int launch_query_views_lattice_batch(mp_ctx *ctx, const Mlp &m, const ViewLatticeBatchDev &set, int h, int w,
                                     float z_scale, long long max_points, hipStream_t st) {
  if (set.nv < 1 || set.nv > kMaxViews)
    return fail(ctx, MP_ERR_UNSUPPORTED, "multi-view octree: 1..%d views, got %d", kMaxViews, set.nv);
  if (m.c != 256 || m.cout != 1 || m.precision != MP_PREC_F32)
    return fail(ctx, MP_ERR_UNSUPPORTED, "multi-view octree: f32 netG heads (C=256, Cout=1); got C=%d Cout=%d precision %d",
                m.c, m.cout, m.precision);
  if (set.view < 0 || set.view >= set.nv)
    return fail(ctx, MP_ERR_ARG, "multi-view octree: view %d of %d", set.view, set.nv);
  if (set.n < 1 || set.n > kMaxFrames || set.n * set.nv > kMaxFrameViews)
    return fail(ctx, MP_ERR_ARG, "multi-view octree: 1..%d frames and at most %d frames x views per launch, got %d x %d",
                kMaxFrames, kMaxFrameViews, set.n, set.nv);
  constexpr int C = 256, WPS = 2;
  constexpr int lds = kTilePts * C * 4 + kHbBytes;
  auto kern = pifu_query_views_kernel<C, 1, WPS, false, true, true>;
  if (const int rc = raise_lds_limit(ctx, reinterpret_cast<const void *>(kern), lds)) return rc;
  const long long gpts = kTilePts / set.nv;
  const long long tiles = (max_points + gpts - 1) / gpts * set.n;
  if (tiles <= 0) return MP_OK;
  const long long grid = query_grid(tiles, (long long)ctx->n_cu * WPS, set.it[0].n_dev != nullptr);
  if (const int rc = prof_begin(ctx, st)) return rc;
  hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(kQueryThreads), lds, st, m.pack(), h, w, z_scale, m.act,
                     set);
  if (const int rc = prof_end(ctx, st)) return rc;
  MP_HIP(ctx, hipGetLastError());
  return MP_OK;
}

template <int C, int COUT, int WPS>
static int launch_views_counted_t(mp_ctx *ctx, const Mlp &m, const ViewPointsBatchDev &set, int h, int w,
                                  float z_scale, hipStream_t st) {
  constexpr int lds = kTilePts * C * 4 + kHbBytes;
  auto kern = pifu_query_views_kernel<C, COUT, WPS, false, false, true>;
  if (const int rc = raise_lds_limit(ctx, reinterpret_cast<const void *>(kern), lds)) return rc;
  const long long gpts = kTilePts / set.nv;
  const long long tiles = (set.capacity + gpts - 1) / gpts * set.n;
  if (tiles <= 0) return MP_OK;
  const long long grid = query_grid(tiles, (long long)ctx->n_cu * WPS, true);
  if (const int rc = prof_begin(ctx, st)) return rc;
  hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(kQueryThreads), lds, st, m.pack(), h, w, z_scale, m.act,
                     set);
  if (const int rc = prof_end(ctx, st)) return rc;
  MP_HIP(ctx, hipGetLastError());
  return MP_OK;
}

// Explicit points of set.n frames, counted on the device: the resident grid strides over the frames' tiles, each
// frame's rounded up on its own (view_tile_owner); the heads are those of launch_query_views.
int launch_query_views_counted_batch(mp_ctx *ctx, const Mlp &m, const ViewPointsBatchDev &set, int h, int w,
                                     float z_scale, hipStream_t st) {
  const char *who = "mp_query_views_counted_batch";
  if (set.nv < 1 || set.nv > kMaxViews)
    return fail(ctx, MP_ERR_UNSUPPORTED, "%s: 1..%d views, got %d", who, kMaxViews, set.nv);
  if (m.precision != MP_PREC_F32)
    return fail(ctx, MP_ERR_UNSUPPORTED, "%s: the multi-view kernel is f32 only (head precision %d)", who, m.precision);
  if (set.view < 0 || set.view >= set.nv) return fail(ctx, MP_ERR_ARG, "%s: view %d of %d", who, set.view, set.nv);
  if (set.n < 1 || set.n > kMaxFrames || set.n * set.nv > kMaxFrameViews)
    return fail(ctx, MP_ERR_ARG, "%s: 1..%d frames and at most %d frames x views per launch, got %d x %d", who,
                kMaxFrames, kMaxFrameViews, set.n, set.nv);
#define MP_VCASE(CC, CO, WP) \
  if (m.c == CC && m.cout == CO) return launch_views_counted_t<CC, CO, WP>(ctx, m, set, h, w, z_scale, st);
  MP_VCASE(256, 1, 2)
  MP_VCASE(256, 3, 2)
  MP_VCASE(512, 1, 1)
  MP_VCASE(512, 3, 1)
#undef MP_VCASE
  return fail(ctx, MP_ERR_UNSUPPORTED,
              "%s: multi-view query kernels are built for C in {256,512}, Cout in {1,3}; got C=%d Cout=%d", who, m.c,
              m.cout);
}

int launch_query_views(mp_ctx *ctx, const Mlp &m, const ViewSetDev &set, int h, int w, float z_scale,
                       hipStream_t st) {
  if (set.nv < 1 || set.nv > kMaxViews)
    return fail(ctx, MP_ERR_UNSUPPORTED, "multi-view query: 1..%d views, got %d", kMaxViews, set.nv);
  const bool direct = set.feat[0] == nullptr;
#define MP_VCASE(CC, CO, WP)                                                                     \
  if (m.c == CC && m.cout == CO) {                                                               \
    if (direct) return launch_views_t<CC, CO, WP, true>(ctx, m, set, h, w, z_scale, st);         \
    return launch_views_t<CC, CO, WP, false>(ctx, m, set, h, w, z_scale, st);                    \
  }
  MP_VCASE(256, 1, 2)
  MP_VCASE(256, 3, 2)
  MP_VCASE(512, 1, 1)
  MP_VCASE(512, 3, 1)
#undef MP_VCASE
  return fail(ctx, MP_ERR_UNSUPPORTED,
              "multi-view query kernels are built for C in {256,512}, Cout in {1,3}; got C=%d Cout=%d", m.c, m.cout);
}

}  // namespace mp
