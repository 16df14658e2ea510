// Internal declarations shared by the HIP translation units of libmonoport_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <mutex>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "../../include/monoport_hip.h"

namespace mp {

constexpr int kTilePts = 64;     // query points per workgroup tile
constexpr int kQueryThreads = 256;
constexpr int kHidden[4] = {1024, 512, 256, 128};  // SurfaceClassifier.py:76 / :84
// rows of a feature map's skip table (mp_skip_table): the feature segments of layers 0-3 back to back
// (1024 + 512 + 256 + 128), then the last layer's (<= 3 outputs, padded to one 16-byte slot)
constexpr int kTableL[5] = {0, 1024, 1536, 1792, 1920};
// 1923 used floats, padded to 61 x 32: a texel's row is then 61 cache lines of 128 bytes and every 32-row block a
// query lane group reads (128 bytes) is ONE line -- with the minimal padding (1924) a texel's row started 16 bytes
// further every texel and 7 of 8 blocks straddled two lines: twice the lines per gathered block (round 4)
constexpr int kTableRows = 1952;

// Device-side view of one packed SurfaceClassifier (see pack.hip for the fragment order).
// One base pointer + float offsets keeps the kernel's SGPR footprint small.
struct MlpPack {
  const float *base;
  int ah[4];    // hidden-segment A fragments of MFMA layers 0..3 (ah[0] unused)
  int ax[4];    // feature-segment A fragments
  int az[4];    // z-column A fragments [n_out/32][64]
  int bias[5];  // biases of layers 0..4
  int w4;       // last layer, row-major [Cout][pad4(128 + C + 1)]
  int n_floats; // size of the whole packed buffer (buffer-resource bound of the weight loads)
};

// Split-precision copy of the same weights for the 3-term f16 MFMA kernel (query16.hip): every
// weight w is stored as hi = f16(w * S), lo = f16(w * S - hi) with a per-layer power-of-two scale
// S; fragments are [rb][g][hi|lo][lane] of 8 halves (16 bytes), K walked in groups of 16.
struct MlpPack16 {
  const void *base;   // half data, offsets below in units of 16 bytes
  int ah[4], ax[4];   // hidden / feature segments
  int az[4];          // z column: [rb][hi|lo][lane], only element 0 of lanes 0-31 non-zero
  float scale[4];     // S of layers 0..3
  int n16;            // size of the buffer in 16-byte units (buffer-resource bound)
};

// Where a query launch takes its points from and where it puts the results.
struct PointSrc {
  // explicit mode (packed == nullptr): world coords, element (c, i) at pts[i*sn + c*sc]
  const float *pts;
  long long sn, sc;
  // lattice mode: packed level-local node coords x | y<<10 | z<<20, scaled by `stride` into the
  // final-resolution index space and mapped to world like Seg3dLossless.batch_eval
  const uint32_t *packed;
  int stride;       // final-res index step of this level
  int level_res;    // nodes per axis at this level (scatter index = (z*res + y)*res + x)
  float res_final;  // R as float
  float half_step;  // (1/R)/2
  float bmin[3], blen[3];
  // count: *n_dev if n_dev != nullptr else n
  const int32_t *n_dev;
  long long n;
  long long out_stride;  // explicit mode: out[o*out_stride + i]
};

// One launch of the fused query kernels serves up to kMaxFrames independent frames (their own
// feature map, calibration, points and output): the tiles of all frames form one index space, so
// the small coarse levels of several frames fill the machine together.
constexpr int kMaxFrames = 32;  // a power of two <= 64 (query_table.hip: one lane per frame)
static_assert((kMaxFrames & (kMaxFrames - 1)) == 0 && kMaxFrames <= 64, "kMaxFrames");
struct QueryItem {
  const float *feat;   // channels-last feature map [H,W,C]
  const float *calib;  // [3,4] rows of the 4x4
  float *out;
  PointSrc src;
  const float *l0;     // optional skip table of `feat` [H,W,kTableRows] (mp_skip_table; filled in by the launcher)
  int proj;            // MP_PROJ_ORTHOGONAL / MP_PROJ_PERSPECTIVE (query_common.h: project_mode)
};
// host-side description of a launch (the launchers turn it into a QuerySetDev)
struct QuerySet {
  int n;
  QueryItem it[kMaxFrames];
};

// What the kernels receive (kernel arguments are limited to 4 KB: 32 full QueryItems would be 4.1 KB).
// The frames of one launch share the point layout (explicit strides, or the lattice of one octree level);
// per frame only the pointers, the count and the projection mode differ: 64 B per item, 2 KB for 32.
struct QueryItemDev {
  const float *feat, *calib;
  float *out;
  const float *l0;
  const void *pts;        // PointSrc::packed when `lattice`, else PointSrc::pts
  const int32_t *n_dev;
  long long n;
  int proj;
};
static_assert(sizeof(QueryItemDev) == 64, "QueryItemDev: 64 B per frame");
struct QuerySetDev {
  int n;
  int lattice;
  long long sn, sc, out_stride;
  int stride, level_res;
  float res_final, half_step, bmin[3], blen[3];
  QueryItemDev it[kMaxFrames];
#ifdef __HIPCC__
  __device__ __forceinline__ long long count(int f) const {
    const int32_t *p = it[f].n_dev;
    return p ? (long long)*p : it[f].n;
  }
  __device__ __forceinline__ QueryItem item(int f) const {
    QueryItem q;
    const QueryItemDev &d = it[f];
    q.feat = d.feat;
    q.calib = d.calib;
    q.out = d.out;
    q.l0 = d.l0;
    q.proj = d.proj;
    q.src.pts = lattice ? nullptr : static_cast<const float *>(d.pts);
    q.src.packed = lattice ? static_cast<const uint32_t *>(d.pts) : nullptr;
    q.src.sn = sn;
    q.src.sc = sc;
    q.src.out_stride = out_stride;
    q.src.stride = stride;
    q.src.level_res = level_res;
    q.src.res_final = res_final;
    q.src.half_step = half_step;
    for (int i = 0; i < 3; ++i) {
      q.src.bmin[i] = bmin[i];
      q.src.blen[i] = blen[i];
    }
    q.src.n_dev = d.n_dev;
    q.src.n = d.n;
    return q;
  }
#endif
};
static_assert(sizeof(QuerySetDev) + 256 <= 4096, "kernel arguments: the set + two MLP descriptors must stay below 4 KB");

// One multi-view launch (query_views.hip, SurfaceClassifier num_views = V > 1): V views of the same N points,
// each with its own feature map, calibration, points and output row; one projection mode and one point layout
// (element (c, i) of view v at pts[v][i*sn + c*sc]; output (o, i) at out[v][o*out_stride + i]).  feat[0] ==
// nullptr: SurfaceClassifier.forward on explicit features, pts[v] = view v's [C+1, N] rows (row stride sc),
// one output out[0].
constexpr int kMaxViews = MP_MAX_VIEWS;
struct ViewSetDev {
  int nv, proj;
  long long n, sn, sc, out_stride;
  const float *feat[kMaxViews];
  const float *calib[kMaxViews];
  const float *pts[kMaxViews];
  float *out[kMaxViews];
};
// The views of one octree level (mp_recon_views): the points are the level's packed node list `src` (lattice
// mode of PointSrc, count *src.n_dev or src.n), shared by all views; n / sn / sc / pts / out of the base are
// unused.  Only row `view` of the [V,1,N] result exists: it is scattered to vol[z,y,x] of the level's
// src.level_res^3 buffer.
struct ViewLatticeDev : ViewSetDev {
  PointSrc src;
  float *vol;
  int view;
};
// One octree level of n frames x nv views (mp_recon_views_batch): what ViewLatticeDev holds, for every frame of the
// call.  The frames share nv, view, the projection mode and the lattice fields of PointSrc; per frame: the packed
// node list, the level's volume and the count (*n_dev, or n where n_dev == nullptr); per (frame, view), frame-major:
// the map and the calibration.  16 + 40 + 32 * 32 + 2 * 64 * 8 = 2104 B of kernel arguments.
constexpr int kMaxFrameViews = MP_MAX_FRAME_VIEWS;
struct ViewFrameDev {
  const uint32_t *packed;
  float *vol;
  const int32_t *n_dev;
  long long n;
};
struct ViewLatticeBatchDev {
  int nv, proj, view;
  int n;  // frames
  int stride, level_res;
  float res_final, half_step, bmin[3], blen[3];
  ViewFrameDev it[kMaxFrames];
  const float *feat[kMaxFrameViews];   // [f * nv + v]
  const float *calib[kMaxFrameViews];
#ifdef __HIPCC__
  __device__ __forceinline__ long long count(int f) const {
    const int32_t *p = it[f].n_dev;
    return p ? (long long)*p : it[f].n;
  }
#endif
};
static_assert(sizeof(ViewLatticeBatchDev) + 256 <= 4096, "kernel arguments: the frames + the MLP descriptor must stay below 4 KB");
// Explicit points of n frames x nv views, counted on the device (mp_query_views_counted_batch): the frames share nv,
// view, the projection mode and the capacity; per frame: the points [3, capacity] (contiguous, shared by the frame's
// views), the output [Cout, capacity] (row `view` of the [V,Cout,N] result) and the count *n_dev, which the kernel
// clamps to [0, capacity]; per (frame, view), frame-major: the map and the calibration.
// 16 + 8 + 32 * 24 + 2 * 64 * 8 = 1816 B of kernel arguments.
struct ViewPointsFrameDev {
  const float *pts;
  float *out;
  const int32_t *n_dev;
};
struct ViewPointsBatchDev {
  int nv, proj, view;
  int n;  // frames
  long long capacity;
  ViewPointsFrameDev it[kMaxFrames];
  const float *feat[kMaxFrameViews];   // [f * nv + v]
  const float *calib[kMaxFrameViews];
#ifdef __HIPCC__
  __device__ __forceinline__ long long count(int f) const {
    const long long c = (long long)*it[f].n_dev;
    return c < 0 ? 0 : c > capacity ? capacity : c;
  }
#endif
};
static_assert(sizeof(ViewPointsBatchDev) + 256 <= 4096, "kernel arguments: the frames + the MLP descriptor must stay below 4 KB");
// launch_recon's second way to evaluate a level's nodes: feat_hwc / calib are then the views' arrays ([f * nv + v]
// of the call's frames), proj[0] their one projection.  batch == 0 (mp_recon_views): one frame on the one-frame
// lattice kernel; batch != 0 (mp_recon_views_batch): 1..kMaxFrames frames, nv * frames <= kMaxFrameViews, every
// level of all of them in one launch of the batched lattice kernel
struct ReconViews {
  int nv, view, batch;
};
// launch_recon's second way to SELECT a level's nodes (mp_recon_topk_batch, topk.hip): the num_points[l] most uncertain
// nodes within max_dist[l] (NULL: no bound) instead of the dilated boundary; scratch: topk_scratch_bytes(n_frames, r_last)
struct ReconTopk {
  const long long *num_points;
  const float *max_dist;
  void *scratch;
};

struct Mlp {
  bool used = false;
  int c = 0, cout = 0, act = 0;
  bool loaded[5] = {false, false, false, false, false};
  hipStream_t load_stream = nullptr;  // stream of the most recent mp_mlp_load
  float *buf = nullptr;  // one allocation holding every packed segment
  size_t off_ah[4], off_ax[4], off_az[4], off_bias[5], off_w4;
  size_t total = 0;
  MlpPack pack() const;
  // f16x3 copy (C == 256 heads only)
  int precision = 0;        // MP_PREC_F32 / MP_PREC_F16X3
  void *buf16 = nullptr;
  float *raw = nullptr;     // un-packed [out,in] copies of layers 0..3 (source for re-packing)
  size_t off_raw[4];
  size_t off16_ah[4], off16_ax[4], off16_az[4], total16 = 0;
  float scale16[4] = {1.f, 1.f, 1.f, 1.f};
  MlpPack16 pack16() const;
};

}  // namespace mp

struct mp_ctx {
  int device = 0;
  int n_cu = 0;
  std::mutex mu;
  std::vector<mp::Mlp> mlps;
  // scratch arenas, one per stream the context has been used on (grown on demand): calls that
  // are in flight on different streams never share scratch; calls on one stream are ordered.
  struct Arena {
    void *ptr = nullptr;  // current block
    size_t bytes = 0;
    std::vector<void *> retired;  // outgrown blocks, kept until mp_stream_release / mp_destroy
    size_t retired_bytes = 0;
  };
  std::unordered_map<void *, Arena> arenas;
  // kernels whose dynamic-LDS limit has been raised on this context's device (guarded by mu)
  std::unordered_set<const void *> lds_attr_done;
  // skip tables registered for feature maps (mp_skip_table): feat pointer -> table + the packed
  // head it was computed with
  struct SkipTable {
    const float *table;
    const float *mlp_buf;
    int h, w;
  };
  std::unordered_map<const float *, SkipTable> skip_tables;
  // optional event bracketing of query launches (mp_profile_begin / mp_profile_end)
  std::vector<hipEvent_t> prof_events;  // start/stop pairs
  int prof_used = 0;                    // pairs recorded
};

namespace mp {

int fail(mp_ctx *ctx, int code, const char *fmt, ...);
int ensure_scratch(mp_ctx *ctx, hipStream_t st, size_t bytes, void **out);

#define MP_HIP(ctx, expr)                                                            \
  do {                                                                               \
    hipError_t e_ = (expr);                                                          \
    if (e_ != hipSuccess)                                                            \
      return mp::fail(ctx, MP_ERR_HIP, "%s: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                      __FILE__, __LINE__);                                           \
  } while (0)

// clock_probe.hip
int launch_mfma_clock_probe(mp_ctx *ctx, float ms_target, double *out, hipStream_t st);

// query.hip
// raises a kernel's dynamic-LDS limit to `bytes`, once per kernel and context (= device); every launcher with
// more than 64 KB of dynamic LDS calls it
int raise_lds_limit(mp_ctx *ctx, const void *kern, int bytes);
// what the launchers of the query kernels share:
// workgroups of a launch that strides over `tiles`.  Device-side counts: the resident grid, which strides;
// host-side counts: one workgroup per tile up to a few waves of the machine
inline long long query_grid(long long tiles, long long resident, bool device_counts) {
  const long long cap = device_counts ? resident : 8 * resident;
  return tiles < cap ? tiles : cap;
}
// the event pair around one query launch while mp_profile_begin's pairs last (mp_profile_end reads them)
int prof_begin(mp_ctx *ctx, hipStream_t st);
int prof_end(mp_ctx *ctx, hipStream_t st);
int launch_query(mp_ctx *ctx, const Mlp &m, const float *feat_hwc, int h, int w,
                 const float *calib, float z_scale, const PointSrc &src, float *out,
                 long long max_points, hipStream_t st);
int launch_query_set(mp_ctx *ctx, const Mlp &m, const QuerySet &set, int h, int w, float z_scale,
                     long long max_points, bool device_counts, hipStream_t st);
int launch_index(mp_ctx *ctx, const float *feat_hwc, int c, int h, int w, const float *uv,
                 long long n, float *out, hipStream_t st);
int launch_orthogonal(mp_ctx *ctx, const float *pts, long long n, const float *calib, float *out,
                      hipStream_t st);
int launch_perspective(mp_ctx *ctx, const float *pts, long long n, const float *calib, float *out,
                       hipStream_t st);
// query_views.hip: the multi-view query (f32, plain kernel only: registered skip tables are not looked at)
int launch_query_views(mp_ctx *ctx, const Mlp &m, const ViewSetDev &set, int h, int w, float z_scale,
                       hipStream_t st);
// one octree level of mp_recon_views (netG f32 heads): at most max_points nodes, counted on the device when
// set.src.n_dev is set
int launch_query_views_lattice(mp_ctx *ctx, const Mlp &m, const ViewLatticeDev &set, int h, int w, float z_scale,
                               long long max_points, hipStream_t st);
// one octree level of mp_recon_views_batch: the frames of `set`, at most max_points nodes EACH
int launch_query_views_lattice_batch(mp_ctx *ctx, const Mlp &m, const ViewLatticeBatchDev &set, int h, int w,
                                     float z_scale, long long max_points, hipStream_t st);
// mp_query_views_counted_batch: the frames of `set`, at most set.capacity points EACH, counted on the device
int launch_query_views_counted_batch(mp_ctx *ctx, const Mlp &m, const ViewPointsBatchDev &set, int h, int w,
                                     float z_scale, hipStream_t st);
// pack.hip
int launch_pack_hwc(mp_ctx *ctx, const float *src, int c_src, int h, int w, float *dst, int c_dst,
                    int c_off, hipStream_t st);
int launch_pack_layer(mp_ctx *ctx, Mlp &m, int layer, const float *w, const float *b,
                      hipStream_t st);
int launch_pack_layer16(mp_ctx *ctx, Mlp &m, int layer, const float *w, hipStream_t st);
int launch_copy(mp_ctx *ctx, const float *src, float *dst, long long n, hipStream_t st);
int launch_absmax(mp_ctx *ctx, const float *src, long long n, unsigned int *out_bits, hipStream_t st);
int launch_absmax_accumulate(mp_ctx *ctx, const float *src, long long n, unsigned int *out_bits,
                             hipStream_t st);
bool find_skip_tables(mp_ctx *ctx, const Mlp &m, const QuerySet &set, int h, int w, QuerySet &tset);
// host set -> kernel argument; MP_ERR_ARG if the frames do not share point layout / lattice
int compact_query_set(mp_ctx *ctx, const QuerySet &set, QuerySetDev &dset);
// query_small.hip: the netG f32 query on 32-point tiles, for launches of fewer than
// kSmallGateTiles 64-point tiles
constexpr int kSmallGateTiles = 2048;
int launch_query32(mp_ctx *ctx, const Mlp &m, const QuerySet &set, int h, int w, float z_scale,
                   long long max_points, bool device_counts, int gate_tiles64, hipStream_t st);
// query_table.hip: the skip table of a feature map and the query kernel that blends its rows
int launch_skip_table(mp_ctx *ctx, const Mlp &m, const float *feat_hwc, int h, int w, float *table,
                    hipStream_t st);
int launch_query_tab(mp_ctx *ctx, const Mlp &m, const QuerySet &set, int h, int w, float z_scale,
                     long long max_points, bool device_counts, hipStream_t st);
void query_small_set_gate(int gate);  // 0 never, 1 always, n > 1 gate in 64-point tiles, < 0 default
int query_small_gate();
// query16.hip
int launch_query16(mp_ctx *ctx, const Mlp &m, const QuerySet &set, int h, int w, float z_scale,
                   long long max_points, bool device_counts, hipStream_t st);
int launch_concat3_add(mp_ctx *ctx, const float *a, int ca, const float *b, int cb, const float *c,
                       int cc, const float *sc, int n, long long hw, float *y, hipStream_t st);
int launch_prepare_inputs(mp_ctx *ctx, const float *segm, long long hw, const float *mean,
                          const float *std, float *g, float *c, hipStream_t st);
// octree.hip
// per frame; h, w: the map size (the histogram of the texel sort, point_order.hip)
size_t recon_scratch_bytes(const int *res, int n_levels, int h, int w);
int launch_recon(mp_ctx *ctx, void *scratch, const Mlp &m, int n_frames,
                 const float *const *feat_hwc, int h, int w, const float *const *calib,
                 const int *proj, float z_scale, const float *bmin, const float *bmax, const int *res,
                 int n_levels, float balance, int final_level, float *const *volume,
                 int32_t *const *status, const mp_recon_early *early, hipStream_t st,
                 const ReconViews *views = nullptr, const ReconTopk *topk = nullptr);
int launch_octree_select(mp_ctx *ctx, const float *prev, int rp, float *cur, int r,
                         const unsigned long long *ev_prev, unsigned long long *ev_cur,
                         unsigned long long *bnd, int box, float balance, uint32_t *packed,
                         int32_t *count, hipStream_t st);
// one level of the fixed-budget engine: upsample prev into cur, then topk.hip's selection; bnd: r * r * ceil(r / 64)
// words the upsample kernel writes its (unused) flags to; topk_scratch: topk_scratch_bytes(1, r)
size_t topk_scratch_bytes(int n_frames, int r);
int launch_octree_select_topk(mp_ctx *ctx, void *bnd, void *topk_scratch, const float *prev, int rp, float *cur, int r,
                              const unsigned long long *ev_prev, unsigned long long *ev_cur, long long k,
                              float max_dist, float balance, uint32_t *packed, int32_t *count, hipStream_t st);
int octree_box_of_level(int level);
int launch_octree_conflicts(mp_ctx *ctx, const uint32_t *packed, const int32_t *count, long long cap,
                            int r, const float *values, const float *vol, float balance,
                            unsigned long long *ev, uint32_t *out, int32_t *out_count,
                            hipStream_t st);
int launch_lattice_points(mp_ctx *ctx, const uint32_t *packed, const int32_t *count, long long cap,
                          int stride, int res_final, const float *bmin, const float *bmax,
                          float *pts, hipStream_t st);
int launch_scatter_nodes(mp_ctx *ctx, const uint32_t *packed, const int32_t *count, long long cap,
                         int r, const float *values, float *vol, hipStream_t st);
// vertices.hip
size_t forward_vertices_scratch_bytes(int r);
int launch_forward_vertices_batch(mp_ctx *ctx, void *scratch, int n_frames, const float *const *vol, int r, int dir,
                                  int64_t *const *x, int64_t *const *y, float *const *z, float *const *norm,
                                  int32_t *const *count, hipStream_t st);
int launch_paint_batch(mp_ctx *ctx, int n_frames, const int64_t *const *x, const int64_t *const *y,
                       const float *const *vals, int ch_major, const int32_t *const *count, long long cap, int res,
                       float scale, float bias, float lo, float hi, float *const *image, hipStream_t st);
int launch_vertex_points(mp_ctx *ctx, const int64_t *x, const int64_t *y, const float *z,
                         const int32_t *count, long long cap, int res, const float *mat16,
                         float *pts, hipStream_t st);

int launch_visualize(mp_ctx *ctx, const float *image, int res, int size, float *out, uint8_t *mask,
                     hipStream_t st);
// mcubes.hip
size_t mc_scratch_bytes(int r);
// n_frames volumes of one resolution; scratch: n_frames * mc_scratch_bytes(r); gate: NULL or n_frames entries
int launch_marching_cubes_batch(mp_ctx *ctx, void *scratch, int n_frames, const float *const *vol, int r, float level,
                                const float *bmin, const float *bmax, float *const *verts, long long max_v,
                                int32_t *const *faces, long long max_f, int32_t *const *counts,
                                const int32_t *const *gate, hipStream_t st);
// components.hip: the largest connected body of n_frames volumes of one resolution (out[f] may be vol[f]); scratch:
// n_frames * cc_scratch_bytes(r); gate: NULL or n_frames entries
size_t cc_scratch_bytes(int r);
int launch_keep_largest_batch(mp_ctx *ctx, void *scratch, int n_frames, const float *const *vol, int r, float level,
                              int connectivity, float fill, float *const *out, int32_t *const *stats,
                              const int32_t *const *gate, hipStream_t st);
// mesh.hip
size_t mesh_normals_scratch_bytes(int n_frames, long long max_v, long long max_f);
int launch_mesh_normals_batch(mp_ctx *ctx, void *scratch, int n_frames, const float *const *verts, long long max_v,
                              const int32_t *const *faces, long long max_f, const int32_t *const *counts, int mode,
                              float *const *normals, hipStream_t st);
int launch_mesh_points_batch(mp_ctx *ctx, int n_frames, const float *const *verts, long long max_v,
                             const int32_t *const *counts, float *const *points, int32_t *const *count_out,
                             hipStream_t st);
// simplify.hip: vertex clustering of n_frames meshes of one capacity on an n^3 grid of cells; inv[a] = n / (b_max[a] -
// b_min[a]) in f32; vmap: nullptr or n_frames entries; scratch: mesh_simplify_scratch_bytes(n_frames, n, ...)
size_t mesh_simplify_scratch_bytes(int n_frames, int n, long long max_v, long long max_f);
int launch_mesh_simplify_batch(mp_ctx *ctx, void *scratch, int n_frames, const float *const *verts, long long max_v,
                               const int32_t *const *faces, long long max_f, const int32_t *const *counts,
                               const float *bmin, const float *inv, int n, float *const *verts_out,
                               int32_t *const *faces_out, int32_t *const *counts_out, int32_t *const *vmap,
                               hipStream_t st);
// smooth.hip: `iterations` lambda | mu passes over n_frames meshes of one capacity; pin: fix the border vertices; ring:
// nullptr or n_frames entries (each may be nullptr); scratch: mesh_smooth_scratch_bytes(n_frames, ...)
size_t mesh_smooth_scratch_bytes(int n_frames, long long max_v, long long max_f);
int launch_mesh_smooth_batch(mp_ctx *ctx, void *scratch, int n_frames, const float *const *verts, long long max_v,
                             const int32_t *const *faces, long long max_f, const int32_t *const *counts,
                             int iterations, float lambda, float mu, int pin, float *const *verts_out,
                             int32_t *const *ring, hipStream_t st);
// raster.hip: n_frames meshes x n_views cameras (calibs: host, 12 floats per image, frame-major); attr / image / depth /
// face_id: nullptr or n_frames entries, each frame's views back to back; scratch: mesh_render_scratch_bytes(n_frames *
// n_views, ..., clip != nullptr).  clip: nullptr = mp_mesh_render_batch; else the near plane and MP_RENDER_* flags of
// mp_mesh_render_clip_batch (perspective cameras only: the caller has checked that)
struct MeshRenderClip {
  float near;
  int flags;
};
size_t mesh_render_scratch_bytes(int n_images, long long max_v, long long max_f, int h, int w, bool clip);
int launch_mesh_render_batch(mp_ctx *ctx, void *scratch, int n_frames, int n_views, const float *const *verts,
                             long long max_v, const int32_t *const *faces, long long max_f,
                             const int32_t *const *counts, const float *const *attr, int ch_major, const float *calibs,
                             int proj, int nearest, int h, int w, float scale, float bias, float lo, float hi,
                             float background, float *const *image, float *const *depth, int32_t *const *face_id,
                             const MeshRenderClip *clip, hipStream_t st);
// picture.hip: the covered pixels of n_frames flat pictures of n_pixels each -> counted point lists in ascending pixel
// order (scratch: picture_points_scratch_bytes(n_frames, n_pixels)), and the scatter of [3,capacity] values back
size_t picture_points_scratch_bytes(int n_frames, long long n_pixels);
int launch_picture_points_batch(mp_ctx *ctx, void *scratch, int n_frames, const int32_t *const *face_id,
                                const float *const *position, long long n_pixels, long long capacity,
                                float *const *points, int32_t *const *pixels, int32_t *const *count, hipStream_t st);
int launch_picture_paint_batch(mp_ctx *ctx, int n_frames, const float *const *values, const int32_t *const *pixels,
                               const int32_t *const *count, long long capacity, long long n_pixels, float scale,
                               float bias, float lo, float hi, float *const *image, hipStream_t st);
// scene.hip: the mip pyramid of a texture [ht,wt,3] (one launch per level), its lookup per pixel of n_frames UV
// pictures of n_pixels = n_views * h * w each, and the composite of two pictures per frame (depth / mask: nullptr or
// n_frames entries).  No scratch.  texture_sizes_ok: ht, wt in 1..8192, levels in 1..14 and no more than reach 1 x 1
bool texture_sizes_ok(int ht, int wt, int levels);
long long texture_pyramid_floats(int ht, int wt, int levels);
int launch_texture_mips(mp_ctx *ctx, const float *tex, int ht, int wt, int levels, float *pyramid, hipStream_t st);
int launch_picture_texture_batch(mp_ctx *ctx, int n_frames, const float *const *uv, const int32_t *const *face_id,
                                 long long n_pixels, int h, int w, const float *pyramid, int ht, int wt, int levels,
                                 int wrap, float scale, float bias, float lo, float hi, float background,
                                 float *const *image, hipStream_t st);
int launch_picture_composite_batch(mp_ctx *ctx, int n_frames, const float *const *front_image,
                                   const float *const *front_depth, const int32_t *const *front_face,
                                   const float *const *back_image, const float *const *back_depth,
                                   const int32_t *const *back_face, long long n_pixels, int mode, int nearest,
                                   float background, float *const *image, float *const *depth, uint8_t *const *mask,
                                   hipStream_t st);
// resolve.hip: the resolve of n_frames x n_views (<= kMaxFrames) supersampled pictures [samples h, samples w] to [h,w];
// a frame's views lie back to back.  Every array: nullptr (the plane is not given / not wanted) or n_frames entries.
// samples 2..4.  No scratch.
int launch_picture_resolve_batch(mp_ctx *ctx, int n_frames, int n_views, const float *const *image,
                                 const float *const *depth, const int32_t *const *face_id, const uint8_t *const *mask,
                                 int h, int w, int samples, int nearest, float *const *image_out,
                                 float *const *depth_out, int32_t *const *face_out, uint8_t *const *mask_out,
                                 float *const *coverage, hipStream_t st);
// scene.hip: the shadow of n_frames shadow maps [hs,ws] (depth, face ids: what the rasteriser wrote under each frame's
// light, light_calibs: host, 12 floats per frame) on n_frames pictures of n_pixels each.  image_in / image_out: both
// nullptr or both n_frames entries (image_out[f] may be image_in[f]); shade: nullptr or n_frames entries.  radius 0..3
int launch_picture_shadow_batch(mp_ctx *ctx, int n_frames, const float *const *image_in, const float *const *position,
                                const int32_t *const *face_id, long long n_pixels, const float *const *map_depth,
                                const int32_t *const *map_face, int hs, int ws, const float *light_calibs, int proj,
                                int nearest, float bias, int radius, float strength, float *const *image_out,
                                float *const *shade, hipStream_t st);
// light.hip: n_frames pictures of n_pixels = n_views * (pixels per view) each, lit by one parameter set (sh[27],
// direct_dir[3], direct_rgb[3], gamma, background: host).  albedo: nullptr (then albedo_rgb[3], host) or n_frames
// entries; visibility, image_out (may be albedo[f]), shading: nullptr or n_frames entries.  normal_mats: nullptr or
// host, n_frames * n_views (<= kLightMaxMats) row-major 3x3.  ambient: nullptr, or n_frames entries [n_pixels,3] that
// stand in for the SH term (mp_picture_light_transfer: sh and normal_mats unused, normal may be nullptr)
constexpr int kLightMaxMats = 32;
int launch_picture_light_batch(mp_ctx *ctx, int n_frames, const float *const *normal, const int32_t *const *face_id,
                               const float *const *albedo, const float *albedo_rgb, const float *const *visibility,
                               const float *const *ambient, long long n_pixels, int n_views, const float *sh,
                               const float *direct_dir, const float *direct_rgb, float gamma, const float *normal_mats,
                               float background, float *const *image_out, float *const *shading, hipStream_t st);
// jpeg.hip: [n_pixels,3] f32 -> uint8, and n pictures [h,w,3] f32 of one size -> n baseline JFIF files in out [n,capacity]
// with info [n,2] = {bytes, overflowed}; s420: 0 = 4:4:4, 1 = 4:2:0; restart: MCUs per interval, 0 = one MCU row;
// scratch: jpeg_scratch_bytes(n, ...).  jpeg_max_bytes: what no file of that geometry exceeds
int launch_picture_u8(mp_ctx *ctx, const float *image, long long n_pixels, uint8_t *out, hipStream_t st);
int jpeg_header_bytes();
long long jpeg_max_bytes(int h, int w, int s420, int restart);
size_t jpeg_scratch_bytes(int n, int h, int w, int s420, int restart);
int launch_picture_jpeg(mp_ctx *ctx, void *scratch, const float *images, int n, int h, int w, int quality, int s420,
                        int restart, uint8_t *out, long long capacity, int32_t *info, hipStream_t st);
// png.hip: the 16-bit and RGBA samples, and n pictures of one size -> n PNG files in out [n,capacity] with info [n,2] =
// {bytes, overflowed}.  format / filter: MP_PNG_* (checked by the caller); alpha: nullptr or [n,h,w]; scratch:
// png_scratch_bytes(n, ..., capacity).  png_max_bytes: what no file of that geometry exceeds
struct PngCall {  // host values of one call
  int n, h, w, format, filter, unmatte;
  float lo, scale, background;
  long long capacity;
};
int launch_picture_u16(mp_ctx *ctx, const float *depth, long long n_pixels, float lo, float scale, uint16_t *out,
                       hipStream_t st);
int launch_picture_rgba8(mp_ctx *ctx, const float *image, const float *alpha, long long n_pixels, int unmatte,
                         float background, uint8_t *out, hipStream_t st);
int png_min_bytes();
long long png_max_bytes(int h, int w, int format);
size_t png_scratch_bytes(const PngCall &c);
int launch_picture_png(mp_ctx *ctx, void *scratch, const float *images, const float *alpha, const PngCall &c,
                       uint8_t *out, int32_t *info, hipStream_t st);
// glb.hip: n_frames meshes of one capacity -> n_frames binary glTF files in out [n,capacity] with info [n,2] = {bytes,
// overflowed}.  normals / colors: nullptr as a whole, or one pointer per frame; inv: 65535 / (b_max - b_min) per axis;
// scratch: glb_scratch_bytes(n_frames).  glb_bytes: the closed form of the file size (flags: MP_GLB_*, checked by the
// caller; counts >= 0)
struct GlbCall {  // host values of one call
  int n_frames, color_planes;
  long long max_v, max_f, capacity;
  float color_scale, color_bias;
  float b_min[3], b_max[3], inv[3];
};
long long glb_bytes(long long nv, long long nf, int flags);
size_t glb_scratch_bytes(int n_frames);
int launch_mesh_glb_batch(mp_ctx *ctx, void *scratch, const GlbCall &c, const float *const *verts,
                          const int32_t *const *faces, const int32_t *const *counts, const float *const *normals,
                          const float *const *colors, uint8_t *out, int32_t *info, hipStream_t st);
// glb.hip: the textured file: GlbCall without its colour fields, and the atlas (size, cell) with the PNGs of the
// frames' atlases, png [n,png_capacity] and png_info [n,2] on the device.  Scratch: glb_scratch_bytes(n_frames).
// glb_textured_bytes: the closed form (flags: MP_GLB_NORMALS or 0, checked by the caller; nf, png_bytes >= 0)
struct GlbTextureCall {
  int size, cell;
  const uint8_t *png;
  long long png_capacity;
  const int32_t *png_info;
};
long long glb_textured_bytes(long long nf, int flags, long long png_bytes);
int launch_mesh_glb_textured_batch(mp_ctx *ctx, void *scratch, const GlbCall &c, const GlbTextureCall &tc,
                                   const float *const *verts, const int32_t *const *faces,
                                   const int32_t *const *counts, const float *const *normals, uint8_t *out,
                                   int32_t *info, hipStream_t st);
// atlas.hip: the texture-space G-buffer of n_frames meshes of one capacity: face_id [size^2], position [size^2,3] and
// info[2] per frame.  size: a power of two >= 64; cell: 4..64 (checked by the caller).  No scratch
int launch_mesh_atlas_batch(mp_ctx *ctx, int n_frames, const float *const *verts, long long max_v,
                            const int32_t *const *faces, long long max_f, const int32_t *const *counts, int size,
                            int cell, float background, int32_t *const *face_id, float *const *position,
                            int32_t *const *info, hipStream_t st);
#ifdef __HIPCC__
// v / |v|, or (0, 0, 0) where |v|^2 is not finite or not > 0 (a zero, a NaN, an inf, an overflow)
__device__ __forceinline__ void light_normalise(float x, float y, float z, float &ox, float &oy, float &oz) {
  const float s = (x * x + y * y) + z * z;
  if (!(__builtin_isfinite(s) && s > 0.0f)) {
    ox = oy = oz = 0.0f;
    return;
  }
  const float len = sqrtf(s);  // the correctly rounded one (vertices.hip)
  ox = x / len;
  oy = y / len;
  oz = z / len;
}
#endif
// transfer.hip: occupancy bits of n_frames volumes of one resolution (fine bits, then one bit per 8^3 block), the
// radiance transfer of n_frames meshes traced through them, and its product with the lighting's coefficients
long long volume_bits_words(int r);
int launch_volume_bits_batch(mp_ctx *ctx, int n_frames, const float *const *vol, int r, float level,
                             uint32_t *const *bits, const int32_t *const *gate, hipStream_t st);
struct TransferRays {  // host values of one call
  float bmin[3], bmax[3];
  int r, n_dirs, max_steps;
  const float *dirs, *basis;  // device [n_dirs,3], [n_dirs,9]
  float weight, bias_w, step_w;
};
int launch_mesh_transfer_batch(mp_ctx *ctx, int n_frames, const float *const *verts, const float *const *normals,
                               long long max_v, const int32_t *const *counts, const uint32_t *const *bits,
                               const TransferRays &rays, uint64_t *const *mask, float *const *prt, hipStream_t st);
int launch_mesh_transfer_shade_batch(mp_ctx *ctx, int n_frames, const float *const *prt, long long max_v,
                                     const int32_t *const *counts, const float *sh, float *const *out, hipStream_t st);

// conv3x3.hip
int launch_conv3x3_pack(mp_ctx *ctx, const float *w, int cout, int cin, float *wp, hipStream_t st);
int conv3x3_stat_slices(int cout, int n, int h, int w, bool f16);
void conv3x3_set_nr(int nr);
bool conv3x3_supported(int cin, int cout, int h, int w);
bool conv_stats_supported(int cout);
int launch_conv3x3_pack16(mp_ctx *ctx, const float *w, int cout, int cin, void *wp, float *wmax,
                          hipStream_t st);
int launch_conv3x3_gn(mp_ctx *ctx, const float *x, int n, int cin, int h, int w, const float *ss,
                      int relu, int reflect, const float *wp, const float *wmax16, int cout, float *y,
                      double *stats, hipStream_t st);
int launch_scale_shift_add(mp_ctx *ctx, const float *t, const float *ss, const float *res, long long planes,
                           long long hw, float *y, hipStream_t st);
int launch_conv1x1_pack(mp_ctx *ctx, const float *w1, int c1, const float *w2, int c2, int cout, int f16,
                        void *wp, float *wmax, hipStream_t st);
int launch_conv1x1_raw(mp_ctx *ctx, const float *x1, const float *ss1, int relu1, const float *x2, int n,
                       int c1, int c2, int cout, long long hw, const void *wp, int f16, const float *wmax,
                       const float *bias, const float *res, float *y, float *y_hwc, double *stats,
                       hipStream_t st);
int launch_gn_finalize(mp_ctx *ctx, const double *partial, int n, int c, int groups, int slices,
                       double count, const float *gamma, const float *beta, float eps, float *ss,
                       hipStream_t st);
// encoder_ops.hip
int gn_stat_slices();
int launch_gn_stats(mp_ctx *ctx, const float *x, int n, int c, long long hw, int groups,
                    double *partial, hipStream_t st);
size_t gn_scratch_bytes(int groups);
int launch_group_norm(mp_ctx *ctx, void *scratch, const float *x, int n, int c, long long hw,
                      int groups, const float *gamma, const float *beta, float eps, int relu,
                      float *y, hipStream_t st);
int launch_upsample_bicubic2x(mp_ctx *ctx, const float *x, int c, int h, int w, const float *add,
                              float *y, hipStream_t st);

}  // namespace mp
