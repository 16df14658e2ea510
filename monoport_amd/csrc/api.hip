// C-ABI entry points of libmonoport_hip.so (see include/monoport_hip.h for the contract).
#include <cstdarg>
#include <cmath>
#include <cstring>

#include "mp_internal.h"
#include "encoder_kernels.h"
#include "octree_common.h"

namespace mp {

// The last error message is kept PER HOST THREAD (like errno): the stage threads of a pipeline
// share one context, and a message must not be overwritten -- or its storage reallocated --
// between a failing call and the caller's mp_last_error on the same thread.
static thread_local std::string g_last_error;

int fail(mp_ctx *ctx, int code, const char *fmt, ...) {
  (void)ctx;
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_last_error = buf;
  return code;
}

// Scratch grows by ADDING a block: the previous block stays allocated until mp_stream_release /
// mp_destroy, because a hipGraph captured on this stream (the encoder graph of a pipeline slot
// bakes mp_group_norm's scratch pointer) or work still queued on it may reference it.  Sizes are
// rounded up geometrically so a stream retires at most a handful of blocks.
int ensure_scratch(mp_ctx *ctx, hipStream_t st, size_t bytes, void **out) {
  mp_ctx::Arena &a = ctx->arenas[(void *)st];
  if (bytes > a.bytes) {
    size_t want = a.bytes + a.bytes / 2;
    if (want < bytes) want = bytes;
    want = (want + 0xFFFF) & ~size_t(0xFFFF);
    void *p = nullptr;
    if (hipMalloc(&p, want) != hipSuccess) {
      (void)hipGetLastError();  // the failed attempt must not surface as the next launch's error
      if (want == bytes || hipMalloc(&p, want = bytes) != hipSuccess) {
        (void)hipGetLastError();
        return fail(ctx, MP_ERR_NOMEM, "scratch arena: hipMalloc(%zu) failed", want);
      }
    }
    if (a.ptr) {
      a.retired.push_back(a.ptr);
      a.retired_bytes += a.bytes;
    }
    a.ptr = p;
    a.bytes = want;
  }
  *out = a.ptr;
  return MP_OK;
}

MlpPack Mlp::pack() const {
  MlpPack p;
  p.base = buf;
  for (int l = 0; l < 4; ++l) {
    p.ah[l] = (int)off_ah[l];
    p.ax[l] = (int)off_ax[l];
    p.az[l] = (int)off_az[l];
  }
  for (int l = 0; l < 5; ++l) p.bias[l] = (int)off_bias[l];
  p.w4 = (int)off_w4;
  p.n_floats = (int)total;
  return p;
}

MlpPack16 Mlp::pack16() const {
  MlpPack16 p;
  p.base = buf16;
  for (int l = 0; l < 4; ++l) {
    p.ah[l] = (int)off16_ah[l];
    p.ax[l] = (int)off16_ax[l];
    p.az[l] = (int)off16_az[l];
    p.scale[l] = scale16[l];
  }
  p.n16 = (int)total16;
  return p;
}

static bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

struct DeviceGuard {
  int prev = -1;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != dev) (void)hipSetDevice(dev);
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

static Mlp *get_mlp(mp_ctx *ctx, int id) {
  if (id < 0 || id >= (int)ctx->mlps.size() || !ctx->mlps[id].used) return nullptr;
  return &ctx->mlps[id];
}

static int check_ready(mp_ctx *ctx, const Mlp *m, int c) {
  if (!m) return fail(ctx, MP_ERR_ARG, "unknown mlp id");
  for (int l = 0; l < 5; ++l)
    if (!m->loaded[l]) return fail(ctx, MP_ERR_STATE, "mlp layer %d has not been loaded", l);
  if (m->c != c)
    return fail(ctx, MP_ERR_ARG, "feature map has C=%d but the mlp was built for C=%d", c, m->c);
  return MP_OK;
}

// per-frame projection modes of a call (host array; NULL = every frame orthogonal)
static int check_projection(mp_ctx *ctx, const char *who, const int *proj, int n_frames) {
  if (!proj) return MP_OK;
  for (int f = 0; f < n_frames; ++f)
    if (proj[f] != MP_PROJ_ORTHOGONAL && proj[f] != MP_PROJ_PERSPECTIVE)
      return fail(ctx, MP_ERR_ARG, "%s: frame %d has projection %d (MP_PROJ_ORTHOGONAL / MP_PROJ_PERSPECTIVE)", who,
                  f, proj[f]);
  return MP_OK;
}

// ---- the argument checks and marshalling the query / recon entry points share ----------------------------------
// Every check refuses before anything is launched or allocated; `who` is the entry point's name in the message.

// Prologue of an entry point that evaluates a head: context, lock, the head exists, is loaded and was built for `c`
// feature channels.  The lock is held while the object lives.  `who` != nullptr (mp_mlp_forward*: no feature map):
// the head's own width is taken, and an unknown id is reported under that name.
struct HeadCall {
  std::unique_lock<std::mutex> lk;
  const Mlp *m = nullptr;
  int rc = MP_ERR_ARG;
  HeadCall(mp_ctx *ctx, int mlp, int c, const char *who = nullptr) {
    if (!ctx) return;
    lk = std::unique_lock<std::mutex>(ctx->mu);
    m = get_mlp(ctx, mlp);
    if (who && !m)
      rc = fail(ctx, MP_ERR_ARG, "%s: unknown mlp id %d", who, mlp);
    else
      rc = check_ready(ctx, m, who ? m->c : c);
  }
};

static int bad_argument(mp_ctx *ctx, const char *who) { return fail(ctx, MP_ERR_ARG, "%s: bad argument", who); }

// 1..max frames (MP_ERR_ARG) / views (MP_ERR_UNSUPPORTED) per call
static int check_count(mp_ctx *ctx, const char *who, const char *what, int n, int max, int code) {
  if (n < 1 || n > max) return fail(ctx, code, "%s: 1..%d %ss per call, got %d", who, max, what, n);
  return MP_OK;
}

// The n items of a call's host arrays, one per frame / view (`what`): every device map set and 16-byte aligned (the
// kernels read texels as float4), every item of the `other` arrays set; an array passed as nullptr is one this call
// does not read.  The arrays themselves and the map size are part of the caller's own "bad argument" line, which keeps
// each entry point's order of refusals.
template <class... P>
static int check_maps(mp_ctx *ctx, const char *who, const char *what, int n, const float *const *maps, P... other) {
  for (int i = 0; i < n; ++i) {
    if (!maps[i] || (... || (other && !other[i])))
      return fail(ctx, MP_ERR_ARG, "%s: null buffer for %s %d", who, what, i);
    if (!aligned16(maps[i])) return fail(ctx, MP_ERR_ARG, "%s: feat_hwc must be 16-byte aligned", who);
  }
  return MP_OK;
}

// The n frames of a mesh / render stage's host arrays: every buffer set and 4-byte aligned (the kernels read them as
// float / int32 / int64).  A `rows` array passed as nullptr is one this call does not read (rows of a capacity of 0);
// `gate` may be nullptr, and so may each of its entries.
template <class... P>
static int check_frames(mp_ctx *ctx, const char *who, int n, const int32_t *const *gate, P... rows) {
  for (int f = 0; f < n; ++f) {
    if ((... || (rows && !rows[f]))) return fail(ctx, MP_ERR_ARG, "%s: null buffer for frame %d", who, f);
    if (((gate ? (uintptr_t)gate[f] : uintptr_t(0)) | ... | (rows ? (uintptr_t)rows[f] : uintptr_t(0))) & 3)
      return fail(ctx, MP_ERR_ARG, "%s: misaligned buffer for frame %d", who, f);
  }
  return MP_OK;
}

// What a launcher gets of such an array: rows of a capacity of 0 (`rows` == nullptr) are no pointer at all
template <class T>
struct FrameRows {
  T *p[kMaxFrames];
  FrameRows(T *const *rows, int n) {
    for (int f = 0; f < n; ++f) p[f] = rows ? rows[f] : nullptr;
  }
};

static int check_f32_views(mp_ctx *ctx, const char *who, const Mlp *m) {
  if (m->precision != MP_PREC_F32)
    return fail(ctx, MP_ERR_UNSUPPORTED, "%s: the multi-view kernel is f32 only (head precision %d)", who,
                m->precision);
  return MP_OK;
}

static int check_final_level(mp_ctx *ctx, const char *who, int final_level) {
  if (final_level != MP_FINAL_DILATE3 && final_level != MP_FINAL_UPSTREAM && final_level != MP_FINAL_INTERPOLATE)
    return fail(ctx, MP_ERR_ARG, "%s: final_level must be MP_FINAL_DILATE3 / _UPSTREAM / _INTERPOLATE, got %d", who,
                final_level);
  return MP_OK;
}

// `code`: MP_ERR_UNSUPPORTED from the single-view family, MP_ERR_ARG from mp_recon_views (include/monoport_hip.h)
static int check_resolutions(mp_ctx *ctx, const char *who, const int *resolutions, int n_levels, int code) {
  for (int l = 0; l < n_levels; ++l) {
    if (resolutions[l] < 2 || resolutions[l] > 1023)
      return fail(ctx, code, "%s: resolution %d outside [2,1023]", who, resolutions[l]);
    if (l > 0 && resolutions[l] != 2 * resolutions[l - 1] - 1)
      return fail(ctx, code, "%s: resolutions must follow r -> 2r-1 (got %d after %d)", who, resolutions[l],
                  resolutions[l - 1]);
  }
  return MP_OK;
}

// `field`: how the entry point's message names the first of the two buffers
static int check_early(mp_ctx *ctx, const char *who, const mp_recon_early *early, const char *field) {
  if (early && (!early->flags_dev || !early->flags_host))
    return fail(ctx, MP_ERR_ARG, "%s: %s and flags_host are required", who, field);
  return MP_OK;
}

// Point layouts of the explicit (non-lattice) query calls: element (c, i) at pts[i*sn + c*sc], output (o, i) at
// out[o*n + i], n points counted on the host ...
static PointSrc strided_points(const float *pts, long long n, long long sn, long long sc) {
  PointSrc src;
  std::memset(&src, 0, sizeof(src));
  src.pts = pts;
  src.sn = sn;
  src.sc = sc;
  src.n = n;
  src.out_stride = n;
  return src;
}

// ... or contiguous rows [rows,capacity] of which the first *count (device) are points
static PointSrc counted_points(const float *pts, long long capacity, const int32_t *count) {
  PointSrc src = strided_points(pts, 0, 1, capacity);
  src.n_dev = count;
  src.out_stride = capacity;
  return src;
}

// n frames of one layout: frame f takes its points (and device count, if the layout has one) from points[f] / count[f]
static QuerySet query_set(int n, const float *const *feat_hwc, const float *const *calib, const int *projection,
                          const float *const *points, const int32_t *const *count, float *const *out,
                          const PointSrc &layout) {
  QuerySet set;
  std::memset(&set, 0, sizeof(set));
  set.n = n;
  for (int f = 0; f < n; ++f) {
    QueryItem &q = set.it[f];
    q.feat = feat_hwc[f];
    q.calib = calib[f];
    q.proj = projection ? projection[f] : MP_PROJ_ORTHOGONAL;
    q.out = out[f];
    q.src = layout;
    q.src.pts = points[f];
    if (count) q.src.n_dev = count[f];
  }
  return set;
}

// nv views of n points in the layout of strided_points
static ViewSetDev view_set(int nv, int projection, long long n, long long sn, long long sc) {
  ViewSetDev set;
  std::memset(&set, 0, sizeof(set));
  set.nv = nv;
  set.proj = projection;
  set.n = n;
  set.sn = sn;
  set.sc = sc;
  set.out_stride = n;
  return set;
}

// budget and bound of one top-k level of r^3 nodes
static int check_topk(mp_ctx *ctx, const char *who, int r, long long k, float max_dist) {
  if (k < 0 || k > (long long)r * r * r)
    return fail(ctx, MP_ERR_ARG, "%s: a budget of %lld points for %d^3 nodes", who, k, r);
  if (max_dist != max_dist || max_dist < 0.0f)
    return fail(ctx, MP_ERR_ARG, "%s: max_dist must be >= 0 (or +inf for none), got %g", who, (double)max_dist);
  return MP_OK;
}

// What mp_recon_batch_proj (views == nullptr: n_frames frames with a projection each, NULL = orthogonal) and
// mp_recon_views / mp_recon_views_batch (n_frames frames seen by views->nv maps each, all with projection[0]) do once
// head, counts and maps are accepted.
// num_points != nullptr (mp_recon_topk_batch): the fixed-budget selection with these per-level budgets and bounds.
static int recon_checked(mp_ctx *ctx, const char *who, const Mlp &m, int n_frames, const float *const *feat_hwc, int h,
                         int w, const float *const *calib, const int *projection, float z_scale, const float *b_min,
                         const float *b_max, const int *resolutions, int n_levels, int resolution_code, float balance,
                         int final_level, float *const *volume, int32_t *const *status, const mp_recon_early *early,
                         const char *early_field, mp_stream stream, const ReconViews *views,
                         const long long *num_points = nullptr, const float *max_dist = nullptr) {
  int rc = check_final_level(ctx, who, final_level);
  if (rc == MP_OK) rc = check_resolutions(ctx, who, resolutions, n_levels, resolution_code);
  if (rc == MP_OK) rc = check_projection(ctx, who, projection, views ? 1 : n_frames);
  if (rc == MP_OK) rc = check_early(ctx, who, early, early_field);
  for (int l = 1; rc == MP_OK && num_points && l < n_levels; ++l)  // the top-k selection: entry 0 is not looked at
    rc = check_topk(ctx, who, resolutions[l], num_points[l], max_dist ? max_dist[l] : INFINITY);
  if (rc != MP_OK) return rc;
  DeviceGuard g(ctx->device);
  void *scratch = nullptr;
  const size_t lossless_bytes = n_frames * recon_scratch_bytes(resolutions, n_levels, h, w);
  const size_t topk_bytes = num_points ? topk_scratch_bytes(n_frames, resolutions[n_levels - 1]) : 0;
  rc = ensure_scratch(ctx, (hipStream_t)stream, lossless_bytes + topk_bytes, &scratch);
  if (rc != MP_OK) return rc;
  const ReconTopk topk = {num_points, max_dist, static_cast<unsigned char *>(scratch) + lossless_bytes};
  return launch_recon(ctx, scratch, m, n_frames, feat_hwc, h, w, calib, projection, z_scale, b_min, b_max, resolutions,
                      n_levels, balance, final_level, volume, status, early, (hipStream_t)stream, views,
                      num_points ? &topk : nullptr);
}

// ---- the mesh and render stages: one checked body each ---------------------------------------------------------------
// mp_<stage>_batch passes its arguments on; mp_<stage> is the batched call with one frame: it passes 1 and the addresses
// of its own arguments, so both forms refuse the same and launch the same.  `who` is the entry the caller used.

static int forward_vertices_checked(mp_ctx *ctx, const char *who, int n_frames, const float *const *volume, int r,
                                    int direction, int64_t *const *x, int64_t *const *y, float *const *z,
                                    float *const *norm, int32_t *const *count, mp_stream stream) {
  if (!ctx) return MP_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  int rc = check_count(ctx, who, "frame", n_frames, kMaxFrames, MP_ERR_ARG);
  if (rc != MP_OK) return rc;
  if (!volume || !x || !y || !z || !norm || !count || r < 1 || r > 4096 || direction < MP_DIR_FRONT ||
      direction > MP_DIR_RIGHT)
    return bad_argument(ctx, who);
  rc = check_frames(ctx, who, n_frames, nullptr, volume, x, y, z, norm, count);
  if (rc != MP_OK) return rc;
  DeviceGuard g(ctx->device);
  void *scratch = nullptr;
  rc = ensure_scratch(ctx, (hipStream_t)stream, (size_t)n_frames * forward_vertices_scratch_bytes(r) + 4096, &scratch);
  if (rc != MP_OK) return rc;
  return launch_forward_vertices_batch(ctx, scratch, n_frames, volume, r, direction, x, y, z, norm, count,
                                       (hipStream_t)stream);
}

static int paint_checked(mp_ctx *ctx, const char *who, int n_frames, const int64_t *const *x, const int64_t *const *y,
                         const float *const *values, int channel_major, const int32_t *const *count, int64_t capacity,
                         int res, float scale, float bias, float lo, float hi, float *const *image, mp_stream stream) {
  if (!ctx) return MP_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  int rc = check_count(ctx, who, "frame", n_frames, kMaxFrames, MP_ERR_ARG);
  if (rc != MP_OK) return rc;
  if (!x || !y || !values || !count || !image || capacity < 0 || res < 1) return bad_argument(ctx, who);
  rc = check_frames(ctx, who, n_frames, nullptr, x, y, values, count, image);
  if (rc != MP_OK) return rc;
  DeviceGuard g(ctx->device);
  return launch_paint_batch(ctx, n_frames, x, y, values, channel_major, count, capacity, res, scale, bias, lo, hi,
                            image, (hipStream_t)stream);
}

static int marching_cubes_checked(mp_ctx *ctx, const char *who, int n_frames, const float *const *volume, int r,
                                  float level, const float *b_min, const float *b_max, float *const *verts,
                                  int64_t max_verts, int32_t *const *faces, int64_t max_faces, int32_t *const *counts,
                                  const int32_t *const *gate, mp_stream stream) {
  if (!ctx) return MP_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  int rc = check_count(ctx, who, "frame", n_frames, kMaxFrames, MP_ERR_ARG);
  if (rc != MP_OK) return rc;
  if (!volume || !b_min || !b_max || !counts || r < 2 || r > 1023 || max_verts < 0 || max_faces < 0 ||
      (max_verts > 0 && !verts) || (max_faces > 0 && !faces))
    return bad_argument(ctx, who);
  if (max_verts == 0) verts = nullptr;
  if (max_faces == 0) faces = nullptr;
  rc = check_frames(ctx, who, n_frames, gate, volume, counts, verts, faces);
  if (rc != MP_OK) return rc;
  const FrameRows verts_p(verts, n_frames);
  const FrameRows faces_p(faces, n_frames);
  DeviceGuard g(ctx->device);
  void *scratch = nullptr;
  rc = ensure_scratch(ctx, (hipStream_t)stream, (size_t)n_frames * mc_scratch_bytes(r), &scratch);
  if (rc != MP_OK) return rc;
  return launch_marching_cubes_batch(ctx, scratch, n_frames, volume, r, level, b_min, b_max, verts_p.p, max_verts,
                                     faces_p.p, max_faces, counts, gate, (hipStream_t)stream);
}

static int mesh_normals_checked(mp_ctx *ctx, const char *who, int n_frames, const float *const *verts,
                                int64_t max_verts, const int32_t *const *faces, int64_t max_faces,
                                const int32_t *const *counts, int mode, float *const *normals, mp_stream stream) {
  if (!ctx) return MP_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  int rc = check_count(ctx, who, "frame", n_frames, kMaxFrames, MP_ERR_ARG);
  if (rc != MP_OK) return rc;
  if (!counts || max_verts < 0 || max_faces < 0 || (max_verts > 0 && (!verts || !normals)) ||
      (max_faces > 0 && !faces) || (mode != MP_NORMALS_REFERENCE && mode != MP_NORMALS_ACCUMULATE))
    return bad_argument(ctx, who);
  if (max_verts > 0x7fffffffLL / 3 || max_faces > 0x7fffffffLL / 3)
    return fail(ctx, MP_ERR_UNSUPPORTED, "%s: capacities beyond 2^31 / 3 need 64-bit indices", who);
  if (max_verts == 0) verts = nullptr, normals = nullptr;
  if (max_faces == 0) faces = nullptr;
  rc = check_frames(ctx, who, n_frames, nullptr, counts, verts, normals, faces);
  if (rc != MP_OK) return rc;
  if (max_verts == 0) return MP_OK;
  const FrameRows faces_p(faces, n_frames);
  DeviceGuard g(ctx->device);
  void *scratch = nullptr;
  rc = ensure_scratch(ctx, (hipStream_t)stream, mesh_normals_scratch_bytes(n_frames, max_verts, max_faces), &scratch);
  if (rc != MP_OK) return rc;
  return launch_mesh_normals_batch(ctx, scratch, n_frames, verts, max_verts, faces_p.p, max_faces, counts, mode,
                                   normals, (hipStream_t)stream);
}

// true if [a, a + na) and [b, b + nb) share a byte (either empty or null: no)
static bool ranges_overlap(const void *a, size_t na, const void *b, size_t nb) {
  const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
  return a && b && na && nb && pa < pb + nb && pb < pa + na;
}

// the buffers of one kind of a batched mesh call: rows[f] is frame f's, `bytes` long (rows null as a whole: none)
struct FrameSpans {
  const void *const *rows;
  size_t bytes;
  template <typename T>
  FrameSpans(T *const *r, size_t b) : rows((const void *const *)r), bytes(b) {}
  const void *of(int f) const { return rows ? rows[f] : nullptr; }
};

// MP_OK unless an output of some frame shares a byte with an input of some frame
template <int N_OUT, int N_IN>
static int check_no_alias(mp_ctx *ctx, const char *who, int n_frames, const FrameSpans (&outs)[N_OUT],
                          const FrameSpans (&ins)[N_IN]) {
  for (int f = 0; f < n_frames; ++f)
    for (int i = 0; i < n_frames; ++i)
      for (const FrameSpans &o : outs)
        for (const FrameSpans &k : ins)
          if (ranges_overlap(o.of(f), o.bytes, k.of(i), k.bytes))
            return fail(ctx, MP_ERR_ARG, "%s: an output of frame %d aliases an input of frame %d", who, f, i);
  return MP_OK;
}

static int mesh_simplify_checked(mp_ctx *ctx, const char *who, int n_frames, const float *const *verts,
                                 int64_t max_verts, const int32_t *const *faces, int64_t max_faces,
                                 const int32_t *const *counts, const float *b_min, const float *b_max, int n,
                                 float *const *verts_out, int32_t *const *faces_out, int32_t *const *counts_out,
                                 int32_t *const *vmap, mp_stream stream) {
  if (!ctx) return MP_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  int rc = check_count(ctx, who, "frame", n_frames, kMaxFrames, MP_ERR_ARG);
  if (rc != MP_OK) return rc;
  if (!counts || !counts_out || !b_min || !b_max || max_verts < 0 || max_faces < 0 ||
      (max_verts > 0 && (!verts || !verts_out)) || (max_faces > 0 && (!faces || !faces_out)))
    return bad_argument(ctx, who);
  if (n < 1 || n > 512) return fail(ctx, MP_ERR_ARG, "%s: 1..512 cells per axis, got %d", who, n);
  float inv[3];
  for (int a = 0; a < 3; ++a) {
    if (!std::isfinite(b_min[a]) || !std::isfinite(b_max[a]) || !(b_max[a] > b_min[a]))
      return fail(ctx, MP_ERR_ARG, "%s: the box needs finite bounds with b_max > b_min, got [%g, %g] on axis %d", who,
                  (double)b_min[a], (double)b_max[a], a);
    inv[a] = (float)n / (b_max[a] - b_min[a]);
    if (!std::isfinite(inv[a]))
      return fail(ctx, MP_ERR_ARG, "%s: the box is too thin on axis %d for %d cells (%g wide)", who, a, n,
                  (double)(b_max[a] - b_min[a]));
  }
  if (max_verts > (1LL << 27))
    return fail(ctx, MP_ERR_UNSUPPORTED, "%s: more than 2^27 vertices could overflow the 64-bit coordinate sums", who);
  if (max_faces > 0x7fffffffLL / 3)
    return fail(ctx, MP_ERR_UNSUPPORTED, "%s: capacities beyond 2^31 / 3 need 64-bit indices", who);
  if (max_verts == 0) verts = nullptr, verts_out = nullptr, vmap = nullptr;  // rows of a capacity of 0 are not looked at
  if (max_faces == 0) faces = nullptr, faces_out = nullptr;
  rc = check_frames(ctx, who, n_frames, nullptr, counts, counts_out, verts, verts_out, faces, faces_out, vmap);
  if (rc != MP_OK) return rc;
  const size_t vbytes = (size_t)max_verts * 12, fbytes = (size_t)max_faces * 12;
  const FrameSpans ins[3] = {{verts, vbytes}, {faces, fbytes}, {counts, 8}};
  const FrameSpans outs[4] = {{verts_out, vbytes}, {faces_out, fbytes}, {counts_out, 8}, {vmap, (size_t)max_verts * 4}};
  rc = check_no_alias(ctx, who, n_frames, outs, ins);
  if (rc != MP_OK) return rc;
  DeviceGuard g(ctx->device);
  if (max_verts == 0) {  // no vertex, hence no face: the counts are all there is to write
    for (int f = 0; f < n_frames; ++f) MP_HIP(ctx, hipMemsetAsync(counts_out[f], 0, 8, (hipStream_t)stream));
    return MP_OK;
  }
  const FrameRows faces_p(faces, n_frames);
  const FrameRows faces_out_p(faces_out, n_frames);
  void *scratch = nullptr;
  rc = ensure_scratch(ctx, (hipStream_t)stream, mesh_simplify_scratch_bytes(n_frames, n, max_verts, max_faces),
                      &scratch);
  if (rc != MP_OK) return rc;
  return launch_mesh_simplify_batch(ctx, scratch, n_frames, verts, max_verts, faces_p.p, max_faces, counts, b_min, inv,
                                    n, verts_out, faces_out_p.p, counts_out, vmap, (hipStream_t)stream);
}

static int mesh_smooth_checked(mp_ctx *ctx, const char *who, int n_frames, const float *const *verts,
                               int64_t max_verts, const int32_t *const *faces, int64_t max_faces,
                               const int32_t *const *counts, int iterations, float lambda, float mu, int flags,
                               float *const *verts_out, int32_t *const *ring, mp_stream stream) {
  if (!ctx) return MP_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  int rc = check_count(ctx, who, "frame", n_frames, kMaxFrames, MP_ERR_ARG);
  if (rc != MP_OK) return rc;
  if (!counts || max_verts < 0 || max_faces < 0 || (max_verts > 0 && (!verts || !verts_out)) ||
      (max_faces > 0 && !faces))
    return bad_argument(ctx, who);
  if (iterations < 1 || iterations > 64) return fail(ctx, MP_ERR_ARG, "%s: 1..64 iterations, got %d", who, iterations);
  if (!std::isfinite(lambda) || !std::isfinite(mu))
    return fail(ctx, MP_ERR_ARG, "%s: lambda and mu must be finite, got %g and %g", who, (double)lambda, (double)mu);
  if (flags & ~MP_SMOOTH_PIN_BORDER) return fail(ctx, MP_ERR_ARG, "%s: unknown flags 0x%x", who, (unsigned)flags);
  if (max_faces > 0x7fffffffLL / 6)
    return fail(ctx, MP_ERR_UNSUPPORTED, "%s: capacities beyond 2^31 / 6 faces need a 64-bit edge list", who);
  if (max_verts == 0) verts = nullptr, verts_out = nullptr, ring = nullptr;  // rows of a capacity of 0 are not looked at
  if (max_faces == 0) faces = nullptr;
  rc = check_frames(ctx, who, n_frames, nullptr, counts, verts, verts_out, faces);
  if (rc != MP_OK) return rc;
  if (ring)  // each entry may be NULL: that frame's ring is not wanted
    for (int f = 0; f < n_frames; ++f)
      if ((uintptr_t)ring[f] & 3) return fail(ctx, MP_ERR_ARG, "%s: misaligned buffer for frame %d", who, f);
  const size_t vbytes = (size_t)max_verts * 12, fbytes = (size_t)max_faces * 12;
  const FrameSpans ins[3] = {{verts, vbytes}, {faces, fbytes}, {counts, 8}};
  const FrameSpans outs[2] = {{verts_out, vbytes}, {ring, (size_t)max_verts * 4}};
  rc = check_no_alias(ctx, who, n_frames, outs, ins);
  if (rc != MP_OK) return rc;
  if (max_verts == 0) return MP_OK;  // no vertex: nothing to move
  DeviceGuard g(ctx->device);
  const FrameRows faces_p(faces, n_frames);
  void *scratch = nullptr;
  rc = ensure_scratch(ctx, (hipStream_t)stream, mesh_smooth_scratch_bytes(n_frames, max_verts, max_faces), &scratch);
  if (rc != MP_OK) return rc;
  return launch_mesh_smooth_batch(ctx, scratch, n_frames, verts, max_verts, faces_p.p, max_faces, counts, iterations,
                                  lambda, mu, flags & MP_SMOOTH_PIN_BORDER, verts_out, ring, (hipStream_t)stream);
}

static int mesh_points_checked(mp_ctx *ctx, const char *who, int n_frames, const float *const *verts,
                               int64_t max_verts, const int32_t *const *counts, float *const *points,
                               int32_t *const *count_out, mp_stream stream) {
  if (!ctx) return MP_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  int rc = check_count(ctx, who, "frame", n_frames, kMaxFrames, MP_ERR_ARG);
  if (rc != MP_OK) return rc;
  if (!counts || !count_out || max_verts < 0 || (max_verts > 0 && (!verts || !points))) return bad_argument(ctx, who);
  if (max_verts == 0) verts = nullptr, points = nullptr;
  rc = check_frames(ctx, who, n_frames, nullptr, counts, count_out, verts, points);
  if (rc != MP_OK) return rc;
  const FrameRows verts_p(verts, n_frames);
  const FrameRows points_p(points, n_frames);
  DeviceGuard g(ctx->device);
  return launch_mesh_points_batch(ctx, n_frames, verts_p.p, max_verts, counts, points_p.p, count_out,
                                  (hipStream_t)stream);
}

static int mesh_render_checked(mp_ctx *ctx, const char *who, int n_frames, const float *const *verts, int64_t max_verts,
                               const int32_t *const *faces, int64_t max_faces, const int32_t *const *counts,
                               const float *const *attr, int channel_major, int n_views, const float *calibs,
                               int projection, int nearest, int h, int w, float scale, float bias, float lo, float hi,
                               float background, float *const *image, float *const *depth, int32_t *const *face_id,
                               const MeshRenderClip *clip, mp_stream stream) {
  if (!ctx) return MP_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (n_frames < 1 || n_views < 1 || (long long)n_frames * n_views > kMaxFrames)
    return fail(ctx, MP_ERR_ARG, "%s: 1..%d images (frames x views) per call, got %d x %d", who, kMaxFrames, n_frames,
                n_views);
  if (h < 1 || h > 4096 || w < 1 || w > 4096)
    return fail(ctx, MP_ERR_ARG, "%s: image size %d x %d outside 1..4096", who, h, w);
  if (projection != MP_PROJ_ORTHOGONAL && projection != MP_PROJ_PERSPECTIVE)
    return fail(ctx, MP_ERR_ARG, "%s: unknown projection mode %d", who, projection);
  if (nearest != MP_NEAREST_MAX_Z && nearest != MP_NEAREST_MIN_Z)
    return fail(ctx, MP_ERR_ARG, "%s: nearest must be MP_NEAREST_MAX_Z / _MIN_Z, got %d", who, nearest);
  if (clip) {
    if (projection != MP_PROJ_PERSPECTIVE)
      return fail(ctx, MP_ERR_ARG, "%s: the near plane clips perspective cameras only (MP_PROJ_PERSPECTIVE)", who);
    if (!std::isfinite(clip->near) || !(clip->near > 0.0f))
      return fail(ctx, MP_ERR_ARG, "%s: near must be finite and > 0, got %g", who, (double)clip->near);
    if (clip->flags & ~MP_RENDER_PERSPECTIVE_CORRECT)
      return fail(ctx, MP_ERR_ARG, "%s: unknown flag bits 0x%x (MP_RENDER_PERSPECTIVE_CORRECT)", who,
                  (unsigned)(clip->flags & ~MP_RENDER_PERSPECTIVE_CORRECT));
  }
  if (!image && !depth && !face_id) return fail(ctx, MP_ERR_ARG, "%s: no output requested", who);
  if (image && !attr) return fail(ctx, MP_ERR_ARG, "%s: an image needs attr", who);
  if (!counts || !calibs || max_verts < 0 || max_faces < 0 || (max_verts > 0 && !verts) || (max_faces > 0 && !faces))
    return bad_argument(ctx, who);
  if (max_verts > 0x7fffffffLL / 3 || max_faces > 0x7fffffffLL / 3)
    return fail(ctx, MP_ERR_UNSUPPORTED, "%s: capacities beyond 2^31 / 3 need 64-bit indices", who);
  if (max_verts == 0) verts = nullptr;  // rows of a capacity of 0 are not looked at
  if (max_faces == 0) faces = nullptr;
  int rc = check_frames(ctx, who, n_frames, nullptr, counts, verts, faces, max_verts > 0 ? attr : nullptr, image, depth,
                        face_id);
  if (rc != MP_OK) return rc;
  DeviceGuard g(ctx->device);
  void *scratch = nullptr;
  rc = ensure_scratch(ctx, (hipStream_t)stream,
                      mesh_render_scratch_bytes(n_frames * n_views, max_verts, max_faces, h, w, clip != nullptr),
                      &scratch);
  if (rc != MP_OK) return rc;
  return launch_mesh_render_batch(ctx, scratch, n_frames, n_views, verts, max_verts, faces, max_faces, counts, attr,
                                  channel_major, calibs, projection, nearest, h, w, scale, bias, lo, hi, background,
                                  image, depth, face_id, clip, (hipStream_t)stream);
}

// what mp_picture_points and mp_picture_paint refuse alike, in the header's order; the caller holds the lock
static int picture_sizes_checked(mp_ctx *ctx, const char *who, int n_frames, int64_t n_pixels, int64_t capacity) {
  int rc = check_count(ctx, who, "frame", n_frames, kMaxFrames, MP_ERR_ARG);
  if (rc != MP_OK) return rc;
  if (n_pixels < 1 || capacity < 1)
    return fail(ctx, MP_ERR_ARG, "%s: n_pixels and capacity must be >= 1, got %lld and %lld", who, (long long)n_pixels,
                (long long)capacity);
  if (n_pixels > 0x7fffffffLL / 3)
    return fail(ctx, MP_ERR_UNSUPPORTED, "%s: pictures beyond 2^31 / 3 pixels need 64-bit indices", who);
  return MP_OK;
}

static int picture_points_checked(mp_ctx *ctx, const char *who, int n_frames, const int32_t *const *face_id,
                                  const float *const *position, int64_t n_pixels, int64_t capacity,
                                  float *const *points, int32_t *const *pixels, int32_t *const *count,
                                  mp_stream stream) {
  if (!ctx) return MP_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  int rc = picture_sizes_checked(ctx, who, n_frames, n_pixels, capacity);
  if (rc != MP_OK) return rc;
  if (!face_id || !position || !points || !pixels || !count) return bad_argument(ctx, who);
  rc = check_frames(ctx, who, n_frames, nullptr, face_id, position, points, pixels, count);
  if (rc != MP_OK) return rc;
  DeviceGuard g(ctx->device);
  void *scratch = nullptr;
  rc = ensure_scratch(ctx, (hipStream_t)stream, picture_points_scratch_bytes(n_frames, n_pixels), &scratch);
  if (rc != MP_OK) return rc;
  return launch_picture_points_batch(ctx, scratch, n_frames, face_id, position, n_pixels, capacity, points, pixels,
                                     count, (hipStream_t)stream);
}

static int picture_paint_checked(mp_ctx *ctx, const char *who, int n_frames, const float *const *values,
                                 const int32_t *const *pixels, const int32_t *const *count, int64_t capacity,
                                 int64_t n_pixels, float scale, float bias, float lo, float hi, float *const *image,
                                 mp_stream stream) {
  if (!ctx) return MP_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  int rc = picture_sizes_checked(ctx, who, n_frames, n_pixels, capacity);
  if (rc != MP_OK) return rc;
  if (!values || !pixels || !count || !image) return bad_argument(ctx, who);
  rc = check_frames(ctx, who, n_frames, nullptr, values, pixels, count, image);
  if (rc != MP_OK) return rc;
  DeviceGuard g(ctx->device);
  return launch_picture_paint_batch(ctx, n_frames, values, pixels, count, capacity, n_pixels, scale, bias, lo, hi, image,
                                    (hipStream_t)stream);
}

// what the texture calls refuse alike: the caller holds the lock
static int texture_sizes_checked(mp_ctx *ctx, const char *who, int ht, int wt, int levels) {
  if (ht < 1 || ht > 8192 || wt < 1 || wt > 8192)
    return fail(ctx, MP_ERR_ARG, "%s: texture size %d x %d outside 1..8192", who, ht, wt);
  if (!texture_sizes_ok(ht, wt, levels))
    return fail(ctx, MP_ERR_ARG, "%s: levels must be in 1..14 and no more than reach 1 x 1 from %d x %d, got %d", who,
                ht, wt, levels);
  return MP_OK;
}

static int texture_mips_checked(mp_ctx *ctx, const char *who, const float *tex, int ht, int wt, int levels,
                                float *pyramid, mp_stream stream) {
  if (!ctx) return MP_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  int rc = texture_sizes_checked(ctx, who, ht, wt, levels);
  if (rc != MP_OK) return rc;
  if (!tex || !pyramid) return bad_argument(ctx, who);
  if (((uintptr_t)tex | (uintptr_t)pyramid) & 3) return fail(ctx, MP_ERR_ARG, "%s: misaligned buffer", who);
  if (ranges_overlap(tex, (size_t)ht * wt * 12, pyramid, (size_t)texture_pyramid_floats(ht, wt, levels) * 4))
    return fail(ctx, MP_ERR_ARG, "%s: the pyramid aliases the texture", who);
  DeviceGuard g(ctx->device);
  return launch_texture_mips(ctx, tex, ht, wt, levels, pyramid, (hipStream_t)stream);
}

static int picture_texture_checked(mp_ctx *ctx, const char *who, int n_frames, const float *const *uv,
                                   const int32_t *const *face_id, int n_views, int h, int w, const float *pyramid,
                                   int ht, int wt, int levels, int wrap, float scale, float bias, float lo, float hi,
                                   float background, float *const *image, mp_stream stream) {
  if (!ctx) return MP_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  int rc = check_count(ctx, who, "frame", n_frames, kMaxFrames, MP_ERR_ARG);
  if (rc != MP_OK) return rc;
  if (n_views < 1 || h < 1 || h > 4096 || w < 1 || w > 4096)
    return fail(ctx, MP_ERR_ARG, "%s: n_views >= 1 and an image size in 1..4096, got %d views of %d x %d", who, n_views,
                h, w);
  const long long n_pixels = (long long)n_views * h * w;
  if (n_pixels > 0x7fffffffLL / 3)
    return fail(ctx, MP_ERR_UNSUPPORTED, "%s: pictures beyond 2^31 / 3 pixels need 64-bit indices", who);
  rc = texture_sizes_checked(ctx, who, ht, wt, levels);
  if (rc != MP_OK) return rc;
  if (wrap != MP_WRAP_REPEAT && wrap != MP_WRAP_CLAMP)
    return fail(ctx, MP_ERR_ARG, "%s: wrap must be MP_WRAP_REPEAT / _CLAMP, got %d", who, wrap);
  if (!uv || !face_id || !image || !pyramid) return bad_argument(ctx, who);
  if ((uintptr_t)pyramid & 3) return fail(ctx, MP_ERR_ARG, "%s: misaligned pyramid", who);
  rc = check_frames(ctx, who, n_frames, nullptr, uv, face_id, image);
  if (rc != MP_OK) return rc;
  // a pixel reads its neighbours' uv: the image may not be the UV picture, nor share a byte with any input
  const size_t bytes = (size_t)n_pixels * 12;
  const FrameSpans ins[2] = {{uv, bytes}, {face_id, (size_t)n_pixels * 4}};
  const FrameSpans outs[1] = {{image, bytes}};
  rc = check_no_alias(ctx, who, n_frames, outs, ins);
  if (rc != MP_OK) return rc;
  for (int f = 0; f < n_frames; ++f)
    if (ranges_overlap(image[f], bytes, pyramid, (size_t)texture_pyramid_floats(ht, wt, levels) * 4))
      return fail(ctx, MP_ERR_ARG, "%s: the image of frame %d aliases the pyramid", who, f);
  DeviceGuard g(ctx->device);
  return launch_picture_texture_batch(ctx, n_frames, uv, face_id, n_pixels, h, w, pyramid, ht, wt, levels, wrap, scale,
                                      bias, lo, hi, background, image, (hipStream_t)stream);
}

static int picture_composite_checked(mp_ctx *ctx, const char *who, int n_frames, const float *const *front_image,
                                     const float *const *front_depth, const int32_t *const *front_face,
                                     const float *const *back_image, const float *const *back_depth,
                                     const int32_t *const *back_face, int64_t n_pixels, int mode, int nearest,
                                     float background, float *const *image, float *const *depth, uint8_t *const *mask,
                                     mp_stream stream) {
  if (!ctx) return MP_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  int rc = check_count(ctx, who, "frame", n_frames, kMaxFrames, MP_ERR_ARG);
  if (rc != MP_OK) return rc;
  if (n_pixels < 1) return fail(ctx, MP_ERR_ARG, "%s: n_pixels must be >= 1, got %lld", who, (long long)n_pixels);
  if (n_pixels > 0x7fffffffLL / 3)
    return fail(ctx, MP_ERR_UNSUPPORTED, "%s: pictures beyond 2^31 / 3 pixels need 64-bit indices", who);
  if (mode != MP_COMPOSITE_OVER && mode != MP_COMPOSITE_DEPTH)
    return fail(ctx, MP_ERR_ARG, "%s: mode must be MP_COMPOSITE_OVER / _DEPTH, got %d", who, mode);
  if (nearest != MP_NEAREST_MAX_Z && nearest != MP_NEAREST_MIN_Z)
    return fail(ctx, MP_ERR_ARG, "%s: nearest must be MP_NEAREST_MAX_Z / _MIN_Z, got %d", who, nearest);
  if (!front_image || !front_depth || !front_face || !back_image || !back_depth || !back_face || !image)
    return bad_argument(ctx, who);
  rc = check_frames(ctx, who, n_frames, nullptr, front_image, front_depth, front_face, back_image, back_depth,
                    back_face, image, depth);
  if (rc != MP_OK) return rc;
  if (mask)  // bytes: no alignment asked
    for (int f = 0; f < n_frames; ++f)
      if (!mask[f]) return fail(ctx, MP_ERR_ARG, "%s: null buffer for frame %d", who, f);
  // an output may BE an input of its own kind and frame (a thread reads its pixel before it writes it); any other
  // shared byte is refused
  const size_t px = (size_t)n_pixels;
  const FrameSpans ins[6] = {{front_image, px * 12}, {back_image, px * 12}, {front_depth, px * 4},
                             {back_depth, px * 4},   {front_face, px * 4},  {back_face, px * 4}};
  const FrameSpans outs[3] = {{image, px * 12}, {depth, px * 4}, {mask, px}};
  for (int f = 0; f < n_frames; ++f)
    for (int i = 0; i < n_frames; ++i)
      for (int o = 0; o < 3; ++o)
        for (int k = 0; k < 6; ++k) {
          if (!ranges_overlap(outs[o].of(f), outs[o].bytes, ins[k].of(i), ins[k].bytes)) continue;
          const bool same_kind = (o == 0 && k < 2) || (o == 1 && (k == 2 || k == 3));
          if (!(same_kind && f == i && outs[o].of(f) == ins[k].of(i)))
            return fail(ctx, MP_ERR_ARG, "%s: an output of frame %d aliases an input of frame %d", who, f, i);
        }
  DeviceGuard g(ctx->device);
  return launch_picture_composite_batch(ctx, n_frames, front_image, front_depth, front_face, back_image, back_depth,
                                        back_face, n_pixels, mode, nearest, background, image, depth, mask,
                                        (hipStream_t)stream);
}

static int picture_resolve_checked(mp_ctx *ctx, const char *who, int n_frames, int n_views, const float *const *image,
                                   const float *const *depth, const int32_t *const *face_id,
                                   const uint8_t *const *mask, int h, int w, int samples, int nearest,
                                   float *const *image_out, float *const *depth_out, int32_t *const *face_out,
                                   uint8_t *const *mask_out, float *const *coverage, mp_stream stream) {
  if (!ctx) return MP_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (samples < 2 || samples > 4) return fail(ctx, MP_ERR_ARG, "%s: samples must be in 2..4, got %d", who, samples);
  if (n_frames < 1 || n_views < 1 || (long long)n_frames * n_views > kMaxFrames)
    return fail(ctx, MP_ERR_ARG, "%s: 1..%d pictures (frames x views) per call, got %d x %d", who, kMaxFrames, n_frames,
                n_views);
  if (h < 1 || w < 1 || (long long)samples * h > 4096 || (long long)samples * w > 4096)
    return fail(ctx, MP_ERR_ARG, "%s: h, w >= 1 and samples * h, samples * w in 1..4096, got %d x %d at %d samples", who,
                h, w, samples);
  if (nearest != MP_NEAREST_MAX_Z && nearest != MP_NEAREST_MIN_Z)
    return fail(ctx, MP_ERR_ARG, "%s: nearest must be MP_NEAREST_MAX_Z / _MIN_Z, got %d", who, nearest);
  if (!image_out && !depth_out && !face_out && !mask_out && !coverage)
    return fail(ctx, MP_ERR_ARG, "%s: no output is asked for", who);
  if (image_out && !image) return fail(ctx, MP_ERR_ARG, "%s: image_out needs image", who);
  if ((depth_out || face_out) && !(depth && face_id))
    return fail(ctx, MP_ERR_ARG, "%s: depth_out and face_out need depth and face_id", who);
  if (mask_out && !mask) return fail(ctx, MP_ERR_ARG, "%s: mask_out needs mask", who);
  if (coverage && !mask && !face_id) return fail(ctx, MP_ERR_ARG, "%s: coverage needs mask or face_id", who);
  int rc = check_frames(ctx, who, n_frames, nullptr, image, depth, face_id, image_out, depth_out, face_out, coverage);
  if (rc != MP_OK) return rc;
  for (int f = 0; f < n_frames; ++f)  // bytes: no alignment asked
    if ((mask && !mask[f]) || (mask_out && !mask_out[f]))
      return fail(ctx, MP_ERR_ARG, "%s: null buffer for frame %d", who, f);
  const size_t coarse = (size_t)n_views * h * w, fine = coarse * samples * samples;
  const FrameSpans ins[4] = {{image, fine * 12}, {depth, fine * 4}, {face_id, fine * 4}, {mask, fine}};
  const FrameSpans outs[5] = {
      {image_out, coarse * 12}, {depth_out, coarse * 4}, {face_out, coarse * 4}, {mask_out, coarse}, {coverage, coarse * 4}};
  rc = check_no_alias(ctx, who, n_frames, outs, ins);
  if (rc != MP_OK) return rc;
  DeviceGuard g(ctx->device);
  return launch_picture_resolve_batch(ctx, n_frames, n_views, image, depth, face_id, mask, h, w, samples, nearest,
                                      image_out, depth_out, face_out, mask_out, coverage, (hipStream_t)stream);
}

static int picture_shadow_checked(mp_ctx *ctx, const char *who, int n_frames, const float *const *image_in,
                                  const float *const *position, const int32_t *const *face_id, int64_t n_pixels,
                                  const float *const *map_depth, const int32_t *const *map_face, int hs, int ws,
                                  const float *light_calibs, int projection, int nearest, float bias, int radius,
                                  float strength, float *const *image_out, float *const *shade, mp_stream stream) {
  if (!ctx) return MP_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  int rc = check_count(ctx, who, "frame", n_frames, kMaxFrames, MP_ERR_ARG);
  if (rc != MP_OK) return rc;
  if (n_pixels < 1) return fail(ctx, MP_ERR_ARG, "%s: n_pixels must be >= 1, got %lld", who, (long long)n_pixels);
  if (n_pixels > 0x7fffffffLL / 3)
    return fail(ctx, MP_ERR_UNSUPPORTED, "%s: pictures beyond 2^31 / 3 pixels need 64-bit indices", who);
  if (hs < 1 || hs > 4096 || ws < 1 || ws > 4096)
    return fail(ctx, MP_ERR_ARG, "%s: shadow map size %d x %d outside 1..4096", who, hs, ws);
  if (projection != MP_PROJ_ORTHOGONAL && projection != MP_PROJ_PERSPECTIVE)
    return fail(ctx, MP_ERR_ARG, "%s: unknown projection mode %d", who, projection);
  if (nearest != MP_NEAREST_MAX_Z && nearest != MP_NEAREST_MIN_Z)
    return fail(ctx, MP_ERR_ARG, "%s: nearest must be MP_NEAREST_MAX_Z / _MIN_Z, got %d", who, nearest);
  if (!std::isfinite(bias) || !(bias >= 0.0f))
    return fail(ctx, MP_ERR_ARG, "%s: bias must be finite and >= 0, got %g", who, (double)bias);
  if (radius < 0 || radius > 3) return fail(ctx, MP_ERR_ARG, "%s: radius must be in 0..3, got %d", who, radius);
  if (!(strength >= 0.0f && strength <= 1.0f))
    return fail(ctx, MP_ERR_ARG, "%s: strength must be in [0, 1], got %g", who, (double)strength);
  if (!image_out && !shade) return fail(ctx, MP_ERR_ARG, "%s: no output requested", who);
  if (!image_in != !image_out)
    return fail(ctx, MP_ERR_ARG, "%s: image_in and image_out go together (both, or neither)", who);
  if (!position || !face_id || !map_depth || !map_face || !light_calibs) return bad_argument(ctx, who);
  rc = check_frames(ctx, who, n_frames, nullptr, image_in, position, face_id, map_depth, map_face, image_out, shade);
  if (rc != MP_OK) return rc;
  // image_out may BE image_in of the same frame (a thread reads its pixel before it writes it); any other byte shared
  // between an output and an input is refused
  const size_t px = (size_t)n_pixels, texels = (size_t)hs * ws;
  const FrameSpans ins[5] = {{image_in, px * 12}, {position, px * 12}, {face_id, px * 4},
                             {map_depth, texels * 4}, {map_face, texels * 4}};
  const FrameSpans outs[2] = {{image_out, px * 12}, {shade, px * 4}};
  for (int f = 0; f < n_frames; ++f)
    for (int i = 0; i < n_frames; ++i)
      for (int o = 0; o < 2; ++o)
        for (int k = 0; k < 5; ++k) {
          if (!ranges_overlap(outs[o].of(f), outs[o].bytes, ins[k].of(i), ins[k].bytes)) continue;
          if (!(o == 0 && k == 0 && f == i && outs[o].of(f) == ins[k].of(i)))
            return fail(ctx, MP_ERR_ARG, "%s: an output of frame %d aliases an input of frame %d", who, f, i);
        }
  DeviceGuard g(ctx->device);
  return launch_picture_shadow_batch(ctx, n_frames, image_in, position, face_id, n_pixels, map_depth, map_face, hs, ws,
                                     light_calibs, projection, nearest, bias, radius, strength, image_out, shade,
                                     (hipStream_t)stream);
}

static bool all_finite(const float *v, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (!std::isfinite(v[i])) return false;
  return true;
}

static int picture_light_checked(mp_ctx *ctx, const char *who, int n_frames, const float *const *normal,
                                 const int32_t *const *face_id, const float *const *albedo, const float *albedo_rgb,
                                 const float *const *visibility, const float *const *ambient, bool transfer,
                                 int64_t n_pixels, int n_views, const float *sh, const float *direct_dir,
                                 const float *direct_rgb, float gamma, const float *normal_mats, float background,
                                 float *const *image_out, float *const *shading, mp_stream stream) {
  if (!ctx) return MP_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  int rc = check_count(ctx, who, "frame", n_frames, kMaxFrames, MP_ERR_ARG);
  if (rc != MP_OK) return rc;
  if (n_pixels < 1) return fail(ctx, MP_ERR_ARG, "%s: n_pixels must be >= 1, got %lld", who, (long long)n_pixels);
  if (n_pixels > 0x7fffffffLL / 3)
    return fail(ctx, MP_ERR_UNSUPPORTED, "%s: pictures beyond 2^31 / 3 pixels need 64-bit indices", who);
  if (n_views < 1 || n_pixels % n_views != 0)
    return fail(ctx, MP_ERR_ARG, "%s: n_views must be >= 1 and divide n_pixels = %lld, got %d", who,
                (long long)n_pixels, n_views);
  if (normal_mats && (long long)n_frames * n_views > kLightMaxMats)
    return fail(ctx, MP_ERR_ARG, "%s: at most %d normal matrices (frames x views) per call, got %d x %d", who,
                kLightMaxMats, n_frames, n_views);
  // mp_picture_light_transfer: ambient stands in for sh; the normals are read by the direct term only
  if (!direct_dir || !direct_rgb || !face_id || (transfer ? !ambient : !sh || !normal)) return bad_argument(ctx, who);
  if (!albedo == !albedo_rgb)
    return fail(ctx, MP_ERR_ARG, "%s: either albedo buffers or a constant albedo_rgb, not %s", who,
                albedo ? "both" : "neither");
  if (!std::isfinite(gamma) || !(gamma > 0.0f))
    return fail(ctx, MP_ERR_ARG, "%s: gamma must be finite and > 0, got %g", who, (double)gamma);
  if ((sh && !all_finite(sh, 27)) || !all_finite(direct_dir, 3) || !all_finite(direct_rgb, 3) ||
      (albedo_rgb && !all_finite(albedo_rgb, 3)) || !std::isfinite(background) ||
      (normal_mats && !all_finite(normal_mats, (size_t)9 * n_frames * n_views)))
    return fail(ctx, MP_ERR_ARG, "%s: sh, direct_dir, direct_rgb, albedo_rgb, background and normal_mats must be finite",
                who);
  if (!image_out && !shading) return fail(ctx, MP_ERR_ARG, "%s: no output requested", who);
  if (transfer && !normal && (direct_rgb[0] != 0.0f || direct_rgb[1] != 0.0f || direct_rgb[2] != 0.0f))
    return fail(ctx, MP_ERR_ARG, "%s: the direct term needs the normal pictures", who);
  rc = check_frames(ctx, who, n_frames, nullptr, normal, face_id, albedo, visibility, ambient, image_out, shading);
  if (rc != MP_OK) return rc;
  // image_out may BE albedo of the same frame (a thread reads its pixel before it writes it); any other byte shared
  // between an output and an input, or between the two outputs, is refused
  const size_t px = (size_t)n_pixels;
  const FrameSpans ins[5] = {{albedo, px * 12}, {normal, px * 12}, {face_id, px * 4}, {visibility, px * 4},
                             {ambient, px * 12}};
  const FrameSpans outs[2] = {{image_out, px * 12}, {shading, px * 12}};
  for (int f = 0; f < n_frames; ++f)
    for (int i = 0; i < n_frames; ++i) {
      for (int o = 0; o < 2; ++o)
        for (int k = 0; k < 5; ++k) {
          if (!ranges_overlap(outs[o].of(f), outs[o].bytes, ins[k].of(i), ins[k].bytes)) continue;
          if (!(o == 0 && k == 0 && f == i && outs[o].of(f) == ins[k].of(i)))
            return fail(ctx, MP_ERR_ARG, "%s: an output of frame %d aliases an input of frame %d", who, f, i);
        }
      if (ranges_overlap(outs[0].of(f), px * 12, outs[1].of(i), px * 12) ||
          (f != i && (ranges_overlap(outs[0].of(f), px * 12, outs[0].of(i), px * 12) ||
                      ranges_overlap(outs[1].of(f), px * 12, outs[1].of(i), px * 12))))
        return fail(ctx, MP_ERR_ARG, "%s: an output of frame %d aliases an output of frame %d", who, f, i);
    }
  DeviceGuard g(ctx->device);
  return launch_picture_light_batch(ctx, n_frames, normal, face_id, albedo, albedo_rgb, visibility, ambient, n_pixels,
                                    n_views, sh, direct_dir, direct_rgb, gamma, normal_mats, background, image_out,
                                    shading, (hipStream_t)stream);
}

static int volume_bits_checked(mp_ctx *ctx, const char *who, int n_frames, const float *const *volume, int r,
                               float level, uint32_t *const *bits, const int32_t *const *gate, mp_stream stream) {
  if (!ctx) return MP_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  int rc = check_count(ctx, who, "frame", n_frames, kMaxFrames, MP_ERR_ARG);
  if (rc != MP_OK) return rc;
  if (!volume || !bits) return bad_argument(ctx, who);
  if (r < 1 || r > MP_TRANSFER_MAX_RES)
    return fail(ctx, MP_ERR_ARG, "%s: resolution must be 1..%d, got %d", who, MP_TRANSFER_MAX_RES, r);
  rc = check_frames(ctx, who, n_frames, gate, volume, bits);
  if (rc != MP_OK) return rc;
  const FrameSpans outs[1] = {{bits, (size_t)volume_bits_words(r) * 4}};
  const FrameSpans ins[1] = {{volume, (size_t)r * r * r * 4}};
  rc = check_no_alias(ctx, who, n_frames, outs, ins);
  if (rc != MP_OK) return rc;
  for (int f = 0; f < n_frames; ++f)
    for (int i = 0; i < f; ++i)
      if (ranges_overlap(outs[0].of(f), outs[0].bytes, outs[0].of(i), outs[0].bytes))
        return fail(ctx, MP_ERR_ARG, "%s: an output of frame %d aliases an output of frame %d", who, f, i);
  DeviceGuard g(ctx->device);
  return launch_volume_bits_batch(ctx, n_frames, volume, r, level, bits, gate, (hipStream_t)stream);
}

static int mesh_transfer_checked(mp_ctx *ctx, const char *who, int n_frames, const float *const *verts,
                                 const float *const *normals, int64_t max_verts, const int32_t *const *counts,
                                 const uint32_t *const *bits, int r, const float *b_min, const float *b_max, int n_dirs,
                                 const float *dirs, const float *basis, float weight, float bias_w, float step_w,
                                 int max_steps, uint64_t *const *mask, float *const *prt, mp_stream stream) {
  if (!ctx) return MP_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  int rc = check_count(ctx, who, "frame", n_frames, kMaxFrames, MP_ERR_ARG);
  if (rc != MP_OK) return rc;
  if (!counts || !bits || !b_min || !b_max || !dirs || !basis || max_verts < 0 || (max_verts > 0 && (!verts || !normals)))
    return bad_argument(ctx, who);
  if (r < 1 || r > MP_TRANSFER_MAX_RES)
    return fail(ctx, MP_ERR_ARG, "%s: resolution must be 1..%d, got %d", who, MP_TRANSFER_MAX_RES, r);
  if (n_dirs < 64 || n_dirs > MP_TRANSFER_MAX_DIRS || n_dirs % 64 != 0)
    return fail(ctx, MP_ERR_ARG, "%s: n_dirs must be a multiple of 64 in 64..%d, got %d", who, MP_TRANSFER_MAX_DIRS,
                n_dirs);
  if (max_steps < 1 || max_steps > (1 << 24))
    return fail(ctx, MP_ERR_ARG, "%s: max_steps must be 1..2^24, got %d", who, max_steps);
  if (!all_finite(b_min, 3) || !all_finite(b_max, 3) || !(b_max[0] > b_min[0]) || !(b_max[1] > b_min[1]) ||
      !(b_max[2] > b_min[2]))
    return fail(ctx, MP_ERR_ARG, "%s: b_min and b_max must be finite with b_max > b_min on every axis", who);
  if (!std::isfinite(weight) || !std::isfinite(bias_w) || !std::isfinite(step_w) || !(step_w > 0.0f))
    return fail(ctx, MP_ERR_ARG, "%s: weight, bias_w and step_w must be finite and step_w > 0", who);
  if (!mask && !prt) return fail(ctx, MP_ERR_ARG, "%s: no output requested", who);
  if (max_verts > 0x7fffffffLL / 9)
    return fail(ctx, MP_ERR_UNSUPPORTED, "%s: capacities beyond 2^31 / 9 are not supported", who);
  if (((uintptr_t)dirs | (uintptr_t)basis) & 3) return fail(ctx, MP_ERR_ARG, "%s: misaligned table", who);
  if (max_verts == 0) verts = nullptr, normals = nullptr;
  rc = check_frames(ctx, who, n_frames, nullptr, counts, bits, verts, normals, max_verts ? prt : nullptr);
  if (rc != MP_OK) return rc;
  if (mask && max_verts)
    for (int f = 0; f < n_frames; ++f)
      if (!mask[f] || ((uintptr_t)mask[f] & 7))
        return fail(ctx, MP_ERR_ARG, "%s: null or misaligned mask for frame %d", who, f);
  if (max_verts == 0) return MP_OK;
  const size_t nv = (size_t)max_verts;
  const FrameSpans outs[2] = {{mask, nv * (size_t)(n_dirs / 64) * 8}, {prt, nv * 36}};
  const FrameSpans ins[4] = {{verts, nv * 12}, {normals, nv * 12}, {counts, 4}, {bits, (size_t)volume_bits_words(r) * 4}};
  rc = check_no_alias(ctx, who, n_frames, outs, ins);
  if (rc != MP_OK) return rc;
  for (int f = 0; f < n_frames; ++f)
    for (int i = 0; i < n_frames; ++i)
      if (ranges_overlap(outs[0].of(f), outs[0].bytes, outs[1].of(i), outs[1].bytes) ||
          (f != i && (ranges_overlap(outs[0].of(f), outs[0].bytes, outs[0].of(i), outs[0].bytes) ||
                      ranges_overlap(outs[1].of(f), outs[1].bytes, outs[1].of(i), outs[1].bytes))))
        return fail(ctx, MP_ERR_ARG, "%s: an output of frame %d aliases an output of frame %d", who, f, i);
  // the per-call device tables are inputs of every frame
  for (int f = 0; f < n_frames; ++f)
    for (const FrameSpans &o : outs)
      if (ranges_overlap(o.of(f), o.bytes, dirs, (size_t)n_dirs * 12) ||
          ranges_overlap(o.of(f), o.bytes, basis, (size_t)n_dirs * 36))
        return fail(ctx, MP_ERR_ARG, "%s: an output of frame %d aliases dirs or basis", who, f);
  TransferRays rays;
  for (int a = 0; a < 3; ++a) rays.bmin[a] = b_min[a], rays.bmax[a] = b_max[a];
  rays.r = r;
  rays.n_dirs = n_dirs;
  rays.max_steps = max_steps;
  rays.dirs = dirs;
  rays.basis = basis;
  rays.weight = weight;
  rays.bias_w = bias_w;
  rays.step_w = step_w;
  DeviceGuard g(ctx->device);
  return launch_mesh_transfer_batch(ctx, n_frames, verts, normals, max_verts, counts, bits, rays, mask, prt,
                                    (hipStream_t)stream);
}

static int transfer_shade_checked(mp_ctx *ctx, const char *who, int n_frames, const float *const *prt,
                                  int64_t max_verts, const int32_t *const *counts, const float *sh, float *const *out,
                                  mp_stream stream) {
  if (!ctx) return MP_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  int rc = check_count(ctx, who, "frame", n_frames, kMaxFrames, MP_ERR_ARG);
  if (rc != MP_OK) return rc;
  if (!counts || !sh || max_verts < 0 || (max_verts > 0 && (!prt || !out))) return bad_argument(ctx, who);
  if (!all_finite(sh, 27)) return fail(ctx, MP_ERR_ARG, "%s: sh must be finite", who);
  if (max_verts > 0x7fffffffLL / 9)
    return fail(ctx, MP_ERR_UNSUPPORTED, "%s: capacities beyond 2^31 / 9 are not supported", who);
  if (max_verts == 0) prt = nullptr, out = nullptr;
  rc = check_frames(ctx, who, n_frames, nullptr, counts, prt, out);
  if (rc != MP_OK) return rc;
  if (max_verts == 0) return MP_OK;
  const FrameSpans outs[1] = {{out, (size_t)max_verts * 12}};
  const FrameSpans ins[2] = {{prt, (size_t)max_verts * 36}, {counts, 4}};
  rc = check_no_alias(ctx, who, n_frames, outs, ins);
  if (rc != MP_OK) return rc;
  for (int f = 0; f < n_frames; ++f)
    for (int i = 0; i < f; ++i)
      if (ranges_overlap(outs[0].of(f), outs[0].bytes, outs[0].of(i), outs[0].bytes))
        return fail(ctx, MP_ERR_ARG, "%s: an output of frame %d aliases an output of frame %d", who, f, i);
  DeviceGuard g(ctx->device);
  return launch_mesh_transfer_shade_batch(ctx, n_frames, prt, max_verts, counts, sh, out, (hipStream_t)stream);
}

static int keep_largest_checked(mp_ctx *ctx, const char *who, int n_frames, const float *const *volume, int r,
                                float level, int connectivity, float fill, float *const *out, int32_t *const *stats,
                                const int32_t *const *gate, mp_stream stream) {
  if (!ctx) return MP_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  int rc = check_count(ctx, who, "frame", n_frames, kMaxFrames, MP_ERR_ARG);
  if (rc != MP_OK) return rc;
  if (!volume || !out || !stats || r < 1) return bad_argument(ctx, who);
  if (connectivity != MP_CONN_6 && connectivity != MP_CONN_26)
    return fail(ctx, MP_ERR_ARG, "%s: connectivity must be 6 or 26, got %d", who, connectivity);
  if (!(fill <= level))  // a NaN fill fails this test too
    return fail(ctx, MP_ERR_ARG, "%s: fill %g would be foreground at level %g", who, (double)fill, (double)level);
  rc = check_frames(ctx, who, n_frames, gate, volume, out, stats);
  if (rc != MP_OK) return rc;
  if (r > 1290)  // 1291^3 > 2^31
    return fail(ctx, MP_ERR_UNSUPPORTED, "%s: resolution %d needs 64-bit voxel indices", who, r);
  DeviceGuard g(ctx->device);
  void *scratch = nullptr;
  rc = ensure_scratch(ctx, (hipStream_t)stream, (size_t)n_frames * cc_scratch_bytes(r), &scratch);
  if (rc != MP_OK) return rc;
  return launch_keep_largest_batch(ctx, scratch, n_frames, volume, r, level, connectivity, fill, out, stats, gate,
                                   (hipStream_t)stream);
}

}  // namespace mp

using namespace mp;

extern "C" {

int mp_version(void) { return 100; }

int mp_create(int device, mp_ctx **out) {
  if (!out) return fail(nullptr, MP_ERR_ARG, "mp_create: out is NULL");
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
    return fail(nullptr, MP_ERR_HIP, "mp_create: no HIP device visible (there is no CPU fallback)");
  if (device < 0 || device >= count)
    return fail(nullptr, MP_ERR_ARG, "mp_create: device %d out of range (%d visible)", device, count);
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess)
    return fail(nullptr, MP_ERR_HIP, "mp_create: hipGetDeviceProperties failed");
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(nullptr, MP_ERR_UNSUPPORTED, "mp_create: kernels are built for gfx950 only, device is %s",
                prop.gcnArchName);
  mp_ctx *ctx = new mp_ctx();
  ctx->device = device;
  ctx->n_cu = prop.multiProcessorCount;
  *out = ctx;
  return MP_OK;
}

void mp_destroy(mp_ctx *ctx) {
  if (!ctx) return;
  {
    DeviceGuard g(ctx->device);
    for (auto &m : ctx->mlps) {
      if (m.buf) (void)hipFree(m.buf);
      if (m.buf16) (void)hipFree(m.buf16);
      if (m.raw) (void)hipFree(m.raw);
    }
    for (hipEvent_t e : ctx->prof_events) (void)hipEventDestroy(e);
    for (auto &kv : ctx->arenas) {
      if (kv.second.ptr) (void)hipFree(kv.second.ptr);
      for (void *p : kv.second.retired) (void)hipFree(p);
    }
  }
  delete ctx;
}

const char *mp_last_error(mp_ctx *ctx) {
  (void)ctx;
  return g_last_error.c_str();
}

int mp_stream_release(mp_ctx *ctx, mp_stream stream) {
  if (!ctx) return MP_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  auto it = ctx->arenas.find((void *)stream);
  if (it == ctx->arenas.end()) return MP_OK;
  DeviceGuard g(ctx->device);
  // the stream may already be destroyed (that is when this is called): drain the device instead
  MP_HIP(ctx, hipDeviceSynchronize());
  // free every block and forget the arena even if one hipFree fails (mp_destroy must not free twice)
  hipError_t first = hipSuccess;
  if (it->second.ptr) first = hipFree(it->second.ptr);
  for (void *p : it->second.retired) {
    const hipError_t e = hipFree(p);
    if (first == hipSuccess) first = e;
  }
  ctx->arenas.erase(it);
  MP_HIP(ctx, first);
  return MP_OK;
}

int mp_memory_stats(mp_ctx *ctx, int64_t *out4) {
  if (!ctx || !out4) return MP_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  int64_t arena = 0, weights = 0;
  for (const auto &kv : ctx->arenas) arena += (int64_t)(kv.second.bytes + kv.second.retired_bytes);
  for (const Mlp &m : ctx->mlps) {
    if (!m.used) continue;
    if (m.buf) weights += (int64_t)m.total * 4;
    if (m.raw) weights += (int64_t)(m.off_raw[3] + (size_t)kHidden[3] * (kHidden[2] + m.c + 1)) * 4;
    if (m.buf16) weights += (int64_t)m.total16 * 16;
  }
  out4[0] = arena;
  out4[1] = weights;
  out4[2] = (int64_t)ctx->arenas.size();
  out4[3] = (int64_t)ctx->skip_tables.size();
  return MP_OK;
}

// Test hook: the arena pointer never leaves the library, so this is how a test makes a stage start on residue.
int mp_scratch_fill(mp_ctx *ctx, int64_t bytes, int value, int64_t *block_bytes, mp_stream stream) {
  if (!ctx) return MP_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (bytes < 0 || value < 0 || value > 255)
    return fail(ctx, MP_ERR_ARG, "mp_scratch_fill: %lld bytes of value %d (bytes >= 0, value 0..255)",
                (long long)bytes, value);
  DeviceGuard g(ctx->device);
  void *scratch = nullptr;
  const int rc = ensure_scratch(ctx, (hipStream_t)stream, (size_t)bytes, &scratch);
  if (rc != MP_OK) return rc;
  const size_t block = ctx->arenas[(void *)stream].bytes;  // the whole current block; retired blocks stay as they are
  if (block) MP_HIP(ctx, hipMemsetAsync(scratch, value, block, (hipStream_t)stream));
  if (block_bytes) *block_bytes = (int64_t)block;
  return MP_OK;
}

int mp_max_frames(void) { return kMaxFrames; }

int mp_mlp_create(mp_ctx *ctx, int n_layers, const int *channels, int last_op, int *mlp_out) {
  if (!ctx) return MP_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (!channels || !mlp_out) return fail(ctx, MP_ERR_ARG, "mp_mlp_create: NULL argument");
  if (last_op < MP_ACT_NONE || last_op > MP_ACT_TANH)
    return fail(ctx, MP_ERR_ARG, "mp_mlp_create: bad last_op %d", last_op);
  if (n_layers != 5)
    return fail(ctx, MP_ERR_UNSUPPORTED, "mp_mlp_create: only the 5-layer PIFu heads are built (got %d)",
                n_layers);
  const int c = channels[0] - 1, cout = channels[5];
  bool ok = (c == 256 || c == 512) && (cout == 1 || cout == 3);
  for (int l = 0; l < 4; ++l) ok = ok && channels[l + 1] == kHidden[l];
  if (!ok)
    return fail(ctx, MP_ERR_UNSUPPORTED,
                "mp_mlp_create: channels must be {C+1,1024,512,256,128,Cout}, C in {256,512}, Cout in {1,3}");
  DeviceGuard g(ctx->device);
  Mlp m;
  m.used = true;
  m.c = c;
  m.cout = cout;
  m.act = last_op;
  size_t off = 0;
  auto take = [&](size_t n) {
    size_t o = off;
    off += (n + 63) & ~size_t(63);
    return o;
  };
  for (int l = 0; l < 4; ++l) {
    const size_t n_out = kHidden[l], k_h = l == 0 ? 0 : kHidden[l - 1];
    m.off_ah[l] = take(n_out * k_h);
    m.off_ax[l] = take(n_out * c);
    m.off_az[l] = take(n_out * 2);
    m.off_bias[l] = take(n_out);
  }
  m.off_w4 = take((size_t)cout * ((kHidden[3] + c + 1 + 3) & ~3));
  m.off_bias[4] = take(cout);
  m.total = off;
  if (hipMalloc(reinterpret_cast<void **>(&m.buf), off * sizeof(float)) != hipSuccess)
    return fail(ctx, MP_ERR_NOMEM, "mp_mlp_create: hipMalloc of %zu floats failed", off);
  // raw copies (source for re-packing into other operand formats)
  size_t roff = 0;
  for (int l = 0; l < 4; ++l) {
    m.off_raw[l] = roff;
    roff += (size_t)kHidden[l] * ((l == 0 ? 0 : kHidden[l - 1]) + c + 1);
  }
  if (hipMalloc(reinterpret_cast<void **>(&m.raw), roff * sizeof(float)) != hipSuccess) {
    (void)hipFree(m.buf);
    return fail(ctx, MP_ERR_NOMEM, "mp_mlp_create: hipMalloc of %zu floats failed", roff);
  }
  int id = -1;
  for (size_t i = 0; i < ctx->mlps.size(); ++i)
    if (!ctx->mlps[i].used) id = (int)i;
  if (id < 0) {
    ctx->mlps.push_back(m);
    id = (int)ctx->mlps.size() - 1;
  } else {
    ctx->mlps[id] = m;
  }
  *mlp_out = id;
  return MP_OK;
}

int mp_mlp_load(mp_ctx *ctx, int mlp, int layer, const float *W, const float *b, int out_ch,
                int in_ch, mp_stream stream) {
  if (!ctx) return MP_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  Mlp *m = get_mlp(ctx, mlp);
  if (!m) return fail(ctx, MP_ERR_ARG, "mp_mlp_load: unknown mlp id %d", mlp);
  if (!W || !b || layer < 0 || layer > 4) return fail(ctx, MP_ERR_ARG, "mp_mlp_load: bad argument");
  const int want_out = layer < 4 ? kHidden[layer] : m->cout;
  const int want_in = (layer == 0 ? 0 : kHidden[layer - 1]) + m->c + 1;
  if (out_ch != want_out || in_ch != want_in)
    return fail(ctx, MP_ERR_ARG, "mp_mlp_load: layer %d expects weight [%d,%d], got [%d,%d]", layer,
                want_out, want_in, out_ch, in_ch);
  DeviceGuard g(ctx->device);
  // skip tables hold products of THESE weights (layer 0 + the skip segments): a table made before
  // the reload would blend the old head into the new one's hidden layers -- forget them
  for (auto it = ctx->skip_tables.begin(); it != ctx->skip_tables.end();)
    it = it->second.mlp_buf == m->buf ? ctx->skip_tables.erase(it) : std::next(it);
  int rc = launch_pack_layer(ctx, *m, layer, W, b, (hipStream_t)stream);
  if (rc == MP_OK && layer < 4)
    rc = launch_copy(ctx, W, m->raw + m->off_raw[layer], (long long)out_ch * in_ch,
                     (hipStream_t)stream);
  if (rc == MP_OK) {
    m->loaded[layer] = true;
    m->load_stream = (hipStream_t)stream;  // mp_mlp_set_precision orders itself behind it
  }
  if (rc == MP_OK && m->precision != MP_PREC_F32) {
    // weights changed under an f16-packed MLP: drop back to f32 until precision is selected again
    m->precision = MP_PREC_F32;
  }
  return rc;
}

int mp_mlp_set_precision(mp_ctx *ctx, int mlp, int precision) {
  if (!ctx) return MP_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  Mlp *m = get_mlp(ctx, mlp);
  if (!m) return fail(ctx, MP_ERR_ARG, "mp_mlp_set_precision: unknown mlp id %d", mlp);
  if (precision < MP_PREC_F32 || precision > MP_PREC_F16)
    return fail(ctx, MP_ERR_ARG, "mp_mlp_set_precision: bad precision %d", precision);
  if (precision == MP_PREC_F32) {
    m->precision = MP_PREC_F32;
    return MP_OK;
  }
  int rc = check_ready(ctx, m, m->c);
  if (rc != MP_OK) return rc;
  if (m->c != 256)
    return fail(ctx, MP_ERR_UNSUPPORTED, "mp_mlp_set_precision: the f16 kernels are built for C = 256 heads only");
  DeviceGuard g(ctx->device);
  if (!m->buf16) {
    size_t off = 0;  // units of 16 bytes (8 halves)
    for (int l = 0; l < 4; ++l) {
      const size_t n_rb = kHidden[l] / 32, k_h = l == 0 ? 0 : kHidden[l - 1];
      m->off16_ah[l] = off;
      off += n_rb * (k_h / 16) * 128;
      m->off16_ax[l] = off;
      off += n_rb * (m->c / 16) * 128;
      m->off16_az[l] = off;
      off += n_rb * 128;
    }
    if (hipMalloc(&m->buf16, off * 16) != hipSuccess)
      return fail(ctx, MP_ERR_NOMEM, "mp_mlp_set_precision: hipMalloc(%zu) failed", off * 16);
    m->total16 = off;
  }
  // The raw weight copies were written by mp_mlp_load on the caller's stream; torch's side
  // streams do not synchronise with the NULL stream, so the re-pack runs on that same stream
  // (ordered behind the loads) and is drained before returning.
  const hipStream_t st = m->load_stream;
  unsigned int *d_bits = nullptr;
  MP_HIP(ctx, hipMalloc(reinterpret_cast<void **>(&d_bits), sizeof(unsigned int)));
  for (int l = 0; l < 4 && rc == MP_OK; ++l) {
    const long long n = (long long)kHidden[l] * ((l == 0 ? 0 : kHidden[l - 1]) + m->c + 1);
    rc = launch_absmax(ctx, m->raw + m->off_raw[l], n, d_bits, st);
    unsigned int bits = 0;
    if (rc == MP_OK &&
        (hipMemcpyAsync(&bits, d_bits, sizeof(bits), hipMemcpyDeviceToHost, st) != hipSuccess ||
         hipStreamSynchronize(st) != hipSuccess))
      rc = fail(ctx, MP_ERR_HIP, "mp_mlp_set_precision: reading max|W| back failed");
    float wmax;
    memcpy(&wmax, &bits, sizeof(wmax));
    // largest power of two S with max|w| * S <= 2^14 (f16 tops out at 65504), clamped
    int e = 0;
    if (wmax > 0.0f && wmax < 3.0e38f) {
      (void)frexpf(wmax, &e);  // wmax = f * 2^e, f in [0.5, 1)
      e = 14 - e;
    }
    if (e > 14) e = 14;
    if (e < -14) e = -14;
    m->scale16[l] = ldexpf(1.0f, e);
    if (rc == MP_OK) rc = launch_pack_layer16(ctx, *m, l, m->raw + m->off_raw[l], st);
  }
  // drained: the packed f16 weights are complete before any stream can launch a query on them
  if (hipStreamSynchronize(st) != hipSuccess && rc == MP_OK)
    rc = fail(ctx, MP_ERR_HIP, "mp_mlp_set_precision: hipStreamSynchronize failed");
  (void)hipFree(d_bits);
  if (rc == MP_OK) m->precision = precision;
  return rc;
}

int mp_mlp_destroy(mp_ctx *ctx, int mlp) {
  if (!ctx) return MP_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  Mlp *m = get_mlp(ctx, mlp);
  if (!m) return fail(ctx, MP_ERR_ARG, "mp_mlp_destroy: unknown mlp id %d", mlp);
  DeviceGuard g(ctx->device);
  MP_HIP(ctx, hipDeviceSynchronize());
  // skip tables made with this head die with it (a later head may get the same buffer address)
  for (auto it = ctx->skip_tables.begin(); it != ctx->skip_tables.end();)
    it = it->second.mlp_buf == m->buf ? ctx->skip_tables.erase(it) : std::next(it);
  if (m->buf) MP_HIP(ctx, hipFree(m->buf));
  if (m->buf16) MP_HIP(ctx, hipFree(m->buf16));
  if (m->raw) MP_HIP(ctx, hipFree(m->raw));
  *m = Mlp();
  return MP_OK;
}

int mp_feat_pack_hwc(mp_ctx *ctx, const float *src_chw, int c_src, int h, int w, float *dst_hwc,
                     int c_dst, int c_offset, mp_stream stream) {
  if (!ctx) return MP_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (!src_chw || !dst_hwc || c_src <= 0 || h <= 0 || w <= 0 || c_offset < 0 ||
      c_offset + c_src > c_dst)
    return fail(ctx, MP_ERR_ARG, "mp_feat_pack_hwc: bad argument");
  DeviceGuard g(ctx->device);
  return launch_pack_hwc(ctx, src_chw, c_src, h, w, dst_hwc, c_dst, c_offset, (hipStream_t)stream);
}

static_assert(MP_SKIP_TABLE_ROWS == mp::kTableRows, "header and kernels disagree on the table row length");

int mp_skip_table(mp_ctx *ctx, int mlp, const float *feat_hwc, int c, int h, int w, float *table,
                mp_stream stream) {
  if (!ctx) return MP_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  const Mlp *m = get_mlp(ctx, mlp);
  int rc = check_ready(ctx, m, c);
  if (rc != MP_OK) return rc;
  if (!feat_hwc || !table || h <= 0 || w <= 0) return fail(ctx, MP_ERR_ARG, "mp_skip_table: bad argument");
  if (!aligned16(feat_hwc) || !aligned16(table))
    return fail(ctx, MP_ERR_ARG, "mp_skip_table: feat_hwc and table must be 16-byte aligned");
  DeviceGuard g(ctx->device);
  rc = launch_skip_table(ctx, *m, feat_hwc, h, w, table, (hipStream_t)stream);
  if (rc != MP_OK) return rc;
  ctx->skip_tables[feat_hwc] = mp_ctx::SkipTable{table, m->buf, h, w};
  return MP_OK;
}

int mp_skip_table_batch(mp_ctx *ctx, int mlp, int n_maps, const float *feat_hwc, int c, int h, int w,
                      float *table, mp_stream stream) {
  if (!ctx) return MP_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  const Mlp *m = get_mlp(ctx, mlp);
  int rc = check_ready(ctx, m, c);
  if (rc != MP_OK) return rc;
  if (!feat_hwc || !table || h <= 0 || w <= 0 || n_maps <= 0 || (long long)n_maps * h > (1 << 20))
    return fail(ctx, MP_ERR_ARG, "mp_skip_table_batch: bad argument");
  if (!aligned16(feat_hwc) || !aligned16(table))
    return fail(ctx, MP_ERR_ARG, "mp_skip_table_batch: feat_hwc and table must be 16-byte aligned");
  DeviceGuard g(ctx->device);
  // the maps are contiguous: one launch over n_maps * H rows of texels
  rc = launch_skip_table(ctx, *m, feat_hwc, n_maps * h, w, table, (hipStream_t)stream);
  if (rc != MP_OK) return rc;
  for (int i = 0; i < n_maps; ++i)
    ctx->skip_tables[feat_hwc + (size_t)i * h * w * c] =
        mp_ctx::SkipTable{table + (size_t)i * h * w * kTableRows, m->buf, h, w};
  return MP_OK;
}

int mp_skip_table_release(mp_ctx *ctx, const float *feat_hwc, const float *table) {
  if (!ctx) return MP_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (!feat_hwc) {
    ctx->skip_tables.clear();
    return MP_OK;
  }
  auto it = ctx->skip_tables.find(feat_hwc);
  if (it != ctx->skip_tables.end() && (!table || it->second.table == table)) ctx->skip_tables.erase(it);
  return MP_OK;
}

int mp_index(mp_ctx *ctx, const float *feat_hwc, int c, int h, int w, const float *uv, int64_t n,
             float *out, mp_stream stream) {
  if (!ctx) return MP_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (!feat_hwc || (n > 0 && (!uv || !out)) || n < 0 || h <= 0 || w <= 0)
    return fail(ctx, MP_ERR_ARG, "mp_index: bad argument");
  if (!aligned16(feat_hwc)) return fail(ctx, MP_ERR_ARG, "mp_index: feat_hwc must be 16-byte aligned");
  DeviceGuard g(ctx->device);
  return launch_index(ctx, feat_hwc, c, h, w, uv, n, out, (hipStream_t)stream);
}

int mp_orthogonal(mp_ctx *ctx, const float *points, int64_t n, const float *calib, float *out,
                  mp_stream stream) {
  if (!ctx) return MP_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (n < 0 || !calib || (n > 0 && (!points || !out)))
    return fail(ctx, MP_ERR_ARG, "mp_orthogonal: bad argument");
  DeviceGuard g(ctx->device);
  return launch_orthogonal(ctx, points, n, calib, out, (hipStream_t)stream);
}

int mp_perspective(mp_ctx *ctx, const float *points, int64_t n, const float *calib, float *out,
                   mp_stream stream) {
  if (!ctx) return MP_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (n < 0 || !calib || (n > 0 && (!points || !out)))
    return fail(ctx, MP_ERR_ARG, "mp_perspective: bad argument");
  DeviceGuard g(ctx->device);
  return launch_perspective(ctx, points, n, calib, out, (hipStream_t)stream);
}

int mp_query(mp_ctx *ctx, int mlp, const float *feat_hwc, int c, int h, int w, const float *points,
             int64_t n, int64_t stride_n, int64_t stride_c, const float *calib, float z_scale,
             float *out, mp_stream stream) {
  HeadCall call(ctx, mlp, c);
  if (call.rc != MP_OK) return call.rc;
  if (!feat_hwc || !calib || n < 0 || h <= 0 || w <= 0 || (n > 0 && (!points || !out)))
    return bad_argument(ctx, "mp_query");
  const int rc = check_maps(ctx, "mp_query", "frame", 1, &feat_hwc);
  if (rc != MP_OK || n == 0) return rc;
  DeviceGuard g(ctx->device);
  return launch_query(ctx, *call.m, feat_hwc, h, w, calib, z_scale, strided_points(points, n, stride_n, stride_c), out,
                      n, (hipStream_t)stream);
}

int mp_query_batch(mp_ctx *ctx, int mlp, int n_frames, const float *const *feat_hwc, int c, int h, int w,
                   const float *const *points, int64_t n, int64_t stride_n, int64_t stride_c,
                   const float *const *calib, const int *projection, float z_scale, float *const *out,
                   mp_stream stream) {
  const char *who = "mp_query_batch";
  HeadCall call(ctx, mlp, c);
  if (call.rc != MP_OK) return call.rc;
  int rc = check_count(ctx, who, "frame", n_frames, kMaxFrames, MP_ERR_ARG);
  if (rc != MP_OK) return rc;
  if (!feat_hwc || !points || !calib || !projection || !out || n < 0 || h <= 0 || w <= 0)
    return bad_argument(ctx, who);
  rc = check_projection(ctx, who, projection, n_frames);
  if (rc == MP_OK)
    rc = check_maps(ctx, who, "frame", n_frames, feat_hwc, calib, n > 0 ? points : nullptr, n > 0 ? out : nullptr);
  if (rc != MP_OK || n == 0) return rc;
  DeviceGuard g(ctx->device);
  return launch_query_set(ctx, *call.m,
                          query_set(n_frames, feat_hwc, calib, projection, points, nullptr, out,
                                    strided_points(nullptr, n, stride_n, stride_c)),
                          h, w, z_scale, n * n_frames, false, (hipStream_t)stream);
}

int mp_mlp_forward(mp_ctx *ctx, int mlp, const float *feature, int64_t n, float *out,
                   mp_stream stream) {
  HeadCall call(ctx, mlp, 0, "mp_mlp_forward");
  if (call.rc != MP_OK) return call.rc;
  if (n < 0 || (n > 0 && (!feature || !out))) return bad_argument(ctx, "mp_mlp_forward");
  if (n == 0) return MP_OK;
  DeviceGuard g(ctx->device);
  return launch_query(ctx, *call.m, /*feat_hwc=*/nullptr, 0, 0, /*calib=*/nullptr, 0.0f,
                      strided_points(feature, n, 1, n), out, n, (hipStream_t)stream);
}

int mp_query_views(mp_ctx *ctx, int mlp, int n_views, const float *const *feat_hwc, int c, int h, int w,
                   const float *const *points, int64_t n, int64_t stride_n, int64_t stride_c,
                   const float *const *calib, int projection, float z_scale, float *const *out,
                   mp_stream stream) {
  const char *who = "mp_query_views";
  HeadCall call(ctx, mlp, c);
  if (call.rc != MP_OK) return call.rc;
  int rc = check_count(ctx, who, "view", n_views, kMaxViews, MP_ERR_UNSUPPORTED);
  if (rc == MP_OK) rc = check_f32_views(ctx, who, call.m);
  if (rc != MP_OK) return rc;
  if (!feat_hwc || !points || !calib || !out || n < 0 || h <= 0 || w <= 0) return bad_argument(ctx, who);
  rc = check_projection(ctx, who, &projection, 1);
  if (rc == MP_OK)
    rc = check_maps(ctx, who, "view", n_views, feat_hwc, calib, n > 0 ? points : nullptr, n > 0 ? out : nullptr);
  if (rc != MP_OK || n == 0) return rc;
  ViewSetDev set = view_set(n_views, projection, n, stride_n, stride_c);
  for (int v = 0; v < n_views; ++v) {
    set.feat[v] = feat_hwc[v];
    set.calib[v] = calib[v];
    set.pts[v] = points[v];
    set.out[v] = out[v];
  }
  DeviceGuard g(ctx->device);
  return launch_query_views(ctx, *call.m, set, h, w, z_scale, (hipStream_t)stream);
}

int mp_mlp_forward_views(mp_ctx *ctx, int mlp, int n_views, const float *feature, int64_t n, float *out,
                         mp_stream stream) {
  const char *who = "mp_mlp_forward_views";
  HeadCall call(ctx, mlp, 0, who);
  if (call.rc != MP_OK) return call.rc;
  int rc = check_count(ctx, who, "view", n_views, kMaxViews, MP_ERR_UNSUPPORTED);
  if (rc == MP_OK) rc = check_f32_views(ctx, who, call.m);
  if (rc != MP_OK) return rc;
  if (n < 0 || (n > 0 && (!feature || !out))) return bad_argument(ctx, who);
  if (n == 0) return MP_OK;
  ViewSetDev set = view_set(n_views, /*projection=*/0, n, 1, n);
  for (int v = 0; v < n_views; ++v) set.pts[v] = feature + (long long)v * (call.m->c + 1) * n;
  set.out[0] = out;
  DeviceGuard g(ctx->device);
  return launch_query_views(ctx, *call.m, set, 0, 0, 0.0f, (hipStream_t)stream);
}

int mp_query_counted(mp_ctx *ctx, int mlp, const float *feat_hwc, int c, int h, int w,
                     const float *points, int64_t capacity, const int32_t *count,
                     const float *calib, float z_scale, float *out, mp_stream stream) {
  HeadCall call(ctx, mlp, c);
  if (call.rc != MP_OK) return call.rc;
  if (!feat_hwc || !calib || !count || capacity < 0 || h <= 0 || w <= 0 || (capacity > 0 && (!points || !out)))
    return bad_argument(ctx, "mp_query_counted");
  const int rc = check_maps(ctx, "mp_query_counted", "frame", 1, &feat_hwc);
  if (rc != MP_OK || capacity == 0) return rc;
  DeviceGuard g(ctx->device);
  return launch_query(ctx, *call.m, feat_hwc, h, w, calib, z_scale, counted_points(points, capacity, count), out,
                      capacity, (hipStream_t)stream);
}

int mp_query_counted_batch(mp_ctx *ctx, int mlp, int n_frames, const float *const *feat_hwc, int c,
                           int h, int w, const float *const *points, int64_t capacity,
                           const int32_t *const *count, const float *const *calib, float z_scale,
                           float *const *out, mp_stream stream) {
  return mp_query_counted_batch_proj(ctx, mlp, n_frames, feat_hwc, c, h, w, points, capacity, count, calib,
                                     nullptr, z_scale, out, stream);
}

int mp_query_counted_batch_proj(mp_ctx *ctx, int mlp, int n_frames, const float *const *feat_hwc, int c,
                                int h, int w, const float *const *points, int64_t capacity,
                                const int32_t *const *count, const float *const *calib,
                                const int *projection, float z_scale, float *const *out, mp_stream stream) {
  const char *who = "mp_query_counted_batch";  // the name both entry points report under
  HeadCall call(ctx, mlp, c);
  if (call.rc != MP_OK) return call.rc;
  int rc = check_count(ctx, who, "frame", n_frames, kMaxFrames, MP_ERR_ARG);
  if (rc != MP_OK) return rc;
  if (!feat_hwc || !points || !count || !calib || !out || capacity < 0 || h <= 0 || w <= 0)
    return bad_argument(ctx, who);
  rc = check_projection(ctx, who, projection, n_frames);
  if (rc != MP_OK || capacity == 0) return rc;  // an empty call returns before its frames' buffers are looked at
  rc = check_maps(ctx, who, "frame", n_frames, feat_hwc, points, count, calib, out);
  if (rc != MP_OK) return rc;
  DeviceGuard g(ctx->device);
  return launch_query_set(ctx, *call.m,
                          query_set(n_frames, feat_hwc, calib, projection, points, count, out,
                                    counted_points(nullptr, capacity, nullptr)),
                          h, w, z_scale, capacity * n_frames, true, (hipStream_t)stream);
}

int mp_recon_batch(mp_ctx *ctx, int mlp, int n_frames, const float *const *feat_hwc, int c, int h,
                   int w, const float *const *calib, float z_scale, const float *b_min,
                   const float *b_max, const int *resolutions, int n_levels, float balance,
                   float *const *volume, int32_t *const *status, mp_stream stream) {
  return mp_recon_batch_ex(ctx, mlp, n_frames, feat_hwc, c, h, w, calib, z_scale, b_min, b_max, resolutions,
                           n_levels, balance, MP_FINAL_DILATE3, volume, status, stream);
}

int mp_recon_batch_ex(mp_ctx *ctx, int mlp, int n_frames, const float *const *feat_hwc, int c, int h,
                      int w, const float *const *calib, float z_scale, const float *b_min,
                      const float *b_max, const int *resolutions, int n_levels, float balance,
                      int final_level, float *const *volume, int32_t *const *status, mp_stream stream) {
  return mp_recon_batch_early(ctx, mlp, n_frames, feat_hwc, c, h, w, calib, z_scale, b_min, b_max, resolutions,
                              n_levels, balance, final_level, volume, status, nullptr, stream);
}

int mp_recon_batch_early(mp_ctx *ctx, int mlp, int n_frames, const float *const *feat_hwc, int c, int h,
                         int w, const float *const *calib, float z_scale, const float *b_min,
                         const float *b_max, const int *resolutions, int n_levels, float balance,
                         int final_level, float *const *volume, int32_t *const *status,
                         const mp_recon_early *early, mp_stream stream) {
  return mp_recon_batch_proj(ctx, mlp, n_frames, feat_hwc, c, h, w, calib, nullptr, z_scale, b_min, b_max,
                             resolutions, n_levels, balance, final_level, volume, status, early, stream);
}

// mp_recon, mp_recon_batch, _ex and _early end here: all five report under this one's name
int mp_recon_batch_proj(mp_ctx *ctx, int mlp, int n_frames, const float *const *feat_hwc, int c, int h,
                        int w, const float *const *calib, const int *projection, float z_scale,
                        const float *b_min, const float *b_max, const int *resolutions, int n_levels,
                        float balance, int final_level, float *const *volume, int32_t *const *status,
                        const mp_recon_early *early, mp_stream stream) {
  const char *who = "mp_recon_batch_proj";
  HeadCall call(ctx, mlp, c);
  if (call.rc != MP_OK) return call.rc;
  int rc = check_count(ctx, who, "frame", n_frames, kMaxFrames, MP_ERR_ARG);
  if (rc != MP_OK) return rc;
  if (!feat_hwc || !calib || !b_min || !b_max || !resolutions || !volume || !status || n_levels < 1 ||
      n_levels > 8 || h <= 0 || w <= 0)
    return bad_argument(ctx, who);
  rc = check_maps(ctx, who, "frame", n_frames, feat_hwc, calib, volume, status);
  if (rc != MP_OK) return rc;
  if (call.m->cout != 1) return fail(ctx, MP_ERR_ARG, "%s: needs a 1-channel (occupancy) mlp", who);
  return recon_checked(ctx, who, *call.m, n_frames, feat_hwc, h, w, calib, projection, z_scale, b_min, b_max,
                       resolutions, n_levels, MP_ERR_UNSUPPORTED, balance, final_level, volume, status, early,
                       "flags_dev", stream, nullptr);
}

int mp_recon_topk_batch(mp_ctx *ctx, int mlp, int n_frames, const float *const *feat_hwc, int c, int h, int w,
                        const float *const *calib, const int *projection, float z_scale, const float *b_min,
                        const float *b_max, const int *resolutions, int n_levels, const int64_t *num_points,
                        const float *max_dist, float balance, float *const *volume, int32_t *const *status,
                        const mp_recon_early *early, mp_stream stream) {
  const char *who = "mp_recon_topk_batch";
  HeadCall call(ctx, mlp, c);
  if (call.rc != MP_OK) return call.rc;
  int rc = check_count(ctx, who, "frame", n_frames, kMaxFrames, MP_ERR_ARG);
  if (rc != MP_OK) return rc;
  if (!feat_hwc || !calib || !b_min || !b_max || !resolutions || !num_points || !volume || !status || n_levels < 1 ||
      n_levels > 8 || h <= 0 || w <= 0)
    return bad_argument(ctx, who);
  rc = check_maps(ctx, who, "frame", n_frames, feat_hwc, calib, volume, status);
  if (rc != MP_OK) return rc;
  if (call.m->cout != 1) return fail(ctx, MP_ERR_ARG, "%s: needs a 1-channel (occupancy) mlp", who);
  long long k[8];
  for (int l = 0; l < n_levels; ++l) k[l] = num_points[l];
  return recon_checked(ctx, who, *call.m, n_frames, feat_hwc, h, w, calib, projection, z_scale, b_min, b_max,
                       resolutions, n_levels, MP_ERR_ARG, balance, MP_FINAL_DILATE3, volume, status, early, "flags_dev",
                       stream, nullptr, k, max_dist);
}

// mp_recon_views (batch == 0: one frame, today's one-frame lattice kernel) and mp_recon_views_batch (batch != 0:
// n_frames frames on the batched one) refuse the same, in the same order, and end in the same driver call
static int recon_views_checked(mp_ctx *ctx, const char *who, int mlp, int n_frames, int n_views, int batch,
                               const float *const *feat_hwc, int c, int h, int w, const float *const *calib,
                               int projection, float z_scale, const float *b_min, const float *b_max,
                               const int *resolutions, int n_levels, float balance, int final_level, int view,
                               float *const *volume, int32_t *const *status, const mp_recon_early *early,
                               mp_stream stream) {
  HeadCall call(ctx, mlp, c);
  if (call.rc != MP_OK) return call.rc;
  const Mlp *m = call.m;
  int rc = check_count(ctx, who, "view", n_views, kMaxViews, MP_ERR_UNSUPPORTED);
  if (rc == MP_OK) rc = check_f32_views(ctx, who, m);
  if (rc != MP_OK) return rc;
  if (m->c != 256 || m->cout != 1)
    return fail(ctx, MP_ERR_UNSUPPORTED, "%s: needs a netG head (C=256, 1 occupancy channel); got C=%d Cout=%d", who,
                m->c, m->cout);
  if (view < 0 || view >= n_views)
    return fail(ctx, MP_ERR_ARG, "%s: view %d outside 0..%d", who, view, n_views - 1);
  if (batch) {
    rc = check_count(ctx, who, "frame", n_frames, kMaxFrames, MP_ERR_ARG);
    if (rc != MP_OK) return rc;
    if (n_frames * n_views > kMaxFrameViews)
      return fail(ctx, MP_ERR_ARG, "%s: at most %d frames x views per call, got %d x %d", who, kMaxFrameViews, n_frames,
                  n_views);
  }
  if (!feat_hwc || !calib || !b_min || !b_max || !resolutions || !volume || !status || n_levels < 1 ||
      n_levels > 8 || h <= 0 || w <= 0)
    return bad_argument(ctx, who);
  rc = check_maps(ctx, who, "view", n_frames * n_views, feat_hwc, calib);
  if (rc != MP_OK) return rc;
  for (int f = 0; f < n_frames; ++f)
    if (!volume[f] || !status[f]) return fail(ctx, MP_ERR_ARG, "%s: null buffer for frame %d", who, f);
  const ReconViews views = {n_views, view, batch};
  return recon_checked(ctx, who, *m, n_frames, feat_hwc, h, w, calib, &projection, z_scale, b_min, b_max, resolutions,
                       n_levels, MP_ERR_ARG, balance, final_level, volume, status, early, "early->flags_dev", stream,
                       &views);
}

int mp_recon_views(mp_ctx *ctx, int mlp, int n_views, const float *const *feat_hwc, int c, int h, int w,
                   const float *const *calib, int projection, float z_scale,
                   const float *b_min, const float *b_max, const int *resolutions, int n_levels,
                   float balance, int final_level, int view, float *volume, int32_t *status,
                   const mp_recon_early *early, mp_stream stream) {
  // a null volume / status stays this entry's "bad argument"
  return recon_views_checked(ctx, "mp_recon_views", mlp, 1, n_views, 0, feat_hwc, c, h, w, calib, projection, z_scale,
                             b_min, b_max, resolutions, n_levels, balance, final_level, view,
                             volume ? &volume : nullptr, status ? &status : nullptr, early, stream);
}

int mp_max_frame_views(void) { return kMaxFrameViews; }

int mp_recon_views_batch(mp_ctx *ctx, int mlp, int n_frames, int n_views, const float *const *feat_hwc, int c, int h,
                         int w, const float *const *calib, int projection, float z_scale, const float *b_min,
                         const float *b_max, const int *resolutions, int n_levels, float balance, int final_level,
                         int view, float *const *volume, int32_t *const *status, const mp_recon_early *early,
                         mp_stream stream) {
  return recon_views_checked(ctx, "mp_recon_views_batch", mlp, n_frames, n_views, 1, feat_hwc, c, h, w, calib,
                             projection, z_scale, b_min, b_max, resolutions, n_levels, balance, final_level, view,
                             volume, status, early, stream);
}

int mp_query_views_counted_batch(mp_ctx *ctx, int mlp, int n_frames, int n_views, const float *const *feat_hwc, int c,
                                 int h, int w, const float *const *points, int64_t capacity,
                                 const int32_t *const *count, const float *const *calib, int projection,
                                 float z_scale, int view, float *const *out, mp_stream stream) {
  const char *who = "mp_query_views_counted_batch";
  HeadCall call(ctx, mlp, c);
  if (call.rc != MP_OK) return call.rc;
  const Mlp *m = call.m;
  int rc = check_count(ctx, who, "view", n_views, kMaxViews, MP_ERR_UNSUPPORTED);
  if (rc == MP_OK) rc = check_f32_views(ctx, who, m);
  if (rc != MP_OK) return rc;
  if ((m->c != 256 && m->c != 512) || (m->cout != 1 && m->cout != 3))
    return fail(ctx, MP_ERR_UNSUPPORTED,
                "%s: multi-view query kernels are built for C in {256,512}, Cout in {1,3}; got C=%d Cout=%d", who,
                m->c, m->cout);
  rc = check_count(ctx, who, "frame", n_frames, kMaxFrames, MP_ERR_ARG);
  if (rc != MP_OK) return rc;
  if (n_frames * n_views > kMaxFrameViews)
    return fail(ctx, MP_ERR_ARG, "%s: at most %d frames x views per call, got %d x %d", who, kMaxFrameViews, n_frames,
                n_views);
  if (view < 0 || view >= n_views)
    return fail(ctx, MP_ERR_ARG, "%s: view %d outside 0..%d", who, view, n_views - 1);
  if (!feat_hwc || !points || !count || !calib || !out || capacity < 0 || h <= 0 || w <= 0)
    return bad_argument(ctx, who);
  rc = check_projection(ctx, who, &projection, 1);
  if (rc != MP_OK || capacity == 0) return rc;  // an empty call returns before its frames' buffers are looked at
  rc = check_maps(ctx, who, "view", n_frames * n_views, feat_hwc, calib);
  if (rc == MP_OK) rc = check_frames(ctx, who, n_frames, count, points, out);
  if (rc != MP_OK) return rc;
  for (int f = 0; f < n_frames; ++f)
    if (!count[f]) return fail(ctx, MP_ERR_ARG, "%s: null buffer for frame %d", who, f);
  for (int i = 0; i < n_frames * n_views; ++i)
    if ((uintptr_t)calib[i] & 3) return fail(ctx, MP_ERR_ARG, "%s: misaligned buffer for view %d", who, i);
  ViewPointsBatchDev set = {};
  set.nv = n_views;
  set.proj = projection;
  set.view = view;
  set.n = n_frames;
  set.capacity = capacity;
  for (int f = 0; f < n_frames; ++f) {
    set.it[f].pts = points[f];
    set.it[f].out = out[f];
    set.it[f].n_dev = count[f];
  }
  for (int i = 0; i < n_frames * n_views; ++i) {
    set.feat[i] = feat_hwc[i];
    set.calib[i] = calib[i];
  }
  DeviceGuard g(ctx->device);
  return launch_query_views_counted_batch(ctx, *m, set, h, w, z_scale, (hipStream_t)stream);
}

int mp_recon(mp_ctx *ctx, int mlp, const float *feat_hwc, int c, int h, int w, const float *calib,
             float z_scale, const float *b_min, const float *b_max, const int *resolutions,
             int n_levels, float balance, float *volume, int32_t *status, mp_stream stream) {
  return mp_recon_batch(ctx, mlp, 1, &feat_hwc, c, h, w, &calib, z_scale, b_min, b_max, resolutions,
                        n_levels, balance, &volume, &status, stream);
}

static int octree_select_impl(mp_ctx *ctx, const float *prev, int rp, float *cur, int r,
                              const uint64_t *ev_prev, uint64_t *ev_cur, uint64_t *bnd, int level,
                              int box, float balance, uint32_t *packed, int32_t *count,
                              mp_stream stream) {
  if (!ctx) return MP_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (!ev_cur || !packed || !count || r < 2 || r > 1023 || level < 0)
    return fail(ctx, MP_ERR_ARG, "mp_octree_select: bad argument");
  if (prev && (!cur || !ev_prev || !bnd || r != 2 * rp - 1 || level < 1))
    return fail(ctx, MP_ERR_ARG, "mp_octree_select: refinement needs cur, ev_prev, bnd and r == 2 rp - 1");
  if (box != 0 && box != 1 && box != 3 && box != 7 && box != 9)
    return fail(ctx, MP_ERR_UNSUPPORTED, "mp_octree_select_box: dilation box must be 0, 1, 3, 7 or 9, got %d", box);
  DeviceGuard g(ctx->device);
  return launch_octree_select(ctx, prev, rp, cur, r,
                              reinterpret_cast<const unsigned long long *>(ev_prev),
                              reinterpret_cast<unsigned long long *>(ev_cur),
                              reinterpret_cast<unsigned long long *>(bnd), box, balance, packed,
                              count, (hipStream_t)stream);
}

int mp_octree_select(mp_ctx *ctx, const float *prev, int rp, float *cur, int r,
                     const uint64_t *ev_prev, uint64_t *ev_cur, uint64_t *bnd, int level,
                     float balance, uint32_t *packed, int32_t *count, mp_stream stream) {
  return octree_select_impl(ctx, prev, rp, cur, r, ev_prev, ev_cur, bnd, level,
                            octree_box_of_level(level), balance, packed, count, stream);
}

int mp_octree_select_box(mp_ctx *ctx, const float *prev, int rp, float *cur, int r,
                         const uint64_t *ev_prev, uint64_t *ev_cur, uint64_t *bnd, int box,
                         float balance, uint32_t *packed, int32_t *count, mp_stream stream) {
  return octree_select_impl(ctx, prev, rp, cur, r, ev_prev, ev_cur, bnd, prev ? 1 : 0, box, balance,
                            packed, count, stream);
}

int mp_octree_select_topk(mp_ctx *ctx, const float *prev, int rp, float *cur, int r, const uint64_t *ev_prev,
                          uint64_t *ev_cur, int64_t k, float max_dist, float balance, uint32_t *packed, int32_t *count,
                          mp_stream stream) {
  const char *who = "mp_octree_select_topk";
  if (!ctx) return MP_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (!prev || !cur || !ev_prev || !ev_cur || !packed || !count) return bad_argument(ctx, who);
  if (rp < 2 || r > 1023 || r != 2 * rp - 1) return fail(ctx, MP_ERR_ARG, "%s: needs r == 2 rp - 1 <= 1023", who);
  if ((reinterpret_cast<uintptr_t>(prev) | reinterpret_cast<uintptr_t>(cur) | reinterpret_cast<uintptr_t>(packed) |
       reinterpret_cast<uintptr_t>(count)) & 3u)
    return fail(ctx, MP_ERR_ARG, "%s: prev, cur, packed and count must be 4-byte aligned", who);
  if ((reinterpret_cast<uintptr_t>(ev_prev) | reinterpret_cast<uintptr_t>(ev_cur)) & 7u)
    return fail(ctx, MP_ERR_ARG, "%s: ev_prev and ev_cur must be 8-byte aligned", who);
  int rc = check_topk(ctx, who, r, k, max_dist);
  if (rc != MP_OK) return rc;
  DeviceGuard g(ctx->device);
  const size_t bnd_bytes = ((size_t)r * r * ((r + 63) / 64) * sizeof(uint64_t) + 255) & ~size_t(255);
  void *scratch = nullptr;
  rc = ensure_scratch(ctx, (hipStream_t)stream, bnd_bytes + topk_scratch_bytes(1, r), &scratch);
  if (rc != MP_OK) return rc;
  return launch_octree_select_topk(ctx, scratch, static_cast<unsigned char *>(scratch) + bnd_bytes, prev, rp, cur, r,
                                   reinterpret_cast<const unsigned long long *>(ev_prev),
                                   reinterpret_cast<unsigned long long *>(ev_cur), k, max_dist, balance, packed, count,
                                   (hipStream_t)stream);
}

int mp_octree_conflicts(mp_ctx *ctx, const uint32_t *packed, const int32_t *count, int64_t capacity,
                        int r, const float *values, const float *volume, float balance,
                        uint64_t *ev, uint32_t *out_packed, int32_t *out_count, mp_stream stream) {
  if (!ctx) return MP_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (!packed || !count || capacity < 0 || r < 2 || r > 1023 || !volume || !ev || !out_packed ||
      !out_count || (capacity > 0 && !values))
    return fail(ctx, MP_ERR_ARG, "mp_octree_conflicts: bad argument");
  DeviceGuard g(ctx->device);
  return launch_octree_conflicts(ctx, packed, count, capacity, r, values, volume, balance,
                                 reinterpret_cast<unsigned long long *>(ev), out_packed, out_count,
                                 (hipStream_t)stream);
}

int mp_lattice_points(mp_ctx *ctx, const uint32_t *packed, const int32_t *count, int64_t capacity,
                      int stride, int res_final, const float *b_min, const float *b_max,
                      float *points, mp_stream stream) {
  if (!ctx) return MP_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (!packed || !count || capacity < 0 || stride < 1 || res_final < 2 || !b_min || !b_max ||
      (capacity > 0 && !points))
    return fail(ctx, MP_ERR_ARG, "mp_lattice_points: bad argument");
  DeviceGuard g(ctx->device);
  return launch_lattice_points(ctx, packed, count, capacity, stride, res_final, b_min, b_max,
                               points, (hipStream_t)stream);
}

int mp_octree_order_points(mp_ctx *ctx, int n_frames, uint32_t *const *packed, const int32_t *const *count,
                           const float *const *calib, const int *projection, int level_res, int stride, int res_final,
                           const float *b_min, const float *b_max, int h, int w, mp_stream stream) {
  const char *who = "mp_octree_order_points";
  if (!ctx) return MP_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  int rc = check_count(ctx, who, "frame", n_frames, kMaxFrames, MP_ERR_ARG);
  if (rc != MP_OK) return rc;
  if (!packed || !count || !calib || !b_min || !b_max || level_res < 2 || level_res > 1023 || stride < 1 ||
      res_final < 2 || h < 1 || w < 1 || (long long)h * w >= (1ll << 30))
    return bad_argument(ctx, who);
  for (int f = 0; f < n_frames; ++f)
    if (!packed[f] || !count[f] || !calib[f]) return fail(ctx, MP_ERR_ARG, "%s: frame %d has a NULL buffer", who, f);
  rc = check_projection(ctx, who, projection, n_frames);
  if (rc != MP_OK) return rc;
  DeviceGuard g(ctx->device);
  const long long cap = (long long)level_res * level_res * level_res / 8;
  const size_t per_frame = point_order_scratch_bytes(cap, h, w);
  void *scratch = nullptr;
  rc = ensure_scratch(ctx, (hipStream_t)stream, n_frames * per_frame, &scratch);
  if (rc != MP_OK) return rc;
  OrderFrames of;
  std::memset(&of, 0, sizeof(of));
  for (int f = 0; f < n_frames; ++f) {
    of.packed[f] = packed[f];
    of.count[f] = count[f];
    of.calib[f] = calib[f];
    of.proj[f] = projection ? projection[f] : MP_PROJ_ORTHOGONAL;
    point_order_carve(static_cast<unsigned char *>(scratch) + f * per_frame, cap, of, f);
  }
  PointSrc lattice;
  std::memset(&lattice, 0, sizeof(lattice));
  lattice.stride = stride;
  lattice.level_res = level_res;
  lattice.res_final = (float)res_final;
  lattice.half_step = (1.0f / (float)res_final) / 2.0f;
  for (int i = 0; i < 3; ++i) {
    lattice.bmin[i] = b_min[i];
    lattice.blen[i] = b_max[i] - b_min[i];
  }
  return launch_point_order(ctx, of, n_frames, lattice, h, w, cap, (hipStream_t)stream);
}

int mp_scatter_nodes(mp_ctx *ctx, const uint32_t *packed, const int32_t *count, int64_t capacity,
                     int r, const float *values, float *volume, mp_stream stream) {
  if (!ctx) return MP_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (!packed || !count || capacity < 0 || r < 2 || !volume || (capacity > 0 && !values))
    return fail(ctx, MP_ERR_ARG, "mp_scatter_nodes: bad argument");
  DeviceGuard g(ctx->device);
  return launch_scatter_nodes(ctx, packed, count, capacity, r, values, volume, (hipStream_t)stream);
}

int mp_forward_vertices(mp_ctx *ctx, const float *volume, int r, int direction, int64_t *x,
                        int64_t *y, float *z, float *norm, int32_t *count, mp_stream stream) {
  return forward_vertices_checked(ctx, "mp_forward_vertices", 1, &volume, r, direction, &x, &y, &z, &norm, &count,
                                  stream);
}

int mp_forward_vertices_batch(mp_ctx *ctx, int n_frames, const float *const *volume, int r, int direction,
                              int64_t *const *x, int64_t *const *y, float *const *z, float *const *norm,
                              int32_t *const *count, mp_stream stream) {
  return forward_vertices_checked(ctx, "mp_forward_vertices_batch", n_frames, volume, r, direction, x, y, z, norm,
                                  count, stream);
}

int mp_vertex_points(mp_ctx *ctx, const int64_t *x, const int64_t *y, const float *z,
                     const int32_t *count, int64_t capacity, int res, const float *mat,
                     float *points, mp_stream stream) {
  if (!ctx) return MP_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (!x || !y || !z || !count || !mat || !points || capacity < 0 || res < 1)
    return fail(ctx, MP_ERR_ARG, "mp_vertex_points: bad argument");
  DeviceGuard g(ctx->device);
  return launch_vertex_points(ctx, x, y, z, count, capacity, res, mat, points, (hipStream_t)stream);
}

int mp_paint(mp_ctx *ctx, const int64_t *x, const int64_t *y, const float *values,
             int channel_major, const int32_t *count, int64_t capacity, int res, float scale,
             float bias, float lo, float hi, float *image, mp_stream stream) {
  return paint_checked(ctx, "mp_paint", 1, &x, &y, &values, channel_major, &count, capacity, res, scale, bias, lo, hi,
                       &image, stream);
}

int mp_paint_batch(mp_ctx *ctx, int n_frames, const int64_t *const *x, const int64_t *const *y,
                   const float *const *values, int channel_major, const int32_t *const *count, int64_t capacity,
                   int res, float scale, float bias, float lo, float hi, float *const *image, mp_stream stream) {
  return paint_checked(ctx, "mp_paint_batch", n_frames, x, y, values, channel_major, count, capacity, res, scale,
                       bias, lo, hi, image, stream);
}

int mp_visualize(mp_ctx *ctx, const float *image, int res, int size, float *out, uint8_t *mask,
                 mp_stream stream) {
  if (!ctx) return MP_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (!image || !out || !mask || res < 1 || size < 1 || size > 16384)
    return fail(ctx, MP_ERR_ARG, "mp_visualize: bad argument");
  DeviceGuard g(ctx->device);
  return launch_visualize(ctx, image, res, size, out, mask, (hipStream_t)stream);
}

int mp_prepare_inputs(mp_ctx *ctx, const float *segm, int64_t hw, const float *mean,
                      const float *std, float *input_g, float *input_c, mp_stream stream) {
  if (!ctx) return MP_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (!segm || !mean || !std || !input_g || hw < 0)
    return fail(ctx, MP_ERR_ARG, "mp_prepare_inputs: bad argument");
  if (hw == 0) return MP_OK;
  DeviceGuard g(ctx->device);
  return launch_prepare_inputs(ctx, segm, hw, mean, std, input_g, input_c, (hipStream_t)stream);
}

int mp_marching_cubes(mp_ctx *ctx, const float *volume, int r, float level, const float *b_min,
                      const float *b_max, float *verts, int64_t max_verts, int32_t *faces,
                      int64_t max_faces, int32_t *counts, mp_stream stream) {
  return marching_cubes_checked(ctx, "mp_marching_cubes", 1, &volume, r, level, b_min, b_max, &verts, max_verts,
                                &faces, max_faces, &counts, nullptr, stream);
}

int mp_marching_cubes_batch(mp_ctx *ctx, int n_frames, const float *const *volume, int r, float level,
                            const float *b_min, const float *b_max, float *const *verts, int64_t max_verts,
                            int32_t *const *faces, int64_t max_faces, int32_t *const *counts,
                            const int32_t *const *gate, mp_stream stream) {
  return marching_cubes_checked(ctx, "mp_marching_cubes_batch", n_frames, volume, r, level, b_min, b_max, verts,
                                max_verts, faces, max_faces, counts, gate, stream);
}

int mp_mesh_normals(mp_ctx *ctx, const float *verts, int64_t max_verts, const int32_t *faces, int64_t max_faces,
                    const int32_t *counts, int mode, float *normals, mp_stream stream) {
  return mesh_normals_checked(ctx, "mp_mesh_normals", 1, &verts, max_verts, &faces, max_faces, &counts, mode, &normals,
                              stream);
}

int mp_mesh_render(mp_ctx *ctx, const float *verts, int64_t max_verts, const int32_t *faces, int64_t max_faces,
                   const int32_t *counts, const float *attr, int channel_major, const float *calib, int projection,
                   int nearest, int h, int w, float scale, float bias, float lo, float hi, float background,
                   float *image, float *depth, int32_t *face_id, mp_stream stream) {
  return mesh_render_checked(ctx, "mp_mesh_render", 1, &verts, max_verts, &faces, max_faces, &counts,
                             attr ? &attr : nullptr, channel_major, 1, calib, projection, nearest, h, w, scale, bias, lo,
                             hi, background, image ? &image : nullptr, depth ? &depth : nullptr,
                             face_id ? &face_id : nullptr, nullptr, stream);
}

int mp_mesh_render_batch(mp_ctx *ctx, int n_frames, const float *const *verts, int64_t max_verts,
                         const int32_t *const *faces, int64_t max_faces, const int32_t *const *counts,
                         const float *const *attr, int channel_major, int n_views, const float *calibs,
                         int projection, int nearest, int h, int w, float scale, float bias, float lo, float hi,
                         float background, float *const *image, float *const *depth, int32_t *const *face_id,
                         mp_stream stream) {
  return mesh_render_checked(ctx, "mp_mesh_render_batch", n_frames, verts, max_verts, faces, max_faces, counts, attr,
                             channel_major, n_views, calibs, projection, nearest, h, w, scale, bias, lo, hi, background,
                             image, depth, face_id, nullptr, stream);
}

int mp_mesh_render_clip(mp_ctx *ctx, const float *verts, int64_t max_verts, const int32_t *faces, int64_t max_faces,
                        const int32_t *counts, const float *attr, int channel_major, const float *calib,
                        int projection, int nearest, int h, int w, float scale, float bias, float lo, float hi,
                        float background, float *image, float *depth, int32_t *face_id, float near, int flags,
                        mp_stream stream) {
  const MeshRenderClip clip = {near, flags};
  return mesh_render_checked(ctx, "mp_mesh_render_clip", 1, &verts, max_verts, &faces, max_faces, &counts,
                             attr ? &attr : nullptr, channel_major, 1, calib, projection, nearest, h, w, scale, bias, lo,
                             hi, background, image ? &image : nullptr, depth ? &depth : nullptr,
                             face_id ? &face_id : nullptr, &clip, stream);
}

int mp_mesh_render_clip_batch(mp_ctx *ctx, int n_frames, const float *const *verts, int64_t max_verts,
                              const int32_t *const *faces, int64_t max_faces, const int32_t *const *counts,
                              const float *const *attr, int channel_major, int n_views, const float *calibs,
                              int projection, int nearest, int h, int w, float scale, float bias, float lo, float hi,
                              float background, float *const *image, float *const *depth, int32_t *const *face_id,
                              float near, int flags, mp_stream stream) {
  const MeshRenderClip clip = {near, flags};
  return mesh_render_checked(ctx, "mp_mesh_render_clip_batch", n_frames, verts, max_verts, faces, max_faces, counts,
                             attr, channel_major, n_views, calibs, projection, nearest, h, w, scale, bias, lo, hi,
                             background, image, depth, face_id, &clip, stream);
}

int mp_mesh_normals_batch(mp_ctx *ctx, int n_frames, const float *const *verts, int64_t max_verts,
                          const int32_t *const *faces, int64_t max_faces, const int32_t *const *counts, int mode,
                          float *const *normals, mp_stream stream) {
  return mesh_normals_checked(ctx, "mp_mesh_normals_batch", n_frames, verts, max_verts, faces, max_faces, counts, mode,
                              normals, stream);
}

int mp_mesh_simplify(mp_ctx *ctx, const float *verts, int64_t max_verts, const int32_t *faces, int64_t max_faces,
                     const int32_t *counts, const float *b_min, const float *b_max, int n, float *verts_out,
                     int32_t *faces_out, int32_t *counts_out, int32_t *vmap, mp_stream stream) {
  return mesh_simplify_checked(ctx, "mp_mesh_simplify", 1, &verts, max_verts, &faces, max_faces, &counts, b_min, b_max,
                               n, &verts_out, &faces_out, &counts_out, vmap ? &vmap : nullptr, stream);
}

int mp_mesh_simplify_batch(mp_ctx *ctx, int n_frames, const float *const *verts, int64_t max_verts,
                           const int32_t *const *faces, int64_t max_faces, const int32_t *const *counts,
                           const float *b_min, const float *b_max, int n, float *const *verts_out,
                           int32_t *const *faces_out, int32_t *const *counts_out, int32_t *const *vmap,
                           mp_stream stream) {
  return mesh_simplify_checked(ctx, "mp_mesh_simplify_batch", n_frames, verts, max_verts, faces, max_faces, counts,
                               b_min, b_max, n, verts_out, faces_out, counts_out, vmap, stream);
}

int mp_mesh_smooth(mp_ctx *ctx, const float *verts, int64_t max_verts, const int32_t *faces, int64_t max_faces,
                   const int32_t *counts, int iterations, float lambda, float mu, int flags, float *verts_out,
                   int32_t *ring, mp_stream stream) {
  return mesh_smooth_checked(ctx, "mp_mesh_smooth", 1, &verts, max_verts, &faces, max_faces, &counts, iterations,
                             lambda, mu, flags, &verts_out, ring ? &ring : nullptr, stream);
}

int mp_mesh_smooth_batch(mp_ctx *ctx, int n_frames, const float *const *verts, int64_t max_verts,
                         const int32_t *const *faces, int64_t max_faces, const int32_t *const *counts, int iterations,
                         float lambda, float mu, int flags, float *const *verts_out, int32_t *const *ring,
                         mp_stream stream) {
  return mesh_smooth_checked(ctx, "mp_mesh_smooth_batch", n_frames, verts, max_verts, faces, max_faces, counts,
                             iterations, lambda, mu, flags, verts_out, ring, stream);
}

static bool glb_flags_ok(int flags) { return (flags & ~(MP_GLB_NORMALS | MP_GLB_COLORS)) == 0; }

int64_t mp_glb_bytes(int64_t nv, int64_t nf, int flags) {
  if (nv < 0 || nf < 0 || nv > (1LL << 40) || nf > (1LL << 40) || !glb_flags_ok(flags)) return 0;
  return (int64_t)glb_bytes(nv, nf, flags);
}

int64_t mp_glb_max_bytes(int64_t max_verts, int64_t max_faces, int flags) {
  return mp_glb_bytes(max_verts, max_faces, flags);
}

// the box of the 16-bit positions and the capacity of a file, as mp_mesh_glb and mp_mesh_glb_textured refuse them
static int glb_box_checked(mp_ctx *ctx, const char *who, const float *b_min, const float *b_max, int64_t capacity,
                           GlbCall *c) {
  for (int a = 0; a < 3; ++a) {
    if (!std::isfinite(b_min[a]) || !std::isfinite(b_max[a]) || !(b_max[a] > b_min[a]))
      return fail(ctx, MP_ERR_ARG, "%s: the box needs finite bounds with b_max > b_min, got [%g, %g] on axis %d", who,
                  (double)b_min[a], (double)b_max[a], a);
    c->b_min[a] = b_min[a], c->b_max[a] = b_max[a];
    c->inv[a] = 65535.0f / (b_max[a] - b_min[a]);
    if (!std::isfinite(c->inv[a]))
      return fail(ctx, MP_ERR_ARG, "%s: the box is too thin on axis %d for 16-bit positions (%g wide)", who, a,
                  (double)(b_max[a] - b_min[a]));
  }
  if (capacity < MP_GLB_MIN_BYTES || capacity > ((int64_t)1 << 31))
    return fail(ctx, MP_ERR_ARG, "%s: capacity %lld (at least the empty file's %d bytes, at most 2^31)", who,
                (long long)capacity, MP_GLB_MIN_BYTES);
  return MP_OK;
}

static int mesh_glb_checked(mp_ctx *ctx, const char *who, int n_frames, const float *const *verts, int64_t max_verts,
                            const int32_t *const *faces, int64_t max_faces, const int32_t *const *counts,
                            const float *const *normals, const float *const *colors, int color_layout,
                            float color_scale, float color_bias, const float *b_min, const float *b_max, uint8_t *out,
                            int64_t capacity, int32_t *info, mp_stream stream) {
  if (!ctx) return MP_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  int rc = check_count(ctx, who, "frame", n_frames, kMaxFrames, MP_ERR_ARG);
  if (rc != MP_OK) return rc;
  if (!counts || !b_min || !b_max || !out || !info || ((uintptr_t)info & 3u) || max_verts < 0 || max_faces < 0 ||
      (max_verts > 0 && !verts) || (max_faces > 0 && !faces))
    return bad_argument(ctx, who);
  if (color_layout != MP_GLB_COLOR_ROWS && color_layout != MP_GLB_COLOR_PLANES)
    return fail(ctx, MP_ERR_ARG, "%s: color_layout %d (MP_GLB_COLOR_ROWS or MP_GLB_COLOR_PLANES)", who, color_layout);
  if (!std::isfinite(color_scale) || !std::isfinite(color_bias))
    return fail(ctx, MP_ERR_ARG, "%s: a non-finite color_scale or color_bias", who);
  GlbCall c;
  rc = glb_box_checked(ctx, who, b_min, b_max, capacity, &c);
  if (rc != MP_OK) return rc;
  const int flags = (normals ? MP_GLB_NORMALS : 0) | (colors ? MP_GLB_COLORS : 0);
  if (max_verts > (1LL << 40) || max_faces > (1LL << 40) || glb_bytes(max_verts, max_faces, flags) >= (1LL << 31))
    return fail(ctx, MP_ERR_UNSUPPORTED, "%s: capacities of %lld vertices and %lld faces: a file could reach 2^31 bytes",
                who, (long long)max_verts, (long long)max_faces);
  if (max_verts == 0) verts = nullptr, normals = nullptr, colors = nullptr;  // rows of a capacity of 0 are not looked at
  if (max_faces == 0) faces = nullptr;
  rc = check_frames(ctx, who, n_frames, nullptr, counts, verts, faces, normals, colors);
  if (rc != MP_OK) return rc;
  const size_t vbytes = (size_t)max_verts * 12, out_bytes = (size_t)n_frames * (size_t)capacity;
  const size_t info_bytes = (size_t)n_frames * 8;
  if (ranges_overlap(out, out_bytes, info, info_bytes)) return fail(ctx, MP_ERR_ARG, "%s: out aliases info", who);
  const FrameSpans ins[5] = {{verts, vbytes}, {faces, (size_t)max_faces * 12}, {counts, 8}, {normals, vbytes},
                             {colors, vbytes}};
  for (int f = 0; f < n_frames; ++f)
    for (const FrameSpans &k : ins)
      if (ranges_overlap(out, out_bytes, k.of(f), k.bytes) || ranges_overlap(info, info_bytes, k.of(f), k.bytes))
        return fail(ctx, MP_ERR_ARG, "%s: out or info aliases an input of frame %d", who, f);
  DeviceGuard g(ctx->device);
  c.n_frames = n_frames, c.color_planes = color_layout == MP_GLB_COLOR_PLANES;
  c.max_v = max_verts, c.max_f = max_faces, c.capacity = capacity;
  c.color_scale = color_scale, c.color_bias = color_bias;
  void *scratch = nullptr;
  rc = ensure_scratch(ctx, (hipStream_t)stream, glb_scratch_bytes(n_frames), &scratch);
  if (rc != MP_OK) return rc;
  return launch_mesh_glb_batch(ctx, scratch, c, verts, faces, counts, normals, colors, out, info, (hipStream_t)stream);
}

int mp_mesh_glb(mp_ctx *ctx, const float *verts, int64_t max_verts, const int32_t *faces, int64_t max_faces,
                const int32_t *counts, const float *normals, const float *colors, int color_layout, float color_scale,
                float color_bias, const float *b_min, const float *b_max, uint8_t *out, int64_t capacity, int32_t *info,
                mp_stream stream) {
  return mesh_glb_checked(ctx, "mp_mesh_glb", 1, &verts, max_verts, &faces, max_faces, &counts,
                          normals ? &normals : nullptr, colors ? &colors : nullptr, color_layout, color_scale,
                          color_bias, b_min, b_max, out, capacity, info, stream);
}

int mp_mesh_glb_batch(mp_ctx *ctx, int n_frames, const float *const *verts, int64_t max_verts,
                      const int32_t *const *faces, int64_t max_faces, const int32_t *const *counts,
                      const float *const *normals, const float *const *colors, int color_layout, float color_scale,
                      float color_bias, const float *b_min, const float *b_max, uint8_t *out, int64_t capacity,
                      int32_t *info, mp_stream stream) {
  return mesh_glb_checked(ctx, "mp_mesh_glb_batch", n_frames, verts, max_verts, faces, max_faces, counts, normals,
                          colors, color_layout, color_scale, color_bias, b_min, b_max, out, capacity, info, stream);
}

// the atlas's sizes, as mp_mesh_atlas and mp_mesh_glb_textured refuse them
static int atlas_sizes_checked(mp_ctx *ctx, const char *who, int atlas_size, int cell) {
  if (atlas_size < MP_ATLAS_MIN_SIZE || atlas_size > MP_ATLAS_MAX_SIZE || (atlas_size & (atlas_size - 1)))
    return fail(ctx, MP_ERR_ARG, "%s: atlas_size must be a power of two in %d..%d, got %d", who, MP_ATLAS_MIN_SIZE,
                MP_ATLAS_MAX_SIZE, atlas_size);
  if (cell < MP_ATLAS_MIN_CELL || cell > MP_ATLAS_MAX_CELL)
    return fail(ctx, MP_ERR_ARG, "%s: cell must be in %d..%d, got %d", who, MP_ATLAS_MIN_CELL, MP_ATLAS_MAX_CELL, cell);
  return MP_OK;
}

static int mesh_atlas_checked(mp_ctx *ctx, const char *who, int n_frames, const float *const *verts, int64_t max_verts,
                              const int32_t *const *faces, int64_t max_faces, const int32_t *const *counts,
                              int atlas_size, int cell, float background, int32_t *const *face_id,
                              float *const *position, int32_t *const *info, mp_stream stream) {
  if (!ctx) return MP_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  int rc = atlas_sizes_checked(ctx, who, atlas_size, cell);
  if (rc != MP_OK) return rc;
  rc = check_count(ctx, who, "frame", n_frames, kMaxFrames, MP_ERR_ARG);
  if (rc != MP_OK) return rc;
  if (!counts || !face_id || !position || !info || max_verts < 0 || max_faces < 0 || (max_verts > 0 && !verts) ||
      (max_faces > 0 && !faces))
    return bad_argument(ctx, who);
  if (!std::isfinite(background)) return fail(ctx, MP_ERR_ARG, "%s: a non-finite background", who);
  if (max_verts > 0x7fffffffLL / 3 || max_faces > 0x7fffffffLL / 3)
    return fail(ctx, MP_ERR_UNSUPPORTED, "%s: capacities beyond 2^31 / 3 need 64-bit indices", who);
  if (max_verts == 0) verts = nullptr;  // rows of a capacity of 0 are not looked at
  if (max_faces == 0) faces = nullptr;
  rc = check_frames(ctx, who, n_frames, nullptr, counts, verts, faces, face_id, position, info);
  if (rc != MP_OK) return rc;
  const size_t texels = (size_t)atlas_size * (size_t)atlas_size;
  const FrameSpans outs[3] = {{face_id, texels * 4}, {position, texels * 12}, {info, 8}};
  const FrameSpans ins[3] = {{verts, (size_t)max_verts * 12}, {faces, (size_t)max_faces * 12}, {counts, 8}};
  rc = check_no_alias(ctx, who, n_frames, outs, ins);
  if (rc != MP_OK) return rc;
  for (int f = 0; f < n_frames; ++f)  // no output shares a byte with another output, of any frame
    for (int i = 0; i < n_frames; ++i)
      for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b)
          if ((f != i || a != b) && ranges_overlap(outs[a].of(f), outs[a].bytes, outs[b].of(i), outs[b].bytes))
            return fail(ctx, MP_ERR_ARG, "%s: an output of frame %d aliases an output of frame %d", who, f, i);
  DeviceGuard g(ctx->device);
  return launch_mesh_atlas_batch(ctx, n_frames, verts, max_verts, faces, max_faces, counts, atlas_size, cell, background,
                                 face_id, position, info, (hipStream_t)stream);
}

int mp_mesh_atlas(mp_ctx *ctx, const float *verts, int64_t max_verts, const int32_t *faces, int64_t max_faces,
                  const int32_t *counts, int atlas_size, int cell, float background, int32_t *face_id, float *position,
                  int32_t *info, mp_stream stream) {
  return mesh_atlas_checked(ctx, "mp_mesh_atlas", 1, &verts, max_verts, &faces, max_faces, &counts, atlas_size, cell,
                            background, &face_id, &position, &info, stream);
}

int mp_mesh_atlas_batch(mp_ctx *ctx, int n_frames, const float *const *verts, int64_t max_verts,
                        const int32_t *const *faces, int64_t max_faces, const int32_t *const *counts, int atlas_size,
                        int cell, float background, int32_t *const *face_id, float *const *position,
                        int32_t *const *info, mp_stream stream) {
  return mesh_atlas_checked(ctx, "mp_mesh_atlas_batch", n_frames, verts, max_verts, faces, max_faces, counts,
                            atlas_size, cell, background, face_id, position, info, stream);
}

int64_t mp_glb_textured_bytes(int64_t nf, int flags, int64_t png_bytes) {
  if (nf < 0 || png_bytes < 0 || nf > (1LL << 40) || png_bytes > (1LL << 40) || (flags & ~MP_GLB_NORMALS)) return 0;
  return (int64_t)glb_textured_bytes(nf, flags, png_bytes);
}

int64_t mp_glb_textured_max_bytes(int64_t max_faces, int flags, int atlas_size) {
  if (atlas_size < MP_ATLAS_MIN_SIZE || atlas_size > MP_ATLAS_MAX_SIZE || (atlas_size & (atlas_size - 1))) return 0;
  const int64_t png = mp_png_max_bytes(atlas_size, atlas_size, MP_PNG_RGB8);
  return png > 0 ? mp_glb_textured_bytes(max_faces, flags, png) : 0;
}

static int mesh_glb_textured_checked(mp_ctx *ctx, const char *who, int n_frames, const float *const *verts,
                                     int64_t max_verts, const int32_t *const *faces, int64_t max_faces,
                                     const int32_t *const *counts, const float *const *normals, bool colors,
                                     int atlas_size, int cell, const uint8_t *png, int64_t png_capacity,
                                     const int32_t *png_info, const float *b_min, const float *b_max, uint8_t *out,
                                     int64_t capacity, int32_t *info, mp_stream stream) {
  if (!ctx) return MP_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  int rc = check_count(ctx, who, "frame", n_frames, kMaxFrames, MP_ERR_ARG);
  if (rc != MP_OK) return rc;
  if (colors)
    return fail(ctx, MP_ERR_ARG, "%s: COLOR_0 together with a texture: glTF multiplies the two; colors must be NULL", who);
  rc = atlas_sizes_checked(ctx, who, atlas_size, cell);
  if (rc != MP_OK) return rc;
  if (!counts || !b_min || !b_max || !out || !info || ((uintptr_t)info & 3u) || !png || !png_info ||
      ((uintptr_t)png_info & 3u) || max_verts < 0 || max_faces < 0 || (max_verts > 0 && !verts) ||
      (max_faces > 0 && !faces))
    return bad_argument(ctx, who);
  GlbCall c;
  rc = glb_box_checked(ctx, who, b_min, b_max, capacity, &c);
  if (rc != MP_OK) return rc;
  if (png_capacity < MP_PNG_MIN_BYTES || png_capacity > ((int64_t)1 << 31))
    return fail(ctx, MP_ERR_ARG, "%s: png_capacity %lld (at least a PNG's %d bytes, at most 2^31)", who,
                (long long)png_capacity, MP_PNG_MIN_BYTES);
  const int flags = normals ? MP_GLB_NORMALS : 0;
  if (max_verts > 0x7fffffffLL / 3 || max_faces > (1LL << 40) ||
      mp_glb_textured_max_bytes(max_faces, flags, atlas_size) >= (1LL << 31))
    return fail(ctx, MP_ERR_UNSUPPORTED, "%s: capacities of %lld vertices and %lld faces: a file could reach 2^31 bytes",
                who, (long long)max_verts, (long long)max_faces);
  if (max_verts == 0) verts = nullptr, normals = nullptr;  // rows of a capacity of 0 are not looked at
  if (max_faces == 0) faces = nullptr;
  rc = check_frames(ctx, who, n_frames, nullptr, counts, verts, faces, normals);
  if (rc != MP_OK) return rc;
  const size_t vbytes = (size_t)max_verts * 12, out_bytes = (size_t)n_frames * (size_t)capacity;
  const size_t info_bytes = (size_t)n_frames * 8, png_bytes = (size_t)n_frames * (size_t)png_capacity;
  if (ranges_overlap(out, out_bytes, info, info_bytes)) return fail(ctx, MP_ERR_ARG, "%s: out aliases info", who);
  for (const void *o : {(const void *)out, (const void *)info}) {
    const size_t ob = o == (const void *)out ? out_bytes : info_bytes;
    if (ranges_overlap(o, ob, png, png_bytes) || ranges_overlap(o, ob, png_info, info_bytes))
      return fail(ctx, MP_ERR_ARG, "%s: out or info aliases png or png_info", who);
  }
  const FrameSpans ins[4] = {{verts, vbytes}, {faces, (size_t)max_faces * 12}, {counts, 8}, {normals, vbytes}};
  for (int f = 0; f < n_frames; ++f)
    for (const FrameSpans &k : ins)
      if (ranges_overlap(out, out_bytes, k.of(f), k.bytes) || ranges_overlap(info, info_bytes, k.of(f), k.bytes))
        return fail(ctx, MP_ERR_ARG, "%s: out or info aliases an input of frame %d", who, f);
  DeviceGuard g(ctx->device);
  c.n_frames = n_frames, c.color_planes = 0;
  c.max_v = max_verts, c.max_f = max_faces, c.capacity = capacity;
  c.color_scale = 1.0f, c.color_bias = 0.0f;
  const GlbTextureCall tc = {atlas_size, cell, png, (long long)png_capacity, png_info};
  void *scratch = nullptr;
  rc = ensure_scratch(ctx, (hipStream_t)stream, glb_scratch_bytes(n_frames), &scratch);
  if (rc != MP_OK) return rc;
  return launch_mesh_glb_textured_batch(ctx, scratch, c, tc, verts, faces, counts, normals, out, info,
                                        (hipStream_t)stream);
}

int mp_mesh_glb_textured(mp_ctx *ctx, const float *verts, int64_t max_verts, const int32_t *faces, int64_t max_faces,
                         const int32_t *counts, const float *normals, const float *colors, int atlas_size, int cell,
                         const uint8_t *png, int64_t png_capacity, const int32_t *png_info, const float *b_min,
                         const float *b_max, uint8_t *out, int64_t capacity, int32_t *info, mp_stream stream) {
  return mesh_glb_textured_checked(ctx, "mp_mesh_glb_textured", 1, &verts, max_verts, &faces, max_faces, &counts,
                                   normals ? &normals : nullptr, colors != nullptr, atlas_size, cell, png, png_capacity,
                                   png_info, b_min, b_max, out, capacity, info, stream);
}

int mp_mesh_glb_textured_batch(mp_ctx *ctx, int n_frames, const float *const *verts, int64_t max_verts,
                               const int32_t *const *faces, int64_t max_faces, const int32_t *const *counts,
                               const float *const *normals, const float *const *colors, int atlas_size, int cell,
                               const uint8_t *png, int64_t png_capacity, const int32_t *png_info, const float *b_min,
                               const float *b_max, uint8_t *out, int64_t capacity, int32_t *info, mp_stream stream) {
  return mesh_glb_textured_checked(ctx, "mp_mesh_glb_textured_batch", n_frames, verts, max_verts, faces, max_faces,
                                   counts, normals, colors != nullptr, atlas_size, cell, png, png_capacity, png_info,
                                   b_min, b_max, out, capacity, info, stream);
}

int mp_mesh_points(mp_ctx *ctx, const float *verts, int64_t max_verts, const int32_t *counts, float *points,
                   int32_t *count_out, mp_stream stream) {
  return mesh_points_checked(ctx, "mp_mesh_points", 1, &verts, max_verts, &counts, &points, &count_out, stream);
}

int mp_mesh_points_batch(mp_ctx *ctx, int n_frames, const float *const *verts, int64_t max_verts,
                         const int32_t *const *counts, float *const *points, int32_t *const *count_out,
                         mp_stream stream) {
  return mesh_points_checked(ctx, "mp_mesh_points_batch", n_frames, verts, max_verts, counts, points, count_out,
                             stream);
}

int mp_picture_points(mp_ctx *ctx, const int32_t *face_id, const float *position, int64_t n_pixels, int64_t capacity,
                      float *points, int32_t *pixels, int32_t *count, mp_stream stream) {
  return picture_points_checked(ctx, "mp_picture_points", 1, &face_id, &position, n_pixels, capacity, &points, &pixels,
                                &count, stream);
}

int mp_picture_points_batch(mp_ctx *ctx, int n_frames, const int32_t *const *face_id, const float *const *position,
                            int64_t n_pixels, int64_t capacity, float *const *points, int32_t *const *pixels,
                            int32_t *const *count, mp_stream stream) {
  return picture_points_checked(ctx, "mp_picture_points_batch", n_frames, face_id, position, n_pixels, capacity, points,
                                pixels, count, stream);
}

int mp_picture_paint(mp_ctx *ctx, const float *values, const int32_t *pixels, const int32_t *count, int64_t capacity,
                     int64_t n_pixels, float scale, float bias, float lo, float hi, float *image, mp_stream stream) {
  return picture_paint_checked(ctx, "mp_picture_paint", 1, &values, &pixels, &count, capacity, n_pixels, scale, bias, lo,
                               hi, &image, stream);
}

int mp_picture_paint_batch(mp_ctx *ctx, int n_frames, const float *const *values, const int32_t *const *pixels,
                           const int32_t *const *count, int64_t capacity, int64_t n_pixels, float scale, float bias,
                           float lo, float hi, float *const *image, mp_stream stream) {
  return picture_paint_checked(ctx, "mp_picture_paint_batch", n_frames, values, pixels, count, capacity, n_pixels, scale,
                               bias, lo, hi, image, stream);
}

int64_t mp_texture_pyramid_floats(int ht, int wt, int levels) {
  return texture_sizes_ok(ht, wt, levels) ? (int64_t)texture_pyramid_floats(ht, wt, levels) : 0;
}

int mp_texture_mips(mp_ctx *ctx, const float *tex, int ht, int wt, int levels, float *pyramid, mp_stream stream) {
  return texture_mips_checked(ctx, "mp_texture_mips", tex, ht, wt, levels, pyramid, stream);
}

int mp_picture_texture(mp_ctx *ctx, const float *uv, const int32_t *face_id, int n_views, int h, int w,
                       const float *pyramid, int ht, int wt, int levels, int wrap, float scale, float bias, float lo,
                       float hi, float background, float *image, mp_stream stream) {
  return picture_texture_checked(ctx, "mp_picture_texture", 1, &uv, &face_id, n_views, h, w, pyramid, ht, wt, levels,
                                 wrap, scale, bias, lo, hi, background, &image, stream);
}

int mp_picture_texture_batch(mp_ctx *ctx, int n_frames, const float *const *uv, const int32_t *const *face_id,
                             int n_views, int h, int w, const float *pyramid, int ht, int wt, int levels, int wrap,
                             float scale, float bias, float lo, float hi, float background, float *const *image,
                             mp_stream stream) {
  return picture_texture_checked(ctx, "mp_picture_texture_batch", n_frames, uv, face_id, n_views, h, w, pyramid, ht, wt,
                                 levels, wrap, scale, bias, lo, hi, background, image, stream);
}

int mp_picture_composite(mp_ctx *ctx, const float *front_image, const float *front_depth, const int32_t *front_face,
                         const float *back_image, const float *back_depth, const int32_t *back_face, int64_t n_pixels,
                         int mode, int nearest, float background, float *image, float *depth, uint8_t *mask,
                         mp_stream stream) {
  return picture_composite_checked(ctx, "mp_picture_composite", 1, &front_image, &front_depth, &front_face, &back_image,
                                   &back_depth, &back_face, n_pixels, mode, nearest, background, &image,
                                   depth ? &depth : nullptr, mask ? &mask : nullptr, stream);
}

int mp_picture_composite_batch(mp_ctx *ctx, int n_frames, const float *const *front_image,
                               const float *const *front_depth, const int32_t *const *front_face,
                               const float *const *back_image, const float *const *back_depth,
                               const int32_t *const *back_face, int64_t n_pixels, int mode, int nearest,
                               float background, float *const *image, float *const *depth, uint8_t *const *mask,
                               mp_stream stream) {
  return picture_composite_checked(ctx, "mp_picture_composite_batch", n_frames, front_image, front_depth, front_face,
                                   back_image, back_depth, back_face, n_pixels, mode, nearest, background, image, depth,
                                   mask, stream);
}

int mp_picture_resolve(mp_ctx *ctx, const float *image, const float *depth, const int32_t *face_id,
                       const uint8_t *mask, int h, int w, int samples, int nearest, float *image_out, float *depth_out,
                       int32_t *face_out, uint8_t *mask_out, float *coverage, mp_stream stream) {
  return picture_resolve_checked(ctx, "mp_picture_resolve", 1, 1, image ? &image : nullptr, depth ? &depth : nullptr,
                                 face_id ? &face_id : nullptr, mask ? &mask : nullptr, h, w, samples, nearest,
                                 image_out ? &image_out : nullptr, depth_out ? &depth_out : nullptr,
                                 face_out ? &face_out : nullptr, mask_out ? &mask_out : nullptr,
                                 coverage ? &coverage : nullptr, stream);
}

int mp_picture_resolve_batch(mp_ctx *ctx, int n_frames, int n_views, const float *const *image,
                             const float *const *depth, const int32_t *const *face_id, const uint8_t *const *mask,
                             int h, int w, int samples, int nearest, float *const *image_out, float *const *depth_out,
                             int32_t *const *face_out, uint8_t *const *mask_out, float *const *coverage,
                             mp_stream stream) {
  return picture_resolve_checked(ctx, "mp_picture_resolve_batch", n_frames, n_views, image, depth, face_id, mask, h, w,
                                 samples, nearest, image_out, depth_out, face_out, mask_out, coverage, stream);
}

int mp_picture_shadow(mp_ctx *ctx, const float *image_in, const float *position, const int32_t *face_id,
                      int64_t n_pixels, const float *map_depth, const int32_t *map_face, int hs, int ws,
                      const float *light_calib, int projection, int nearest, float bias, int radius, float strength,
                      float *image_out, float *shade, mp_stream stream) {
  return picture_shadow_checked(ctx, "mp_picture_shadow", 1, image_in ? &image_in : nullptr, &position, &face_id,
                                n_pixels, &map_depth, &map_face, hs, ws, light_calib, projection, nearest, bias, radius,
                                strength, image_out ? &image_out : nullptr, shade ? &shade : nullptr, stream);
}

int mp_picture_shadow_batch(mp_ctx *ctx, int n_frames, const float *const *image_in, const float *const *position,
                            const int32_t *const *face_id, int64_t n_pixels, const float *const *map_depth,
                            const int32_t *const *map_face, int hs, int ws, const float *light_calibs, int projection,
                            int nearest, float bias, int radius, float strength, float *const *image_out,
                            float *const *shade, mp_stream stream) {
  return picture_shadow_checked(ctx, "mp_picture_shadow_batch", n_frames, image_in, position, face_id, n_pixels,
                                map_depth, map_face, hs, ws, light_calibs, projection, nearest, bias, radius, strength,
                                image_out, shade, stream);
}

int mp_picture_light(mp_ctx *ctx, const float *normal, const int32_t *face_id, const float *albedo,
                     const float *albedo_rgb, const float *visibility, int64_t n_pixels, int n_views, const float *sh,
                     const float *direct_dir, const float *direct_rgb, float gamma, const float *normal_mats,
                     float background, float *image_out, float *shading, mp_stream stream) {
  return picture_light_checked(ctx, "mp_picture_light", 1, &normal, &face_id, albedo ? &albedo : nullptr, albedo_rgb,
                               visibility ? &visibility : nullptr, nullptr, false, n_pixels, n_views, sh, direct_dir,
                               direct_rgb, gamma, normal_mats, background, image_out ? &image_out : nullptr,
                               shading ? &shading : nullptr, stream);
}

int mp_picture_light_batch(mp_ctx *ctx, int n_frames, const float *const *normal, const int32_t *const *face_id,
                           const float *const *albedo, const float *albedo_rgb, const float *const *visibility,
                           int64_t n_pixels, int n_views, const float *sh, const float *direct_dir,
                           const float *direct_rgb, float gamma, const float *normal_mats, float background,
                           float *const *image_out, float *const *shading, mp_stream stream) {
  return picture_light_checked(ctx, "mp_picture_light_batch", n_frames, normal, face_id, albedo, albedo_rgb, visibility,
                               nullptr, false, n_pixels, n_views, sh, direct_dir, direct_rgb, gamma, normal_mats,
                               background, image_out, shading, stream);
}

int mp_picture_light_transfer(mp_ctx *ctx, const float *normal, const int32_t *face_id, const float *albedo,
                              const float *albedo_rgb, const float *visibility, const float *ambient, int64_t n_pixels,
                              const float *direct_dir, const float *direct_rgb, float gamma, float background,
                              float *image_out, float *shading, mp_stream stream) {
  return picture_light_checked(ctx, "mp_picture_light_transfer", 1, normal ? &normal : nullptr, &face_id,
                               albedo ? &albedo : nullptr, albedo_rgb, visibility ? &visibility : nullptr,
                               ambient ? &ambient : nullptr, true, n_pixels, 1, nullptr, direct_dir, direct_rgb, gamma,
                               nullptr, background, image_out ? &image_out : nullptr, shading ? &shading : nullptr,
                               stream);
}

int mp_picture_light_transfer_batch(mp_ctx *ctx, int n_frames, const float *const *normal,
                                    const int32_t *const *face_id, const float *const *albedo, const float *albedo_rgb,
                                    const float *const *visibility, const float *const *ambient, int64_t n_pixels,
                                    const float *direct_dir, const float *direct_rgb, float gamma, float background,
                                    float *const *image_out, float *const *shading, mp_stream stream) {
  return picture_light_checked(ctx, "mp_picture_light_transfer_batch", n_frames, normal, face_id, albedo, albedo_rgb,
                               visibility, ambient, true, n_pixels, 1, nullptr, direct_dir, direct_rgb, gamma, nullptr,
                               background, image_out, shading, stream);
}

int mp_picture_u8(mp_ctx *ctx, const float *image, int64_t n_pixels, uint8_t *out, mp_stream stream) {
  if (!ctx) return MP_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (n_pixels < 0) return fail(ctx, MP_ERR_ARG, "mp_picture_u8: n_pixels %lld", (long long)n_pixels);
  if (n_pixels > 0x7fffffffLL / 3)
    return fail(ctx, MP_ERR_UNSUPPORTED, "mp_picture_u8: n_pixels %lld (at most 2^31 / 3)", (long long)n_pixels);
  if (n_pixels == 0) return MP_OK;
  if (!image || !out || ((uintptr_t)image & 3u))
    return fail(ctx, MP_ERR_ARG, "mp_picture_u8: a null or misaligned buffer");
  if (ranges_overlap(out, (size_t)n_pixels * 3, image, (size_t)n_pixels * 12))
    return fail(ctx, MP_ERR_ARG, "mp_picture_u8: out aliases image");
  DeviceGuard g(ctx->device);
  return launch_picture_u8(ctx, image, n_pixels, out, (hipStream_t)stream);
}

static bool jpeg_geometry_ok(int h, int w, int subsampling, int restart) {
  return h >= 1 && h <= MP_JPEG_MAX_SIDE && w >= 1 && w <= MP_JPEG_MAX_SIDE &&
         (subsampling == MP_JPEG_444 || subsampling == MP_JPEG_420) && restart >= 0 && restart <= 65535;
}

int64_t mp_jpeg_max_bytes(int h, int w, int subsampling, int restart) {
  return jpeg_geometry_ok(h, w, subsampling, restart) ? (int64_t)jpeg_max_bytes(h, w, subsampling == MP_JPEG_420, restart)
                                                      : 0;
}

int mp_picture_jpeg(mp_ctx *ctx, const float *images, int n, int h, int w, int quality, int subsampling, int restart,
                    uint8_t *out, int64_t capacity, int32_t *info, mp_stream stream) {
  const char *who = "mp_picture_jpeg";
  if (!ctx) return MP_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (h < 1 || h > MP_JPEG_MAX_SIDE || w < 1 || w > MP_JPEG_MAX_SIDE)
    return fail(ctx, MP_ERR_UNSUPPORTED, "%s: a picture of %d x %d (sides 1..%d)", who, h, w, MP_JPEG_MAX_SIDE);
  if (subsampling != MP_JPEG_444 && subsampling != MP_JPEG_420)
    return fail(ctx, MP_ERR_UNSUPPORTED, "%s: subsampling %d (MP_JPEG_444 or MP_JPEG_420)", who, subsampling);
  if (quality < 1 || quality > 100) return fail(ctx, MP_ERR_ARG, "%s: quality %d (1..100)", who, quality);
  if (restart < 0 || restart > 65535)
    return fail(ctx, MP_ERR_ARG, "%s: restart %d (0: one MCU row, or 1..65535 MCUs)", who, restart);
  if (n < 1) return fail(ctx, MP_ERR_ARG, "%s: n %d pictures", who, n);
  if (n > 65535) return fail(ctx, MP_ERR_UNSUPPORTED, "%s: n %d pictures (at most 65535 per call)", who, n);
  if (capacity < jpeg_header_bytes() || capacity > ((int64_t)1 << 31))
    return fail(ctx, MP_ERR_ARG, "%s: capacity %lld (at least the header's %d bytes, at most 2^31)", who,
                (long long)capacity, jpeg_header_bytes());
  if (!images || !out || !info || ((uintptr_t)images & 3u) || ((uintptr_t)info & 3u))
    return fail(ctx, MP_ERR_ARG, "%s: a null or misaligned buffer", who);
  const size_t in_bytes = (size_t)n * h * w * 12, out_bytes = (size_t)n * (size_t)capacity, info_bytes = (size_t)n * 8;
  if (ranges_overlap(out, out_bytes, images, in_bytes) || ranges_overlap(info, info_bytes, images, in_bytes) ||
      ranges_overlap(out, out_bytes, info, info_bytes))
    return fail(ctx, MP_ERR_ARG, "%s: out / info aliases images or each other", who);
  DeviceGuard g(ctx->device);
  const int s420 = subsampling == MP_JPEG_420;
  void *scratch = nullptr;
  const int rc = ensure_scratch(ctx, (hipStream_t)stream, jpeg_scratch_bytes(n, h, w, s420, restart), &scratch);
  if (rc != MP_OK) return rc;
  return launch_picture_jpeg(ctx, scratch, images, n, h, w, quality, s420, restart, out, capacity, info,
                             (hipStream_t)stream);
}

int mp_picture_u16(mp_ctx *ctx, const float *depth, int64_t n_pixels, float lo, float scale, uint16_t *out,
                   mp_stream stream) {
  const char *who = "mp_picture_u16";
  if (!ctx) return MP_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (n_pixels < 0) return fail(ctx, MP_ERR_ARG, "%s: n_pixels %lld", who, (long long)n_pixels);
  if (n_pixels > 0x7fffffffLL)
    return fail(ctx, MP_ERR_UNSUPPORTED, "%s: n_pixels %lld (at most 2^31)", who, (long long)n_pixels);
  if (!std::isfinite(lo) || !std::isfinite(scale)) return fail(ctx, MP_ERR_ARG, "%s: a non-finite lo or scale", who);
  if (n_pixels == 0) return MP_OK;
  if (!depth || !out || ((uintptr_t)depth & 3u) || ((uintptr_t)out & 1u))
    return fail(ctx, MP_ERR_ARG, "%s: a null or misaligned buffer", who);
  if (ranges_overlap(out, (size_t)n_pixels * 2, depth, (size_t)n_pixels * 4))
    return fail(ctx, MP_ERR_ARG, "%s: out aliases depth", who);
  DeviceGuard g(ctx->device);
  return launch_picture_u16(ctx, depth, n_pixels, lo, scale, out, (hipStream_t)stream);
}

int mp_picture_rgba8(mp_ctx *ctx, const float *image, const float *alpha, int64_t n_pixels, int unmatte,
                     float background, uint8_t *out, mp_stream stream) {
  const char *who = "mp_picture_rgba8";
  if (!ctx) return MP_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (n_pixels < 0) return fail(ctx, MP_ERR_ARG, "%s: n_pixels %lld", who, (long long)n_pixels);
  if (n_pixels > 0x7fffffffLL / 4)
    return fail(ctx, MP_ERR_UNSUPPORTED, "%s: n_pixels %lld (at most 2^31 / 4)", who, (long long)n_pixels);
  if (!std::isfinite(background)) return fail(ctx, MP_ERR_ARG, "%s: a non-finite background", who);
  if (n_pixels == 0) return MP_OK;
  if (!image || !alpha || !out || ((uintptr_t)image & 3u) || ((uintptr_t)alpha & 3u) || ((uintptr_t)out & 3u))
    return fail(ctx, MP_ERR_ARG, "%s: a null or misaligned buffer", who);
  if (ranges_overlap(out, (size_t)n_pixels * 4, image, (size_t)n_pixels * 12) ||
      ranges_overlap(out, (size_t)n_pixels * 4, alpha, (size_t)n_pixels * 4))
    return fail(ctx, MP_ERR_ARG, "%s: out aliases image or alpha", who);
  DeviceGuard g(ctx->device);
  return launch_picture_rgba8(ctx, image, alpha, n_pixels, unmatte != 0, background, out, (hipStream_t)stream);
}

static bool png_geometry_ok(int h, int w, int format) {
  return h >= 1 && h <= MP_PNG_MAX_SIDE && w >= 1 && w <= MP_PNG_MAX_SIDE && format >= MP_PNG_RGB8 &&
         format <= MP_PNG_GRAY16;
}

int64_t mp_png_max_bytes(int h, int w, int format) {
  return png_geometry_ok(h, w, format) ? (int64_t)png_max_bytes(h, w, format) : 0;
}

int mp_picture_png(mp_ctx *ctx, const float *images, const float *alpha, int n, int h, int w, int format, int filter,
                   float lo, float scale, int unmatte, float background, uint8_t *out, int64_t capacity, int32_t *info,
                   mp_stream stream) {
  const char *who = "mp_picture_png";
  if (!ctx) return MP_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (h < 1 || h > MP_PNG_MAX_SIDE || w < 1 || w > MP_PNG_MAX_SIDE)
    return fail(ctx, MP_ERR_UNSUPPORTED, "%s: a picture of %d x %d (sides 1..%d)", who, h, w, MP_PNG_MAX_SIDE);
  if (format < MP_PNG_RGB8 || format > MP_PNG_GRAY16)
    return fail(ctx, MP_ERR_UNSUPPORTED, "%s: format %d (MP_PNG_RGB8, MP_PNG_RGBA8 or MP_PNG_GRAY16)", who, format);
  if (filter < MP_PNG_NONE || filter > MP_PNG_ADAPTIVE)
    return fail(ctx, MP_ERR_UNSUPPORTED, "%s: filter %d (MP_PNG_NONE .. MP_PNG_ADAPTIVE)", who, filter);
  if (n < 1) return fail(ctx, MP_ERR_ARG, "%s: n %d pictures", who, n);
  if (n > 65535) return fail(ctx, MP_ERR_UNSUPPORTED, "%s: n %d pictures (at most 65535 per call)", who, n);
  if (capacity < png_min_bytes() || capacity > ((int64_t)1 << 31))
    return fail(ctx, MP_ERR_ARG, "%s: capacity %lld (at least the smallest file's %d bytes, at most 2^31)", who,
                (long long)capacity, png_min_bytes());
  if (alpha && format != MP_PNG_RGBA8) return fail(ctx, MP_ERR_ARG, "%s: alpha for a format without it", who);
  if (!alpha && format == MP_PNG_RGBA8) return fail(ctx, MP_ERR_ARG, "%s: MP_PNG_RGBA8 without alpha", who);
  if (unmatte && !alpha) return fail(ctx, MP_ERR_ARG, "%s: unmatte without alpha", who);
  if (!std::isfinite(lo) || !std::isfinite(scale) || !std::isfinite(background))
    return fail(ctx, MP_ERR_ARG, "%s: a non-finite lo, scale or background", who);
  if (!images || !out || !info || ((uintptr_t)images & 3u) || ((uintptr_t)alpha & 3u) || ((uintptr_t)info & 3u))
    return fail(ctx, MP_ERR_ARG, "%s: a null or misaligned buffer", who);
  const size_t px = (size_t)n * h * w, in_bytes = px * (format == MP_PNG_GRAY16 ? 4 : 12);
  const size_t al_bytes = alpha ? px * 4 : 0, out_bytes = (size_t)n * (size_t)capacity, info_bytes = (size_t)n * 8;
  if (ranges_overlap(out, out_bytes, images, in_bytes) || ranges_overlap(info, info_bytes, images, in_bytes) ||
      ranges_overlap(out, out_bytes, info, info_bytes) ||
      (alpha && (ranges_overlap(out, out_bytes, alpha, al_bytes) || ranges_overlap(info, info_bytes, alpha, al_bytes))))
    return fail(ctx, MP_ERR_ARG, "%s: out / info aliases images, alpha or each other", who);
  DeviceGuard g(ctx->device);
  PngCall c;
  c.n = n, c.h = h, c.w = w, c.format = format, c.filter = filter, c.unmatte = unmatte != 0;
  c.lo = lo, c.scale = scale, c.background = background, c.capacity = capacity;
  void *scratch = nullptr;
  const int rc = ensure_scratch(ctx, (hipStream_t)stream, png_scratch_bytes(c), &scratch);
  if (rc != MP_OK) return rc;
  return launch_picture_png(ctx, scratch, images, alpha, c, out, info, (hipStream_t)stream);
}

int64_t mp_volume_bits_words(int r) { return r < 1 || r > MP_TRANSFER_MAX_RES ? 0 : (int64_t)volume_bits_words(r); }

int mp_volume_bits(mp_ctx *ctx, const float *volume, int r, float level, uint32_t *bits, mp_stream stream) {
  return volume_bits_checked(ctx, "mp_volume_bits", 1, &volume, r, level, &bits, nullptr, stream);
}

int mp_volume_bits_batch(mp_ctx *ctx, int n_frames, const float *const *volume, int r, float level,
                         uint32_t *const *bits, const int32_t *const *gates, mp_stream stream) {
  return volume_bits_checked(ctx, "mp_volume_bits_batch", n_frames, volume, r, level, bits, gates, stream);
}

int mp_mesh_transfer(mp_ctx *ctx, const float *verts, const float *normals, int64_t max_verts, const int32_t *counts,
                     const uint32_t *bits, int r, const float *b_min, const float *b_max, int n_dirs, const float *dirs,
                     const float *basis, float weight, float bias_w, float step_w, int max_steps, uint64_t *mask,
                     float *prt, mp_stream stream) {
  return mesh_transfer_checked(ctx, "mp_mesh_transfer", 1, &verts, &normals, max_verts, &counts, &bits, r, b_min, b_max,
                               n_dirs, dirs, basis, weight, bias_w, step_w, max_steps, mask ? &mask : nullptr,
                               prt ? &prt : nullptr, stream);
}

int mp_mesh_transfer_batch(mp_ctx *ctx, int n_frames, const float *const *verts, const float *const *normals,
                           int64_t max_verts, const int32_t *const *counts, const uint32_t *const *bits, int r,
                           const float *b_min, const float *b_max, int n_dirs, const float *dirs, const float *basis,
                           float weight, float bias_w, float step_w, int max_steps, uint64_t *const *mask,
                           float *const *prt, mp_stream stream) {
  return mesh_transfer_checked(ctx, "mp_mesh_transfer_batch", n_frames, verts, normals, max_verts, counts, bits, r,
                               b_min, b_max, n_dirs, dirs, basis, weight, bias_w, step_w, max_steps, mask, prt, stream);
}

int mp_mesh_transfer_shade(mp_ctx *ctx, const float *prt, int64_t max_verts, const int32_t *counts, const float *sh,
                           float *out, mp_stream stream) {
  return transfer_shade_checked(ctx, "mp_mesh_transfer_shade", 1, &prt, max_verts, &counts, sh, &out, stream);
}

int mp_mesh_transfer_shade_batch(mp_ctx *ctx, int n_frames, const float *const *prt, int64_t max_verts,
                                 const int32_t *const *counts, const float *sh, float *const *out, mp_stream stream) {
  return transfer_shade_checked(ctx, "mp_mesh_transfer_shade_batch", n_frames, prt, max_verts, counts, sh, out, stream);
}

int mp_volume_keep_largest(mp_ctx *ctx, const float *volume, int r, float level, int connectivity, float fill,
                           float *out, int32_t *stats, mp_stream stream) {
  return keep_largest_checked(ctx, "mp_volume_keep_largest", 1, &volume, r, level, connectivity, fill, &out, &stats,
                              nullptr, stream);
}

int mp_volume_keep_largest_batch(mp_ctx *ctx, int n_frames, const float *const *volume, int r, float level,
                                 int connectivity, float fill, float *const *out, int32_t *const *stats,
                                 const int32_t *const *gate, mp_stream stream) {
  return keep_largest_checked(ctx, "mp_volume_keep_largest_batch", n_frames, volume, r, level, connectivity, fill, out,
                              stats, gate, stream);
}

int mp_group_norm(mp_ctx *ctx, const float *x, int n, int c, int64_t hw, int groups,
                  const float *gamma, const float *beta, float eps, int relu, float *y,
                  mp_stream stream) {
  if (!ctx) return MP_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (!x || !y || !gamma || !beta || n <= 0 || n > 4096 || c <= 0 || hw <= 0 || groups <= 0 ||
      groups > 4096)
    return fail(ctx, MP_ERR_ARG, "mp_group_norm: bad argument");
  if (c % groups || hw % 4 || !aligned16(x) || !aligned16(y))
    return fail(ctx, MP_ERR_UNSUPPORTED, "mp_group_norm: needs C %% groups == 0, HW %% 4 == 0, 16-byte aligned x/y");
  DeviceGuard g(ctx->device);
  void *scratch = nullptr;
  int rc = ensure_scratch(ctx, (hipStream_t)stream, gn_scratch_bytes(n * groups), &scratch);
  if (rc != MP_OK) return rc;
  return launch_group_norm(ctx, scratch, x, n, c, hw, groups, gamma, beta, eps, relu, y,
                           (hipStream_t)stream);
}

int mp_upsample_bicubic2x(mp_ctx *ctx, const float *x, int c, int h, int w, const float *add,
                          float *y, mp_stream stream) {
  if (!ctx) return MP_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (!x || !y || c <= 0 || h < 2 || w < 2)
    return fail(ctx, MP_ERR_ARG, "mp_upsample_bicubic2x: bad argument");
  DeviceGuard g(ctx->device);
  return launch_upsample_bicubic2x(ctx, x, c, h, w, add, y, (hipStream_t)stream);
}

int mp_concat3_add(mp_ctx *ctx, const float *a, int ca, const float *b, int cb, const float *c,
                   int cc, const float *shortcut, int n, int64_t hw, float *y, mp_stream stream) {
  if (!ctx) return MP_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (!a || !b || !c || !shortcut || !y || ca <= 0 || cb <= 0 || cc <= 0 || n <= 0 || hw <= 0)
    return fail(ctx, MP_ERR_ARG, "mp_concat3_add: bad argument");
  if (hw % 4 || !aligned16(a) || !aligned16(b) || !aligned16(c) || !aligned16(shortcut) || !aligned16(y))
    return fail(ctx, MP_ERR_UNSUPPORTED, "mp_concat3_add: needs HW %% 4 == 0 and 16-byte aligned buffers");
  DeviceGuard g(ctx->device);
  return launch_concat3_add(ctx, a, ca, b, cb, c, cc, shortcut, n, hw, y, (hipStream_t)stream);
}

int mp_conv3x3_pack(mp_ctx *ctx, const float *w, int cout, int cin, float *packed, mp_stream stream) {
  if (!ctx) return MP_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (!w || !packed || cout <= 0 || cin <= 0) return fail(ctx, MP_ERR_ARG, "mp_conv3x3_pack: bad argument");
  if (cin % 16 || cout % 32)
    return fail(ctx, MP_ERR_UNSUPPORTED, "mp_conv3x3_pack: needs Cin %% 16 == 0 and Cout %% 32 == 0");
  DeviceGuard g(ctx->device);
  return launch_conv3x3_pack(ctx, w, cout, cin, packed, (hipStream_t)stream);
}

int mp_conv3x3_pack_wino(mp_ctx *ctx, const float *w, int cout, int cin, float *packed_wino, mp_stream stream) {
  if (!ctx) return MP_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (!w || !packed_wino || cout <= 0 || cin <= 0) return fail(ctx, MP_ERR_ARG, "mp_conv3x3_pack_wino: bad argument");
  if (cin % 16 || cout % 32)
    return fail(ctx, MP_ERR_UNSUPPORTED, "mp_conv3x3_pack_wino: needs Cin %% 16 == 0 and Cout %% 32 == 0");
  if (!aligned16(packed_wino)) return fail(ctx, MP_ERR_ARG, "mp_conv3x3_pack_wino: the output must be 16-byte aligned");
  DeviceGuard g(ctx->device);
  return launch_conv3x3_wino_pack(ctx, w, cout, cin, packed_wino, (hipStream_t)stream);
}

int mp_conv3x3_wino_supported(int cin, int cout, int h, int w) { return conv3x3_wino_supported(cin, cout, h, w) ? 1 : 0; }

int mp_conv3x3_pack16(mp_ctx *ctx, const float *w, int cout, int cin, void *packed16, float *wmax,
                      mp_stream stream) {
  if (!ctx) return MP_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (!w || !packed16 || !wmax || cout <= 0 || cin <= 0)
    return fail(ctx, MP_ERR_ARG, "mp_conv3x3_pack16: bad argument");
  if (cin % 16 || cout % 32)
    return fail(ctx, MP_ERR_UNSUPPORTED, "mp_conv3x3_pack16: needs Cin %% 16 == 0 and Cout %% 32 == 0");
  DeviceGuard g(ctx->device);
  return launch_conv3x3_pack16(ctx, w, cout, cin, packed16, wmax, (hipStream_t)stream);
}

int mp_conv3x3_gn16(mp_ctx *ctx, const float *x, int n, int cin, int h, int w, const float *ss, int relu,
                    int reflect, const void *packed16, const float *wmax, int cout, float *y, double *stats,
                    mp_stream stream) {
  if (!ctx) return MP_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (!x || !packed16 || !wmax || !y || n <= 0 || n > 65535 || cin <= 0 || cout <= 0 || h <= 0 || w <= 0)
    return fail(ctx, MP_ERR_ARG, "mp_conv3x3_gn16: bad argument");
  if (!aligned16(packed16)) return fail(ctx, MP_ERR_ARG, "mp_conv3x3_gn16: packed weights must be 16-byte aligned");
  DeviceGuard g(ctx->device);
  return launch_conv3x3_gn(ctx, x, n, cin, h, w, ss, relu, reflect, static_cast<const float *>(packed16),
                           wmax, cout, y, stats, (hipStream_t)stream);
}

int mp_conv1x1_pack(mp_ctx *ctx, const float *w1, int c1, const float *w2, int c2, int cout, int f16,
                    void *packed, float *wmax, mp_stream stream) {
  if (!ctx) return MP_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (!w1 || !packed || c1 <= 0 || c2 < 0 || (c2 > 0 && !w2) || (f16 && !wmax))
    return fail(ctx, MP_ERR_ARG, "mp_conv1x1_pack: bad argument");
  if (c1 % 64 || c2 % 64 || (cout != 128 && cout != 256))
    return fail(ctx, MP_ERR_UNSUPPORTED,
                "mp_conv1x1_pack: input channel counts must be multiples of 64, output channels 128 or 256");
  DeviceGuard g(ctx->device);
  return launch_conv1x1_pack(ctx, w1, c1, w2, c2, cout, f16, packed, wmax, (hipStream_t)stream);
}

int mp_conv1x1(mp_ctx *ctx, const float *x1, const float *ss1, int relu1, const float *x2, int n, int c1,
               int c2, int cout, int64_t hw, const void *packed, int f16, const float *wmax, const float *bias,
               const float *res, float *y, float *y_hwc, double *stats, mp_stream stream) {
  if (!ctx) return MP_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (!x1 || !packed || n <= 0 || hw <= 0 || (!y && !y_hwc) || (f16 && !wmax))
    return fail(ctx, MP_ERR_ARG, "mp_conv1x1: bad argument");
  if (!aligned16(packed) || (y_hwc && !aligned16(y_hwc)))
    return fail(ctx, MP_ERR_ARG, "mp_conv1x1: packed weights / y_hwc must be 16-byte aligned");
  DeviceGuard g(ctx->device);
  return launch_conv1x1_raw(ctx, x1, ss1, relu1, x2, n, c1, c2, cout, hw, packed, f16, wmax, bias, res, y,
                            y_hwc, stats, (hipStream_t)stream);
}

int mp_scale_shift_add(mp_ctx *ctx, const float *t, const float *ss, const float *res, int n, int c,
                       int64_t hw, float *y, mp_stream stream) {
  if (!ctx) return MP_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (!t || !ss || !res || !y || n <= 0 || c <= 0 || hw <= 0)
    return fail(ctx, MP_ERR_ARG, "mp_scale_shift_add: bad argument");
  if (hw % 4 || !aligned16(t) || !aligned16(res) || !aligned16(y))
    return fail(ctx, MP_ERR_UNSUPPORTED, "mp_scale_shift_add: needs HW %% 4 == 0 and 16-byte aligned buffers");
  DeviceGuard g(ctx->device);
  return launch_scale_shift_add(ctx, t, ss, res, (long long)n * c, hw, y, (hipStream_t)stream);
}

int mp_conv3x3_supported(int cin, int cout, int h, int w) { return conv3x3_supported(cin, cout, h, w) ? 1 : 0; }
int mp_conv_stats_supported(int cout) { return conv_stats_supported(cout) ? 1 : 0; }

int mp_gn_stat_slices(void) { return gn_stat_slices(); }

int mp_conv3x3_stat_slices(int cout, int n, int h, int w, int f16) {
  if (cout < 32 || cout % 32 || n < 1 || h < 1 || w < 32) return 0;
  return conv3x3_stat_slices(cout, n, h, w, f16 != 0);
}

void mp_query_tune(int small_tiles) { mp::query_small_set_gate(small_tiles); }

void mp_conv3x3_tune(int nr) {
  // bit 12 is both | 0x1000 (the 128-channel Winograd kernel) and mrw = 1, which is mp_conv1x1's own choice: the two
  // do not collide.  (Masking with 0xfff here used to strip 0x1000, so that word left the 3x3 launches on the heuristic.)
  conv3x3_set_nr(nr & 0x1fff);
  conv1x1_set_mrw((nr >> 12) & 3);
}

int mp_conv3x3_gn(mp_ctx *ctx, const float *x, int n, int cin, int h, int w, const float *ss, int relu,
                  int reflect, const float *packed, int cout, float *y, double *stats, mp_stream stream) {
  if (!ctx) return MP_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (!x || !packed || !y || n <= 0 || n > 65535 || cin <= 0 || cout <= 0 || h <= 0 || w <= 0)
    return fail(ctx, MP_ERR_ARG, "mp_conv3x3_gn: bad argument");
  if (!aligned16(packed)) return fail(ctx, MP_ERR_ARG, "mp_conv3x3_gn: packed weights must be 16-byte aligned");
  DeviceGuard g(ctx->device);
  return launch_conv3x3_gn(ctx, x, n, cin, h, w, ss, relu, reflect, packed, nullptr, cout, y, stats,
                           (hipStream_t)stream);
}

int mp_gn_stats(mp_ctx *ctx, const float *x, int n, int c, int64_t hw, int groups, double *partial,
                mp_stream stream) {
  if (!ctx) return MP_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (!x || !partial || n <= 0 || c <= 0 || hw <= 0 || groups <= 0)
    return fail(ctx, MP_ERR_ARG, "mp_gn_stats: bad argument");
  if (c % groups || hw % 4 || !aligned16(x))
    return fail(ctx, MP_ERR_UNSUPPORTED, "mp_gn_stats: needs C %% groups == 0, HW %% 4 == 0, 16-byte aligned x");
  DeviceGuard g(ctx->device);
  return launch_gn_stats(ctx, x, n, c, hw, groups, partial, (hipStream_t)stream);
}

int mp_gn_finalize(mp_ctx *ctx, const double *partial, int n, int c, int groups, int slices,
                   int64_t count, const float *gamma, const float *beta, float eps, float *ss,
                   mp_stream stream) {
  if (!ctx) return MP_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (!partial || !gamma || !beta || !ss || n <= 0 || c <= 0 || groups <= 0 || slices <= 0 ||
      count <= 0 || c % groups || c / groups > 64)
    return fail(ctx, MP_ERR_ARG, "mp_gn_finalize: bad argument");
  DeviceGuard g(ctx->device);
  return launch_gn_finalize(ctx, partial, n, c, groups, slices, (double)count, gamma, beta, eps, ss,
                            (hipStream_t)stream);
}

// mp_gn_out / mp_gn_in (C-ABI) -> GnOut / GnIn (kernel arguments); the launchers fill c / S / count
static GnOut to_out(const mp_gn_out *f) {
  GnOut g = gn_out_none();
  if (!f) return g;
  g.acc = reinterpret_cast<long long *>(f->acc);
  g.partial = f->partial;
  return g;
}
static long long out_cap(const mp_gn_out *f) { return f && f->partial ? (long long)f->partial_doubles : -1; }
static GnIn to_in(const mp_gn_in *f) {
  GnIn g = gn_in_none();
  if (!f) return g;
  g.acc = reinterpret_cast<const long long *>(f->acc);
  g.gamma = f->gamma;
  g.beta = f->beta;
  g.eps = f->eps;
  g.ss = f->acc ? nullptr : f->ss;
  return g;
}

int mp_conv3x3_ex(mp_ctx *ctx, const mp_conv3x3_args *q, mp_stream stream) {
  if (!ctx) return MP_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (!q || !q->x || !q->packed || (!q->y && !q->y2) || q->n <= 0 || q->n > 65535 || q->cin <= 0 || q->cout <= 0 ||
      q->h <= 0 || q->w <= 0)
    return fail(ctx, MP_ERR_ARG, "mp_conv3x3_ex: bad argument");
  if (!aligned16(q->packed)) return fail(ctx, MP_ERR_ARG, "mp_conv3x3_ex: packed weights must be 16-byte aligned");
  DeviceGuard g(ctx->device);
  ConvArgs a;
  a.x = q->x;
  a.gn = to_in(&q->gn);
  a.wp = static_cast<const float *>(q->packed);
  a.y = q->y;
  a.y2 = q->y2;
  a.res = q->res;
  a.y2_c = q->y2 ? q->y2_channels : 32;
  a.y2_off = q->y2 ? q->y2_offset : 0;
  a.fin = to_out(&q->fin);
  a.fin2 = to_out(&q->fin2);
  a.n_img = q->n;
  a.cin = q->cin;
  a.cout = q->cout;
  a.h = q->h;
  a.w = q->w;
  a.relu = q->relu;
  a.reflect = q->reflect;
  if (q->packed_wino) {
    if (!aligned16(q->packed_wino)) return fail(ctx, MP_ERR_ARG, "mp_conv3x3_ex: packed_wino must be 16-byte aligned");
    a.wpw = q->packed_wino;
  }
  const long long cap[2] = {out_cap(&q->fin), out_cap(&q->fin2)};
  return launch_conv3x3(ctx, a, q->wmax, cap, (hipStream_t)stream);
}

int mp_conv1x1_ex(mp_ctx *ctx, const mp_conv1x1_args *q, mp_stream stream) {
  if (!ctx) return MP_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (!q || !q->x1 || !q->packed || q->n <= 0 || q->hw <= 0 || (!q->y && !q->y_hwc) || (q->f16 && !q->wmax))
    return fail(ctx, MP_ERR_ARG, "mp_conv1x1_ex: bad argument");
  if (!aligned16(q->packed) || (q->y_hwc && !aligned16(q->y_hwc)))
    return fail(ctx, MP_ERR_ARG, "mp_conv1x1_ex: packed weights / y_hwc must be 16-byte aligned");
  DeviceGuard g(ctx->device);
  Conv1Args a;
  a.x1 = q->x1;
  a.gn1 = to_in(&q->gn1);
  a.x2 = q->x2;
  a.wp = static_cast<const float *>(q->packed);
  a.bias = q->bias;
  a.res = q->res;
  a.y = q->y;
  a.y_hwc = q->y_hwc;
  a.fin = to_out(&q->fin);
  a.n_img = q->n;
  a.c1 = q->c1;
  a.c2 = q->c2;
  a.hw = (int)q->hw;
  a.relu1 = q->relu1;
  a.cout = q->cout;
  return launch_conv1x1(ctx, a, q->f16, q->wmax, out_cap(&q->fin), (hipStream_t)stream);
}

int mp_gn_acc_replicas(void) { return kGnReplicas; }

int mp_conv1x1_stat_slices(int64_t hw) { return hw > 0 ? conv1x1_stat_slices(hw) : 0; }

int mp_convk_supported(int cin, int cout, int ks, int stride, int h, int w) {
  return convk_supported(cin, cout, ks, stride, h, w) ? 1 : 0;
}

int64_t mp_convk_packed_floats(int cin, int cout, int ks) {
  if (cin <= 0 || cout <= 0 || (ks != 3 && ks != 7) || cin % (ks == 7 ? 3 : 16)) return 0;
  return convk_packed_floats(cin, cout, ks);
}

int mp_convk_stat_slices(int ks, int stride, int h, int w) {
  if ((ks != 3 && ks != 7) || stride < 1 || stride > 2 || h <= 0 || w <= 0) return 0;
  return convk_stat_slices(ks, stride, h, w);
}

int mp_convk_pack(mp_ctx *ctx, const float *w, int cout, int cin, int ks, float *packed, mp_stream stream) {
  if (!ctx) return MP_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (!w || !packed || mp_convk_packed_floats(cin, cout, ks) <= 0 || cout % 32)
    return fail(ctx, MP_ERR_ARG, "mp_convk_pack: bad argument");
  DeviceGuard g(ctx->device);
  return launch_convk_pack(ctx, w, cout, cin, ks, packed, (hipStream_t)stream);
}

int mp_convk(mp_ctx *ctx, const mp_convk_args *q, mp_stream stream) {
  if (!ctx) return MP_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (!q || !q->x || !q->packed || !q->y || q->n <= 0 || q->n > 65535 || q->cin <= 0 || q->cout <= 0 ||
      q->h <= 0 || q->w <= 0)
    return fail(ctx, MP_ERR_ARG, "mp_convk: bad argument");
  if (!aligned16(q->packed)) return fail(ctx, MP_ERR_ARG, "mp_convk: packed weights must be 16-byte aligned");
  DeviceGuard g(ctx->device);
  ConvKArgs a;
  a.x = q->x;
  a.gn = to_in(&q->gn);
  a.wp = q->packed;
  a.bias = q->bias;
  a.y = q->y;
  a.fin = to_out(&q->fin);
  a.n_img = q->n;
  a.cin = q->cin;
  a.cout = q->cout;
  a.h = q->h;
  a.w = q->w;
  a.ho = a.wo = 0;
  a.ks = q->ks;
  a.stride = q->stride;
  a.pad = q->ks / 2;
  a.reflect = q->reflect;
  a.relu = q->relu;
  a.wp_floats = 0;
  return launch_convk(ctx, a, out_cap(&q->fin), (hipStream_t)stream);
}

static int check_ew(mp_ctx *ctx, const char *who, const void *x, const void *y, int n, int c, long long hw_out) {
  if (!x || !y || n <= 0 || n > 4096 || c <= 0 || hw_out <= 0) return fail(ctx, MP_ERR_ARG, "%s: bad argument", who);
  if (c % 32 || hw_out % 4 || !aligned16(x) || !aligned16(y))
    return fail(ctx, MP_ERR_UNSUPPORTED, "%s: needs C %% 32 == 0, output H*W %% 4 == 0, 16-byte aligned buffers", who);
  return MP_OK;
}

int mp_avgpool2_gn(mp_ctx *ctx, const float *x, int n, int c, int h, int w, float *y, const mp_gn_out *fin,
                   mp_stream stream) {
  if (!ctx) return MP_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (h < 2 || w < 8 || h % 2 || w % 8) return fail(ctx, MP_ERR_UNSUPPORTED, "mp_avgpool2_gn: needs H %% 2 == 0, W %% 8 == 0");
  int rc = check_ew(ctx, "mp_avgpool2_gn", x, y, n, c, (long long)(h / 2) * (w / 2));
  if (rc != MP_OK) return rc;
  DeviceGuard g(ctx->device);
  return launch_avgpool2_gn(ctx, x, n, c, h, w, y, to_out(fin), out_cap(fin), (hipStream_t)stream);
}

int mp_upsample_bicubic2x_gn(mp_ctx *ctx, const float *x, int n, int c, int h, int w, const float *add, float *y,
                             const mp_gn_out *fin, mp_stream stream) {
  if (!ctx) return MP_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (h < 2 || w < 2 || w % 2) return fail(ctx, MP_ERR_UNSUPPORTED, "mp_upsample_bicubic2x_gn: needs H, W >= 2, W %% 2 == 0");
  int rc = check_ew(ctx, "mp_upsample_bicubic2x_gn", x, y, n, c, 4LL * h * w);
  if (rc != MP_OK) return rc;
  if (add && !aligned16(add)) return fail(ctx, MP_ERR_UNSUPPORTED, "mp_upsample_bicubic2x_gn: add must be 16-byte aligned");
  DeviceGuard g(ctx->device);
  return launch_upsample_add_gn(ctx, x, n, c, h, w, add, y, to_out(fin), out_cap(fin), (hipStream_t)stream);
}

int mp_upsample_gn_banded(int c, int h, int w) { return upsample_gn_banded(c, h, w) ? 1 : 0; }

int mp_gn_apply(mp_ctx *ctx, const float *x, const mp_gn_in *gn, int relu, int n, int c, int64_t hw,
                const float *res, float *y, const mp_gn_out *fin, mp_stream stream) {
  if (!ctx) return MP_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (!gn) return fail(ctx, MP_ERR_ARG, "mp_gn_apply: bad argument");
  int rc = check_ew(ctx, "mp_gn_apply", x, y, n, c, hw);
  if (rc != MP_OK) return rc;
  if (res && !aligned16(res)) return fail(ctx, MP_ERR_UNSUPPORTED, "mp_gn_apply: res must be 16-byte aligned");
  DeviceGuard g(ctx->device);
  return launch_gn_apply_gn(ctx, x, to_in(gn), relu, n, c, hw, res, y, to_out(fin), out_cap(fin), (hipStream_t)stream);
}

int mp_mfma_clock_probe(mp_ctx *ctx, float ms_target, double *out4, mp_stream stream) {
  if (!ctx) return MP_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (!out4 || !(ms_target >= 1.0f) || ms_target > 2000.0f)
    return fail(ctx, MP_ERR_ARG, "mp_mfma_clock_probe: out4 must be given, 1 <= ms_target <= 2000");
  DeviceGuard g(ctx->device);
  return launch_mfma_clock_probe(ctx, ms_target, out4, (hipStream_t)stream);
}

int mp_profile_begin(mp_ctx *ctx, int max_records) {
  if (!ctx) return MP_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (max_records < 1 || max_records > (1 << 20))
    return fail(ctx, MP_ERR_ARG, "mp_profile_begin: bad max_records");
  DeviceGuard g(ctx->device);
  for (hipEvent_t e : ctx->prof_events) (void)hipEventDestroy(e);
  ctx->prof_events.clear();
  ctx->prof_used = 0;
  ctx->prof_events.resize(2 * (size_t)max_records);
  for (auto &e : ctx->prof_events) MP_HIP(ctx, hipEventCreate(&e));
  return MP_OK;
}

int mp_profile_end(mp_ctx *ctx, float *ms_out, int capacity, int *n_out) {
  if (!ctx) return MP_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (!ms_out || !n_out || capacity < 0) return fail(ctx, MP_ERR_ARG, "mp_profile_end: bad argument");
  DeviceGuard g(ctx->device);
  const int n = ctx->prof_used;
  int rc = MP_OK;
  for (int i = 0; i < n && rc == MP_OK; ++i) {
    if (hipEventSynchronize(ctx->prof_events[2 * i + 1]) != hipSuccess) {
      rc = fail(ctx, MP_ERR_HIP, "mp_profile_end: hipEventSynchronize failed");
      break;
    }
    float ms = 0.0f;
    if (hipEventElapsedTime(&ms, ctx->prof_events[2 * i], ctx->prof_events[2 * i + 1]) != hipSuccess)
      rc = fail(ctx, MP_ERR_HIP, "mp_profile_end: hipEventElapsedTime failed");
    if (i < capacity) ms_out[i] = ms;
  }
  *n_out = n;
  for (hipEvent_t e : ctx->prof_events) (void)hipEventDestroy(e);
  ctx->prof_events.clear();
  ctx->prof_used = 0;
  return rc;
}

}  // extern "C"
