/* monoport_hip.h -- C-ABI of the MI355X-native MonoPort reconstruction hot path.
 *
 * Drop-in boundary: plain pointers and sizes, no torch types, no C++
 * exceptions.  Every entry point names the reference interface it replaces (file:line under
 * the MonoPort tree).  The reference is pure Python; its "FFI" for this path is the set of
 * torch ops listed in SURVEY.md section 2a, so a maintainer binds these symbols with ctypes (see
 * INTEGRATION.md) exactly as monoport_amd/_lib.py does.
 *
 * Conventions
 *   - all tensor arguments are DEVICE pointers on the context's GPU unless marked (host);
 *   - fp32 everywhere ("f32" compute on v_mfma_f32_32x32x2_f32); int64 for vertex indices;
 *   - work is enqueued on `stream` (a hipStream_t; NULL = the default stream) and the call
 *     returns without synchronising, except where noted;
 *   - the caller owns every input/output buffer; the context owns only its scratch arena and
 *     the packed MLP weights;
 *   - a context may be used from any host thread; calls on ONE context are serialised by an
 *     internal mutex (RTL/dataloader.py:1026-1053 runs every pipeline stage on its own thread:
 *     give each stage its own context);
 *   - return value: MP_OK or a negative MP_ERR_*; mp_last_error(ctx) gives the message of the
 *     last failing call MADE BY THE CALLING HOST THREAD (per-thread storage, like errno), valid
 *     until that thread's next failing call;
 *   - calls that SYNCHRONISE: mp_mlp_set_precision (drains the stream of the last mp_mlp_load),
 *     mp_mlp_destroy, mp_stream_release and mp_destroy (hipDeviceSynchronize), mp_profile_end
 *     (waits for the recorded events).  Everything else only enqueues.
 *   - scratch: one arena per (context, stream), grown by adding blocks -- a pointer handed to a
 *     kernel stays valid until mp_stream_release / mp_destroy, so work captured in a hipGraph
 *     keeps working after later, larger calls on the same stream.
 */
#ifndef MONOPORT_HIP_H
#define MONOPORT_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mp_ctx mp_ctx;
typedef void *mp_stream; /* hipStream_t */

enum {
  MP_OK = 0,
  MP_ERR_ARG = -1,         /* bad pointer / size / enum */
  MP_ERR_HIP = -2,         /* a HIP runtime call failed */
  MP_ERR_UNSUPPORTED = -3, /* shape outside what the kernels are built for */
  MP_ERR_STATE = -4,       /* e.g. querying an MLP whose layers are not all loaded */
  MP_ERR_NOMEM = -5
};

/* SurfaceClassifier last_op (heads/SurfaceClassifier.py:68-69, :77, :85) */
enum { MP_ACT_NONE = 0, MP_ACT_SIGMOID = 1, MP_ACT_TANH = 2 };

/* projection of a frame's points into its image (MonoPortNet's opt_net.projection, MonoPortNet.py:20-27).
 * Every entry point without a `projection` argument projects orthogonally. */
enum {
  MP_PROJ_ORTHOGONAL = 0, /* xyz = R p + t (geometry.py:19-34) */
  MP_PROJ_PERSPECTIVE = 1 /* (R p + t) = (u, v, z) -> xyz = (u / z, v / z, z) (geometry.py:37-55); a point with
                             z == 0 projects to +-inf / NaN, and a fused query returns NaN for it in every channel
                             (the reference's grid_sample samples NaN there) -- every other out-of-image point is
                             exactly 0.0f; points behind the camera (z < 0) are sampled like any other */
};

/* arithmetic of the MLP GEMMs (mp_mlp_set_precision) */
enum {
  MP_PREC_F32 = 0,   /* v_mfma_f32_32x32x2_f32: exact f32 products, the default */
  MP_PREC_F16X3 = 1, /* f32 emulated on v_mfma_f32_32x32x16_f16: every operand split into two
                        halves (hi + lo, 22 significant bits), three MFMAs per product term
                        (hi*hi + hi*lo + lo*hi), f32 accumulation; netG heads (C = 256) only */
  MP_PREC_F16W = 2,  /* fp16 WEIGHTS (rounded once, per-layer power-of-two scale), activations
                        still split: hi*hi + hi*lo, two MFMAs (BASELINE configs[4]) */
  MP_PREC_F16 = 3    /* fp16 weights and fp16 activations, f32 accumulation: one MFMA */
};

/* forward_vertices direction (RTL/recon.py:39-49) */
enum { MP_DIR_FRONT = 0, MP_DIR_BACK = 1, MP_DIR_LEFT = 2, MP_DIR_RIGHT = 3 };

/* ---- context ---------------------------------------------------------------------------- */
int mp_version(void);
/* Creates a context bound to HIP device `device`.  Fails (MP_ERR_HIP) when no GPU is visible:
 * there is no CPU fallback. */
int mp_create(int device, mp_ctx **out);
void mp_destroy(mp_ctx *ctx);
const char *mp_last_error(mp_ctx *ctx); /* calling thread's last error; ctx may be NULL */
/* Frees the scratch arena the context keeps for `stream` (call when the stream is destroyed, e.g.
 * by the owner of a pipeline slot; arenas are keyed by the stream handle).  Synchronises the
 * device.  Unknown streams are fine (MP_OK). */
int mp_stream_release(mp_ctx *ctx, mp_stream stream);
/* Device memory the context owns right now (host array of 4): [0] scratch arenas incl. outgrown blocks still
 * kept for captured graphs, [1] packed MLP weights (all precisions), [2] number of arenas, [3] number of
 * skip tables registered (the tables themselves are the caller's).  Soak tests assert these stay flat. */
int mp_memory_stats(mp_ctx *ctx, int64_t *out4);
/* TEST HOOK, not part of any frame: grows the scratch arena of `stream` to at least `bytes`, then sets every byte of
 * the arena's whole current block (which may be larger than `bytes`; outgrown blocks are not touched) to `value`
 * (0..255), asynchronously on `stream`, and reports the block's size.  The stages take their temporary memory from
 * this arena and the pointer never leaves the library, so this is how a test lets a stage start on another stage's
 * residue.  MP_ERR_ARG, with the device untouched, for a NULL ctx, bytes < 0 or value outside 0..255. */
int mp_scratch_fill(mp_ctx *ctx, int64_t bytes, int value, int64_t *block_bytes /*host, may be NULL*/,
                    mp_stream stream);
/* Frames one fused-query / mp_recon_batch / mp_query_counted_batch call accepts (kMaxFrames). */
int mp_max_frames(void);

/* ---- SurfaceClassifier weights ------------------------------------------------------------ */
/* Replaces SurfaceClassifier.__init__ (heads/SurfaceClassifier.py:7-37) for the skip-concat
 * MLPs the reference instantiates: channels = {C+1,1024,512,256,128,Cout} with C in {256,512},
 * Cout in {1,3} (PIFuNetGMLP :74-79, PIFuNetCMLP :82-87).  Other shapes: MP_ERR_UNSUPPORTED. */
int mp_mlp_create(mp_ctx *ctx, int n_layers, const int *channels /*host, n_layers+1*/,
                  int last_op, int *mlp_out);
/* Loads filters.{layer}.{weight,bias} (state-dict layout, weight [out,in(,1)] row-major with the
 * K order [hidden | feature | z] of SurfaceClassifier.py:55) and re-packs it into MFMA fragment
 * order.  W and b are DEVICE pointers.  Replaces load_state_dict / load_legacy_pifu
 * (MonoPortNet.py:153-160).  Loading a layer FORGETS every skip table made with this head
 * (mp_skip_table below: a table holds products of the old weights); make them again afterwards. */
int mp_mlp_load(mp_ctx *ctx, int mlp, int layer, const float *W, const float *b, int out_ch,
                int in_ch, mp_stream stream);
int mp_mlp_destroy(mp_ctx *ctx, int mlp); /* synchronises the device before freeing */
/* Selects the arithmetic used by mp_query / mp_recon / mp_query_counted for this MLP.  Call after
 * every layer is loaded.  The f16 variants re-pack the weights ON THE STREAM OF THE LAST
 * mp_mlp_load (so the re-pack is ordered behind the loads), read max |W| of each layer back to
 * the host to choose the per-layer power-of-two operand scale, and drain that stream before
 * returning: SYNCHRONOUS, call it at set-up time. */
int mp_mlp_set_precision(mp_ctx *ctx, int mlp, int precision);

/* ---- feature-map layout ------------------------------------------------------------------ */
/* Copies src [Csrc,H,W] (the NCHW map MonoPortNet.filter emits, MonoPortNet.py:31-46) into
 * channels [c_offset, c_offset+Csrc) of the channels-last map dst [H,W,Cdst] the query kernels
 * read.  netC's cat([feat_prior, feat]) (MonoPortNet.py:44) is two calls into one dst. */
int mp_feat_pack_hwc(mp_ctx *ctx, const float *src_chw, int c_src, int h, int w, float *dst_hwc,
                     int c_dst, int c_offset, mp_stream stream);

/* Optional accelerator of the query of a netG head (C = 256; exact f32 and f16x3 kernels): the SKIP TABLE of a feature
 * map.  SurfaceClassifier (heads/SurfaceClassifier.py:39-71) multiplies weights with the SAMPLED
 * feature in every layer -- layer 0's 1024 x 256 block and the skip connections of layers 1-4 (:55)
 * -- and the sampled feature is a bilinear blend of four texels (geometry.py:4-16).  A linear map
 * commutes with that blend, so  table[y][x][r] = sum_c W[r][c] feat[y][x][c]  for those 1921 weight
 * rows (no bias, no z column; row layout: layers 0-3 at 0 / 1024 / 1536 / 1792, layer 4 at 1920,
 * padded to MP_SKIP_TABLE_ROWS) is computed ONCE per feature map here -- 16 GFLOP for a 128 x 128
 * map -- and the query of a point blends four rows of it instead of multiplying 492 k weights: 42 %
 * of the per-point MFMA work gone.  The result differs from the plain path by f32 rounding only
 * (1-3e-7 on the field, far inside the 1e-4 bar; tests/test_query_gpu.py::test_skip_table_*).
 * The call also REGISTERS the table for feat_hwc in the context: every later fused query launch
 * (mp_query*, mp_recon*) whose feature maps ALL have a registered table made with the same head
 * and map size uses it; others run the plain path.  The caller owns `table`
 * ([H, W, MP_SKIP_TABLE_ROWS] f32, 16-byte aligned -- 128-byte aligned keeps every 32-row block of a texel in
 * one cache line, which is what the row length of 61 x 32 floats is for; H * W a multiple of 64), must call mp_skip_table
 * again after it rewrites the feature map (stream-ordered with the queries, like any producer), and
 * mp_skip_table_release(ctx, feat_hwc, table) before freeing either buffer (table NULL: whatever is
 * registered for feat_hwc; otherwise only if it still is that table; feat_hwc NULL: everything).
 * mp_mlp_destroy and mp_mlp_load (new weights) drop the tables made with that head. */
#define MP_SKIP_TABLE_ROWS 1952
int mp_skip_table(mp_ctx *ctx, int mlp, const float *feat_hwc, int c, int h, int w, float *table,
                mp_stream stream);
/* The same for n_maps maps stored back to back ([n_maps, H, W, C] -> table [n_maps, H, W, MP_SKIP_TABLE_ROWS]):
 * one launch, one registration per map. */
int mp_skip_table_batch(mp_ctx *ctx, int mlp, int n_maps, const float *feat_hwc, int c, int h, int w,
                      float *table, mp_stream stream);
int mp_skip_table_release(mp_ctx *ctx, const float *feat_hwc, const float *table);

/* ---- per-point ops ------------------------------------------------------------------------- */
/* index(feat, uv) (geometry.py:4-16): bilinear grid_sample, align_corners=True, zero padding.
 * feat_hwc [H,W,C]; uv [2,N] in [-1,1]; out [C,N]. */
int mp_index(mp_ctx *ctx, const float *feat_hwc, int c, int h, int w, const float *uv, int64_t n,
             float *out, mp_stream stream);
/* orthogonal(points, calib) (geometry.py:19-34, transforms=None): out = R p + t.
 * points/out [3,N]; calib = row-major [>=3,4] matrix (rows 0-2 used, row stride 4). */
int mp_orthogonal(mp_ctx *ctx, const float *points, int64_t n, const float *calib, float *out,
                  mp_stream stream);
/* perspective(points, calib) (geometry.py:37-55, transforms=None): u, v, z = R p + t as in mp_orthogonal,
 * then out = (u / z, v / z, z) with IEEE divisions (+-inf / NaN where z == 0).  Layout as mp_orthogonal. */
int mp_perspective(mp_ctx *ctx, const float *points, int64_t n, const float *calib, float *out,
                   mp_stream stream);
/* MonoPortNet.query in eval mode, one feature stage (MonoPortNet.py:48-91):
 * project -> in-image mask -> z*z_scale -> bilinear sample -> skip-concat MLP -> mask.
 * points: element (c, i) at points[i*stride_n + c*stride_c] (so both the [3,N] layout netG.query
 * takes and the [N,3] one query_func receives, RTL/main.py:169-183, bind without a copy).
 * out [Cout,N]; out-of-image points are exactly 0.0f. */
int mp_query(mp_ctx *ctx, int mlp, const float *feat_hwc, int c, int h, int w,
             const float *points, int64_t n, int64_t stride_n, int64_t stride_c,
             const float *calib, float z_scale, float *out, mp_stream stream);

/* mp_query over n_frames (1..32) independent frames in ONE launch, n points each (MonoPortNet.query with
 * B > 1).  feat_hwc / points / calib / out are HOST arrays of n_frames device pointers, each as in mp_query
 * (one n and one stride convention for all); projection is a HOST array of n_frames MP_PROJ_* modes.  Each
 * frame takes its registered skip table under the same all-or-none rule as every fused launch: if EVERY
 * frame's map has one, the launch blends table rows.  A frame's result equals mp_query's bit for bit when
 * both take the same kernel. */
int mp_query_batch(mp_ctx *ctx, int mlp, int n_frames, const float *const *feat_hwc, int c, int h, int w,
                   const float *const *points, int64_t n, int64_t stride_n, int64_t stride_c,
                   const float *const *calib, const int *projection /*host*/, float z_scale,
                   float *const *out, mp_stream stream);

/* ---- multi-view queries (SurfaceClassifier num_views = V > 1, heads/SurfaceClassifier.py:60-66) ---- */
/* Views one mp_query_views / mp_mlp_forward_views call accepts. */
#define MP_MAX_VIEWS 8

/* MonoPortNet.query with a multi-view head (multi-view PIFu): the same n points seen by n_views (1..MP_MAX_VIEWS)
 * calibrated cameras.  Row v of the reference's [V,Cout,N] result: view v projects the points with calib[v]
 * (one MP_PROJ_* `projection` for all views) and samples feat_hwc[v]; layers 0-2 run per view; after layer 2
 * the hidden rows and the features (z_feat included) are averaged over the views; layers 3-4 run once on the
 * means, and out[v] [Cout,N] is that prediction times view v's in-image mask (MonoPortNet.py:89).  A finite
 * view outside its image still feeds the mean with grid_sample's zero-padded samples; a view with a non-finite
 * projection (perspective, z == 0) makes the point NaN in every row.  feat_hwc / points / calib / out are HOST
 * arrays of n_views device pointers, each as in mp_query.  The f32 kernel only (query_views.hip): a head whose
 * precision is not MP_PREC_F32 returns MP_ERR_UNSUPPORTED, as does n_views outside 1..MP_MAX_VIEWS.  Registered
 * skip tables are not used; with n_views = 1 the result equals mp_query's on the plain kernels bit for bit. */
int mp_query_views(mp_ctx *ctx, int mlp, int n_views, const float *const *feat_hwc, int c, int h, int w,
                   const float *const *points, int64_t n, int64_t stride_n, int64_t stride_c,
                   const float *const *calib, int projection, float z_scale, float *const *out,
                   mp_stream stream);

/* SurfaceClassifier.forward of a multi-view head on explicit features of ONE point set: feature
 * [n_views][C+1][N] (row v*(C+1) + c, contiguous) -> out [Cout,N], the view means taken after layer 2 as in
 * mp_query_views (no mask).  As in mp_query_views, n_views outside 1..MP_MAX_VIEWS or a head whose precision is not
 * MP_PREC_F32 (at any n_views) returns MP_ERR_UNSUPPORTED.  With n_views = 1 the result is mp_mlp_forward's. */
int mp_mlp_forward_views(mp_ctx *ctx, int mlp, int n_views, const float *feature, int64_t n, float *out,
                         mp_stream stream);

/* SurfaceClassifier.forward on explicit features (heads/SurfaceClassifier.py:39-71; the shape of
 * the reference's own micro-benchmark, :95-116): feature [C+1,N] (sampled features + z_feat as
 * the last row, MonoPortNet.py:82-83) -> out [Cout,N] with the last_op applied. */
int mp_mlp_forward(mp_ctx *ctx, int mlp, const float *feature, int64_t n, float *out,
                   mp_stream stream);

/* Same, with the point count read from device memory at run time (netC.query over the vertices
 * forward_vertices found, RTL/main.py:239-242, without a host round trip).  points [3,capacity],
 * out [Cout,capacity]; only the first *count columns are read / written. */
int mp_query_counted(mp_ctx *ctx, int mlp, const float *feat_hwc, int c, int h, int w,
                     const float *points, int64_t capacity, const int32_t *count,
                     const float *calib, float z_scale, float *out, mp_stream stream);

/* mp_query_counted over n_frames (1..32) independent frames in ONE launch (the per-vertex colour
 * queries of all frames of a pipeline slot: ~14 k points each cannot fill 256 CUs alone).
 * feat_hwc / points / count / calib / out are HOST arrays of n_frames device pointers, each as in
 * mp_query_counted (one `capacity` for all); results are identical to n_frames separate calls. */
int mp_query_counted_batch(mp_ctx *ctx, int mlp, int n_frames, const float *const *feat_hwc, int c,
                           int h, int w, const float *const *points, int64_t capacity,
                           const int32_t *const *count, const float *const *calib, float z_scale,
                           float *const *out, mp_stream stream);
/* mp_query_counted_batch with a per-frame projection: projection is a HOST array of n_frames MP_PROJ_*
 * modes (NULL = every frame orthogonal, which is mp_query_counted_batch). */
int mp_query_counted_batch_proj(mp_ctx *ctx, int mlp, int n_frames, const float *const *feat_hwc, int c,
                                int h, int w, const float *const *points, int64_t capacity,
                                const int32_t *const *count, const float *const *calib,
                                const int *projection /*host*/, float z_scale, float *const *out,
                                mp_stream stream);

/* ---- coarse-to-fine reconstruction --------------------------------------------------------- */
/* Replaces implicit_seg.functional.Seg3dLossless.forward(faster=True) driving query_func
 * (RTL/main.py:185-195, :392-394; un-vendored dependency, requirements.txt:15).
 * resolutions (host) must satisfy r[i+1] = 2 r[i] - 1, r <= 1023.  volume [R,R,R] (z,y,x) f32
 * with R = resolutions[n_levels-1].  status (device, int32[1+n_levels]): status[0] = 1 if the
 * coarsest level has any value > balance (0 -> the reference returns None and `volume` is
 * unspecified), status[1+l] = points queried at level l.  Fully asynchronous. */
int mp_recon(mp_ctx *ctx, int mlp, const float *feat_hwc, int c, int h, int w, const float *calib,
             float z_scale, const float *b_min /*host[3]*/, const float *b_max /*host[3]*/,
             const int *resolutions /*host*/, int n_levels, float balance, float *volume,
             int32_t *status, mp_stream stream);

/* mp_recon over n_frames (1..32) independent frames sharing the MLP, box and resolutions: every
 * octree level evaluates the selected nodes of ALL frames in one fused-query launch, so the coarse
 * levels (5-25 k nodes per frame) fill the 256 CUs together.  feat_hwc / calib / volume / status
 * are HOST arrays of n_frames device pointers, each as in mp_recon; results are identical to
 * n_frames mp_recon calls. */
int mp_recon_batch(mp_ctx *ctx, int mlp, int n_frames, const float *const *feat_hwc, int c, int h,
                   int w, const float *const *calib, float z_scale, const float *b_min,
                   const float *b_max, const int *resolutions, int n_levels, float balance,
                   float *const *volume, int32_t *const *status, mp_stream stream);

/* mp_recon_batch with the selection rule of the LAST level as an argument.  The un-vendored upstream
 * engine (implicit_seg, RTL/main.py:188-195 constructs it with faster=True) is recalled to treat its last
 * level differently from the others; nothing under the reference pins it, so the
 * rule is the caller's choice:
 *   MP_FINAL_DILATE3      boundary nodes (0 < upsampled mask < 1) dilated by 3^3, as at levels >= 3: the
 *                         lossless schedule -- thresholded volume == thresholded dense evaluation on
 *                         ordinary bodies.  mp_recon / mp_recon_batch use it.
 *   MP_FINAL_UPSTREAM     only nodes whose upsampled mask is EXACTLY 0.5 (`is_boundary = valid == 0.5`,
 *                         no dilation): ~4x fewer points at the last level; ~0.4 % of the inside voxels
 *                         differ from dense evaluation (tests/test_recon_gpu.py::test_final_level_*).
 *   MP_FINAL_INTERPOLATE  nothing is evaluated at the last level ("last step no examine"): the volume is
 *                         the trilinear upsample of the level before; status[n_levels] = 0. */
enum { MP_FINAL_DILATE3 = 0, MP_FINAL_UPSTREAM = 1, MP_FINAL_INTERPOLATE = 2 };
int mp_recon_batch_ex(mp_ctx *ctx, int mlp, int n_frames, const float *const *feat_hwc, int c, int h,
                      int w, const float *const *calib, float z_scale, const float *b_min,
                      const float *b_max, const int *resolutions, int n_levels, float balance,
                      int final_level, float *const *volume, int32_t *const *status, mp_stream stream);

/* mp_recon_batch_ex with an EARLY hand-over (round 6).  The reference's engine returns None for a frame whose
 * coarsest level is empty (RTL/recon.py:32-33) and our drop-in class must know whether the caller's query_func is
 * the plain netG.query the fused kernels implement -- both facts are known after the coarsest level, ~0.1 ms into
 * a ~3.5 ms call.  With `early`, right after that level the call
 *   - compares frame f's coarsest-level values with expect_level0[f] (device, res[0]^3 floats in (z,y,x) order:
 *     what query_func returned for those nodes; NULL entry or NULL array = no comparison),
 *   - writes flags_dev[2f] = status[f][0] and flags_dev[2f+1] = 1 if any value differs (float !=, a NaN agrees with a NaN),
 *   - copies the 2*n_frames flags to flags_host (PINNED host memory) and records `event` (a hipEvent_t, may be
 *     NULL) on `stream`, then enqueues the remaining levels.
 * A stage thread waits for `event`, reads two integers and hands the volume on while the GPU is still refining
 * it; the per-level counts in `status` are complete when the stream is.  Results are those of mp_recon_batch_ex. */
typedef struct mp_recon_early {
  const float *const *expect_level0;
  int32_t *flags_dev;  /* device int32[2 * n_frames] */
  int32_t *flags_host; /* pinned host int32[2 * n_frames] */
  void *event;
} mp_recon_early;
int mp_recon_batch_early(mp_ctx *ctx, int mlp, int n_frames, const float *const *feat_hwc, int c, int h,
                         int w, const float *const *calib, float z_scale, const float *b_min,
                         const float *b_max, const int *resolutions, int n_levels, float balance,
                         int final_level, float *const *volume, int32_t *const *status,
                         const mp_recon_early *early, mp_stream stream);
/* mp_recon_batch_early with a per-frame projection: projection is a HOST array of n_frames MP_PROJ_* modes
 * (NULL = every frame orthogonal, which is mp_recon_batch_early); early may be NULL (mp_recon_batch_ex).
 * Nodes of a perspective frame with z == 0 take the value NaN, which no threshold selects. */
int mp_recon_batch_proj(mp_ctx *ctx, int mlp, int n_frames, const float *const *feat_hwc, int c, int h,
                        int w, const float *const *calib, const int *projection /*host*/, float z_scale,
                        const float *b_min, const float *b_max, const int *resolutions, int n_levels,
                        float balance, int final_level, float *const *volume, int32_t *const *status,
                        const mp_recon_early *early, mp_stream stream);

/* mp_recon for a multi-view head (multi-view PIFu, SurfaceClassifier num_views = n_views): the occupancy volume of
 * ONE subject seen by n_views (1..MP_MAX_VIEWS) cameras, as one call.  Every octree level evaluates its nodes with
 * the multi-view kernel of mp_query_views reading the level's packed node list directly (no point tensor exists) and
 * writes row `view` (0..n_views-1) of the reference's [n_views,1,N] result -- the view-averaged prediction times
 * view `view`'s in-image mask (MonoPortNet.py:89) -- straight into the level's volume; the other rows are never
 * made.  feat_hwc / calib: HOST arrays of n_views device pointers as in mp_query_views (maps [h,w,c], 16-byte
 * aligned; 4x4 calibrations); projection: ONE MP_PROJ_* mode for all views (a node whose perspective projection
 * is non-finite in ANY view takes the value NaN).  b_min .. final_level, volume and status as in
 * mp_recon_batch_proj with one frame; early (may be NULL) likewise: expect_level0[0] and two flags.  Fully
 * asynchronous.  n_views outside 1..MP_MAX_VIEWS or a head whose precision is not MP_PREC_F32 returns
 * MP_ERR_UNSUPPORTED; `view` outside 0..n_views-1, a null or misaligned buffer, or resolutions that break
 * r[i+1] = 2 r[i] - 1 return MP_ERR_ARG.  Registered skip tables are not used; with n_views = 1 the volume and
 * status equal mp_recon's on the plain kernels (no table registered for the map) bit for bit. */
int mp_recon_views(mp_ctx *ctx, int mlp, int n_views, const float *const *feat_hwc, int c, int h, int w,
                   const float *const *calib, int projection, float z_scale,
                   const float *b_min, const float *b_max, const int *resolutions, int n_levels,
                   float balance, int final_level, int view, float *volume, int32_t *status,
                   const mp_recon_early *early, mp_stream stream);

/* mp_recon_views over n_frames independent subjects that share the head, n_views, `view`, the projection mode, the
 * box and the resolutions: every octree level evaluates the selected nodes of ALL frames in one launch of the
 * multi-view kernel (the tiles of the frames form one index space, as in mp_recon_batch), so the coarse levels of a
 * capture rig's frames fill the machine together.  feat_hwc / calib: HOST arrays of n_frames * n_views device
 * pointers, frame-major ([f * n_views + v]); volume / status: HOST arrays of n_frames device pointers, each as in
 * mp_recon_views; early (may be NULL): n_frames entries of expect_level0 and 2 * n_frames flags, as in
 * mp_recon_batch_early.  Frame f's volume and status equal mp_recon_views on frame f's inputs bit for bit; a frame
 * whose coarsest level is empty has status[f][0] == 0, an unspecified volume and zero finer counts, and touches
 * nothing of the other frames.  Fully asynchronous.  Refusals as in mp_recon_views; in addition n_frames outside
 * 1..mp_max_frames() or n_frames * n_views > MP_MAX_FRAME_VIEWS (mp_max_frame_views(): what the kernel's argument
 * block holds) returns MP_ERR_ARG.  A refused call launches nothing and leaves the context usable. */
#define MP_MAX_FRAME_VIEWS 64
int mp_max_frame_views(void);
int mp_recon_views_batch(mp_ctx *ctx, int mlp, int n_frames, int n_views, const float *const *feat_hwc, int c, int h,
                         int w, const float *const *calib, int projection, float z_scale, const float *b_min,
                         const float *b_max, const int *resolutions, int n_levels, float balance, int final_level,
                         int view, float *const *volume, int32_t *const *status, const mp_recon_early *early,
                         mp_stream stream);

/* mp_query_views over n_frames independent subjects whose point counts live on the device (multi-view netC colours
 * over the vertex lists forward_vertices / marching cubes counted, without a host round trip): frame f has its own
 * n_views maps and calibrations (feat_hwc / calib: HOST arrays of n_frames * n_views device pointers, frame-major
 * [f * n_views + v]) and ONE point set points[f] [3,capacity] (contiguous f32) that all its views see; the frames
 * share the head, n_views, `view`, the projection mode and `capacity`.  For i < *count[f] (clamped to
 * [0, capacity] in the kernel; the contract is count <= capacity, as for mp_query_counted), out[f][:, i] of the
 * [Cout,capacity] output equals row `view` of mp_query_views on frame f's maps and calibrations with the same points
 * given to every view, bit for bit; everything else of `out` is untouched.  One launch: the tiles of the frames form
 * one index space and a frame whose count is 0 owns none.  Fully asynchronous, no host sync; registered skip tables
 * are not used.  n_views outside 1..MP_MAX_VIEWS, a head whose precision is not MP_PREC_F32 or whose (C, Cout) is
 * outside {256,512} x {1,3} returns MP_ERR_UNSUPPORTED; n_frames outside 1..mp_max_frames(), n_frames * n_views >
 * MP_MAX_FRAME_VIEWS, `view` outside 0..n_views-1, a bad projection or a null or misaligned buffer returns
 * MP_ERR_ARG; capacity == 0 returns MP_OK before the frames' buffers are looked at.  A refused call launches nothing
 * and leaves the context usable. */
int mp_query_views_counted_batch(mp_ctx *ctx, int mlp, int n_frames, int n_views, const float *const *feat_hwc, int c,
                                 int h, int w, const float *const *points, int64_t capacity,
                                 const int32_t *const *count, const float *const *calib, int projection,
                                 float z_scale, int view, float *const *out, mp_stream stream);

/* The same engine one level at a time, for an arbitrary Python ``query_func`` (the general
 * Seg3dLossless contract, RTL/main.py:169-195): the caller evaluates the selected nodes itself.
 *   mp_octree_select: level 0 (prev == NULL) selects every node; otherwise upsamples prev [rp^3]
 *     into cur [r^3] (r = 2 rp - 1), flags boundary nodes, dilates by the level's box, drops nodes
 *     evaluated earlier.  ev_prev / ev_cur / bnd are u64 bitsets of r*r*ceil(r/64) words (rp for
 *     ev_prev); packed (u32 [r^3]) receives x | y<<10 | z<<20, count (device int32) their number.
 *   mp_lattice_points: packed nodes -> world points [capacity,3] (row i = x,y,z of node i).
 *   mp_scatter_nodes: volume[z,y,x] = values[i] for the first *count nodes. */
int mp_octree_select(mp_ctx *ctx, const float *prev, int rp, float *cur, int r,
                     const uint64_t *ev_prev, uint64_t *ev_cur, uint64_t *bnd, int level,
                     float balance, uint32_t *packed, int32_t *count, mp_stream stream);
/* mp_octree_select with an explicit dilation box (3, 7 or 9) instead of the faster-mode schedule
 * 9 / 7 / 3 by level: the upstream engine's faster=False mode dilates by 3^3 at every level.
 * box 1: the MP_FINAL_UPSTREAM rule (nodes whose upsampled mask is exactly 0.5, undilated);
 * box 0: the MP_FINAL_INTERPOLATE rule (upsample only, *count = 0). */
int mp_octree_select_box(mp_ctx *ctx, const float *prev, int rp, float *cur, int r,
                         const uint64_t *ev_prev, uint64_t *ev_cur, uint64_t *bnd, int box,
                         float balance, uint32_t *packed, int32_t *count, mp_stream stream);
/* FIXED-BUDGET refinement (the upstream package's Seg3dTopk; un-vendored and unpinned like Seg3dLossless, so the
 * definition is stated here and restated in numpy in tests/topk_ref.py, which the kernels match bit for bit).
 * Resolutions obey r[l+1] = 2 r[l] - 1.  num_points[l] is the budget of level l; entry 0 is ignored: level 0
 * evaluates every node, exactly as mp_recon does.  max_dist[l] is an optional bound (+inf, or a NULL array, for none).
 * status[0] is 0 or 1 as in mp_recon and status[1+l] the number of points queried at level l.
 * Each level l >= 1, with r = r[l] and k = num_points[l]:
 *   1. cur = upsample2x(prev): the same bits as mp_octree_select_box with box 0;
 *   2. u(v) = fabsf(cur[v] - balance) in f32;
 *   3. a node is a CANDIDATE if it is not in the evaluated set (the even-coordinate image of the previous level's
 *      set), u is not NaN and u <= max_dist[l];
 *   4. selected are the min(k, #candidates) candidates smallest under the key (u, z r^2 + y r + x) compared
 *      lexicographically: ties in u go to the smaller linear index, whatever order the list is emitted in;
 *   5. the selected nodes are evaluated, scattered into cur and added to the evaluated set; status[1+l] = their count;
 *   6. k == 0: the level is only upsampled (count 0, no query launch).
 * A frame whose level 0 has nothing > balance (status[0] == 0) selects nothing at any level: all its counts are 0 and
 * its volume is unspecified, as in mp_recon.  The ORDER of `packed` is unspecified; the selected set and the volume
 * are a pure function of the inputs (integer atomics only: the same bits in every run).  Upstream's names:
 * uncertainty = -|occ - balance|, and clip_min keeps uncertainty >= clip_min, so max_dist = -clip_min.
 *
 * mp_octree_select_topk: one level (steps 1-4 and the evaluated set of step 5) for the level-at-a-time engine; the
 * caller evaluates `packed` and calls mp_scatter_nodes.  prev must not be NULL (level 0 stays mp_octree_select);
 * ev_prev / ev_cur / packed as in mp_octree_select, *count is written on the device.  MP_ERR_ARG: k < 0 or k > r^3,
 * a NaN or negative max_dist, a NULL or misaligned buffer, r != 2 rp - 1. */
int mp_octree_select_topk(mp_ctx *ctx, const float *prev, int rp, float *cur, int r, const uint64_t *ev_prev,
                          uint64_t *ev_cur, int64_t k, float max_dist, float balance, uint32_t *packed, int32_t *count,
                          mp_stream stream);
/* The fused call: mp_recon_batch_proj with the selection above instead of the lossless rule, 1..mp_max_frames()
 * frames; every level's nodes of all frames go through one query launch whose grid is sized by the budget
 * (num_points[l] * n_frames), not by r^3.  num_points: HOST int64[n_levels]; max_dist: HOST float[n_levels] or NULL;
 * every other argument as in mp_recon_batch_proj.  Fully asynchronous.  MP_ERR_ARG: num_points[l] < 0 or > r[l]^3
 * (l >= 1), a NaN or negative max_dist[l], NULL or misaligned buffers, resolutions that break r[l+1] = 2 r[l] - 1,
 * n_frames outside 1..mp_max_frames(). */
int mp_recon_topk_batch(mp_ctx *ctx, int mlp, int n_frames, const float *const *feat_hwc, int c, int h, int w,
                        const float *const *calib, const int *projection /*host, may be NULL*/, float z_scale,
                        const float *b_min, const float *b_max, const int *resolutions, int n_levels,
                        const int64_t *num_points /*host*/, const float *max_dist /*host, may be NULL*/, float balance,
                        float *const *volume, int32_t *const *status, const mp_recon_early *early, mp_stream stream);
/* Conflict re-examination of the upstream engine's faster=False mode.  For each of the first
 * *count nodes of `packed` (just evaluated: values[i]; volume [r^3] still holds the value
 * INTERPOLATED from the coarser level at that node): if (interp - balance) * (value - balance) < 0
 * every node of its 3x3x3 neighbourhood that is not yet in the evaluated bitset `ev` is claimed
 * (bit set atomically) and appended to out_packed (capacity r^3; order unspecified); *out_count
 * = their number.  Call mp_scatter_nodes for `packed` afterwards, then evaluate out_packed and
 * repeat until *out_count is 0. */
int mp_octree_conflicts(mp_ctx *ctx, const uint32_t *packed, const int32_t *count, int64_t capacity,
                        int r, const float *values, const float *volume, float balance,
                        uint64_t *ev, uint32_t *out_packed, int32_t *out_count, mp_stream stream);
int mp_lattice_points(mp_ctx *ctx, const uint32_t *packed, const int32_t *count, int64_t capacity,
                      int stride, int res_final, const float *b_min /*host[3]*/,
                      const float *b_max /*host[3]*/, float *points, mp_stream stream);
int mp_scatter_nodes(mp_ctx *ctx, const uint32_t *packed, const int32_t *count, int64_t capacity,
                     int r, const float *values, float *volume, mp_stream stream);
/* The ordering step mp_recon_batch* runs between a level's selection and its query (levels of 65 nodes per axis and
 * more; not for mp_recon_views, mp_recon_topk_batch or the mp_octree_select* entries, whose lists stay as selected):
 * each frame's list packed[f][0 .. *count[f]) of a level of level_res nodes per axis is sorted IN PLACE by the texel
 * cell its points sample in an h x w map -- y0 * w + x0 of the first bilinear tap of the point that `stride`,
 * res_final, b_min, b_max (as mp_lattice_points), calib[f] and projection[f] (NULL: all orthogonal) give, computed
 * exactly as the query kernels compute it; points outside the image come last.  The order of points of one cell is
 * unspecified and may differ from call to call.  *count[f] and the entries past it are not written.  A frame with
 * more than level_res^3 / 8 points is left as it is.  Nothing is synchronised; 1..32 frames. */
int mp_octree_order_points(mp_ctx *ctx, int n_frames, uint32_t *const *packed /*host[n] of device*/,
                           const int32_t *const *count /*host[n] of device int32*/,
                           const float *const *calib /*host[n] of device [3,4]*/,
                           const int *projection /*host[n] of MP_PROJ_*, may be NULL*/, int level_res, int stride,
                           int res_final, const float *b_min /*host[3]*/, const float *b_max /*host[3]*/, int h, int w,
                           mp_stream stream);

/* ---- per-frame and batched forms of the mesh and render calls -------------------------------------------------------
 * mp_forward_vertices, mp_paint, mp_marching_cubes, mp_mesh_simplify, mp_mesh_smooth, mp_mesh_normals, mp_mesh_points,
 * mp_mesh_render and mp_volume_keep_largest are
 * each the batched call with one frame: mp_<call>(..., p, ...) is mp_<call>_batch(..., 1, &p, ..., gate = NULL), with
 * the same argument tests, scratch and launches; only the name at the head of an mp_last_error message is that of the
 * entry called.  The rules of the batched calls are therefore the rules of both forms:
 *   - a device pointer that is read and is not 4-byte aligned is refused with MP_ERR_ARG ("misaligned buffer for
 *     frame f"), a NULL one with MP_ERR_ARG ("null buffer for frame f"); nothing is launched.  (The per-frame calls
 *     used to pass a misaligned pointer on, and neither form of mp_forward_vertices / mp_paint tested alignment.)
 *   - mp_mesh_normals with max_verts == 0 returns MP_OK without a launch (it used to launch).
 *   - mp_volume_keep_largest's refusals name mp_volume_keep_largest (they used to name the _batch entry).
 *   - rows of a capacity of 0 (verts / faces / normals / points) are not looked at and may be NULL. */

/* ---- visible-surface extraction ------------------------------------------------------------ */
/* forward_vertices (RTL/recon.py:27-89).  volume [R,R,R]; outputs sized for R*R rows:
 * X, Y int64 [R*R]; Z f32 [R*R]; norm f32 [R*R,3]; count (device int32[1]) = rows written,
 * in the reference's row order (x-major, RTL/recon.py:62).  The batched call with one frame. */
int mp_forward_vertices(mp_ctx *ctx, const float *volume, int r, int direction, int64_t *x,
                        int64_t *y, float *z, float *norm, int32_t *count, mp_stream stream);

/* mp_forward_vertices over n_frames (1..32) volumes of one size in ONE set of launches (the vertex extraction of a
 * single 257^3 volume is three launches of 65-2300 workgroups: launch-bound).  volume / x / y / z / norm / count are
 * HOST arrays of n_frames device pointers, each as in mp_forward_vertices; results are identical to n_frames calls. */
int mp_forward_vertices_batch(mp_ctx *ctx, int n_frames, const float *const *volume, int r, int direction,
                              int64_t *const *x, int64_t *const *y, float *const *z, float *const *norm,
                              int32_t *const *count, mp_stream stream);

/* ---- colorization (RTL/main.py:212-249) ---------------------------------------------------- */
/* verts = (X, Y, res - Z) mapped through the voxel->world matrix `mat` (host, row-major 4x4,
 * RTL/main.py:204-210, :231-237) -> points [3,N] for netC.query.  `count` (device int32) gives N
 * (<= capacity); rows beyond it are left untouched. */
int mp_vertex_points(mp_ctx *ctx, const int64_t *x, const int64_t *y, const float *z,
                     const int32_t *count, int64_t capacity, int res, const float *mat,
                     float *points, mp_stream stream);
/* image [res,res,3] = 1.0 then image[X[i],Y[i],:] = clamp(values[:,i]*scale + bias, lo, hi);
 * values is [3,capacity] when channel_major != 0 (netC preds, main.py:244-248: scale=bias=0.5)
 * or [capacity,3] otherwise (normals, main.py:220-225: scale=bias=0.5, clamp 0..1).  The batched call with one
 * frame. */
int mp_paint(mp_ctx *ctx, const int64_t *x, const int64_t *y, const float *values,
             int channel_major, const int32_t *count, int64_t capacity, int res, float scale,
             float bias, float lo, float hi, float *image, mp_stream stream);

/* mp_paint over n_frames (1..32) renders of one size in two launches; x / y / values / count / image are HOST arrays
 * of n_frames device pointers, each as in mp_paint (one `capacity` for all). */
int mp_paint_batch(mp_ctx *ctx, int n_frames, const int64_t *const *x, const int64_t *const *y,
                   const float *const *values, int channel_major, const int32_t *const *count, int64_t capacity,
                   int res, float scale, float bias, float lo, float hi, float *const *image, mp_stream stream);

/* visulization (sic, RTL/main.py:252-281) for one render: out[i,j,:] = 255 * image[rot90, nearest
 * resized res -> size]; image [res,res,3] f32 in [0,1], out [size,size,3] f32, mask [size,size]
 * uint8 = 0 where all three channels are exactly 255 (the white background), else 1. */
int mp_visualize(mp_ctx *ctx, const float *image, int res, int size, float *out, uint8_t *mask,
                 mp_stream stream);

/* Background removal + normalisation in front of the encoders (RTL/main.py:352-364): segm is the
 * segmentation engine's [4,H,W] output (RGB in [-1,1], then the soft mask);
 *   input_g[c] = (((segm[c] * 0.5 + 0.5) - mean[c]) / std[c]) * segm[3]     (netG input)
 *   input_c[c] = segm[c] * segm[3]                                          (netC input, may be NULL)
 * in exactly this operation order (bit-identical to the reference's chain of torch ops).
 * mean / std: host float[3] (cfg.netG.mean / .std, RTL/main.py:288-289). */
int mp_prepare_inputs(mp_ctx *ctx, const float *segm, int64_t hw, const float *mean,
                      const float *std, float *input_g, float *input_c, mp_stream stream);

/* ---- triangle mesh (north star; no counterpart in the reference) ----------------- */
/* Marching cubes of volume [R,R,R] at `level` (inside = value > level) with the face-consistent
 * case table of tools/gen_mc_tables.py.  One welded vertex per crossing lattice edge, in edge-id
 * order ((z*R+y)*R+x)*3 + axis, positioned at the linear crossing and mapped to world space like
 * the octree lattice; triangles in cell order, wound counter-clockwise seen from the outside.
 * verts f32 [max_verts,3], faces int32 [max_faces,3]; counts (device int32[2]) = vertices and
 * faces NEEDED (compare with the capacities to detect truncation).  The batched call with one frame
 * and no gate. */
int mp_marching_cubes(mp_ctx *ctx, const float *volume, int r, float level,
                      const float *b_min /*host[3]*/, const float *b_max /*host[3]*/, float *verts,
                      int64_t max_verts, int32_t *faces, int64_t max_faces, int32_t *counts,
                      mp_stream stream);

/* Per-vertex normals of a triangle mesh: compute_normal (monoport/lib/mesh_util.py:201-220).  Each face has the
 * unit normal n = normalize_v3(cross(v1 - v0, v2 - v0)) (normalize_v3: length clamped from below at 1e-8, so a
 * zero-area face has n = 0); a vertex's normal is normalize_v3 of a sum of its faces' n, added in f32 to +0:
 *   MP_NORMALS_REFERENCE   what the reference computes, bit for bit on f32 vertices: its `norm[faces[:,c]] += n`
 *                          does not accumulate over repeated indices, so for each corner c = 0, 1, 2 (in this order)
 *                          only the LAST face (highest index) that has the vertex at corner c is added;
 *   MP_NORMALS_ACCUMULATE  what its comments describe: every incident (face, corner) is added, in ascending
 *                          (face index, corner) order (numpy's np.add.at), bit for bit and independent of the run.
 * A vertex no face references gets (0, 0, 0). */
enum { MP_NORMALS_REFERENCE = 0, MP_NORMALS_ACCUMULATE = 1 };
/* verts f32 [max_verts,3], faces int32 [max_faces,3]; counts (device int32[2]) = vertices and faces present, as
 * mp_marching_cubes writes them: only min(counts[0], max_verts) vertices and min(counts[1], max_faces) faces are
 * read / written (rows of `normals` beyond them are left untouched).  normals f32 [max_verts,3].  A face with an
 * index outside [0, vertices) is skipped (never read out of bounds).  Asynchronous; no float atomics.  The batched
 * call with one frame: a pointer that is not 4-byte aligned is MP_ERR_ARG, max_verts == 0 is MP_OK without a launch. */
int mp_mesh_normals(mp_ctx *ctx, const float *verts, int64_t max_verts, const int32_t *faces, int64_t max_faces,
                    const int32_t *counts, int mode, float *normals, mp_stream stream);
/* verts [max_verts,3] -> points [3,max_verts] (the layout mp_query_counted reads, capacity = max_verts) for the
 * first min(counts[0], max_verts) vertices, and count_out (device int32[1]) = that number: the per-vertex colour
 * query of a marching-cubes mesh without a host round trip.  The batched call with one frame. */
int mp_mesh_points(mp_ctx *ctx, const float *verts, int64_t max_verts, const int32_t *counts, float *points,
                   int32_t *count_out, mp_stream stream);

/* The three calls above over n_frames (1..mp_max_frames(), else MP_ERR_ARG) meshes in ONE set of launches each: four
 * for marching cubes, three (reference) or six (accumulate, memsets included) for the normals, one for the points --
 * the numbers of a single mesh.  volume / verts / faces / counts / gate / normals / points / count_out are HOST
 * arrays of n_frames device pointers, each as in the per-mesh call; all volumes have resolution r, and ONE capacity
 * (max_verts, max_faces) serves all frames.
 *   Frame f's outputs equal those of the per-mesh call (mp_marching_cubes, mp_mesh_normals, mp_mesh_points) on frame
 * f's inputs BIT FOR BIT, truncation included: counts[f] holds the vertices and faces needed, only the capacities
 * are written, faces that name a vertex outside [0, vertices) are skipped by the normals, and rows beyond a frame's
 * counts are left untouched.  All per-frame sizes are read from that frame's device counts; no float atomics.
 *   gate (mp_marching_cubes_batch; NULL, or entries NULL = frame on): gate[f] is a device int32; if it reads 0, frame
 * f's counts become {0, 0} and nothing else of that frame is read or written (its volume may hold anything: the
 * unspecified volume of an mp_recon_batch frame whose status[0] is 0) -- the normals / points calls then see a zero
 * count and leave that frame alone.
 *   Scratch comes from the stream's arena: n_frames * (4 r^3 + 8 ceil(r^3 / 1024) + 1024) bytes for marching cubes
 * (68 MB per frame at 257^3), n_frames * (24 max_faces + 12 max_verts + 4) + 256 bytes for the normals, none for the
 * points.  Refusals as in the per-mesh calls, each with an mp_last_error message: r^3 >= 2^31 and capacities beyond
 * 2^31 / 3 (MP_ERR_UNSUPPORTED), a null or not 4-byte aligned buffer of any frame (MP_ERR_ARG).  Asynchronous. */
int mp_marching_cubes_batch(mp_ctx *ctx, int n_frames, const float *const *volume, int r, float level,
                            const float *b_min /*host[3]*/, const float *b_max /*host[3]*/, float *const *verts,
                            int64_t max_verts, int32_t *const *faces, int64_t max_faces, int32_t *const *counts,
                            const int32_t *const *gate, mp_stream stream);
int mp_mesh_normals_batch(mp_ctx *ctx, int n_frames, const float *const *verts, int64_t max_verts,
                          const int32_t *const *faces, int64_t max_faces, const int32_t *const *counts, int mode,
                          float *const *normals, mp_stream stream);
int mp_mesh_points_batch(mp_ctx *ctx, int n_frames, const float *const *verts, int64_t max_verts,
                         const int32_t *const *counts, float *const *points, int32_t *const *count_out,
                         mp_stream stream);

/* ---- mesh simplification (no counterpart in the reference): the level-of-detail dial of the mesh chain -------------
 * Vertex clustering of a triangle mesh as mp_marching_cubes leaves it, between marching cubes and the normals /
 * colours.  Defined bit for bit (integer atomics only: the result is a pure function of its inputs, the same bits in
 * every run).  Per mesh: verts f32 [max_verts,3], faces int32 [max_faces,3], counts (device int32[2]; only nv =
 * min(counts[0], max_verts) vertices and nf = min(counts[1], max_faces) faces are read), a box b_min / b_max (HOST
 * float[3]) and n, the cells per axis (the same for x, y and z).
 *   1 Cell.  Per axis a, on the host in f32: inv_a = (float)n / (b_max_a - b_min_a).  On the device, in f32 and in this
 *     order: t_a = (v_a - b_min_a) * inv_a; c_a = clamp((int)floorf(t_a), 0, n - 1) (the clamp holds for every t, +-inf
 *     included: a vertex outside the box belongs to the border cell); key = (c_z * n + c_y) * n + c_x.  A vertex is
 *     invalid if a coordinate is not finite or |v_a| >= 32768; it joins no cell.
 *   2 New vertices: one per occupied cell, in ascending key order.  vmap[v] = new index of old vertex v, -1 for an
 *     invalid one; rows of vmap at or beyond nv are left untouched.
 *   3 Position: the members' mean in fixed point.  Q_a = llrint((double)v_a * 1048576.0) (ties to even), S_a = the
 *     int64 sum of Q_a over the members, m = their number, out_a = (float)((double)S_a / ((double)m * 1048576.0)):
 *     both int64 -> double conversions round to nearest-even, the division is IEEE.  With max_verts <= 2^27 the sum
 *     cannot overflow; a larger max_verts is MP_ERR_UNSUPPORTED.
 *   4 Faces.  A face with an index outside [0, nv) or with an invalid vertex is dropped; the others are mapped through
 *     vmap, and a face with two equal mapped indices is dropped.  Survivors keep their input order and their corner
 *     order (the winding is kept).  Two faces that land on the same three vertices BOTH stay: removing such pairs is
 *     not part of this call (every undirected edge of a closed input then still lies in an even number of faces).  An
 *     output vertex that no surviving face names stays (n = 1: one vertex, no faces; mp_mesh_normals gives it 0).
 *   5 Outputs: verts_out f32 [max_verts,3] and faces_out int32 [max_faces,3] (the capacities of the inputs: the output
 *     is never larger, nothing truncates here), counts_out (device int32[2]) = new vertices and faces, vmap int32
 *     [max_verts] or NULL.  Rows beyond the new counts are left untouched.  Outputs must not alias inputs (MP_ERR_ARG).
 *     counts reading {0, 0} (a gated-off frame of mp_marching_cubes_batch) gives counts_out = {0, 0} and touches
 *     nothing else.
 *   Nine launches and one memset (simplify.hip), asynchronous, nothing synchronised.  Scratch from the stream's arena:
 * 4 n^3 + 4 ceil(n^3 / 1024) + 32 max_verts + 4 max_faces + 4 ceil(max_faces / 1024) bytes per mesh, + 256 (8.4 MB of
 * cell table at n = 128, 537 MB at 512).
 * MP_ERR_ARG: n outside 1..512; b_max_a <= b_min_a, a non-finite bound, or a box so thin that inv_a is not finite; a
 * NULL or not 4-byte aligned buffer (rows of a capacity of 0 may be NULL); an output that shares a byte with an input.
 * MP_ERR_UNSUPPORTED: max_verts > 2^27, max_faces > 2^31 / 3.  max_verts == 0: MP_OK, counts_out zeroed.  Each refusal
 * leaves an mp_last_error message.  The batched call with one frame. */
int mp_mesh_simplify(mp_ctx *ctx, const float *verts, int64_t max_verts, const int32_t *faces, int64_t max_faces,
                     const int32_t *counts, const float *b_min /*host[3]*/, const float *b_max /*host[3]*/, int n,
                     float *verts_out, int32_t *faces_out, int32_t *counts_out, int32_t *vmap, mp_stream stream);
/* The call above over n_frames (1..mp_max_frames(), else MP_ERR_ARG) meshes of one capacity, with one box and one n
 * for all, in ONE set of launches.  verts / faces / counts / verts_out / faces_out / counts_out / vmap are HOST arrays
 * of n_frames device pointers (vmap may be NULL as a whole).  Frame f's outputs equal those of mp_mesh_simplify on
 * frame f's inputs BIT FOR BIT.  No output of any frame may alias an input of any frame.  Scratch: n_frames times the
 * per-mesh figure.  Refusals as above, for a buffer of any frame. */
int mp_mesh_simplify_batch(mp_ctx *ctx, int n_frames, const float *const *verts, int64_t max_verts,
                           const int32_t *const *faces, int64_t max_faces, const int32_t *const *counts,
                           const float *b_min /*host[3]*/, const float *b_max /*host[3]*/, int n,
                           float *const *verts_out, int32_t *const *faces_out, int32_t *const *counts_out,
                           int32_t *const *vmap, mp_stream stream);

/* ---- mesh smoothing (no counterpart in the reference): Taubin fairing inside the mesh chain -------------------------
 * lambda | mu passes of the umbrella operator over the one-ring of a triangle mesh as mp_marching_cubes or
 * mp_mesh_simplify leave it, between the mesh and its normals.  Defined bit for bit (integer atomics only: the result
 * is a pure function of its inputs, the same bits in every run).  Per mesh: verts f32 [max_verts,3], faces int32
 * [max_faces,3], counts (device int32[2]; only nv = min(max(counts[0], 0), max_verts) vertices and nf likewise faces
 * are read), iterations (1..64), lambda and mu (f32, finite) and flags (MP_SMOOTH_PIN_BORDER or 0).
 *   1 Ring.  A face is valid if all three indices lie in [0, nv).  Its edges are (c0,c1), (c1,c2), (c2,c0); an edge with
 *     equal ends is skipped.  m(a,b) = the number of (valid face, edge) pairs with ends {a,b}.  N(v) = the b with
 *     m(v,b) > 0 in ascending index order, d(v) = |N(v)|.  v is a BORDER vertex if some m(v,b) is odd (an open edge
 *     has m = 1; every edge of a closed mesh, and of a closed mesh after mp_mesh_simplify with its duplicate faces,
 *     is even: nothing is pinned there).  v is FIXED if d(v) = 0, or if MP_SMOOTH_PIN_BORDER is set and v is a border
 *     vertex.  A fixed vertex still serves as a neighbour.
 *   2 Pass with factor phi.  All vertices are updated at once from the previous pass's positions p.  For a vertex that
 *     is not fixed, per axis: s = +0; for b in N(v) ascending: s = s + p_b; m = s / (float)d; q = p + phi * (m - p).
 *     Every operation is one IEEE f32 operation (no FMA, the division correctly rounded, denormals kept).  A fixed
 *     vertex keeps its bits.  Non-finite input follows from the arithmetic: no vertex is declared invalid.
 *   3 Iterations.  `iterations` times: a pass with lambda, then a pass with mu (Taubin: lambda > 0 > mu, |mu| a
 *     little larger than lambda, keeps the volume that the plain Laplacian, mu = 0, loses).
 *   4 Outputs.  verts_out f32 [max_verts,3]: rows [0, nv) written, rows beyond untouched.  ring int32 [max_verts] or
 *     NULL: d(v), negated for a border vertex, rows beyond nv untouched.  Faces and counts are neither changed nor
 *     written.  No output may share a byte with an input of any frame (MP_ERR_ARG).  counts reading {0, 0} (a
 *     gated-off frame of mp_marching_cubes_batch) touch nothing.
 *   4 + 2 * iterations launches and one memset (smooth.hip), asynchronous, nothing synchronised.  Scratch from the
 * stream's arena: 24 max_faces + 28 max_verts bytes per mesh, + 256.
 * MP_ERR_ARG: iterations outside 1..64; lambda or mu not finite; unknown flag bits; a NULL or not 4-byte aligned buffer
 * (rows of a capacity of 0 may be NULL); an output that shares a byte with an input.  MP_ERR_UNSUPPORTED: max_faces >
 * 2^31 / 6 (the list of directed edges is indexed in int32).  max_verts == 0: MP_OK, nothing is done.  Each refusal
 * leaves an mp_last_error message.  The batched call with one frame. */
enum { MP_SMOOTH_PIN_BORDER = 1 };
int mp_mesh_smooth(mp_ctx *ctx, const float *verts, int64_t max_verts, const int32_t *faces, int64_t max_faces,
                   const int32_t *counts, int iterations, float lambda, float mu, int flags, float *verts_out,
                   int32_t *ring, mp_stream stream);
/* The call above over n_frames (1..mp_max_frames(), else MP_ERR_ARG) meshes of one capacity, with one set of
 * parameters for all, in ONE set of launches.  verts / faces / counts / verts_out / ring are HOST arrays of n_frames
 * device pointers (ring may be NULL as a whole).  Frame f's outputs equal those of mp_mesh_smooth on frame f's inputs
 * BIT FOR BIT.  No output of any frame may alias an input of any frame.  Scratch: n_frames times the per-mesh figure.
 * Refusals as above, for a buffer of any frame. */
int mp_mesh_smooth_batch(mp_ctx *ctx, int n_frames, const float *const *verts, int64_t max_verts,
                         const int32_t *const *faces, int64_t max_faces, const int32_t *const *counts, int iterations,
                         float lambda, float mu, int flags, float *const *verts_out, int32_t *const *ring,
                         mp_stream stream);

/* ---- mesh rasteriser (no counterpart in the reference, which renders through PyOpenGL and an X server) ----------
 * A z-buffered picture of a triangle mesh as mp_marching_cubes leaves it, for any camera and any image size, defined
 * bit for bit (integer atomics only: the picture is a pure function of its inputs, the same bits in every run).
 * Per image: verts f32 [max_verts,3], faces int32 [max_faces,3], counts (device int32[2]; only min(counts, capacity)
 * rows are read), a camera calib (12 floats, the rows of [R|t]), an MP_PROJ_* projection and the size H x W (1..4096).
 *   1 Project.  (x, y, z) of a vertex are the bits mp_orthogonal / mp_perspective give for it (the same device code).
 *   2 Snap to 1/256 pixel, in f32 and in this order: u = ((x + 1.0f) * (0.5f * H)) * 256.0f, v likewise with y and W;
 *     X = rintf(u), Y = rintf(v) as integers.  Pixel (i, j) has its centre at (256 i + 128, 256 j + 128): x runs along
 *     the FIRST image index, as in mp_paint's canvas image[X, Y, :], so the result feeds mp_visualize unchanged, and
 *     with the identity camera and H = W = R pixel i is lattice column i.  A vertex is invalid if u, v or z is not
 *     finite or |u| or |v| exceeds 2^22; a face with an invalid vertex, or with an index outside [0, vertices), is
 *     skipped whole.  There is NO clipping in this call (a face with a vertex behind a perspective camera is drawn
 *     from its projected vertices as they are; mp_mesh_render_clip below clips at a near plane) and NO back-face
 *     culling.
 *   3 Cover, in int64: area2 = (X1-X0)(Y2-Y0) - (Y1-Y0)(X2-X0).  Zero: the face is skipped.  Negative: the second and
 *     third vertex are exchanged with everything attached to them, and area2 negated.  At a pixel centre P,
 *     e0 = edge(V1,V2,P), e1 = edge(V2,V0,P), e2 = edge(V0,V1,P) with edge(A,B,P) = (Bx-Ax)(Py-Ay) - (By-Ay)(Px-Ax).
 *     P is covered iff every e_k > 0, or e_k == 0 on an edge A->B with dy < 0 or (dy == 0 and dx > 0), d = B - A (a
 *     top-left rule: two faces sharing an edge never both cover a centre on it, and never both miss it).
 *   4 Interpolate, screen-space affine (NOT perspective-correct): w_k = (float)e_k / (float)area2 (int64 -> f32 rounds
 *     to nearest, the division is IEEE); depth = (w0*z0 + w1*z1) + w2*z2 without FMA; a fragment with a non-finite
 *     depth is dropped.  Attributes take the same expression per channel, then clamp(a * scale + bias, lo, hi) as
 *     mp_paint (normals: 0.5, 0.5, 0, 1; raw netC predictions: 0.5, 0.5, -inf, inf; finished colours: 1, 0, -inf, inf);
 *     attr is [3,max_verts] when channel_major != 0, else [max_verts,3].
 *   5 Resolve.  Per pixel the fragment with the nearest depth wins, among equal depths the smallest face index:
 *     MP_NEAREST_MAX_Z (the viewer sits at +z: what mp_forward_vertices(MP_DIR_FRONT) sees) or MP_NEAREST_MIN_Z (depth
 *     is a distance, the usual perspective case; it compares -depth, an exact sign flip).  One 64-bit integer maximum
 *     per fragment of key = orderable(depth) << 32 | (0xFFFFFFFF - face), orderable(b) = b ^ (b >> 31 ? 0xFFFFFFFF :
 *     0x80000000); a cleared key of 0 means "no fragment".
 * Outputs, any of which may be NULL but not all three: image f32 [H,W,3] (uncovered pixels = background; the
 * reference's canvas is 1.0), depth f32 [H,W] (the winner's unflipped depth, +0.0 where uncovered), face_id int32
 * [H,W] (-1 where uncovered).  attr == NULL requires image == NULL.  calib is a HOST float[12].
 *   Four launches and one memset (raster.hip).  Scratch from the stream's arena: 8 H W (keys, padded to 256 in all) +
 * 16 max_verts (snapped vertices) + 4 max_faces (the list of faces too large for one thread) bytes per image, + 256.
 * MP_ERR_ARG: h or w outside 1..4096, an unknown projection or nearest, a NULL or not 4-byte aligned buffer, all three
 * outputs NULL, image without attr; MP_ERR_UNSUPPORTED: capacities beyond 2^31 / 3.  Asynchronous, nothing
 * synchronised.  The batched call with one frame and one view. */
enum { MP_NEAREST_MAX_Z = 0, MP_NEAREST_MIN_Z = 1 };
int mp_mesh_render(mp_ctx *ctx, const float *verts, int64_t max_verts, const int32_t *faces, int64_t max_faces,
                   const int32_t *counts, const float *attr, int channel_major, const float *calib /*host[12]*/,
                   int projection, int nearest, int h, int w, float scale, float bias, float lo, float hi,
                   float background, float *image, float *depth, int32_t *face_id, mp_stream stream);
/* The call above over n_frames meshes of one capacity times n_views cameras each, n_frames * n_views in
 * 1..mp_max_frames() (else MP_ERR_ARG), in ONE set of launches.  verts / faces / counts / attr / image / depth /
 * face_id are HOST arrays of n_frames device pointers (attr, image, depth, face_id may be NULL as a whole); frame f's
 * outputs hold its views back to back: image[f] [n_views,H,W,3], depth[f] and face_id[f] [n_views,H,W].  calibs is a
 * HOST float[n_frames * n_views * 12], frame-major.  Image (f, v) equals mp_mesh_render on frame f's mesh with
 * camera (f, v) BIT FOR BIT.  A frame whose counts read 0 (a gated-off frame of mp_marching_cubes_batch) gets pure
 * background.  Refusals as above, for a buffer of any frame, each with an mp_last_error message. */
int mp_mesh_render_batch(mp_ctx *ctx, int n_frames, const float *const *verts, int64_t max_verts,
                         const int32_t *const *faces, int64_t max_faces, const int32_t *const *counts,
                         const float *const *attr, int channel_major, int n_views, const float *calibs,
                         int projection, int nearest, int h, int w, float scale, float bias, float lo, float hi,
                         float background, float *const *image, float *const *depth, int32_t *const *face_id,
                         mp_stream stream);
/* mp_mesh_render for a free PERSPECTIVE camera: faces are clipped at the plane zc = near, and with
 * MP_RENDER_PERSPECTIVE_CORRECT depth and attributes are interpolated perspective-correctly.  MP_PROJ_PERSPECTIVE
 * only; near > 0 and finite.  Stateless: no clipped geometry is stored; the face pass clips each face in registers and
 * the resolve re-derives the same sub-triangles from the winning face index.  It extends steps 1-5 above as follows;
 * every operation is one f32 IEEE operation, in the order written, without FMA.
 *   Camera space.  (xc, yc, zc) of a vertex are the three rows of [R|t] p before the divide: the bits mp_orthogonal
 *     returns for that calib.  A vertex is INSIDE iff zc >= near (a NaN is not inside; zc == near is).  A face with an
 *     index out of range or a non-finite camera coordinate is skipped whole.  An inside vertex takes steps 1-2 as
 *     above (x = xc / zc, y = yc / zc, z = zc); a face with an invalid inside vertex is skipped whole.
 *   cut(I, O), always from the inside vertex I to the outside vertex O of an edge: t = (near - zI) / (zO - zI);
 *     xc = xI + t * (xO - xI), yc likewise, zc = near exactly; then x = xc / near, y = yc / near and the snap of step 2
 *     with its guard; a cut vertex that fails the guard skips the face whole.  Inside / outside is a property of the
 *     vertex, so two faces sharing an edge compute the same bits for its cut: the cut leaves no crack.
 *   Faces by their number of inside vertices.  3: steps 2-5 on the snapped vertices, unchanged.  0: skipped.
 *     1: rotated cyclically so that the inside vertex comes first, (A, B, C): ONE triangle (A, P, Q), P = cut(A, B),
 *     Q = cut(A, C).  2: rotated cyclically so that the outside vertex comes last, (A, B, C): P = cut(B, C),
 *     Q = cut(A, C), sub-triangle 0 = (A, B, P), sub-triangle 1 = (A, P, Q).
 *   Cover (step 3) per sub-triangle, unchanged: area2 (zero: that sub-triangle is skipped), the exchange of its second
 *     and third vertex, the top-left rule.  The two sub-triangles share the diagonal A-P with identical snapped ends.
 *   Interpolate (step 4) with the sub-triangle's own area2 and e_k, w_k = (float)e_k / (float)area2; z of a cut vertex
 *     is near.  Without the flag: depth = (w0*z0 + w1*z1) + w2*z2 and attributes likewise, as above.  With
 *     MP_RENDER_PERSPECTIVE_CORRECT (for every face, cut or not): q_k = w_k / z_k, s = (q0 + q1) + q2,
 *     depth = 1.0f / s, an attribute is ((q0*a0 + q1*a1) + q2*a2) / s, then clamp(a * scale + bias, lo, hi).  Every
 *     z_k >= near > 0.  A fragment with a non-finite depth is dropped.  The attribute of a cut vertex is
 *     aI + t * (aO - aI) per channel.
 *   Resolve (step 5).  The key holds the ORIGINAL face index: the tie-break and face_id are those of the unclipped
 *     call.  The outputs are those of the lowest-numbered sub-triangle of the winning face that covers the centre.
 *   So for a mesh wholly in front of the plane and flags == 0 the result is mp_mesh_render's BIT FOR BIT.
 * NOT built: clipping against the side planes (a clipped face that still exceeds the 2^22 snap guard is skipped
 * whole), a far plane, back-face culling, clipping for orthogonal cameras.
 *   Launches and scratch as mp_mesh_render, + 16 max_verts bytes per image (the camera-space vertices); a face goes to
 *   the list of large faces, at most once, when any of its sub-triangles has a box of more than 64 centres.
 * MP_ERR_ARG: near not finite or <= 0, unknown flag bits, a projection other than MP_PROJ_PERSPECTIVE, and everything
 * mp_mesh_render refuses; a refused call launches nothing.  The batched call with one frame and one view. */
enum { MP_RENDER_PERSPECTIVE_CORRECT = 1 };
int mp_mesh_render_clip(mp_ctx *ctx, const float *verts, int64_t max_verts, const int32_t *faces, int64_t max_faces,
                        const int32_t *counts, const float *attr, int channel_major, const float *calib /*host[12]*/,
                        int projection, int nearest, int h, int w, float scale, float bias, float lo, float hi,
                        float background, float *image, float *depth, int32_t *face_id, float near, int flags,
                        mp_stream stream);
/* mp_mesh_render_batch's arguments and contract with the clipped definition: image (f, v) equals mp_mesh_render_clip
 * on frame f's mesh with camera (f, v) BIT FOR BIT; one near and one flags for all. */
int mp_mesh_render_clip_batch(mp_ctx *ctx, int n_frames, const float *const *verts, int64_t max_verts,
                              const int32_t *const *faces, int64_t max_faces, const int32_t *const *counts,
                              const float *const *attr, int channel_major, int n_views, const float *calibs,
                              int projection, int nearest, int h, int w, float scale, float bias, float lo, float hi,
                              float background, float *const *image, float *const *depth, int32_t *const *face_id,
                              float near, int flags, mp_stream stream);

/* ---- pictures coloured per pixel (deferred shading): netC queried at the visible surface only ------------------------
 * A render with attr = verts and the paint (1, 0, -inf, inf) is a picture of world-space surface positions.  The two
 * calls below turn it into a counted point list for mp_query_counted_batch_proj / mp_query_views_counted_batch and put
 * the predictions back, with no host value in between.  A frame's pictures are ONE flat array, as mp_mesh_render_batch
 * lays them out: L = n_views * H * W pixels, pixel index p = the linear index into [n_views, H, W].  Both calls are
 * defined bit for bit and are pure functions of their inputs.
 *   mp_picture_points.  face_id int32 [L] as the render wrote it (-1 = uncovered), position f32 [L,3] (the render's
 *     image).  Pixel p is covered iff face_id[p] >= 0.  With p_0 < p_1 < ... the covered pixels in ascending order and
 *     K their number: for k < min(K, capacity), pixels[k] = p_k and points[c * capacity + k] = position[3 p_k + c],
 *     the same 32 bits (points f32 [3,capacity], the layout mp_query_counted reads; pixels int32 [capacity]).
 *     count (device int32[2]): count[0] = min(K, capacity), what the counted queries read; count[1] = K, so
 *     count[1] > capacity tells a truncated list.  Columns at or beyond count[0] are not written.  The order is
 *     ascending p, never arrival order: block counts, a scan of them, then the emit (picture.hip, three launches, no
 *     atomic).  Scratch from the stream's arena: 4 ceil(L / 1024) bytes per frame (the block sums), + 256; it is
 *     written before it is read, whatever the arena held.  A frame with no covered pixel gets count = {0, 0}.
 *   mp_picture_paint.  values f32 [3,capacity] channel-major, as the queries write them.  For k < min(count[0],
 *     capacity) (a negative count[0] is 0) with 0 <= pixels[k] < L: image[3 pixels[k] + c] = clamp(values[c * capacity
 *     + k] * scale + bias, lo, hi), the two operations and the clamp of mp_paint (raw netC predictions: 0.5, 0.5,
 *     -inf, inf).  An index outside the range is skipped, never written; no other pixel of image f32 [L,3] is touched.
 *     With the pixels of mp_picture_points no pixel is named twice; a caller's list that names one twice leaves either
 *     value.  `image` may be the buffer `position` was read from: the calls are ordered on the stream.  One launch.
 * MP_ERR_ARG: n_frames outside 1..mp_max_frames(); n_pixels or capacity < 1; a NULL or not 4-byte aligned buffer of any
 * frame.  MP_ERR_UNSUPPORTED: n_pixels beyond 2^31 / 3.  Each refusal leaves an mp_last_error message and launches
 * nothing.  Asynchronous, nothing synchronised.  The per-frame calls are the batched ones with one frame; in the
 * batched ones face_id / position / points / pixels / count / values / image are HOST arrays of n_frames device
 * pointers (one n_pixels and one capacity for all), blockIdx.y is the frame and one set of launches serves all frames:
 * frame f's outputs equal the per-frame call's on frame f's inputs BIT FOR BIT. */
int mp_picture_points(mp_ctx *ctx, const int32_t *face_id, const float *position, int64_t n_pixels, int64_t capacity,
                      float *points, int32_t *pixels, int32_t *count, mp_stream stream);
int mp_picture_points_batch(mp_ctx *ctx, int n_frames, const int32_t *const *face_id, const float *const *position,
                            int64_t n_pixels, int64_t capacity, float *const *points, int32_t *const *pixels,
                            int32_t *const *count, mp_stream stream);
int mp_picture_paint(mp_ctx *ctx, const float *values, const int32_t *pixels, const int32_t *count, int64_t capacity,
                     int64_t n_pixels, float scale, float bias, float lo, float hi, float *image, mp_stream stream);
int mp_picture_paint_batch(mp_ctx *ctx, int n_frames, const float *const *values, const int32_t *const *pixels,
                           const int32_t *const *count, int64_t capacity, int64_t n_pixels, float scale, float bias,
                           float lo, float hi, float *const *image, mp_stream stream);

/* ---- the scene behind the subject (RTL/scene.py, RTL/main.py: the textured floor and mask * render + (1 - mask) *
 * background): a mip pyramid, a texture lookup per pixel and a composite by coverage or by depth ----------------------
 * The floor goes through the rasteriser above with attr = (u, v, 0) per vertex and the paint (1, 0, -inf, inf): its
 * image is then a UV picture.  The calls below turn it into the textured picture and put the subject's picture over
 * it.  A frame's pictures are ONE flat array as mp_mesh_render_batch lays them out: L = n_views * H * W pixels.  All
 * calls are pure functions of their inputs, defined bit for bit: every float operation below is ONE IEEE f32 +, - or *,
 * in the order written, without FMA; there is no sqrt, log or division (scene.hip; no atomics, no scratch).
 *   Pyramid.  A texture f32 [ht,wt,3] (ht, wt in 1..8192) has levels 0..levels-1, levels in 1..14 and no more than
 *     reach 1 x 1 (1 + floor(log2(max(ht, wt)))).  Level 0 is the texture (h_0 = ht, w_0 = wt); h_l = max(1, h_{l-1}
 *     >> 1), w_l likewise.  Texel (i, j, c) of level l is ((a + b) + (c' + d)) * 0.25f with a, b = level l-1 at row
 *     min(2i, h-1), columns min(2j, w-1) and min(2j+1, w-1), and c', d the same columns of row min(2i+1, h-1) (h, w those
 *     of level l-1).  The levels lie back to back, level l at float offset sum_{k<l} 3 h_k w_k, each [h_l,w_l,3].
 *     mp_texture_pyramid_floats: the float count of all `levels` levels (host only, no context); 0 for sizes out of
 *     range.  mp_texture_mips: tex -> pyramid, one launch per level (a set-up call); the two may not overlap.
 *   mp_picture_texture.  uv f32 [L,3] (channels u, v, unused), face_id int32 [L], both as the rasteriser wrote them;
 *     image f32 [L,3]; EVERY pixel of image is written.  With pixel p = (view, i, j), i along H:
 *     Covered iff face_id >= 0 and |u| <= 65536 and |v| <= 65536 (a NaN and an infinity fail).  Any other pixel gets
 *       `background` in all three channels.
 *     Level.  S = u * (float)wt, T = v * (float)ht.  Along axis i: for each of (i+1, j) and (i-1, j) that lies in the
 *       same view and is covered, dS = S' - S, dT = T' - T, d2 = (dS * dS) + (dT * dT); rho2_i = the smaller of the
 *       available d2, or 0 with none (the smaller, so that a uv seam of a packed mesh does not force the coarsest level
 *       along the seam).  rho2_j likewise with (i, j+1) and (i, j-1); rho2 = rho2_i > rho2_j ? rho2_i : rho2_j.
 *       level = the number of l in 0..levels-2 with rho2 > 2^(2l+1): nearest-mip selection, level 1 from a step of
 *       sqrt(2) texels per pixel on.
 *     Lookup, bilinear in that level (h, w its size): s = u * (float)w - 0.5f, s0 = floorf(s), fs = s - s0, columns
 *       x0 = (int)s0 and x1 = x0 + 1; t = v * (float)h - 0.5f, rows y0, y1 and ft likewise.  Each index k of n is
 *       wrapped: MP_WRAP_REPEAT ((k % n) + n) % n, MP_WRAP_CLAMP min(max(k, 0), n - 1).  With cXY the texel at column
 *       xX, row yY: value = (c00 * (1.0f - fs) + c10 * fs) * (1.0f - ft) + (c01 * (1.0f - fs) + c11 * fs) * ft.
 *     Paint.  clamp(value * scale + bias, lo, hi) as mp_paint (o < lo ? lo : (o > hi ? hi : o)).
 *     One launch, one thread per pixel: 16 B read (+ up to 4 neighbours, cached) and 12 B written per pixel, and twelve
 *     texels per covered one.  image may not share a byte with uv, face_id or the pyramid (a pixel reads its
 *     neighbours' uv): image == uv is refused.
 *   mp_picture_composite.  Per pixel, from front (image f32 [L,3], depth f32 [L], face_id int32 [L]) and back (the
 *     same three): a picture is covered where its face_id >= 0.  Front shows where it is covered and (back is
 *     uncovered, or mode == MP_COMPOSITE_OVER, or back is not STRICTLY nearer: !(db < df) with MP_NEAREST_MIN_Z,
 *     !(db > df) with MP_NEAREST_MAX_Z; a tie and a NaN go to front).  Else back shows where it is covered.  Outputs:
 *     image f32 [L,3] and depth f32 [L] take the showing picture's values as their 32-bit patterns, `background` and
 *     +0.0 where neither is covered; mask uint8 [L]: 0 = neither, 1 = back, 2 = front.  depth and mask may be NULL.
 *     MP_COMPOSITE_OVER is the reference's mask composite (the subject always over the floor); MP_COMPOSITE_DEPTH lets
 *     a part of the scene in front of the subject hide it.  image / depth may BE front's (or back's) image / depth of
 *     the same frame -- the composite in place --, because a thread reads its own pixel before it writes it; any other
 *     byte shared between an output and an input is refused.  One launch: 40 B read, 17 B written per pixel.
 * MP_ERR_ARG: n_frames outside 1..mp_max_frames(); ht, wt or levels out of range; n_views < 1, h or w outside 1..4096,
 * n_pixels < 1; an unknown wrap, mode or nearest; a NULL or not 4-byte aligned buffer of any frame (mask: any
 * alignment); the aliasing above.  MP_ERR_UNSUPPORTED: L beyond 2^31 / 3.  Each refusal leaves an mp_last_error
 * message and launches nothing.  Asynchronous, nothing synchronised, no scratch arena.  The per-frame calls are the
 * batched ones with one frame; in the batched ones uv / face_id / image / front_* / back_* / depth / mask are HOST
 * arrays of n_frames device pointers (one pyramid and one size for all), blockIdx.y is the frame: frame f's outputs
 * equal the per-frame call's on frame f's inputs BIT FOR BIT.
 * NOT built: trilinear and anisotropic filtering; the composite has no alpha (the subject's coverage comes with
 * mp_picture_resolve below).  Shadows of the subject on the scene: mp_picture_shadow below. */
enum { MP_WRAP_REPEAT = 0, MP_WRAP_CLAMP = 1 };
enum { MP_COMPOSITE_OVER = 0, MP_COMPOSITE_DEPTH = 1 };
int64_t mp_texture_pyramid_floats(int ht, int wt, int levels);
int mp_texture_mips(mp_ctx *ctx, const float *tex, int ht, int wt, int levels, float *pyramid, mp_stream stream);
int mp_picture_texture(mp_ctx *ctx, const float *uv, const int32_t *face_id, int n_views, int h, int w,
                       const float *pyramid, int ht, int wt, int levels, int wrap, float scale, float bias, float lo,
                       float hi, float background, float *image, mp_stream stream);
int mp_picture_texture_batch(mp_ctx *ctx, int n_frames, const float *const *uv, const int32_t *const *face_id,
                             int n_views, int h, int w, const float *pyramid, int ht, int wt, int levels, int wrap,
                             float scale, float bias, float lo, float hi, float background, float *const *image,
                             mp_stream stream);
int mp_picture_composite(mp_ctx *ctx, const float *front_image, const float *front_depth, const int32_t *front_face,
                         const float *back_image, const float *back_depth, const int32_t *back_face, int64_t n_pixels,
                         int mode, int nearest, float background, float *image, float *depth, uint8_t *mask,
                         mp_stream stream);
int mp_picture_composite_batch(mp_ctx *ctx, int n_frames, const float *const *front_image,
                               const float *const *front_depth, const int32_t *const *front_face,
                               const float *const *back_image, const float *const *back_depth,
                               const int32_t *const *back_face, int64_t n_pixels, int mode, int nearest,
                               float background, float *const *image, float *const *depth, uint8_t *const *mask,
                               mp_stream stream);

/* ---- anti-aliasing: the resolve of a supersampled picture (the reference's multi_sample_rate attachments and their
 * blit) --------------------------------------------------------------------------------------------------------------
 * The rasteriser puts a vertex at u = (x + 1) * 0.5 * H pixels and pixel i has its centre at i + 0.5, so a picture of
 * s H x s W under the same camera samples every pixel of the H x W one on a regular s x s grid inside it.  Every pass
 * above (attributes, positions, normals, transfer, uv, texture, shadow, lighting, composite) runs at s times the size;
 * this call then makes the final picture, once.  samples = s in 2..4; the inputs are pictures [s h, s w] (s h, s w in
 * 1..4096), the outputs [h, w]: image f32 [.,.,3], depth f32, face_id int32, mask uint8 (the composite's 0 / 1 / 2),
 * coverage f32.  Sample (a, b) of output pixel (i, j) is input pixel (s i + a, s j + b); the samples are visited in
 * row-major order of (a, b).  A pure function of its inputs, defined bit for bit (resolve.hip; one launch, one thread
 * per output pixel, no atomics, no scratch):
 *   image_out[i,j,c] = (((x_0 + x_1) + x_2) + ... + x_{s s - 1}) / (float)(s s): sequential single IEEE f32 additions
 *     starting FROM the first sample (not from 0), without FMA, then one IEEE division.  A region of equal samples x
 *     therefore keeps its bits for s = 2 (2x and 4x are exact and fl(3x) + x rounds to 4x), and for s = 4 wherever x
 *     has at most 20 significant bits, so that every partial sum is exact: the backgrounds and flat colours 0, 1, 0.5,
 *     k / 256.  Any other x may move by a few ulps at s = 4 (fewer than 8), and so may any x at s = 3; a sum beyond
 *     the f32 range is an infinity.  A NaN sample gives a NaN of unspecified payload.
 *   A sample is the SUBJECT's iff mask == 2 when a mask is given, else iff face_id >= 0.  coverage[i,j] = (float)count
 *     / (float)(s s), count the subject's samples: the subject's alpha.  image_out - (1 - coverage) * background is the
 *     premultiplied subject for a consumer who composites elsewhere (with a scene the scene's samples are in image_out
 *     too: the edge between subject and scene is blended here, correctly, which an alpha against a background is not).
 *   A sample SHOWS iff mask != 0 when a mask is given, else iff face_id >= 0.  depth_out / face_out = the depth bits and
 *     the face id of the showing sample that is nearest under `nearest`: the one with the largest key, key = the
 *     rasteriser's orderable key (b ^ (b >> 31 ? 0xFFFFFFFF : 0x80000000) of the bits b) of depth with
 *     MP_NEAREST_MAX_Z, of -depth (the sign bit flipped) with MP_NEAREST_MIN_Z; among equal keys the first in sample
 *     order.  No showing sample: +0.0 and -1.  The face id may be -1 where the scene is nearest.
 *   mask_out = the largest of the samples' masks.
 * Every output needs its input: image_out image; depth_out and face_out BOTH depth and face_id; mask_out mask; coverage
 * mask or face_id.  Any output may be NULL, not all; an input nobody needs may be NULL.  No output may share a byte with
 * an input.  MP_ERR_ARG: samples outside 2..4; n_frames or n_views < 1, n_frames * n_views beyond mp_max_frames(); h or
 * w < 1, samples * h or samples * w beyond 4096; an unknown nearest; no output; an output without its input; a NULL or
 * not 4-byte aligned buffer of any frame (mask, mask_out: any alignment); the aliasing above.  Each refusal leaves an
 * mp_last_error message, launches nothing and writes nothing.  Asynchronous, nothing synchronised, no scratch arena.
 * Inputs that are all 16-byte aligned are read with wider loads (s = 2, 4); the bits do not depend on it.  Traffic per
 * output pixel: s s (12 + 4 + 4 + 1) B read with everything given, 25 B written.
 * mp_picture_resolve_batch: image / depth / face_id / mask / *_out / coverage are HOST arrays of n_frames device
 * pointers, or NULL as a whole; a frame's n_views pictures lie back to back ([n_views, s h, s w] in, [n_views, h, w]
 * out); one launch serves all, blockIdx.y the picture: frame f's outputs equal the single call's on frame f's inputs
 * BIT FOR BIT.
 * NOT built: filters wider than the pixel's own box, gamma-correct (linear-light) averaging, edge-only multisampling
 * that shades once per pixel, the composite of two already resolved pictures. */
int mp_picture_resolve(mp_ctx *ctx, const float *image, const float *depth, const int32_t *face_id,
                       const uint8_t *mask, int h, int w, int samples, int nearest, float *image_out, float *depth_out,
                       int32_t *face_out, uint8_t *mask_out, float *coverage, mp_stream stream);
int mp_picture_resolve_batch(mp_ctx *ctx, int n_frames, int n_views, const float *const *image,
                             const float *const *depth, const int32_t *const *face_id, const uint8_t *const *mask,
                             int h, int w, int samples, int nearest, float *const *image_out, float *const *depth_out,
                             int32_t *const *face_out, uint8_t *const *mask_out, float *const *coverage,
                             mp_stream stream);

/* ---- the shadow of the subject on a picture: a shadow map looked up per pixel, filtered, and the pixel darkened -------
 * A shadow map is what mp_mesh_render(_clip) writes WITHOUT an image for the caster under the light's camera: map_depth
 * f32 [hs,ws] and map_face int32 [hs,ws] (hs, ws in 1..4096), rendered with `nearest`.  The receiver is a picture of L
 * pixels (L = n_views * H * W as mp_mesh_render_batch lays them out): image_in f32 [L,3], face_id int32 [L] and
 * position f32 [L,3], the rasteriser's image for attr = verts with the paint (1, 0, -inf, inf): the world-space point
 * each pixel shows.  light_calib: HOST, 12 floats, the rows of [R|t] of the light; projection: its MP_PROJ_* mode.
 * bias: finite, >= 0; radius: 0..3; strength: in [0, 1].  Outputs: image_out f32 [L,3] and shade f32 [L]; either may
 * be NULL, not both; image_in is NULL exactly when image_out is.  A pure function of its inputs, defined bit for bit:
 * every float operation of steps 3-6 is ONE IEEE f32 +, - or *, in the order written, without FMA; there is no sqrt,
 * log or division (scene.hip; no atomics, no scratch).  Per pixel:
 *   1. Uncovered.  face_id < 0: shade 0.
 *   2. Projection.  (x, y, z) = the bits mp_orthogonal / mp_perspective give for the pixel's position under
 *      light_calib (the device code of step 1 of the rasteriser; z is the camera-space row).  A non-finite x, y or z:
 *      shade 0.  MP_PROJ_PERSPECTIVE and a z that is not > 0: shade 0.
 *   3. Map coordinates, in the rasteriser's pixel-centre convention (texel i has its centre at x = (2 i + 1) / hs - 1):
 *      a = (x + 1.0f) * (0.5f * (float)hs) - 0.5f, b = (y + 1.0f) * (0.5f * (float)ws) - 0.5f.  |a| or |b| > 2^22:
 *      shade 0.  i0 = floorf(a), fa = a - i0; j0 = floorf(b), fb = b - j0.
 *   4. Tap.  occ(i, j) = 1.0f if 0 <= i < hs, 0 <= j < ws, map_face[i,j] >= 0 and the map is STRICTLY nearer than the
 *      pixel by more than the bias: map_depth[i,j] + bias < z with MP_NEAREST_MIN_Z, map_depth[i,j] - bias > z with
 *      MP_NEAREST_MAX_Z.  Else 0.0f: a tap outside the map, an uncovered texel, a tie, a NaN.
 *   5. Filter, a (2r+1)^2 box of bilinear lookups over the (2r+2)^2 texels (i0 + di, j0 + dj), di, dj = -r..r+1, each
 *      touched once.  wi(di) = 1.0f - fa at di = -r, fa at di = r+1, 1.0f between; wj(dj) likewise with fb.
 *      row(di) = 0.0f, then row = row + wj(dj) * occ(i0 + di, j0 + dj) for dj ascending; total = 0.0f, then total =
 *      total + wi(di) * row(di) for di ascending.  shade = min(total * k_r, 1.0f), k_r the f32 nearest to
 *      1 / (2r+1)^2.  Occluded weight is what is summed: a pixel nothing occludes has shade +0.0 exactly.
 *   6. Paint.  shade (if given) is written for EVERY pixel: 0 where steps 1-3 say so.  Where shade == 0, image_out
 *      takes image_in's 32-bit patterns (in place: the pixel is not written at all).  Else factor = 1.0f - strength *
 *      shade and image_out[c] = image_in[c] * factor.
 * So a map without a caster (all face ids < 0) and strength == 0 both leave the picture's bits unchanged.
 * image_out may BE image_in of the same frame (in place); any other byte shared between an output and an input is
 * refused.  One launch, one thread per pixel: 16 B (+ 12 B with an image) read and up to 16 B written per pixel,
 * (2r+2)^2 gathers of 8 B from the map per pixel that reaches step 4; no other pixel touches the map.
 * MP_ERR_ARG: n_frames outside 1..mp_max_frames(); n_pixels < 1; hs or ws outside 1..4096; an unknown projection or
 * nearest; a bias that is negative or not finite; a radius outside 0..3; a strength outside [0, 1] or NaN; no output,
 * image_in without image_out or the reverse; a NULL or not 4-byte aligned buffer of any frame; the aliasing above.
 * MP_ERR_UNSUPPORTED: L beyond 2^31 / 3.  Each refusal leaves an mp_last_error message and launches nothing.
 * Asynchronous, nothing synchronised, no scratch arena.  The per-frame call is the batched one with one frame; in the
 * batched one image_in / position / face_id / map_depth / map_face / image_out / shade are HOST arrays of n_frames
 * device pointers and light_calibs a HOST array of n_frames * 12 floats (one map size and one parameter set for all),
 * blockIdx.y is the frame: frame f's outputs equal the per-frame call's on frame f's inputs BIT FOR BIT.
 * NOT built: the scene casting shadows, more than one light, coloured or area lights, a varying penumbra, cascades. */
int mp_picture_shadow(mp_ctx *ctx, const float *image_in, const float *position, const int32_t *face_id,
                      int64_t n_pixels, const float *map_depth, const int32_t *map_face, int hs, int ws,
                      const float *light_calib, int projection, int nearest, float bias, int radius, float strength,
                      float *image_out, float *shade, mp_stream stream);
int mp_picture_shadow_batch(mp_ctx *ctx, int n_frames, const float *const *image_in, const float *const *position,
                            const int32_t *const *face_id, int64_t n_pixels, const float *const *map_depth,
                            const int32_t *const *map_face, int hs, int ws, const float *light_calibs, int projection,
                            int nearest, float bias, int radius, float strength, float *const *image_out,
                            float *const *shade, mp_stream stream);

/* ---- lighting the subject per pixel: second-order spherical harmonics and one directional light at the normal -------
 * The reference's lighting model (its SH fragment shader and ShRender: nine basis values at the normal, nine RGB
 * coefficients, a gamma, clamp(albedo * shading, 0, 1)), plus one directional light that mp_picture_shadow's shade can
 * occlude.  A frame's pictures are one flat array of L = n_views * H * W pixels as mp_mesh_render_batch lays them out.
 * Per frame: normal f32 [L,3], the rasteriser's image for attr = the mesh's normals with the paint (1, 0, -inf, inf);
 * face_id int32 [L]; albedo f32 [L,3], or NULL as a whole and then albedo_rgb (HOST, 3 floats) is every pixel's albedo;
 * visibility f32 [L] or NULL: the `shade` of mp_picture_shadow, 1 = the light is fully occluded.  Per call, HOST:
 * sh, 27 floats [9][3] (coefficient i, channel c at sh[3 i + c]); direct_dir[3], the direction the light TRAVELS, and
 * direct_rgb[3] (all three == 0: there is no direct term); gamma (finite, > 0); normal_mats, NULL or n_frames * n_views
 * row-major 3x3 matrices, frame-major: SH is then evaluated at the normal turned into the camera's frame (the
 * reference's ModelMat * a_Normal); background: what an uncovered pixel of image_out holds without an albedo buffer.
 * Outputs: image_out f32 [L,3] and shading f32 [L,3]; either may be NULL, not both.  A pure function of its inputs,
 * defined bit for bit: every float operation is ONE IEEE f32 +, -, *, / or sqrtf (the correctly rounded ones), in the
 * order written, without FMA (light.hip; no atomics, no scratch).  max0(a) is a where a > 0, else +0.0 (a NaN, a -0.0:
 * +0.0).  Per pixel p:
 *   1. Uncovered.  face_id < 0: shading = (0, 0, 0); image_out takes albedo's 32-bit patterns (in place: the pixel is
 *      not written at all), or `background` three times without an albedo buffer.
 *   2. The world normal.  s = (nx*nx + ny*ny) + nz*nz.  s not finite or not > 0: u = (0, 0, 0).  Else len = sqrtf(s),
 *      u = (nx / len, ny / len, nz / len).
 *   3. The SH normal.  Without normal_mats: m = u, the same bits.  With them, M = the matrix of the pixel's frame and
 *      view p / (L / n_views): t_r = (M[r][0]*ux + M[r][1]*uy) + M[r][2]*uz for r = 0, 1, 2, and m = t normalised by
 *      the rule of step 2.
 *   4. The basis, with c1..c5 the f32 nearest to 0.429043, 0.511664, 0.743125, 0.886227, 0.247708 and d1 = 2.0f * c1,
 *      d2 = 2.0f * c2 (exact): H0 = c4, H1 = d2 * my, H2 = d2 * mz, H3 = d2 * mx, H4 = (d1 * mx) * my,
 *      H5 = (d1 * my) * mz, H6 = ((c3 * mz) * mz) - c5, H7 = (d1 * mz) * mx, H8 = c1 * ((mx * mx) - (my * my)).
 *      res_c = 0.0f, then res_c = res_c + H[i] * sh[3 i + c] for i = 0..8 ascending.
 *   5. The direct term (skipped as a whole where direct_rgb is all zero), always on the WORLD normal u:
 *      k = max0(-((dx*ux + dy*uy) + dz*uz)); vis = 1.0f - visibility[p], or 1.0f without the buffer;
 *      res_c = res_c + (k * vis) * direct_rgb[c].
 *   6. Gamma.  gamma == 1.0f: nothing (the bit-exact form).  Else res_c = powf(max0(res_c), 1.0f / gamma), the one
 *      step held to a tolerance instead of the bits (1.0f / gamma is one f32 division on the host).
 *   7. shading[c] = res_c; image_out[c] = clamp(albedo_c * res_c): v < 0 gives 0, v > 1 gives 1, else v (mp_paint's
 *      clamp: a NaN stays).
 * image_out may BE albedo of the same frame (in place); any other byte shared between an output and an input, or
 * between the two outputs, is refused.  One launch, one thread per pixel: 16 B (+ 12 B albedo, + 4 B visibility) read
 * and up to 24 B written per covered pixel; an uncovered span reads its face ids only.
 * MP_ERR_ARG: n_frames outside 1..mp_max_frames(); n_pixels < 1; n_views < 1 or not a divisor of n_pixels; with
 * normal_mats, n_frames * n_views > 32 (what the kernel's argument block holds); sh, direct_dir or direct_rgb NULL;
 * albedo and albedo_rgb both NULL or both given; a gamma that is not finite or <= 0; a non-finite value among sh,
 * direct_dir, direct_rgb, albedo_rgb, background or normal_mats; no output; a NULL or not 4-byte aligned buffer of any
 * frame; the aliasing above.  MP_ERR_UNSUPPORTED: L beyond 2^31 / 3.  Each refusal leaves an mp_last_error message and
 * launches nothing.  Asynchronous, nothing synchronised, no scratch arena.  The per-frame call is the batched one with
 * one frame; in the batched one normal / face_id / albedo / visibility / image_out / shading are HOST arrays of
 * n_frames device pointers (one parameter set for all), blockIdx.y is the frame: frame f's outputs equal the per-frame
 * call's on frame f's inputs BIT FOR BIT.
 * NOT built: lighting the scene by the same model, several lights, specular terms.  Precomputed radiance transfer is
 * mp_mesh_transfer + mp_picture_light_transfer below. */
int mp_picture_light(mp_ctx *ctx, const float *normal, const int32_t *face_id, const float *albedo,
                     const float *albedo_rgb, const float *visibility, int64_t n_pixels, int n_views, const float *sh,
                     const float *direct_dir, const float *direct_rgb, float gamma, const float *normal_mats,
                     float background, float *image_out, float *shading, mp_stream stream);
int mp_picture_light_batch(mp_ctx *ctx, int n_frames, const float *const *normal, const int32_t *const *face_id,
                           const float *const *albedo, const float *albedo_rgb, const float *const *visibility,
                           int64_t n_pixels, int n_views, const float *sh, const float *direct_dir,
                           const float *direct_rgb, float gamma, const float *normal_mats, float background,
                           float *const *image_out, float *const *shading, mp_stream stream);

/* ---- self-occluded SH lighting: radiance transfer traced in the occupancy volume -------------------------------------
 * The reference's PRT shaders shade with nine precomputed radiance-transfer coefficients per vertex (shading_c =
 * sum_k prt_k * SHCoeffs[k][c]): the cosine lobe masked by what the body itself occludes.  Here they are traced per
 * frame through the occupancy volume the mesh was cut from.  All float operations below are single IEEE f32 + - * /,
 * sqrtf and floorf in the order written, without FMA (transfer.hip; no float atomics, no scratch arena, 0 B private).
 *
 * mp_volume_bits: one bit per voxel of a cubic volume [R,R,R] (z, y, x) f32, 1 <= R <= MP_TRANSFER_MAX_RES.  Word
 * (z*R + y)*WX + (x >> 5) with WX = ceil(R / 32), bit x & 31, set iff v > level (a NaN voxel is empty); padding bits
 * are 0.  `bits` is the CALLER's buffer of mp_volume_bits_words(R) 32-bit words (0 for an R out of range): the first
 * R*R*WX words are the bits defined here, what follows is the tracer's private data (one bit per 8^3 block), written by
 * the same call.  Batched: `gates` as in mp_marching_cubes_batch (NULL, or per frame NULL / a device int32: a frame
 * whose gate reads 0 is neither read nor written).  MP_ERR_ARG: n_frames outside 1..mp_max_frames(), R out of range, a
 * NULL or not 4-byte aligned buffer, bits sharing a byte with a volume or with another frame's bits.
 *
 * mp_mesh_transfer: per call HOST b_min[3], b_max[3], R, n_dirs = D (a multiple of 64, 64..MP_TRANSFER_MAX_DIRS),
 * weight, bias_w and step_w (world units), max_steps = J (1..2^24); DEVICE tables dirs f32 [D,3] and basis f32 [D,9].
 * Per frame verts [max_verts,3], normals [max_verts,3], counts (device int32, [0] = vertices), bits (of mp_volume_bits
 * at the same R).  Outputs mask u64 [max_verts, D/64] (bit d & 63 of word d >> 6: direction d is seen) and prt f32
 * [max_verts,9]; either may be NULL, not both.  Rows at or beyond counts[0] are not written.  Per vertex p, normal n:
 *   1. u = n normalised by step 2 of mp_picture_light (a zero or non-finite normal: u = 0).
 *   2. vox_a = R / (b_max_a - b_min_a).
 *   3. g_a = ((p_a - b_min_a) / (b_max_a - b_min_a)) * R.  Voxel i covers [i, i+1): the inverse of marching cubes'
 *      lattice coordinate.
 *   4. o_a = g_a + (bias_w * u_a) * vox_a.
 *   5. Direction d = (wx, wy, wz): k_d = (wx*ux + wy*uy) + wz*uz.  k_d > 0 false (a NaN included): bit d = 0, nothing
 *      is traced.  Else delta_a = (step_w * w_a) * vox_a.
 *   6. For j = 0..J-1: s_a = o_a + ((float)j * delta_a).  Not (s_a >= 0 && s_a < R) on some axis: the ray has left,
 *      bit d = 1, stop.  Else voxel (int)floorf(s) set in bits: bit d = 0, stop.  A ray that uses up J samples: bit 1.
 *   7. acc_k = 0.0f; for d ascending over the set bits acc_k = acc_k + (k_d * basis[d][k]); prt_k = acc_k * weight.
 * The mask is an integer result and the sum has one order, so the outputs are defined bit for bit.  One thread per
 * vertex; empty 8^3 blocks are skipped exactly (samples are indexed by j and monotone in j).
 * MP_ERR_ARG: the ranges above; non-finite b_min / b_max or b_max <= b_min; non-finite weight / bias_w / step_w or
 * step_w <= 0; no output; a NULL or misaligned buffer (mask: 8 bytes); an output sharing a byte with an input (dirs
 * and basis included) or with another output.  MP_ERR_UNSUPPORTED: max_verts beyond 2^31 / 9.
 *
 * mp_mesh_transfer_shade: out [max_verts,3]: t_c = 0.0f, then t_c = t_c + prt_k * sh[3 k + c] for k = 0..8 (sh: HOST,
 * 27 finite floats) -- the reference's evaluateLightingModelPRT.  Linear in prt, so rasterising t as the attribute with
 * the paint (1, 0, -inf, inf) equals interpolating the nine coefficients.
 *
 * mp_picture_light_transfer: mp_picture_light with one more per-frame input, ambient f32 [L,3] (the rasterised t),
 * which replaces step 4: res_c = ambient_c.  Steps 1, 2, 5, 6, 7 are unchanged and run in the same kernel body.
 * `normal` may be NULL where direct_rgb is all zero.  No normal_mats: the camera frame would need the reference's band
 * rotation, which is not built.  Refusals as mp_picture_light's, ambient counting as an input.
 * All of these are asynchronous, synchronise nothing, and the per-frame call is the batched one with one frame. */
#define MP_TRANSFER_MAX_RES 513
#define MP_TRANSFER_MAX_DIRS 512
int64_t mp_volume_bits_words(int r);
int mp_volume_bits(mp_ctx *ctx, const float *volume, int r, float level, uint32_t *bits, mp_stream stream);
int mp_volume_bits_batch(mp_ctx *ctx, int n_frames, const float *const *volume, int r, float level,
                         uint32_t *const *bits, const int32_t *const *gates, mp_stream stream);
int mp_mesh_transfer(mp_ctx *ctx, const float *verts, const float *normals, int64_t max_verts, const int32_t *counts,
                     const uint32_t *bits, int r, const float *b_min, const float *b_max, int n_dirs, const float *dirs,
                     const float *basis, float weight, float bias_w, float step_w, int max_steps, uint64_t *mask,
                     float *prt, mp_stream stream);
int mp_mesh_transfer_batch(mp_ctx *ctx, int n_frames, const float *const *verts, const float *const *normals,
                           int64_t max_verts, const int32_t *const *counts, const uint32_t *const *bits, int r,
                           const float *b_min, const float *b_max, int n_dirs, const float *dirs, const float *basis,
                           float weight, float bias_w, float step_w, int max_steps, uint64_t *const *mask,
                           float *const *prt, mp_stream stream);
int mp_mesh_transfer_shade(mp_ctx *ctx, const float *prt, int64_t max_verts, const int32_t *counts, const float *sh,
                           float *out, mp_stream stream);
int mp_mesh_transfer_shade_batch(mp_ctx *ctx, int n_frames, const float *const *prt, int64_t max_verts,
                                 const int32_t *const *counts, const float *sh, float *const *out, mp_stream stream);
int mp_picture_light_transfer(mp_ctx *ctx, const float *normal, const int32_t *face_id, const float *albedo,
                              const float *albedo_rgb, const float *visibility, const float *ambient, int64_t n_pixels,
                              const float *direct_dir, const float *direct_rgb, float gamma, float background,
                              float *image_out, float *shading, mp_stream stream);
int mp_picture_light_transfer_batch(mp_ctx *ctx, int n_frames, const float *const *normal,
                                    const int32_t *const *face_id, const float *const *albedo, const float *albedo_rgb,
                                    const float *const *visibility, const float *const *ambient, int64_t n_pixels,
                                    const float *direct_dir, const float *direct_rgb, float gamma, float background,
                                    float *const *image_out, float *const *shading, mp_stream stream);

/* Pictures as bytes (RTL/main.py:541-553: np.uint8(...), cv2.imencode(".jpg", ...)): the 8-bit picture and the JPEG
 * file of a float picture, made on the device.  The definition is this library's own, all-integer after step 1, and
 * tests/jpeg_ref.py restates it in numpy: the device's bytes equal the restatement's, the same in every run.
 *   Container: baseline sequential DCT JPEG in JFIF: 8-bit samples, components Y, Cb, Cr with ids 1, 2, 3, Huffman
 * coding with the four tables of ITU-T T.81 Annex K.3 (selector 0 for Y, 1 for Cb / Cr).  Segments: SOI, APP0 (JFIF
 * 1.01, no units, 1:1), DQT 0, DQT 1, SOF0, DHT (DC 0, AC 0, DC 1, AC 1), DRI, SOS, the entropy-coded data with RSTm
 * between restart intervals, EOI.  The header is 629 bytes.
 *   Given a picture [H,W,3] f32 (1 <= H, W <= MP_JPEG_MAX_SIDE):
 *   1. 8 bit: t = x > 0 ? (x < 1 ? x : 1) : 0 (a NaN: 0), u = (int)((t * 255) + 0.5): the multiply and the add are two
 *      separately rounded f32 operations (no FMA), the conversion truncates.  mp_picture_u8 is this step alone:
 *      image [n_pixels,3] f32 -> out [n_pixels,3] uint8; n_pixels == 0: MP_OK; a null or misaligned (4 bytes) image, a
 *      null out, n_pixels < 0 or out overlapping image: MP_ERR_ARG; n_pixels > 2^31 / 3: MP_ERR_UNSUPPORTED.
 *   2. Padding to a multiple of the MCU (8 x 8 for MP_JPEG_444, 16 x 16 for MP_JPEG_420) by repeating the last column
 *      and row of u.
 *   3. Colour, int32 with an arithmetic >>:  Y = (19595 R + 38470 G + 7471 B + 32768) >> 16,
 *      Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 32767) >> 16,
 *      Cr = (32768 R - 27439 G - 5329 B + (128 << 16) + 32767) >> 16.
 *   4. Subsampling: MP_JPEG_444 (H = V = 1 everywhere) or MP_JPEG_420 (Y 2 x 2): Cb and Cr are then the 2 x 2 box
 *      (a + b + c + d + 2) >> 2 of step 3's values.
 *   5. Forward DCT per 8 x 8 block P (row y, column x) with C[u][x] = rint(8192 a(u) cos((2x + 1) u pi / 16)),
 *      a(0) = sqrt(1/8), a(u > 0) = 1/2, computed once in float64 (64 integer literals):
 *      rows A[y][u] = (sum_x C[u][x] (P[y][x] - 128) + 1024) >> 11, columns F[v][u] = (sum_y C[v][y] A[y][u] + 16384)
 *      >> 15.  Every intermediate fits int32; |F| <= 1024.
 *   6. Quantisation: the Annex K.1 tables scaled as the IJG library scales them: s = 5000 / quality below 50, else
 *      200 - 2 quality; Q = clamp((base s + 50) / 100, 1, 255) in integer division; the coefficient is
 *      sign(F) ((|F| + (Q >> 1)) / Q), put into zig-zag order.
 *   7. Entropy coding: MCUs in raster order, the blocks of an MCU as Y00 Y01 Y10 Y11 Cb Cr (420) or Y Cb Cr (444).
 *      Per block the DC difference to the previous block of the same component (0 at the start of a restart interval)
 *      as category + magnitude bits, the AC coefficients as (run, size) symbols with ZRL (0xF0) for runs above 15, and
 *      EOB (0x00) unless coefficient 63 is non-zero: at most 1660 bits.  A restart interval is `restart` MCUs (1..65535;
 *      0: the MCUs of one MCU row) and DRI carries it; each interval is padded with 1-bits to a byte, every 0xFF data
 *      byte is followed by 0x00, and RST(k mod 8) follows interval k except the last.
 *   mp_picture_jpeg: n pictures of one size, CONTIGUOUS: images [n,H,W,3] f32 (a slot's pictures already are), so
 *   the call takes one base pointer, no pointer arrays, and is not bound by mp_max_frames() (n <= 65535).  out
 *   [n,capacity] uint8 receives file i at out + i * capacity; info [n,2] int32 = {bytes of file i, overflowed}.  The size
 *   of a file is known on the device before any of it is written: where it exceeds `capacity`, NOTHING of that picture
 *   is written, info[i] = {the size it needs, 1}, and the other pictures are unaffected; no store lands past capacity
 *   under any input.  A second call with capacity >= info[i][0] gives the bytes a sufficient capacity would have given.
 *   mp_jpeg_max_bytes: what no file of that geometry exceeds: 629 + 416 per block (208 bytes of bit string, doubled for
 *   stuffing) + 2 per interval; 0 for a geometry mp_picture_jpeg refuses.  Typical files are a small fraction of it.
 *   Six launches (transform, block coding, interval scan, interval merge, offsets, emit), integer atomics only, nothing
 *   allocated: 552 bytes of the stream's scratch arena per block and 12 per interval.  Asynchronous, no host value.
 *   Refusals (a message, nothing launched): h or w outside 1..MP_JPEG_MAX_SIDE, an unknown subsampling, n > 65535:
 *   MP_ERR_UNSUPPORTED; quality outside 1..100, restart outside 0..65535, n < 1, capacity below the header's 629 bytes or
 *   above 2^31, a null or misaligned (4 bytes: images, info) buffer, out / info overlapping images or each other:
 *   MP_ERR_ARG. */
#define MP_JPEG_MAX_SIDE 4096
enum { MP_JPEG_444 = 0, MP_JPEG_420 = 1 };
int mp_picture_u8(mp_ctx *ctx, const float *image, int64_t n_pixels, uint8_t *out, mp_stream stream);
int64_t mp_jpeg_max_bytes(int h, int w, int subsampling, int restart);
int mp_picture_jpeg(mp_ctx *ctx, const float *images, int n, int h, int w, int quality, int subsampling, int restart,
                    uint8_t *out, int64_t capacity, int32_t *info, mp_stream stream);

/* Pictures as lossless bytes, with their alpha (the reference reads and writes .png throughout its data side): the PNG
 * file of a float picture, made on the device.  As for JPEG the definition is this library's own, all-integer after the
 * samples, and tests/png_ref.py restates it in numpy byte for byte; zlib and any PNG reader give the samples back.
 *   Container: the PNG signature, IHDR (bit depth 8 with colour type 2 (MP_PNG_RGB8) or 6 (MP_PNG_RGBA8), bit depth 16
 * with colour type 0 (MP_PNG_GRAY16); compression 0, filter 0, no interlace), the zlib stream cut into IDAT chunks of
 * MP_PNG_IDAT_BYTES data bytes (the last one shorter), IEND.  Byte k of the zlib stream is byte
 * 41 + 12 (k / MP_PNG_IDAT_BYTES) + k of the file, so every chunk's CRC-32 stands alone.  16-bit samples are big-endian.
 *   Samples.  RGB8: step 1 of the JPEG definition.  RGBA8: the same rule on alpha [H,W] f32 as the fourth byte; with
 * `unmatte` (a resolved pixel is c = a s + (1 - a) bg and PNG alpha is straight) the colour of a pixel with a > 0 is
 * s = (c - (1 - a) * bg) / a in four separately rounded f32 operations, then the 8-bit rule; a <= 0 or a NaN: colour
 * and alpha 0.  GRAY16: t = (d - lo) * scale (two operations), t > 0 ? (t < 1 ? t : 1) : 0 (a NaN: 0),
 * u = (int)((t * 65535) + 0.5), two operations.  mp_picture_u16 (depth [n_pixels] -> uint16 [n_pixels], host order) and
 * mp_picture_rgba8 (image [n_pixels,3], alpha [n_pixels] -> [n_pixels,4]) are these steps alone, refusing as
 * mp_picture_u8 does, and a non-finite lo, scale or background (MP_ERR_ARG).
 *   Filtering, bpp = 3, 4 or 2: every scanline is its filter type and its filtered bytes.  MP_PNG_NONE .. MP_PNG_PAETH
 * use that type on every line; MP_PNG_ADAPTIVE takes per line the type with the smallest sum of min(b, 256 - b) over
 * its filtered bytes, the lowest type on a tie.  The filtered bytes of all lines are the stream x of S = H (1 + W bpp)
 * bytes.
 *   Deflate.  x is cut into blocks of MP_PNG_BLOCK_BYTES = 4096 bytes (the last one shorter); a block is also the parse
 * unit.  Every block is a dynamic-Huffman block, the last one with BFINAL.
 *   Matching: the candidate distances are those of 1, bpp, 2 bpp, stride - bpp, stride, stride + bpp and 2 stride
 * (stride = 1 + W bpp) that lie in 1..32768, ascending, without repeats.  The run of d at i is the count of j = i, i + 1,
 * ... with j - d >= 0 and x[j] == x[j - d], stopped at the block's end and at 258 (sources may lie before the block).
 * The match at i is the longest run if it is >= 3, the smallest distance on a tie.
 *   Parse: greedy from the block's first byte: a match where there is one (then i += length), else the literal x[i];
 * then the end-of-block symbol.  Lengths and distances map to symbols and extra bits by RFC 1951 (258 is symbol 285).
 *   Codes: the counts of the 286 literal/length symbols and of the 30 distance symbols of the block give code lengths:
 * no used symbol: all 0 (one distance code of length 0 is sent: HDIST = 1); one: length 1; else a Huffman tree built by
 * joining, 'used symbols - 1' times, the live node with the smallest (weight, index) and then the next one, where a
 * leaf's index is its symbol and a joined node's index follows every earlier index.  Where the deepest leaf exceeds 15,
 * every non-zero count becomes (c + 1) >> 1 and the tree is built again.  Codes are canonical.  HLIT and HDIST drop
 * trailing zero lengths (257 and 1 at least).  The HLIT + HDIST lengths as one sequence are run-length coded from the
 * left: a run of zeros as 18 (11..138) while >= 11 remain, then 17 (3..10), then single 0s; a run of v > 0 as v, then
 * 16 (3..6) while >= 3 remain, then single v.  Those 19 symbols get lengths by the same rule with limit 7; HCLEN drops
 * trailing zeros in the RFC's order (4 at least).
 *   Stream: 0x78 0x01, the blocks back to back, bits LSB first with Huffman codes bit-reversed, zero bits to a byte,
 * Adler-32 of x big-endian.
 *   mp_png_max_bytes: a token covers at least one byte and costs at most 16 bits per byte (a literal: 15; three bytes
 * of match: 15 + 5 + 15 + 13), a block adds at most 3 + 14 + 19 * 3 + 316 * 7 + 15 = 2301 bits = 288 bytes:
 * z = 6 + 2 S + 288 ceil(S / 4096), file = 57 + 12 ceil(z / MP_PNG_IDAT_BYTES) + z; 0 for a geometry the call refuses.
 *   mp_picture_png: n pictures of one size, CONTIGUOUS: images [n,H,W,3] f32 ([n,H,W] for MP_PNG_GRAY16), alpha [n,H,W]
 * f32 for MP_PNG_RGBA8, else null.  out, capacity, info and overflow are those of mp_picture_jpeg, word for word: the
 * size is known on the device before any byte is written, an overflowing picture writes NOTHING and reports the size it
 * needs, the others are unaffected, no store lands past capacity, and a second call at the reported size gives the
 * bytes a sufficient capacity gives.  lo and scale are read for MP_PNG_GRAY16, background with unmatte != 0.
 *   Six launches (samples + filter, block coding, sizes, clearing the stream words, emit, framing + CRC), integer
 * atomics only, nothing allocated: of the stream's scratch arena 3 bytes per filtered byte, 352 per block, and per
 * picture min(capacity, mp_png_max_bytes) + 16.  Asynchronous, no host value.
 *   Refusals (a message, nothing launched): h or w outside 1..MP_PNG_MAX_SIDE, an unknown format or filter, n > 65535:
 * MP_ERR_UNSUPPORTED; n < 1, capacity below MP_PNG_MIN_BYTES or above 2^31, a null or misaligned (4 bytes: images,
 * alpha, info) buffer, alpha given without MP_PNG_RGBA8 or missing with it, unmatte without alpha, a non-finite lo,
 * scale or background, out / info overlapping the inputs or each other: MP_ERR_ARG. */
#define MP_PNG_MAX_SIDE 4096
#define MP_PNG_BLOCK_BYTES 4096
#define MP_PNG_IDAT_BYTES 8192
#define MP_PNG_MIN_BYTES 57
enum { MP_PNG_RGB8 = 0, MP_PNG_RGBA8 = 1, MP_PNG_GRAY16 = 2 };
enum { MP_PNG_NONE = 0, MP_PNG_SUB = 1, MP_PNG_UP = 2, MP_PNG_AVERAGE = 3, MP_PNG_PAETH = 4, MP_PNG_ADAPTIVE = 5 };
int mp_picture_u16(mp_ctx *ctx, const float *depth, int64_t n_pixels, float lo, float scale, uint16_t *out,
                   mp_stream stream);
int mp_picture_rgba8(mp_ctx *ctx, const float *image, const float *alpha, int64_t n_pixels, int unmatte,
                     float background, uint8_t *out, mp_stream stream);
int64_t mp_png_max_bytes(int h, int w, int format);
int mp_picture_png(mp_ctx *ctx, const float *images, const float *alpha, int n, int h, int w, int format, int filter,
                   float lo, float scale, int unmatte, float background, uint8_t *out, int64_t capacity, int32_t *info,
                   mp_stream stream);

/* Meshes as bytes (the reference writes .obj text on the host, mesh_util.save_obj_mesh*): the binary glTF 2.0 file
 * (.glb) of a mesh as the chain leaves it, quantised under KHR_mesh_quantization and laid out on the device.  No entropy
 * coder: every stage is a stream.  As for JPEG and PNG the definition is this library's own, byte for byte, the same
 * bytes in every run; tests/glb_ref.py restates it in numpy and reads the files back by the glTF specification alone.
 *   Counts: nv = min(max(counts[0], 0), max_verts), nf = min(max(counts[1], 0), max_faces), as in mp_mesh_smooth.  The
 * attribute set is `flags`: MP_GLB_NORMALS (normals given), MP_GLB_COLORS (colors given).
 *   Container: the 12-byte header ("glTF", uint32 2, uint32 total length), one chunk (uint32 length, "JSON", the text)
 * padded with spaces to the next length L with L % 8 == 4 -- a multiple of 4, and the binary data then starts at a
 * multiple of 8 in the file --, one chunk (uint32 length, "BIN\0", the data) padded with zeros to 4 bytes.  All
 * integers little-endian.  EMPTY mesh (nv == 0 or nf == 0; a gated-off frame's counts are {0, 0}): the fixed file of
 * MP_GLB_MIN_BYTES = 100 bytes, the header and the JSON chunk
 *   {"asset":{"version":"2.0","generator":"monoport_amd"},"scene":0,"scenes":[{}]}
 * padded with two spaces; no BIN chunk.
 *   JSON of a mesh, without any white space but the padding of the numbers, in this order, where [N] is present with
 * MP_GLB_NORMALS, [C] with MP_GLB_COLORS, k = the number of attributes (1..3) and c = k - 1:
 *   {"asset":{"version":"2.0","generator":"monoport_amd"},"extensionsUsed":["KHR_mesh_quantization"],
 *   "extensionsRequired":["KHR_mesh_quantization"],"scene":0,"scenes":[{"nodes":[0]}],
 *   "nodes":[{"mesh":0,"translation":[T,T,T],"scale":[S,S,S]}],"materials":[{"doubleSided":true}],
 *   "meshes":[{"primitives":[{"attributes":{"POSITION":0[N: ,"NORMAL":1][C: ,"COLOR_0":c]},"indices":k,"material":0,
 *   "mode":4}]}],"accessors":[
 *   {"bufferView":0,"componentType":5123,"count":<nv>,"type":"VEC3","min":[<m>,<m>,<m>],"max":[<m>,<m>,<m>]}
 *   [N: ,{"bufferView":1,"componentType":5120,"normalized":true,"count":<nv>,"type":"VEC3"}]
 *   [C: ,{"bufferView":c,"componentType":5121,"normalized":true,"count":<nv>,"type":"VEC3"}]
 *   ,{"bufferView":k,"componentType":<ct>,"count":<3 nf>,"type":"SCALAR"}],"bufferViews":[
 *   {"buffer":0,"byteOffset":<o>,"byteLength":<l>,"byteStride":8,"target":34962}
 *   [N: ,{"buffer":0,"byteOffset":<o>,"byteLength":<l>,"byteStride":4,"target":34962}]
 *   [C: ,{"buffer":0,"byteOffset":<o>,"byteLength":<l>,"byteStride":4,"target":34962}]
 *   ,{"buffer":0,"byteOffset":<o>,"byteLength":<l>,"target":34963}],"buffers":[{"byteLength":<b>}]}
 * (the line breaks above are not part of the text).  T = b_min[a] and S = (b_max[a] - b_min[a]) / 65535 in double from
 * the host's f32 box, printed as %24.17g.  Every number in <> depends on the mesh and is a right-aligned decimal
 * padded with leading spaces to a fixed width: 10 for counts, offsets and lengths, 4 for <ct> (5123 UNSIGNED_SHORT or
 * 5125 UNSIGNED_INT), 5 for <m>.  The text has a constant length per attribute set: the host builds it once per call
 * and the device fills the numbers in.  The winding of the chain is kept; the material is double-sided.
 *   Views, in the order positions, normals, colours, indices, back to back (each starts at a multiple of 4):
 * positions 8 nv bytes, normals 4 nv, colours 4 nv, indices 6 nf (16-bit) or 12 nf bytes; <b> = the BIN chunk's
 * length = their sum rounded up to 4.  mp_glb_bytes(nv, nf, flags) = 12 + 8 + L(flags) + 8 + <b>, or MP_GLB_MIN_BYTES
 * for an empty mesh, or 0 for negative counts or unknown flags; mp_glb_max_bytes(max_verts, max_faces, flags) =
 * mp_glb_bytes at the capacities: what no mesh within them exceeds.
 *   POSITION: UNSIGNED_SHORT VEC3, not normalised, 8 bytes per vertex: x, y, z, and a zero uint16.  Per axis
 * inv_a = 65535.0f / (b_max[a] - b_min[a]) in f32 on the host; t = (x - b_min[a]) * inv_a as two separately rounded f32
 * operations (no FMA); q = t > 0 ? (t < 65535 ? (int)(t + 0.5f) : 65535) : 0, so a NaN gives 0.  The node's translation
 * and scale take q back into the box.  <m>: min and max are the exact extremes of q per axis over the nv vertices.
 *   NORMAL: BYTE VEC3, normalised, 4 bytes per vertex: x, y, z, and a zero byte.  t = n != n ? 0 : (n > -1 ? (n < 1 ?
 * n : 1) : -1); q = (int)((t * 127.0f) + (t < 0 ? -0.5f : 0.5f)), two operations.
 *   COLOR_0: UNSIGNED_BYTE VEC3, normalised, 4 bytes per vertex: r, g, b, and a zero byte.  c = (p * color_scale) +
 * color_bias in two operations, then step 1 of the JPEG definition (mp_picture_u8) on c.  colors is [max_verts,3]
 * (MP_GLB_COLOR_ROWS) or [3,max_verts] (MP_GLB_COLOR_PLANES): the chain's raw netC predictions as planes with (0.5, 0.5)
 * give the bytes of the finished colours as rows with (1, 0).
 *   Indices: UNSIGNED_SHORT if nv <= 65535 (index 65535 then never occurs), else UNSIGNED_INT: chosen per mesh on the
 * device.  Faces and corners keep their order.  An index i becomes min(max(i, 0), nv - 1); the chain makes none outside.
 *   mp_mesh_glb: verts f32 [max_verts,3], faces int32 [max_faces,3], counts device int32[2], normals f32 [max_verts,3]
 * or NULL, colors f32 or NULL, b_min / b_max HOST float[3].  out, capacity, info and overflow are those of
 * mp_picture_jpeg, word for word: out [n,capacity] bytes, info int32 [n,2] = {bytes of file f, overflowed}; the size is
 * known on the device before any byte is written, a mesh whose file exceeds capacity writes NOTHING and reports the
 * size it needs, the others are unaffected, no store lands past capacity under any input, and a second call at the
 * reported size gives the bytes a sufficient capacity gives.  Bytes of a row beyond its file are not written.
 *   Three launches for all frames (sizes, info and the reset of the extremes; the attributes and indices with the
 * extremes by a wave reduction and integer atomics into 64 partial slots per frame; the slots joined, the header and
 * the JSON with its numbers), nothing allocated, no host value, asynchronous; 8 KB per frame of the stream's scratch
 * arena (64 slots of one 128-byte line), every word that is read written before.  Rows of `out` that are 4-byte aligned in memory are written in whole dwords (8 bytes per position); any other
 * row byte by byte, to the same bytes.
 *   Refusals (a message, nothing launched): n_frames outside 1..mp_max_frames(), a negative capacity of vertices or
 * faces, a NULL or misaligned (4 bytes; out: any) buffer (verts / normals / colors may be NULL with max_verts == 0,
 * faces with max_faces == 0), an output overlapping an input or the other output, a non-finite box or one without
 * b_max > b_min on an axis or too thin for inv_a to be finite, a non-finite color_scale or color_bias, an unknown
 * color_layout, capacity below MP_GLB_MIN_BYTES or above 2^31: MP_ERR_ARG; capacities for which mp_glb_max_bytes
 * reaches 2^31: MP_ERR_UNSUPPORTED. */
#define MP_GLB_MIN_BYTES 100
enum { MP_GLB_NORMALS = 1, MP_GLB_COLORS = 2 };
enum { MP_GLB_COLOR_ROWS = 0, MP_GLB_COLOR_PLANES = 1 };
int64_t mp_glb_bytes(int64_t nv, int64_t nf, int flags);
int64_t mp_glb_max_bytes(int64_t max_verts, int64_t max_faces, int flags);
int mp_mesh_glb(mp_ctx *ctx, const float *verts, int64_t max_verts, const int32_t *faces, int64_t max_faces,
                const int32_t *counts, const float *normals, const float *colors, int color_layout, float color_scale,
                float color_bias, const float *b_min, const float *b_max, uint8_t *out, int64_t capacity, int32_t *info,
                mp_stream stream);
/* The call above over n_frames (1..mp_max_frames(), else MP_ERR_ARG) meshes of one capacity in the same three
 * launches: verts / faces / counts are HOST arrays of n_frames device pointers, normals / colors such arrays or NULL
 * as a whole; out [n_frames,capacity], info [n_frames,2].  Frame f's bytes and info equal the single call's BIT FOR
 * BIT. */
int mp_mesh_glb_batch(mp_ctx *ctx, int n_frames, const float *const *verts, int64_t max_verts,
                      const int32_t *const *faces, int64_t max_faces, const int32_t *const *counts,
                      const float *const *normals, const float *const *colors, int color_layout, float color_scale,
                      float color_bias, const float *b_min, const float *b_max, uint8_t *out, int64_t capacity,
                      int32_t *info, mp_stream stream);

/* A texture atlas of a mesh (the reference's data side loads textured meshes throughout; COLOR_0 above carries one
 * netC sample per vertex, which a simplified mesh has few of): every face gets a small right triangle of its own in a
 * square picture, and mp_mesh_atlas writes that picture as the G-buffer of a render in TEXTURE space -- face ids and
 * world positions, laid out exactly as one view of H = W = A of the rasteriser's, so that mp_picture_points, the
 * counted netC queries, mp_picture_paint and mp_picture_png run on it unchanged.  Bit for bit, a pure function of its
 * inputs; tests/atlas_ref.py restates it in numpy.
 *   Sizes: the atlas side A is a power of two in MP_ATLAS_MIN_SIZE..MP_ATLAS_MAX_SIZE (64..4096: (k + 0.5) / A is
 * exact in f32 and A <= MP_PNG_MAX_SIDE), the cell side T is in MP_ATLAS_MIN_CELL..MP_ATLAS_MAX_CELL (4..64),
 * G = A / T (integer division) cells per row and per column; the texels beyond G T are unused.  The atlas holds 2 G^2
 * faces.  Counts: nv and nf as in mp_mesh_glb, and nf = 0 where nv == 0; an index i becomes min(max(i, 0), nv - 1).
 *   Cells: face f < F = min(nf, 2 G^2) lives in cell q = f >> 1, at column q % G and row q / G; texel rows count from
 * the top (row 0 is v = 0, glTF's UV origin).  With (i, j) = the (column, row) of a texel inside its cell:
 *   h = f & 1 = 0, the lower half: leg l = T - 2, corners at (0,0), (l,0), (0,l); it owns every texel with
 *     i + j <= T - 1 (the diagonal T - 1 is its gutter); a = i, b = j.
 *   h = 1, the upper half: leg l = T - 3, corners at (T-1,T-1), (T-1-l,T-1), (T-1,T-1-l); it owns i + j >= T (the
 *     diagonal T is its gutter); a = T-1-i, b = T-1-j.
 * Every bilinear footprint of a point inside a face's UV triangle, its edges and corners included, then lies in that
 * face's own texels.
 *   An owned texel gets face_id = f and, with v0, v1, v2 the face's vertices, s = (float)a / (float)l and
 * t = (float)b / (float)l, position = (v0 + s * (v1 - v0)) + t * (v2 - v0) per axis: six f32 operations, each rounded
 * separately, no FMA; gutter texels (a + b > l) are the same map extrapolated.  EVERY other texel -- the unused half of
 * an odd last pair, cells past the last face, the margins -- gets face_id = -1 and position = (background, background,
 * background): all A^2 texels are written whatever the buffers held.  info int32[2] = {F, nf}: info[1] > info[0]
 * tells an atlas that is too small (the faces from F on are laid out nowhere).
 *   UVs are not stored: corner k of face f has (u, v) = ((x_k + 0.5) / A, (y_k + 0.5) / A) with (x_k, y_k) the texel
 * of that corner in the picture (the cell's origin plus the corner above), exact in f32.
 *   mp_mesh_atlas: verts f32 [max_verts,3], faces int32 [max_faces,3], counts device int32[2]; face_id int32 [A A],
 * position f32 [A A,3], info device int32[2].  One launch, one thread per texel, no atomics, no scratch, nothing
 * allocated, asynchronous.  mp_mesh_atlas_batch: n_frames meshes of one capacity in the same ONE launch (host arrays of
 * device pointers); frame f equals the single call BIT FOR BIT.
 *   Refusals (a message, nothing launched): atlas_size not a power of two in 64..4096, cell outside 4..64, n_frames
 * outside 1..mp_max_frames(), a negative capacity, a NULL or misaligned (4 bytes) buffer (verts may be NULL with
 * max_verts == 0, faces with max_faces == 0), an output overlapping an input or another output, a non-finite
 * background: MP_ERR_ARG; capacities beyond 2^31 / 3: MP_ERR_UNSUPPORTED. */
#define MP_ATLAS_MIN_SIZE 64
#define MP_ATLAS_MAX_SIZE 4096
#define MP_ATLAS_MIN_CELL 4
#define MP_ATLAS_MAX_CELL 64
int mp_mesh_atlas(mp_ctx *ctx, const float *verts, int64_t max_verts, const int32_t *faces, int64_t max_faces,
                  const int32_t *counts, int atlas_size, int cell, float background, int32_t *face_id, float *position,
                  int32_t *info, mp_stream stream);
int mp_mesh_atlas_batch(mp_ctx *ctx, int n_frames, const float *const *verts, int64_t max_verts,
                        const int32_t *const *faces, int64_t max_faces, const int32_t *const *counts, int atlas_size,
                        int cell, float background, int32_t *const *face_id, float *const *position,
                        int32_t *const *info, mp_stream stream);

/* Textured meshes as bytes: the .glb of a mesh with the atlas above as its base colour texture, the image inside the
 * file.  Container, padding, the fixed-width number template, out / capacity / info, POSITION and NORMAL quantisation
 * are those of mp_mesh_glb, word for word; tests/glb_texture_ref.py restates the file byte for byte.
 *   Primitive: NOT indexed ("mode":4 without "indices"): 3 nf vertices in face-corner order, vertex 3 f + k = corner k
 * of face f, because a vertex's UV differs per face.  nv, nf and the clamp of an index as in mp_mesh_glb; the mesh is
 * EMPTY (the fixed 100-byte file, the image not looked at) where nv == 0 or nf == 0.
 *   Attributes: POSITION and, with MP_GLB_NORMALS, NORMAL of the corner's vertex, 8 and 4 bytes as above; POSITION's
 * min / max are the exact extremes over the 3 nf corners.  TEXCOORD_0: FLOAT VEC2, 8 bytes: the closed form of the
 * atlas (atlas_size, cell).  COLOR_0 is refused together with a texture: glTF multiplies the two.
 *   JSON, with [N] as above, c = 1 + [N], k = c + 1:
 *   {"asset":{"version":"2.0","generator":"monoport_amd"},"extensionsUsed":["KHR_mesh_quantization"],
 *   "extensionsRequired":["KHR_mesh_quantization"],"scene":0,"scenes":[{"nodes":[0]}],
 *   "nodes":[{"mesh":0,"translation":[T,T,T],"scale":[S,S,S]}],"materials":[{"doubleSided":true,
 *   "pbrMetallicRoughness":{"baseColorTexture":{"index":0},"metallicFactor":0,"roughnessFactor":1}}],
 *   "textures":[{"sampler":0,"source":0}],
 *   "samplers":[{"magFilter":9729,"minFilter":9729,"wrapS":33071,"wrapT":33071}],
 *   "images":[{"bufferView":k,"mimeType":"image/png"}],
 *   "meshes":[{"primitives":[{"attributes":{"POSITION":0[N: ,"NORMAL":1],"TEXCOORD_0":c},"material":0,"mode":4}]}],
 *   "accessors":[
 *   {"bufferView":0,"componentType":5123,"count":<3 nf>,"type":"VEC3","min":[<m>,<m>,<m>],"max":[<m>,<m>,<m>]}
 *   [N: ,{"bufferView":1,"componentType":5120,"normalized":true,"count":<3 nf>,"type":"VEC3"}]
 *   ,{"bufferView":c,"componentType":5126,"count":<3 nf>,"type":"VEC2"}],"bufferViews":[
 *   {"buffer":0,"byteOffset":<o>,"byteLength":<l>,"byteStride":8,"target":34962}
 *   [N: ,{"buffer":0,"byteOffset":<o>,"byteLength":<l>,"byteStride":4,"target":34962}]
 *   ,{"buffer":0,"byteOffset":<o>,"byteLength":<l>,"byteStride":8,"target":34962}
 *   ,{"buffer":0,"byteOffset":<o>,"byteLength":<l>}],"buffers":[{"byteLength":<b>}]}
 * Linear filtering without a mip chain (mips would bleed across cells), clamped at the edges.
 *   Views, back to back: positions 24 nf bytes, normals 12 nf, texture coordinates 24 nf, then the IMAGE as the last
 * view, so that every other offset is a closed form of nf: the p = png_info[f][0] bytes of row f of `png`, the file
 * mp_picture_png (MP_PNG_RGB8, a picture [A,A]) wrote before on the same stream, copied as they are; <b> = the sum
 * rounded up to 4 with zeros.  mp_glb_textured_bytes(nf, flags, png_bytes) = 12 + 8 + L + 8 + <b>, MP_GLB_MIN_BYTES
 * for nf == 0, 0 for negative arguments or flags other than MP_GLB_NORMALS; mp_glb_textured_max_bytes(max_faces, flags,
 * atlas_size) = the same with mp_png_max_bytes(A, A, MP_PNG_RGB8), 0 where that is 0.
 *   info[f] = {bytes, code}: code 0: the file is out[f][:bytes]; 1: the file exceeds `capacity`: NOTHING is written
 * and bytes is the size it needs; 2: the mesh has more faces than the atlas's 2 G^2, or its image is unusable
 * (png_info[f][1] != 0: the PNG overflowed; or png_info[f][0] outside MP_PNG_MIN_BYTES..png_capacity): NOTHING is
 * written and bytes is 0.
 *   mp_mesh_glb_textured: verts, faces, counts, normals (or NULL), b_min, b_max, out, capacity, info as in mp_mesh_glb;
 * colors must be NULL; png uint8 [png_capacity] and png_info int32[2] on the device.  Three launches as there (the PNG
 * is copied by the second), integer atomics only for POSITION's extremes, 8 KB per frame of the stream's scratch
 * arena, no host value, asynchronous.  mp_mesh_glb_textured_batch: n_frames meshes in the same three launches, png
 * [n_frames,png_capacity] and png_info [n_frames,2] CONTIGUOUS as mp_picture_png leaves them; frame f equals the single
 * call BIT FOR BIT.
 *   Refusals: those of mp_mesh_glb and of mp_mesh_atlas's sizes; colors given, a NULL png or png_info, a misaligned
 * png_info, png_capacity below MP_PNG_MIN_BYTES or above 2^31, out or info overlapping png or png_info: MP_ERR_ARG;
 * capacities for which mp_glb_textured_max_bytes reaches 2^31: MP_ERR_UNSUPPORTED. */
int64_t mp_glb_textured_bytes(int64_t nf, int flags, int64_t png_bytes);
int64_t mp_glb_textured_max_bytes(int64_t max_faces, int flags, int atlas_size);
int mp_mesh_glb_textured(mp_ctx *ctx, const float *verts, int64_t max_verts, const int32_t *faces, int64_t max_faces,
                         const int32_t *counts, const float *normals, const float *colors, int atlas_size, int cell,
                         const uint8_t *png, int64_t png_capacity, const int32_t *png_info, const float *b_min,
                         const float *b_max, uint8_t *out, int64_t capacity, int32_t *info, mp_stream stream);
int mp_mesh_glb_textured_batch(mp_ctx *ctx, int n_frames, const float *const *verts, int64_t max_verts,
                               const int32_t *const *faces, int64_t max_faces, const int32_t *const *counts,
                               const float *const *normals, const float *const *colors, int atlas_size, int cell,
                               const uint8_t *png, int64_t png_capacity, const int32_t *png_info, const float *b_min,
                               const float *b_max, uint8_t *out, int64_t capacity, int32_t *info, mp_stream stream);

/* The largest connected body of an occupancy volume [R,R,R] (no counterpart in the reference; the clean-up in front
 * of marching cubes that drops floating blobs).
 *   Foreground: voxels with value > level (marching cubes' "inside"; a NaN and value == level are background).
 *   Components: those of the foreground under `connectivity`: MP_CONN_6 (face neighbours) or MP_CONN_26 (face, edge
 * and corner neighbours).  A component's id is the smallest linear index (z*R + y)*R + x among its voxels.  The
 * component with the most voxels is kept; of several that large, the one with the smallest id.
 *   out[v] = volume[v] (the same bits) for every background voxel and every voxel of the kept component, `fill` for
 * every other foreground voxel; without foreground, out == volume.  `fill` must not be foreground itself: fill > level
 * and a NaN fill are refused (MP_ERR_ARG).  `out` may be `volume`.
 *   stats (device int32[4]): [0] foreground voxels, [1] components, [2] voxels of the kept component, [3] its id
 * (-1 without foreground).
 *   A union-find labelling with integer atomics only: the result is a pure function of the input, the same bits in
 * every run.  Six launches; scratch from the stream's arena: 4 * ceil4(r^3) + 1024 bytes (68 MB at 257^3).
 * r^3 >= 2^31: MP_ERR_UNSUPPORTED.  Asynchronous.  The batched call with one frame and no gate; its refusals carry
 * its own name. */
enum { MP_CONN_6 = 6, MP_CONN_26 = 26 };
int mp_volume_keep_largest(mp_ctx *ctx, const float *volume, int r, float level, int connectivity, float fill,
                           float *out, int32_t *stats, mp_stream stream);
/* The call above over n_frames (1..mp_max_frames(), else MP_ERR_ARG) volumes of one resolution in ONE set of six
 * launches; volume / out / stats / gate are HOST arrays of n_frames device pointers, each as in the per-volume call.
 * Frame f's out and stats equal those of mp_volume_keep_largest on frame f's inputs BIT FOR BIT; every per-frame size
 * comes from that frame's own device data.
 *   gate (NULL, or entries NULL = frame on), as in mp_marching_cubes_batch: gate[f] is a device int32; if it reads 0,
 * frame f's stats become {0, 0, 0, -1} and nothing else of that frame is read or written (its volume may be the
 * unspecified volume of an mp_recon_batch frame whose status[0] is 0).
 *   Scratch from the stream's arena: n_frames * (4 * ceil4(r^3) + 1024) bytes.  Refusals as in the per-volume call,
 * each with an mp_last_error message; a null or not 4-byte aligned buffer of any frame: MP_ERR_ARG.  Asynchronous. */
int mp_volume_keep_largest_batch(mp_ctx *ctx, int n_frames, const float *const *volume, int r, float level,
                                 int connectivity, float fill, float *const *out, int32_t *const *stats,
                                 const int32_t *const *gate, mp_stream stream);

/* ---- encoder helpers (stand-alone GroupNorm / upsample / concat kernels -- the
 * convolutions are the mp_conv* entry points below, nothing of the inference path is left on MIOpen) ---------- */
/* y = [relu](GroupNorm(groups, C)(x)): x, y [N,C,HW] f32 (contiguous NCHW), gamma/beta [C];
 * biased variance, eps inside the sqrt -- torch.nn.GroupNorm as used by
 * backbones/HGFilters.py:23-27 and ResBlkFilters.py:19.  Needs HW % 4 == 0. */
int mp_group_norm(mp_ctx *ctx, const float *x, int n, int c, int64_t hw, int groups,
                  const float *gamma, const float *beta, float eps, int relu, float *y,
                  mp_stream stream);
/* y = [add +] bicubic_x2(x), align_corners=True, A = -0.75 (F.interpolate at HGFilters.py:108 and
 * the skip add at :111).  x [C,H,W] (fold a batch into C); add (may be NULL), y [C,2H,2W]. */
int mp_upsample_bicubic2x(mp_ctx *ctx, const float *x, int c, int h, int w, const float *add,
                          float *y, mp_stream stream);

/* y = cat((a, b, c), channel axis) + shortcut: the tail of the encoders' pyramid block
 * (backbones/HGFilters.py:57-60: torch.cat((out1, out2, out3), 1) followed by `out3 += residual`)
 * in one pass.  a [N,Ca,HW], b [N,Cb,HW], c [N,Cc,HW], shortcut and y [N,Ca+Cb+Cc,HW]; HW % 4 == 0. */
int mp_concat3_add(mp_ctx *ctx, const float *a, int ca, const float *b, int cb, const float *c,
                   int cc, const float *shortcut, int n, int64_t hw, float *y, mp_stream stream);

/* ---- encoder convolutions with fused GroupNorm (hand-written, f32 MFMA) ------------------------ */
/* The pyramid block of the encoders is conv3x3(relu(GroupNorm(x))) three times
 * (backbones/HGFilters.py:40-62).  mp_conv3x3_gn computes
 *     y = conv3x3(v, W),  v = relu?(x * scale[n,c] + shift[n,c])  (v = x when ss == NULL),
 * stride 1, zero padding 1 (applied to v), no bias -- nn.Conv2d(Cin, Cout, 3, 1, 1, bias=False) on
 * the normalised tensor -- as an implicit GEMM on v_mfma_f32_32x32x2_f32, and optionally emits the
 * partial sums the NEXT GroupNorm(32, Cout) needs.  x [N,Cin,H,W], y [N,Cout,H,W] contiguous NCHW;
 * ss [N,Cin,2] = (scale, shift) from mp_gn_finalize; packed = W re-ordered by mp_conv3x3_pack
 * (Cout*Cin*9 floats).  stats: NULL or double [N,32,S,2] (per image, group and tile) with S = mp_conv3x3_stat_slices(Cout,N,H,W,f16) (f16 = 0 here, 1 for mp_conv3x3_gn16).
 * Needs Cin % 16 == 0 (16 .. 512), Cout % 32 == 0, H and W powers of two (H >= 8, W >= 32); else
 * MP_ERR_UNSUPPORTED.  The statistics of y (stats here, fin of mp_conv3x3_ex and mp_convk) are served where
 * mp_conv_stats_supported(Cout): Cout / 32 divides 32 (Cout = 32, 64, 128, 256, 512, 1024) -- the epilogues fold
 * whole groups out of a workgroup's 32- / 64- / 128-channel block; any other Cout gets y (and y2 / fin2) but
 * MP_ERR_UNSUPPORTED when its own statistics are requested.
 * mp_conv3x3_tune(nr): measurement hook -- force nr (1, 2, 4) 32-pixel column blocks per wave
 * instead of the launch-size heuristic (0 restores it); | 0x100 forces the large-tile kernel, | 0x200
 * the split-K kernel, | 0x400 the direct kernels by the heuristic, | 0x800 / | 0x1000 the 64- / 128-channel Winograd
 * kernel, | mrw << 12 the row blocks per wave of mp_conv1x1 (mrw = 1, the same bit as 0x1000, is that kernel's own
 * choice); process-wide, not for production use. */
int mp_conv3x3_pack(mp_ctx *ctx, const float *w /*[Cout,Cin,3,3]*/, int cout, int cin, float *packed,
                    mp_stream stream);
int mp_conv3x3_supported(int cin, int cout, int h, int w); /* 1 if the shape is built, else 0 */
int mp_conv_stats_supported(int cout); /* 1 if a 3x3 / ks x ks launch can emit GroupNorm(32, Cout) statistics of y */
int mp_conv3x3_stat_slices(int cout, int n, int h, int w, int f16);
void mp_conv3x3_tune(int nr);
/* mp_query_tune(small_tiles): measurement hook for the fused f32 query of the netG heads on
 * sampled features -- launches of fewer than small_tiles 64-point tiles run on the 32-point-tile
 * kernel (query_small.hip), the others on the 64-point kernel (query.hip).  0: never, 1: always,
 * negative: the default (2048).  The two kernels return identical bits. */
void mp_query_tune(int small_tiles);
int mp_conv3x3_gn(mp_ctx *ctx, const float *x, int n, int cin, int h, int w, const float *ss, int relu,
                  int reflect, const float *packed, int cout, float *y, double *stats, mp_stream stream);
/* reflect != 0: nn.ReflectionPad2d(1) + an unpadded 3x3 convolution (the residual blocks of the
 * netC encoder, backbones/ResBlkFilters.py:28-84) instead of zero padding.
 * mp_scale_shift_add: y = res + (t * scale[n,c] + shift[n,c]) -- x + GroupNorm(conv(.)) at the end of
 * such a block (no ReLU), ss from mp_gn_finalize; t, res, y [N,C,HW], HW % 4 == 0. */
int mp_scale_shift_add(mp_ctx *ctx, const float *t, const float *ss, const float *res, int n, int c,
                       int64_t hw, float *y, mp_stream stream);
/* The same convolution on split-f16 operands ("f16x3": every operand hi + lo, three
 * v_mfma_f32_32x32x16_f16 per product term, f32 accumulation; f32-class accuracy, the arithmetic of
 * MP_PREC_F16X3).  mp_conv3x3_pack16 writes the pre-split weights (Cout*Cin*9*4 bytes) and
 * max|W| (device float[1], from which pack and convolution derive the same power-of-two operand
 * scale); fully asynchronous. */
int mp_conv3x3_pack16(mp_ctx *ctx, const float *w, int cout, int cin, void *packed16, float *wmax,
                      mp_stream stream);
int mp_conv3x3_gn16(mp_ctx *ctx, const float *x, int n, int cin, int h, int w, const float *ss, int relu,
                    int reflect, const void *packed16, const float *wmax, int cout, float *y, double *stats,
                    mp_stream stream);
/* The 1x1 convolutions of the hourglass tail (backbones/HGFilters.py:184-204: conv_last, l, bl,
 * al; nn.Conv2d(C, 256, 1) with bias) and the 1x1 projection of a pyramid block whose channel
 * count changes (HGFilters.py:47-52: GroupNorm, ReLU, Conv2d(Cin, Cout, 1, bias=False)) as one
 * fused GEMM each:
 *     y = W [relu?(x1 * scale + shift) ; x2] + bias (+ res)
 * cout = 256, or 128 (then no stats / y_hwc); bias may be NULL; x1 [N,C1,HW] with optional fused GroupNorm (ss1 [N,C1,2]) + ReLU; x2 [N,C2,HW] an
 * optional second K segment (bl(y) + al(out) is ONE call with W = [W_bl | W_al], bias = b_bl +
 * b_al, res = x); outputs: y [N,256,HW] and / or y_hwc [N,HW,256] (the channels-last map the
 * query kernels read, written in 1 KB bursts) -- at least one; stats: NULL or the partial sums of
 * GroupNorm(32, 256) over the output, double [N,32,mp_conv1x1_stat_slices(HW),2].  mp_conv1x1_pack re-orders
 * W1 [cout,C1] (and W2 [cout,C2]) into fragment order: cout*(C1+C2) floats, or the same number of
 * (hi, lo) f16 pairs when f16 != 0 (then wmax, device float[1], receives max|W|).  C1, C2 and HW
 * must be multiples of 64. */
int mp_conv1x1_pack(mp_ctx *ctx, const float *w1, int c1, const float *w2, int c2, int cout, int f16,
                    void *packed, float *wmax, mp_stream stream);
int mp_conv1x1(mp_ctx *ctx, const float *x1, const float *ss1, int relu1, const float *x2, int n, int c1,
               int c2, int cout, int64_t hw, const void *packed, int f16, const float *wmax,
               const float *bias, const float *res, float *y, float *y_hwc, double *stats, mp_stream stream);
/* GroupNorm statistics as two steps.  mp_gn_stats: partial (sum, sum of squares) of x [N,C,HW] per
 * (image, group, slice) -> double [N*groups, mp_gn_stat_slices(), 2] (one read pass; for tensors
 * that do not come out of mp_conv3x3_gn).  mp_gn_finalize: partial sums (either source) -> ss [N,C,2] =
 * (gamma rstd, beta - mean gamma rstd), biased variance over `count` elements per group, eps inside
 * the square root (torch.nn.GroupNorm). */
int mp_gn_stat_slices(void);
int mp_gn_stats(mp_ctx *ctx, const float *x, int n, int c, int64_t hw, int groups, double *partial,
                mp_stream stream);
int mp_gn_finalize(mp_ctx *ctx, const double *partial, int n, int c, int groups, int slices,
                   int64_t count, const float *gamma, const float *beta, float eps, float *ss,
                   mp_stream stream);

/* ---- GroupNorm handed from producer to consumer (round 3) --------------------------------------
 * Every GroupNorm(32, C) of the encoders (backbones/HGFilters.py:23-27, ResBlkFilters.py:19) needs
 * the statistics of a whole (image, group) before the first normalised value exists.  The kernels
 * below ADD the per-group sums of the tensor they WRITE into an accumulator (fire-and-forget 64-bit
 * integer atomics on a fixed-point representation: order-independent, hence deterministic), and the
 * kernel that READS the tensor turns the accumulator into (mean, rstd) in its prologue and applies
 * scale = rstd * gamma[c], shift = beta[c] - mean * scale while it stages its input.  A normalised
 * tensor never exists in memory and a GroupNorm costs neither a launch nor a wait (csrc/gn_tail.h
 * records the variants that were measured and dropped).
 *   accumulator  int64 [R,N,32,4] per normalised tensor, R = mp_gn_acc_replicas() copies that the
 *                producers' workgroups spread over (same-address device atomics serialise) and the
 *                consumer adds up; a group's 4 words = (sum hi, sum lo, sumsq hi, sumsq lo) with
 *                value = hi * 2^-16 + lo * 2^-64; it must be ZERO before the producing launch
 *                (hipMemsetAsync one arena per encoder pass) and is complete when that launch has
 *                finished; several launches may fill disjoint groups of one accumulator (the three
 *                convolutions of a pyramid block);
 *   mp_gn_out    producer side: acc and / or the legacy partial-sum buffer (partial_doubles >=
 *                N * 32 * slices * 2 with the launch's mp_*_stat_slices; finalise with
 *                mp_gn_finalize); both NULL = no statistics;
 *   mp_gn_in     consumer side: acc + the GroupNorm's gamma / beta / eps, or the legacy precomputed
 *                ss [N,C,2] from mp_gn_finalize, or all NULL = plain input. */
int mp_gn_acc_replicas(void);
typedef struct mp_gn_out {
  int64_t *acc;
  double *partial;
  int64_t partial_doubles;
} mp_gn_out;
typedef struct mp_gn_in {
  const int64_t *acc;
  const float *gamma;
  const float *beta;
  float eps;
  const float *ss;
} mp_gn_in;

/* mp_conv3x3_gn / mp_conv3x3_gn16 with the pyramid block's tail and the GroupNorm hand-over fused in
 * (backbones/HGFilters.py:40-62).  gn: GroupNorm(32, Cin) of the input (+ ReLU with `relu`).  wmax ==
 * NULL: packed by mp_conv3x3_pack (exact f32); else by mp_conv3x3_pack16.  y may be NULL when y2 is
 * given.  y2 / res [N, y2_channels, H, W]:
 *     y2[n, y2_offset + c] = conv[n, c] + res[n, y2_offset + c]
 * -- torch.cat((out1, out2, out3), 1) + residual (HGFilters.py:57-60) written by the three
 * convolutions themselves.  fin: GroupNorm(32, Cout) over y (the next convolution of the block);
 * fin2: this launch's groups of GroupNorm(32, y2_channels) over y2 (the next block; groups must not
 * straddle launches: y2_offset % (y2_channels / 32) == 0).  Launches too small to fill the chip run
 * a split-K variant (the four waves of a workgroup share one 32-channel x 32/64-pixel tile). */
typedef struct mp_conv3x3_args {
  const float *x;
  int n, cin, h, w;
  mp_gn_in gn;
  int relu, reflect;
  const void *packed;
  const float *wmax;
  int cout;
  float *y;
  float *y2;
  const float *res;
  int y2_channels, y2_offset;
  mp_gn_out fin, fin2;
  /* round 6: NULL, or the Winograd-domain weights of the same convolution (mp_conv3x3_pack_wino, 16 * Cout * Cin
   * floats).  With them, launches that mp_conv3x3_wino_supported serves (zero padding, exact f32, no legacy
   * statistics buffers) run as Winograd F(2x2, 3x3) on the same f32 MFMAs -- 4 / 9 of the multiplies of the direct
   * form; `packed` must still be given (every other launch uses it). */
  const float *packed_wino;
} mp_conv3x3_args;
int mp_conv3x3_ex(mp_ctx *ctx, const mp_conv3x3_args *args, mp_stream stream);
/* U = G g G^T of nn.Conv2d(Cin, Cout, 3, 1, 1) weights (backbones/HGFilters.py:15-19) in the fragment order of
 * csrc/conv_wino.hip, computed in double and rounded once; 16 * Cout * Cin floats, 16-byte aligned. */
int mp_conv3x3_pack_wino(mp_ctx *ctx, const float *w /*[Cout,Cin,3,3]*/, int cout, int cin, float *packed_wino,
                         mp_stream stream);
int mp_conv3x3_wino_supported(int cin, int cout, int h, int w); /* 1 if the Winograd kernel is built for the shape */

/* mp_conv1x1 with the GroupNorm hand-over: gn1 = GroupNorm(32, C1) of x1 (+ ReLU with relu1); fin =
 * GroupNorm(32, 256) over the output (res included), i.e. bn_end after conv_last and the first
 * GroupNorm of the next stack after x + bl(.) + al(.) (HGFilters.py:184-204).  Same tensors and
 * restrictions as mp_conv1x1. */
typedef struct mp_conv1x1_args {
  const float *x1;
  mp_gn_in gn1;
  int relu1;
  const float *x2;
  int n, c1, c2, cout;
  int64_t hw;
  const void *packed;
  int f16;
  const float *wmax;
  const float *bias;
  const float *res;
  float *y;
  float *y_hwc;
  mp_gn_out fin;
} mp_conv1x1_args;
int mp_conv1x1_ex(mp_ctx *ctx, const mp_conv1x1_args *args, mp_stream stream);
int mp_conv1x1_stat_slices(int64_t hw);

/* The encoders' other convolutions on the same MFMA scheme (csrc/convim2col.hip), with an explicit
 * im2col tile in LDS: ks = 7, 3 -> 64 channels, stride 2 + zero padding 3 + bias (the hourglass stem,
 * HGFilters.py:125, :168) or stride 1 + nn.ReflectionPad2d(3) (netC's stem, ResBlkFilters.py:111-113);
 * ks = 3, stride 2, zero padding 1, Cin % 16 == 0, Cout % 128 == 0 (netC's two down-sampling
 * convolutions, ResBlkFilters.py:115-121).  y [N, Cout, H/stride, W/stride], W/stride % 64 == 0.
 * gn / relu: GroupNorm (+ReLU) of the INPUT applied while gathering, as in mp_conv3x3_ex; bias may be
 * NULL; fin: GroupNorm(32, Cout) over y (where mp_conv_stats_supported(Cout): 128, 256, 512 ...; Cout = 384 gets y
 * only).  reflect needs H and W larger than the padding, as nn.ReflectionPad2d does.  packed:
 * mp_convk_packed_floats floats from mp_convk_pack. */
typedef struct mp_convk_args {
  const float *x;
  int n, cin, h, w;
  mp_gn_in gn;
  int relu, reflect;
  const float *packed;
  const float *bias;
  int cout, ks, stride;
  float *y;
  mp_gn_out fin;
} mp_convk_args;
int mp_convk_supported(int cin, int cout, int ks, int stride, int h, int w);
int64_t mp_convk_packed_floats(int cin, int cout, int ks);
int mp_convk_stat_slices(int ks, int stride, int h, int w);
int mp_convk_pack(mp_ctx *ctx, const float *w /*[Cout,Cin,ks,ks]*/, int cout, int cin, int ks, float *packed,
                  mp_stream stream);
int mp_convk(mp_ctx *ctx, const mp_convk_args *args, mp_stream stream);

/* The tensors between the convolutions, written together with their statistics (fin may be NULL;
 * slices of a legacy partial buffer = mp_gn_stat_slices(); C % 32 == 0):
 *   mp_avgpool2_gn            y [N,C,H/2,W/2] = avg_pool2d(x, 2, stride 2)  (HGFilters.py:93, :171), W % 8 == 0
 *   mp_upsample_bicubic2x_gn  y [N,C,2H,2W] = add + bicubic_x2(x)           (HGFilters.py:108-111), add may be NULL
 *   mp_gn_apply               y = [res +] relu?(GroupNorm(x)), gn as above  (the stem's GroupNorm + ReLU, :168;
 *                             x + GroupNorm(conv(.)) at the end of a residual block, ResBlkFilters.py:75-84) */
int mp_avgpool2_gn(mp_ctx *ctx, const float *x, int n, int c, int h, int w, float *y, const mp_gn_out *fin,
                   mp_stream stream);
int mp_upsample_bicubic2x_gn(mp_ctx *ctx, const float *x, int n, int c, int h, int w, const float *add, float *y,
                             const mp_gn_out *fin, mp_stream stream);
int mp_gn_apply(mp_ctx *ctx, const float *x, const mp_gn_in *gn, int relu, int n, int c, int64_t hw,
                const float *res, float *y, const mp_gn_out *fin, mp_stream stream);
/* 1 if mp_upsample_bicubic2x_gn runs the shape on the banded kernel that shares the horizontal sums through LDS
 * (2W divides 256, 2H % 16 == 0, (C / 32 * 2H) % 256 == 0), 0 if on the one-output-per-thread kernel.  Host only: the
 * rule the launcher itself dispatches by; both kernels write the same bits. */
int mp_upsample_gn_banded(int c, int h, int w);

/* ---- recorded launch sequences ------------------------------------------------------------------
 * The reference calls netG.filter once per frame from a stage thread (RTL/main.py:366-370): here that is ~137
 * launches of the entry points above.  A PLAN is that sequence recorded once -- the same argument structs, in
 * order, each with the stream slot it ran on -- and replayed by ONE call: no host interpreter between the
 * launches.  The recorder owns every buffer (inputs, intermediates, outputs: static for the life of the plan,
 * copy in and out around mp_plan_run); the plan stores pointers only.  Slot 0 is the stream passed to
 * mp_plan_run; slots 1..n_side_streams are streams the plan creates (the hourglass's skip branches run on side
 * streams at batch <= 2); MP_PLAN_WAIT makes one slot wait for the work enqueued so far on another.  Replays of
 * one plan must be ordered on one stream (its buffers are static).  mp_plan_run returns the first failing
 * command's status (mp_last_error); the commands after it are not enqueued, and the plan's side streams are joined
 * into `stream` before the call returns, so nothing of the partial replay runs unordered against the caller. */
typedef struct mp_plan mp_plan;
enum {
  MP_PLAN_CONVK = 1,      /* args: mp_convk_args            -> mp_convk */
  MP_PLAN_GN_APPLY = 2,   /* args: mp_plan_gn_apply_args    -> mp_gn_apply */
  MP_PLAN_CONV3X3 = 3,    /* args: mp_conv3x3_args          -> mp_conv3x3_ex */
  MP_PLAN_CONV1X1 = 4,    /* args: mp_conv1x1_args          -> mp_conv1x1_ex */
  MP_PLAN_AVGPOOL2 = 5,   /* args: mp_plan_pool_args        -> mp_avgpool2_gn */
  MP_PLAN_UPSAMPLE2X = 6, /* args: mp_plan_upsample_args    -> mp_upsample_bicubic2x_gn */
  MP_PLAN_MEMSET = 7,     /* args: mp_plan_memset_args      -> hipMemsetAsync (the GroupNorm accumulator arena) */
  MP_PLAN_WAIT = 8        /* args: mp_plan_wait_args        -> event record on one slot, wait on another */
};
typedef struct mp_plan_gn_apply_args {
  const float *x;
  mp_gn_in gn;
  int relu, n, c;
  int64_t hw;
  const float *res;
  float *y;
  mp_gn_out fin;
} mp_plan_gn_apply_args;
typedef struct mp_plan_pool_args {
  const float *x;
  int n, c, h, w;
  float *y;
  mp_gn_out fin;
} mp_plan_pool_args;
typedef struct mp_plan_upsample_args {
  const float *x;
  int n, c, h, w;
  const float *add;
  float *y;
  mp_gn_out fin;
} mp_plan_upsample_args;
typedef struct mp_plan_memset_args {
  void *ptr;
  int64_t bytes;
  int value;
} mp_plan_memset_args;
typedef struct mp_plan_wait_args {
  int waiter_slot, signaller_slot;
} mp_plan_wait_args;
int mp_plan_create(mp_ctx *ctx, int n_side_streams, mp_plan **out);
int mp_plan_add(mp_plan *plan, int kind, const void *args, int64_t bytes, int stream_slot);
int mp_plan_size(mp_plan *plan);
int mp_plan_run(mp_plan *plan, mp_stream stream);
void mp_plan_destroy(mp_plan *plan); /* drains and destroys the plan's side streams */

/* ---- measurement ------------------------------------------------------------------------------ */
/* Brackets every fused-query kernel launch made through this context with a pair of HIP events
 * recorded on the launch stream (bench.py's roofline leg).  mp_profile_end waits for the last
 * event and writes the elapsed milliseconds of up to `capacity` launches, in launch order, to
 * ms_out (host); *n_out = launches recorded. */
int mp_profile_begin(mp_ctx *ctx, int max_records);
int mp_profile_end(mp_ctx *ctx, float *ms_out /*host*/, int capacity, int *n_out /*host*/);

/* What the f32 matrix pipe of this device sustains right now and at which shader clock: a register-only loop of
 * v_mfma_f32_32x32x2_f32 on random mantissas, two 4-wave workgroups per CU, about ms_target (1..2000) milliseconds,
 * timed with HIP events; every workgroup reads the shader clock counter and the 100 MHz reference around its loop.
 * out4 (host): [0] TFLOP/s, [1] average shader clock in MHz during the launch, [2] the launch's ms, [3] workgroups.
 * Synchronises the stream and holds the context's mutex while it runs (every other call on this context waits up
 * to ms_target): a set-up / measurement call, not one for a running pipeline.  bench.py reports it as `roofline.sustained` next to the nominal peak (boxes of one pool
 * hold clocks a few per cent apart under a matrix load).  No counterpart in the reference. */
int mp_mfma_clock_probe(mp_ctx *ctx, float ms_target, double *out4 /*host*/, mp_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* MONOPORT_HIP_H */
