// The texture atlas of a mesh (mp_mesh_atlas[_batch], include/monoport_hip.h): the G-buffer of a render in texture
// space.  Every face has a right triangle of its own in a cell of T x T texels, two faces per cell; the picture of
// face ids and world positions is laid out as one view of H = W = A of the rasteriser's, so the picture stages run on
// it unchanged.
//   atlas_kernel   blockIdx.y = frame, one thread per texel: the texel's cell, half and face from its coordinates
//                  alone, the face's three vertices, the affine map; a 4-byte and a 12-byte store per thread, both
//                  coalesced over the wave.  Texels without a face are written too: the call leaves no texel as it was
// Every float operation is one IEEE f32 operation in the order the header states.
#include "mp_internal.h"
#include "mesh_common.h"

#include <cstring>

#pragma clang fp contract(off)

namespace mp {

constexpr int kAtlasBlock = 256;

struct AtlasFrames {
  const float *verts[kMaxFrames];
  const int32_t *faces[kMaxFrames];
  const int32_t *counts[kMaxFrames];
  int32_t *face_id[kMaxFrames];
  float *position[kMaxFrames];
  int32_t *info[kMaxFrames];
};
static_assert(sizeof(AtlasFrames) + 64 <= 4096, "mp_mesh_atlas: kernel arguments");

__global__ __launch_bounds__(kAtlasBlock) void atlas_kernel(AtlasFrames fr, long long max_v, long long max_f, int size,
                                                            int shift, int cell, int grid, float background) {
  const int f = blockIdx.y;
  const int32_t *__restrict__ counts = fr.counts[f];
  const int nv = mesh_min(counts[0], max_v);
  const int nf = nv > 0 ? mesh_min(counts[1], max_f) : 0;
  const long long room = 2LL * grid * grid;
  const int laid = nf < room ? nf : (int)room;
  const int p = blockIdx.x * kAtlasBlock + threadIdx.x;  // < size * size <= 2^24: the grid is exact
  if (p == 0) fr.info[f][0] = laid, fr.info[f][1] = nf;
  const int x = p & (size - 1), y = p >> shift;
  const int cx = x / cell, cy = y / cell;
  int face = -1;
  float pos[3] = {background, background, background};
  if (cx < grid && cy < grid) {
    const int i = x - cx * cell, j = y - cy * cell;
    const int h = i + j >= cell;
    const int id = 2 * (cy * grid + cx) + h;
    if (id < laid) {
      const int a = h ? cell - 1 - i : i, b = h ? cell - 1 - j : j;
      const int leg = cell - 2 - h;
      const float s = (float)a / (float)leg;
      const float t = (float)b / (float)leg;
      const int32_t *__restrict__ tri = fr.faces[f] + 3LL * id;
      const float *__restrict__ verts = fr.verts[f];
      int c[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const int v = tri[k];
        c[k] = v < 0 ? 0 : (v >= nv ? nv - 1 : v);
      }
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const float v0 = verts[3LL * c[0] + k];
        const float e1 = verts[3LL * c[1] + k] - v0;
        const float e2 = verts[3LL * c[2] + k] - v0;
        const float along = s * e1;
        const float base = v0 + along;
        const float across = t * e2;
        pos[k] = base + across;
      }
      face = id;
    }
  }
  fr.face_id[f][p] = face;
  float *__restrict__ out = fr.position[f] + 3LL * p;
  out[0] = pos[0], out[1] = pos[1], out[2] = pos[2];
}

int launch_mesh_atlas_batch(mp_ctx *ctx, int n_frames, const float *const *verts, long long max_v,
                            const int32_t *const *faces, long long max_f, const int32_t *const *counts, int size,
                            int cell, float background, int32_t *const *face_id, float *const *position,
                            int32_t *const *info, hipStream_t st) {
  AtlasFrames fr;
  std::memset(&fr, 0, sizeof(fr));
  for (int f = 0; f < n_frames; ++f) {
    fr.verts[f] = verts ? verts[f] : nullptr;
    fr.faces[f] = faces ? faces[f] : nullptr;
    fr.counts[f] = counts[f];
    fr.face_id[f] = face_id[f], fr.position[f] = position[f], fr.info[f] = info[f];
  }
  int shift = 0;
  while ((1 << shift) < size) ++shift;
  const dim3 grid((unsigned)(((long long)size * size) / kAtlasBlock), n_frames);  // size >= 64: a whole number
  hipLaunchKernelGGL(atlas_kernel, grid, dim3(kAtlasBlock), 0, st, fr, max_v, max_f, size, shift, cell, size / cell,
                     background);
  MP_HIP(ctx, hipGetLastError());
  return MP_OK;
}

}  // namespace mp
