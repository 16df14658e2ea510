// PNG on the device (mp_picture_u16 / mp_picture_rgba8 / mp_picture_png, include/monoport_hip.h): n float pictures of
// one size -> n PNG files (8-bit RGB, 8-bit RGBA, 16-bit grey), all-integer after the samples and defined byte for byte.
//   png_filter   one wavefront per scanline, lane = byte (strided): the samples of the line and of the one above from
//                the floats, the five filters' sums of |signed byte| (adaptive), the chosen filter's bytes
//   png_block    one workgroup per 4096-byte block, 16 bytes per thread, the block in LDS: per candidate distance the
//                first mismatch behind every byte (a thread's own 16, then at most 17 neighbours' firsts) gives the run;
//                the greedy parse by pointer doubling (12 rounds); LDS histograms; the two Huffman trees in wavefronts 0
//                and 1 (keys in registers, the two smallest by wave reductions); the code-length code; the block's bit
//                count, its code lengths and its Adler-32 part
//   png_sizes    one workgroup per picture: exclusive scan of the blocks' bits, the Adler-32 of the parts, the file's
//                size against the capacity -> info
//   (clear)      the stream words of the call, zeroed
//   png_emit     one workgroup per block: canonical codes, the header by one lane, every token's bits placed by a
//                prefix sum and OR-ed into the block's bit string in LDS, the string stored at its place in the
//                picture's stream (the two words it shares with its neighbours: integer atomicOr)
//   png_frame    one workgroup per IDAT chunk: length, type, data at their final offsets, the CRC-32 from 256 raw CRCs
//                of 33 bytes combined by their exact rule; chunk 0 adds the signature and IHDR, the last one IEND.
//                Nothing of a picture that overflowed is written, and every store is bounded by capacity.
// Bits are LSB first: bit k of a string is bit k & 63 of word k >> 6.  The intermediates live in the stream's scratch
// arena; a stage reads only what an earlier stage of the same call wrote.  No float atomics, no inline assembly, no host
// value.
#include "mp_internal.h"

#include <cstring>

namespace mp {

namespace {

constexpr int kWave = 64;
constexpr int kThreads = 256;
constexpr int kBlock = MP_PNG_BLOCK_BYTES;
constexpr int kPer = kBlock / kThreads;  // bytes per thread
constexpr int kIdat = MP_PNG_IDAT_BYTES;
constexpr int kMaxCand = 7;
constexpr int kLensStride = 336;                              // 286 + 30 + 19 code lengths of a block, padded
constexpr int kOutWords = (2301 + 16 * kBlock + 63) / 64 + 2;  // 64-bit words of a block's bit string at any shift
constexpr int kPiece = 33;                                    // bytes per thread of a chunk's CRC: 256 * 33 >= 4 + 8192
constexpr uint32_t kDead = 0xFFFFFFFFu;
constexpr uint32_t kCrcPoly = 0xEDB88320u;
static_assert(kPer == 16 && kThreads * kPiece >= kIdat + 4, "png: the work per thread");

// a(x) b(x) mod the CRC-32 polynomial, bit 31 = x^0 (as zlib's crc32_combine multiplies)
__host__ __device__ constexpr uint32_t crc_mul(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (uint32_t m = 1u << 31; m; m >>= 1) {
    if (a & m) p ^= b;
    b = (b & 1u) ? (b >> 1) ^ kCrcPoly : b >> 1;
  }
  return p;
}
// x^(8 bytes)
constexpr uint32_t crc_shift(long long bytes) {
  uint32_t r = 1u << 31, base = 1u << 23;
  for (; bytes; bytes >>= 1) {
    if (bytes & 1) r = crc_mul(r, base);
    base = crc_mul(base, base);
  }
  return r;
}

// What every kernel of one call shares: the geometry (host values) and the scratch pointers
struct PngGeom {
  int h, w, format, filter, unmatte, bpp, stride;
  float lo, scale, bg;
  long long s;          // filtered bytes per picture
  int nblk, ncand;
  int cand[kMaxCand], cand_sym[kMaxCand], cand_ebits[kMaxCand], cand_eval[kMaxCand];
  long long capacity, zwords;   // 64-bit words of a picture's stream
  uint8_t *filt;                // [n][s]
  uint16_t *tok;                // [n][s]: 0 no token, 0x8000 a literal, else length << 3 | candidate
  uint8_t *lens;                // [n][nblk][kLensStride]
  int32_t *blen, *boff;         // [n][nblk] bits of a block, and before it
  uint32_t *adl;                // [n][nblk][2] the block's sum of bytes and of (end - i) byte, mod 65521
  uint32_t *pic;                // [n][4] bytes of the zlib stream, Adler-32, chunks
  unsigned long long *zbuf;     // [n][zwords]
  uint32_t crck[8];             // x^(8 * kPiece * 2^l)
  uint8_t head[33];             // signature and IHDR
};

__device__ __forceinline__ int to_u8(float x) {
  const float t = x > 0.0f ? (x < 1.0f ? x : 1.0f) : 0.0f;
  return (int)__fadd_rn(__fmul_rn(t, 255.0f), 0.5f);
}
__device__ __forceinline__ int to_u16(float d, float lo, float scale) {
  const float v = __fmul_rn(__fsub_rn(d, lo), scale);
  const float t = v > 0.0f ? (v < 1.0f ? v : 1.0f) : 0.0f;
  return (int)__fadd_rn(__fmul_rn(t, 65535.0f), 0.5f);
}
// the colour byte of an unmatted pixel with a > 0
__device__ __forceinline__ int unmatted(float c, float a, float bg) {
  const float t = __fmul_rn(__fsub_rn(1.0f, a), bg);
  return to_u8(__fdiv_rn(__fsub_rn(c, t), a));
}

// byte i of scanline y of a picture (0 outside it)
__device__ __forceinline__ int sample_byte(const PngGeom &ge, const float *__restrict__ img,
                                           const float *__restrict__ al, int y, int i) {
  if (y < 0 || i < 0) return 0;
  const long long row = (long long)y * ge.w;
  if (ge.format == MP_PNG_RGB8) return to_u8(img[row * 3 + i]);
  if (ge.format == MP_PNG_GRAY16) {
    const int u = to_u16(img[row + (i >> 1)], ge.lo, ge.scale);
    return (i & 1) ? (u & 255) : (u >> 8);
  }
  const long long px = row + (i >> 2);
  const int ch = i & 3;
  const float a = al[px];
  if (ge.unmatte && !(a > 0.0f)) return 0;
  if (ch == 3) return to_u8(a);
  const float c = img[px * 3 + ch];
  return ge.unmatte ? unmatted(c, a, ge.bg) : to_u8(c);
}

__global__ __launch_bounds__(kThreads) void picture_u16(const float *__restrict__ in, uint16_t *__restrict__ out,
                                                        long long n, float lo, float scale) {
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (i < n) out[i] = (uint16_t)to_u16(in[i], lo, scale);
}

__global__ __launch_bounds__(kThreads) void picture_rgba8(const float *__restrict__ img, const float *__restrict__ al,
                                                          uint32_t *__restrict__ out, long long n, int unmatte,
                                                          float bg) {
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const float a = al[i];
  uint32_t v = 0;
  if (!unmatte)
    v = (uint32_t)to_u8(img[3 * i]) | ((uint32_t)to_u8(img[3 * i + 1]) << 8) | ((uint32_t)to_u8(img[3 * i + 2]) << 16) |
        ((uint32_t)to_u8(a) << 24);
  else if (a > 0.0f)
    v = (uint32_t)unmatted(img[3 * i], a, bg) | ((uint32_t)unmatted(img[3 * i + 1], a, bg) << 8) |
        ((uint32_t)unmatted(img[3 * i + 2], a, bg) << 16) | ((uint32_t)to_u8(a) << 24);
  out[i] = v;
}

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int d = kWave / 2; d > 0; d >>= 1) v += __shfl_xor(v, d, kWave);
  return v;
}
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
  for (int d = kWave / 2; d > 0; d >>= 1) {
    const int t = __shfl_xor(v, d, kWave);
    v = t > v ? t : v;
  }
  return v;
}
__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
#pragma unroll
  for (int d = kWave / 2; d > 0; d >>= 1) {
    const uint32_t t = (uint32_t)__shfl_xor((int)v, d, kWave);
    v = t < v ? t : v;
  }
  return v;
}

// exclusive scan of one value per thread over a workgroup of kThreads; total: the sum.  lds: kThreads / kWave ints
__device__ __forceinline__ int wg_scan(int v, int *lds, int &total) {
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
  int inc = v;
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    const int t = __shfl_up(inc, d, kWave);
    if (lane >= d) inc += t;
  }
  __syncthreads();  // the previous use of lds is over
  if (lane == kWave - 1) lds[wv] = inc;
  __syncthreads();
  int base = 0;
  total = 0;
#pragma unroll
  for (int i = 0; i < kThreads / kWave; ++i) {
    if (i < wv) base += lds[i];
    total += lds[i];
  }
  return base + inc - v;
}

__device__ __forceinline__ int filter_byte(int kind, int x, int a, int b, int c) {
  int pred = 0;
  if (kind == MP_PNG_SUB) {
    pred = a;
  } else if (kind == MP_PNG_UP) {
    pred = b;
  } else if (kind == MP_PNG_AVERAGE) {
    pred = (a + b) >> 1;
  } else if (kind == MP_PNG_PAETH) {
    const int p = a + b - c;
    const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
    pred = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
  }
  return (x - pred) & 255;
}

__global__ __launch_bounds__(kThreads) void png_filter(const float *__restrict__ images,
                                                       const float *__restrict__ alpha, PngGeom ge) {
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
  const int y = blockIdx.x * (kThreads / kWave) + wv, pic = blockIdx.y;
  if (y >= ge.h) return;  // a whole wave; no barrier below
  const long long px = (long long)pic * ge.h * ge.w;
  const float *img = images + px * (ge.format == MP_PNG_GRAY16 ? 1 : 3);
  const float *al = alpha ? alpha + px : nullptr;
  const int nb = ge.w * ge.bpp;
  int kind = ge.filter;
  if (kind == MP_PNG_ADAPTIVE) {
    int cost[5] = {0, 0, 0, 0, 0};
    for (int i = lane; i < nb; i += kWave) {
      const int x = sample_byte(ge, img, al, y, i), a = sample_byte(ge, img, al, y, i - ge.bpp);
      const int b = sample_byte(ge, img, al, y - 1, i), c = sample_byte(ge, img, al, y - 1, i - ge.bpp);
#pragma unroll
      for (int k = 0; k < 5; ++k) {
        const int f = filter_byte(k, x, a, b, c);
        cost[k] += f < 128 ? f : 256 - f;
      }
    }
    int best = 0;
    kind = 0;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      const int s = wave_sum(cost[k]);
      if (k == 0 || s < best) {
        best = s;
        kind = k;
      }
    }
  }
  uint8_t *__restrict__ out = ge.filt + (long long)pic * ge.s + (long long)y * ge.stride;
  if (lane == 0) out[0] = (uint8_t)kind;
  for (int i = lane; i < nb; i += kWave) {
    const int x = sample_byte(ge, img, al, y, i), a = sample_byte(ge, img, al, y, i - ge.bpp);
    const int b = sample_byte(ge, img, al, y - 1, i), c = sample_byte(ge, img, al, y - 1, i - ge.bpp);
    out[1 + i] = (uint8_t)filter_byte(kind, x, a, b, c);
  }
}

// Code lengths of the N counts in cnt (LDS; halved in place where the limit asks for it) by one whole wavefront: every
// lane keeps the keys weight << 10 | index of the nodes lane, lane + 64, ... in registers
template <int N>
__device__ void huff_build(int *cnt, uint8_t *len, uint16_t *par, int limit, int lane) {
  constexpr int NS = (2 * N - 1 + kWave - 1) / kWave;
  constexpr int LS = (N + kWave - 1) / kWave;
  for (;;) {
    uint32_t k[NS];
    int used = 0;
#pragma unroll
    for (int j = 0; j < NS; ++j) {
      const int idx = lane + kWave * j;
      const int c = (j < LS && idx < N) ? cnt[idx] : 0;
      k[j] = c > 0 ? ((uint32_t)c << 10) | (uint32_t)idx : kDead;
      used += c > 0;
    }
    used = wave_sum(used);
    if (used < 2) {
#pragma unroll
      for (int j = 0; j < LS; ++j) {
        const int idx = lane + kWave * j;
        if (idx < N) len[idx] = cnt[idx] > 0 ? 1 : 0;
      }
      __threadfence_block();
      return;
    }
    for (int m = 0; m < used - 1; ++m) {
      uint32_t ab[2];
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        uint32_t v = kDead;
#pragma unroll
        for (int j = 0; j < NS; ++j) v = k[j] < v ? k[j] : v;
        v = wave_min(v);
        ab[r] = v;
        const int idx = (int)(v & 1023u);
#pragma unroll
        for (int j = 0; j < NS; ++j)
          if (idx == lane + kWave * j) k[j] = kDead;
      }
      const int nidx = N + m;
      const uint32_t key = (((ab[0] >> 10) + (ab[1] >> 10)) << 10) | (uint32_t)nidx;
#pragma unroll
      for (int j = 0; j < NS; ++j)
        if (nidx == lane + kWave * j) k[j] = key;
      if (lane == 0) {
        par[ab[0] & 1023u] = (uint16_t)nidx;
        par[ab[1] & 1023u] = (uint16_t)nidx;
      }
    }
    __threadfence_block();  // one wavefront: its LDS operations complete in order
    const int root = N + used - 2;
    int deepest = 0;
#pragma unroll
    for (int j = 0; j < LS; ++j) {
      const int idx = lane + kWave * j;
      if (idx < N) {
        int d = 0;
        if (cnt[idx] > 0)
          for (int p = idx; p != root; p = par[p]) ++d;
        len[idx] = (uint8_t)d;
        deepest = d > deepest ? d : deepest;
      }
    }
    deepest = wave_max(deepest);
    __threadfence_block();
    if (deepest <= limit) return;
#pragma unroll
    for (int j = 0; j < LS; ++j) {
      const int idx = lane + kWave * j;
      if (idx < N) {
        const int c = cnt[idx];
        cnt[idx] = c > 0 ? (c + 1) >> 1 : 0;
      }
    }
    __threadfence_block();
  }
}

// the run-length coded sequence of the hlit + hdist code lengths, in order: f(symbol, extra bits, extra value)
template <class F>
__device__ __forceinline__ void code_length_tokens(const uint8_t *ll, int hlit, const uint8_t *dl, int hdist, F f) {
  const int n = hlit + hdist;
  int i = 0;
  while (i < n) {
    const int v = i < hlit ? ll[i] : dl[i - hlit];
    int r = 1;
    while (i + r < n && (i + r < hlit ? ll[i + r] : dl[i + r - hlit]) == v) ++r;
    i += r;
    if (v == 0) {
      while (r > 0) {
        if (r >= 11) {
          const int k = r < 138 ? r : 138;
          f(18, 7, k - 11);
          r -= k;
        } else if (r >= 3) {
          f(17, 3, r - 3);
          r = 0;
        } else {
          f(0, 0, 0);
          r -= 1;
        }
      }
    } else {
      f(v, 0, 0);
      r -= 1;
      while (r >= 3) {
        const int k = r < 6 ? r : 6;
        f(16, 2, k - 3);
        r -= k;
      }
      for (; r > 0; --r) f(v, 0, 0);
    }
  }
}

__device__ const uint8_t kClOrder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

// HLIT, HDIST and HCLEN of a block's code lengths
__device__ __forceinline__ void header_counts(const uint8_t *ll, const uint8_t *dl, const uint8_t *cl, int &hlit,
                                              int &hdist, int &hclen) {
  hlit = 286;
  while (hlit > 257 && ll[hlit - 1] == 0) --hlit;
  hdist = 30;
  while (hdist > 1 && dl[hdist - 1] == 0) --hdist;
  hclen = 19;
  while (hclen > 4 && cl[kClOrder[hclen - 1]] == 0) --hclen;
}

// a match length 3..258 -> its symbol - 257, extra bits and extra value (RFC 1951)
__device__ __forceinline__ void length_symbol(int len, int &code, int &ebits, int &eval) {
  const int l = len - 3;
  if (len == 258) {
    code = 28, ebits = 0, eval = 0;
  } else if (l < 8) {
    code = l, ebits = 0, eval = 0;
  } else {
    const int e = (31 - __builtin_clz((unsigned)l)) - 2;
    code = 4 * e + 4 + ((l >> e) & 3);
    ebits = e;
    eval = l & ((1 << e) - 1);
  }
}
__device__ __forceinline__ int length_extra_bits(int code) { return code < 8 || code == 28 ? 0 : (code - 4) >> 2; }
__device__ __forceinline__ int dist_extra_bits(int sym) { return sym < 2 ? 0 : (sym - 2) >> 1; }

__global__ __launch_bounds__(kThreads) void png_block(PngGeom ge) {
  __shared__ uint8_t s_x[kBlock];
  __shared__ uint16_t s_best[kBlock];
  __shared__ uint16_t s_jump[kBlock];
  __shared__ uint8_t s_reach[kBlock];
  __shared__ int s_first[kThreads];
  __shared__ int s_llh[288], s_dh[32], s_clh[20];
  __shared__ int s_llc[288], s_dc[32], s_clc[20];
  __shared__ uint16_t s_llp[576], s_dp[64], s_clp[64];
  __shared__ uint8_t s_lll[288], s_dl[32], s_cll[20];
  __shared__ uint32_t s_sum[4];  // Adler parts, the block's bits, the code-length tokens' extra bits
  __shared__ int s_dsym[8];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wv = tid / kWave;
  const int blk = blockIdx.x, pic = blockIdx.y;
  const long long b0 = (long long)blk * kBlock;
  const int len = (int)(ge.s - b0 < kBlock ? ge.s - b0 : kBlock);
  const uint8_t *__restrict__ x = ge.filt + (long long)pic * ge.s;
  const int p0 = tid * kPer;
  {
    uint32_t sa = 0, sb = 0;
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
      const int p = p0 + j;
      const int v = p < len ? x[b0 + p] : 0;
      s_x[p] = (uint8_t)v;
      s_best[p] = 0;
      sa += (uint32_t)v;
      sb += (uint32_t)v * (uint32_t)(len - p);  // 0 behind the end
    }
    for (int i = tid; i < 288; i += kThreads) s_llh[i] = i == 256 ? 1 : 0;
    if (tid < 32) s_dh[tid] = 0;
    if (tid < 20) s_clh[tid] = 0;
    if (tid < 4) s_sum[tid] = 0;
#pragma unroll
    for (int c = 0; c < kMaxCand; ++c)
      if (tid == c) s_dsym[c] = ge.cand_sym[c];
    __syncthreads();
    // 4096 * 4097 / 2 * 255 < 2^32: the sums cannot wrap
    sa = (uint32_t)wave_sum((int)sa);
    sb = sb % 65521u;
    sb = (uint32_t)wave_sum((int)sb);
    if (lane == 0) {
      atomicAdd(&s_sum[0], sa);
      atomicAdd(&s_sum[1], sb);
    }
  }
  // the longest run per byte over the candidate distances, ascending: a longer run replaces, an equal one does not
#pragma unroll
  for (int c = 0; c < kMaxCand; ++c) {
    if (c < ge.ncand) {  // uniform
      const int d = ge.cand[c];
      uint32_t eq = 0;
#pragma unroll
      for (int j = 0; j < kPer; ++j) {
        const int p = p0 + j;
        if (p < len && b0 + p - d >= 0) {
          const int src = p - d >= 0 ? s_x[p - d] : x[b0 + p - d];
          eq |= (uint32_t)(src == s_x[p]) << j;
        }
      }
      const uint32_t miss = ~eq & 0xFFFFu;
      s_first[tid] = miss ? p0 + __builtin_ctz(miss) : kBlock;
      __syncthreads();
      if (eq) {
        int next = (tid + 18) * kPer;  // the first mismatch behind this thread's bytes, or far enough
        for (int k = 1; k <= 17; ++k) {
          if (tid + k >= kThreads) break;
          const int f = s_first[tid + k];
          if (f < kBlock) {
            next = f;
            break;
          }
        }
        next = next < len ? next : len;
#pragma unroll
        for (int j = kPer - 1; j >= 0; --j) {
          const int p = p0 + j;
          if (!((eq >> j) & 1u)) {
            next = p;
          } else {
            int run = next - p;
            run = run < 258 ? run : 258;
            if (run >= 3 && run > (s_best[p] >> 3)) s_best[p] = (uint16_t)((run << 3) | c);
          }
        }
      }
      __syncthreads();
    }
  }
  // the greedy parse: s_reach marks the bytes a token starts at
  {
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
      const int p = p0 + j;
      const int m = s_best[p] >> 3;
      int to = p + (m ? m : 1);
      s_jump[p] = (uint16_t)(to < len ? to : len);
      s_reach[p] = p == 0;
    }
    __syncthreads();
    for (int round = 0; round < 12; ++round) {
      int to[kPer], to2[kPer];
#pragma unroll
      for (int j = 0; j < kPer; ++j) {
        const int p = p0 + j;
        to[j] = p < len ? s_jump[p] : len;
        to2[j] = to[j] < len ? s_jump[to[j]] : len;
      }
      __syncthreads();
#pragma unroll
      for (int j = 0; j < kPer; ++j) {
        const int p = p0 + j;
        if (p < len) {
          if (s_reach[p] && to[j] < len) s_reach[to[j]] = 1;
          s_jump[p] = (uint16_t)to2[j];
        }
      }
      __syncthreads();
    }
  }
  // tokens and their histograms
  {
    uint16_t *__restrict__ tok = ge.tok + (long long)pic * ge.s + b0;
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
      const int p = p0 + j;
      if (p >= len) continue;
      int t = 0;
      if (s_reach[p]) {
        const int best = s_best[p];
        if (best) {
          int code, eb, ev;
          length_symbol(best >> 3, code, eb, ev);
          atomicAdd(&s_llh[257 + code], 1);
          atomicAdd(&s_dh[s_dsym[best & 7]], 1);
          t = best;
        } else {
          atomicAdd(&s_llh[s_x[p]], 1);
          t = 0x8000;
        }
      }
      tok[p] = (uint16_t)t;
    }
  }
  __syncthreads();
  for (int i = tid; i < 288; i += kThreads) s_llc[i] = s_llh[i];
  if (tid < 32) s_dc[tid] = s_dh[tid];
  __syncthreads();
  if (wv == 0) huff_build<286>(s_llc, s_lll, s_llp, 15, lane);
  if (wv == 1) huff_build<30>(s_dc, s_dl, s_dp, 15, lane);
  __syncthreads();
  if (tid == 0) {
    int hlit, hdist, hclen;
    header_counts(s_lll, s_dl, s_cll, hlit, hdist, hclen);  // hclen: not yet
    int extra = 0;
    code_length_tokens(s_lll, hlit, s_dl, hdist, [&](int sym, int eb, int) {
      s_clh[sym] += 1;
      extra += eb;
    });
    s_sum[3] = (uint32_t)extra;
  }
  __syncthreads();
  if (tid < 20) s_clc[tid] = s_clh[tid];
  __syncthreads();
  if (wv == 0) huff_build<19>(s_clc, s_cll, s_clp, 7, lane);
  __syncthreads();
  {
    int bits = 0;
    for (int s = tid; s < 286; s += kThreads)
      bits += s_llh[s] * ((int)s_lll[s] + (s < 257 ? 0 : length_extra_bits(s - 257)));
    if (tid < 30) bits += s_dh[tid] * ((int)s_dl[tid] + dist_extra_bits(tid));
    if (tid < 19) bits += s_clh[tid] * (int)s_cll[tid];
    if (tid == 0) {
      int hlit, hdist, hclen;
      header_counts(s_lll, s_dl, s_cll, hlit, hdist, hclen);
      bits += 17 + 3 * hclen + (int)s_sum[3];
    }
    bits = wave_sum(bits);
    if (lane == 0) atomicAdd(&s_sum[2], (uint32_t)bits);
  }
  __syncthreads();
  const long long gb = (long long)pic * ge.nblk + blk;
  uint8_t *__restrict__ lens = ge.lens + gb * kLensStride;
  for (int i = tid; i < 286; i += kThreads) lens[i] = s_lll[i];
  if (tid < 30) lens[286 + tid] = s_dl[tid];
  if (tid < 19) lens[316 + tid] = s_cll[tid];
  if (tid == 0) {
    ge.blen[gb] = (int)s_sum[2];
    ge.adl[2 * gb] = s_sum[0] % 65521u;
    ge.adl[2 * gb + 1] = s_sum[1] % 65521u;
  }
}

__global__ __launch_bounds__(kThreads) void png_sizes(PngGeom ge, int32_t *__restrict__ info) {
  __shared__ int s_scan[kThreads / kWave];
  const int pic = blockIdx.x;
  const long long base = (long long)pic * ge.nblk;
  int bits = 0;
  uint32_t a = 1, b = 0;
  for (int i0 = 0; i0 < ge.nblk; i0 += kThreads) {  // uniform trip count: wg_scan holds barriers
    const int i = i0 + threadIdx.x;
    const bool live = i < ge.nblk;
    int total;
    const int ex = wg_scan(live ? ge.blen[base + i] : 0, s_scan, total);
    if (live) ge.boff[base + i] = bits + ex;
    bits += total;
    // Adler-32 of a concatenation: the sums add; the second sum gains length * (first sum before the piece)
    const int pa = live ? (int)ge.adl[2 * (base + i)] : 0;
    const int ea = wg_scan(pa, s_scan, total);
    const int ta = total;
    const long long rest = ge.s - (long long)i * kBlock;
    const uint32_t blen = live ? (uint32_t)(rest < kBlock ? rest : kBlock) : 0u;
    const uint32_t before = (a + (uint32_t)ea) % 65521u;
    const int pb = live ? (int)((blen * before + ge.adl[2 * (base + i) + 1]) % 65521u) : 0;
    wg_scan(pb, s_scan, total);
    a = (a + (uint32_t)ta) % 65521u;
    b = (b + (uint32_t)total) % 65521u;
  }
  if (threadIdx.x == 0) {
    const long long z = 2 + (((long long)bits + 7) >> 3) + 4;
    const long long chunks = (z + kIdat - 1) / kIdat;
    const long long file = 45 + 12 * chunks + z;
    ge.pic[4 * pic] = (uint32_t)z;
    ge.pic[4 * pic + 1] = (b << 16) | a;
    ge.pic[4 * pic + 2] = (uint32_t)chunks;
    info[2 * pic] = (int)file;
    info[2 * pic + 1] = file > ge.capacity ? 1 : 0;
  }
}

// RFC 1951 3.2.2 by one thread: the codes of n lengths, bit-reversed.  next: 16 ints of LDS
__device__ void canonical_codes(const uint8_t *len, int n, uint16_t *code, int *next) {
  for (int b = 0; b < 16; ++b) next[b] = 0;
  for (int s = 0; s < n; ++s) next[len[s]] += 1;
  int c = 0, before = 0;
  for (int b = 1; b < 16; ++b) {
    c = (c + before) << 1;
    before = next[b];
    next[b] = c;
  }
  for (int s = 0; s < n; ++s) {
    const int l = len[s];
    code[s] = l ? (uint16_t)(__brev((unsigned)next[l]++) >> (32 - l)) : (uint16_t)0;
  }
}

// n <= 57 bits of v into the string at bit pos
__device__ __forceinline__ void or_bits(unsigned long long *s, int pos, unsigned long long v, int n) {
  if (n <= 0) return;
  const int w = pos >> 6, sh = pos & 63;
  atomicOr(&s[w], v << sh);
  if (sh + n > 64) atomicOr(&s[w + 1], v >> (64 - sh));
}

__global__ __launch_bounds__(kThreads) void png_emit(PngGeom ge, const int32_t *__restrict__ info) {
  __shared__ unsigned long long s_out[kOutWords];
  __shared__ uint8_t s_len[kLensStride];
  __shared__ uint16_t s_llc[286], s_dc[30], s_clc[19];
  __shared__ int s_next[3][16];
  __shared__ int s_scan[kThreads / kWave];
  __shared__ int s_head;  // the bit behind the block's header
  __shared__ int s_dsym[8], s_deb[8], s_dev[8];
  const int tid = threadIdx.x;
  const int blk = blockIdx.x, pic = blockIdx.y;
  if (info[2 * pic + 1]) return;  // uniform: nothing of a picture that does not fit is written
  const long long gb = (long long)pic * ge.nblk + blk;
  const long long b0 = (long long)blk * kBlock;
  const int len = (int)(ge.s - b0 < kBlock ? ge.s - b0 : kBlock);
  for (int i = tid; i < kLensStride; i += kThreads) s_len[i] = ge.lens[gb * kLensStride + i];
  for (int i = tid; i < kOutWords; i += kThreads) s_out[i] = 0ull;
#pragma unroll
  for (int c = 0; c < kMaxCand; ++c)
    if (tid == c) {
      s_dsym[c] = ge.cand_sym[c];
      s_deb[c] = ge.cand_ebits[c];
      s_dev[c] = ge.cand_eval[c];
    }
  __syncthreads();
  const uint8_t *ll = s_len, *dl = s_len + 286, *cl = s_len + 316;
  if (tid == 0) canonical_codes(ll, 286, s_llc, s_next[0]);
  if (tid == kWave) canonical_codes(dl, 30, s_dc, s_next[1]);
  if (tid == 2 * kWave) canonical_codes(cl, 19, s_clc, s_next[2]);
  __syncthreads();
  const long long start = 16 + (long long)ge.boff[gb];  // behind the two bytes of the zlib header
  const int sh0 = (int)(start & 63);
  if (tid == 0) {
    int pos = sh0;
    auto put = [&](unsigned v, int n) {
      or_bits(s_out, pos, (unsigned long long)v, n);
      pos += n;
    };
    if (blk == 0) s_out[0] |= 0x0178ull;
    int hlit, hdist, hclen;
    header_counts(ll, dl, cl, hlit, hdist, hclen);
    put(blk == ge.nblk - 1 ? 1u : 0u, 1);
    put(2u, 2);
    put((unsigned)(hlit - 257), 5);
    put((unsigned)(hdist - 1), 5);
    put((unsigned)(hclen - 4), 4);
    for (int i = 0; i < hclen; ++i) put(cl[kClOrder[i]], 3);
    code_length_tokens(ll, hlit, dl, hdist, [&](int sym, int eb, int ev) {
      put((unsigned)s_clc[sym] | ((unsigned)ev << cl[sym]), cl[sym] + eb);
    });
    s_head = pos;
  }
  // every token's bits
  const uint16_t *__restrict__ tok = ge.tok + (long long)pic * ge.s + b0;
  const uint8_t *__restrict__ x = ge.filt + (long long)pic * ge.s + b0;
  const int p0 = tid * kPer;
  unsigned long long val[kPer];
  int nb[kPer];
  int mine = 0;
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const int p = p0 + j;
    const int t = p < len ? tok[p] : 0;
    val[j] = 0ull;
    nb[j] = 0;
    if (t == 0x8000) {
      const int s = x[p];
      val[j] = s_llc[s];
      nb[j] = ll[s];
    } else if (t) {
      int code, eb, ev;
      length_symbol(t >> 3, code, eb, ev);
      const int c = t & 7, ds = s_dsym[c];
      int n = ll[257 + code];
      unsigned long long v = s_llc[257 + code];
      v |= (unsigned long long)ev << n;
      n += eb;
      v |= (unsigned long long)s_dc[ds] << n;
      n += dl[ds];
      v |= (unsigned long long)s_dev[c] << n;
      n += s_deb[c];
      val[j] = v;
      nb[j] = n;
    }
    mine += nb[j];
  }
  int total;
  int at = wg_scan(mine, s_scan, total);  // its barriers also publish the header and s_head
  at += s_head;
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    or_bits(s_out, at, val[j], nb[j]);
    at += nb[j];
  }
  if (tid == kThreads - 1) or_bits(s_out, at, s_llc[256], ll[256]);
  __syncthreads();
  const int end = sh0 + ge.blen[gb];
  const int nw = (end + 63) >> 6;
  const long long w0 = start >> 6;
  unsigned long long *__restrict__ z = ge.zbuf + (long long)pic * ge.zwords;
  for (int i = tid; i < nw && i < kOutWords; i += kThreads) {
    if (w0 + i >= ge.zwords) continue;  // never: a picture that fits has its stream below the capacity
    if (i == 0 || i == nw - 1)
      atomicOr(&z[w0 + i], s_out[i]);
    else
      z[w0 + i] = s_out[i];
  }
}

__global__ __launch_bounds__(kThreads) void png_frame(PngGeom ge, const int32_t *__restrict__ info,
                                                      uint8_t *__restrict__ out_all) {
  __shared__ uint32_t s_tab[256];
  __shared__ uint32_t s_crc[kThreads / kWave];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wv = tid / kWave;
  const int k = blockIdx.x, pic = blockIdx.y;
  if (info[2 * pic + 1]) return;  // uniform
  const int chunks = (int)ge.pic[4 * pic + 2];
  if (k >= chunks) return;        // uniform
  const long long cap = ge.capacity;
  uint8_t *__restrict__ out = out_all + (long long)pic * cap;
  const long long zlen = ge.pic[4 * pic];
  const uint32_t adler = ge.pic[4 * pic + 1];
  const uint8_t *__restrict__ zb = reinterpret_cast<const uint8_t *>(ge.zbuf + (long long)pic * ge.zwords);
  const long long z0 = (long long)k * kIdat;
  const int dlen = (int)(zlen - z0 < kIdat ? zlen - z0 : kIdat);
  auto put = [&](long long pos, int v) {
    if (pos >= 0 && pos < cap) out[pos] = (uint8_t)v;
  };
  // byte m of the chunk's type and data
  auto message = [&](int m) -> int {
    if (m < 4) return "IDAT"[m];
    const long long j = z0 + (m - 4);
    return j < zlen - 4 ? zb[j] : (int)((adler >> (8 * (3 - (int)(j - (zlen - 4))))) & 255u);
  };
  {
    uint32_t c = (uint32_t)tid;
#pragma unroll
    for (int i = 0; i < 8; ++i) c = (c & 1u) ? (c >> 1) ^ kCrcPoly : c >> 1;
    s_tab[tid] = c;
  }
  long long at = 0;
  if (k == 0)
    for (int i = tid; i < 33; i += kThreads) put(i, ge.head[i]);
  at = 33 + (long long)k * (kIdat + 12);
  if (tid < 4) put(at + tid, (dlen >> (8 * (3 - tid))) & 255);
  for (int m = tid; m < 4 + dlen; m += kThreads) put(at + 4 + m, message(m));
  __syncthreads();
  // the raw CRC (start 0, no final inversion) of the message with its first four bytes inverted, which stand for the
  // standard's start value; the message is right-aligned in 256 pieces of kPiece bytes: leading zeros change nothing
  const int total = 4 + dlen;
  uint32_t c = 0;
  for (int i = 0; i < kPiece; ++i) {
    const int m = total - (kThreads - tid) * kPiece + i;
    if (m < 0) continue;
    const int v = message(m) ^ (m < 4 ? 255 : 0);
    c = s_tab[(c ^ (uint32_t)v) & 255u] ^ (c >> 8);
  }
  // crc(A B) = crc(A) x^(8 |B|) + crc(B)
#pragma unroll
  for (int l = 0; l < 6; ++l) {
    const uint32_t right = (uint32_t)__shfl_down((int)c, 1 << l, kWave);
    c = crc_mul(ge.crck[l], c) ^ right;
  }
  if (lane == 0) s_crc[wv] = c;
  __syncthreads();
  if (tid == 0) {
    const uint32_t c01 = crc_mul(ge.crck[6], s_crc[0]) ^ s_crc[1];
    const uint32_t c23 = crc_mul(ge.crck[6], s_crc[2]) ^ s_crc[3];
    const uint32_t crc = ~(crc_mul(ge.crck[7], c01) ^ c23);
    for (int i = 0; i < 4; ++i) put(at + 8 + dlen + i, (int)((crc >> (8 * (3 - i))) & 255u));
    if (k == chunks - 1) {
      const uint8_t iend[12] = {0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xAE, 0x42, 0x60, 0x82};
#pragma unroll
      for (int i = 0; i < 12; ++i) put(at + 12 + dlen + i, iend[i]);
    }
  }
}

constexpr size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

int png_bpp(int format) { return format == MP_PNG_RGB8 ? 3 : (format == MP_PNG_RGBA8 ? 4 : 2); }

struct PngSizes {
  long long s, nblk, zwords;
};
PngSizes png_sizes_of(const PngCall &c) {
  PngSizes z;
  z.s = (long long)c.h * (1 + (long long)c.w * png_bpp(c.format));
  z.nblk = (z.s + kBlock - 1) / kBlock;
  const long long top = png_max_bytes(c.h, c.w, c.format);
  z.zwords = ((c.capacity < top ? c.capacity : top) + 7) / 8 + 1;
  return z;
}

uint32_t crc32_host(const uint8_t *p, int n) {
  uint32_t c = 0xFFFFFFFFu;
  for (int i = 0; i < n; ++i) {
    c ^= p[i];
    for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ kCrcPoly : c >> 1;
  }
  return ~c;
}

void put32(uint8_t *p, uint32_t v) {
  p[0] = (uint8_t)(v >> 24);
  p[1] = (uint8_t)(v >> 16);
  p[2] = (uint8_t)(v >> 8);
  p[3] = (uint8_t)v;
}

}  // namespace

int launch_picture_u16(mp_ctx *ctx, const float *depth, long long n_pixels, float lo, float scale, uint16_t *out,
                       hipStream_t st) {
  if (n_pixels == 0) return MP_OK;
  hipLaunchKernelGGL(picture_u16, dim3((unsigned)((n_pixels + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, depth,
                     out, n_pixels, lo, scale);
  MP_HIP(ctx, hipGetLastError());
  return MP_OK;
}

int launch_picture_rgba8(mp_ctx *ctx, const float *image, const float *alpha, long long n_pixels, int unmatte,
                         float background, uint8_t *out, hipStream_t st) {
  if (n_pixels == 0) return MP_OK;
  hipLaunchKernelGGL(picture_rgba8, dim3((unsigned)((n_pixels + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, image,
                     alpha, reinterpret_cast<uint32_t *>(out), n_pixels, unmatte, background);
  MP_HIP(ctx, hipGetLastError());
  return MP_OK;
}

int png_min_bytes() { return MP_PNG_MIN_BYTES; }

long long png_max_bytes(int h, int w, int format) {
  const long long s = (long long)h * (1 + (long long)w * png_bpp(format));
  const long long z = 6 + 2 * s + 288 * ((s + kBlock - 1) / kBlock);
  return 45 + 12 * ((z + kIdat - 1) / kIdat) + z;
}

size_t png_scratch_bytes(const PngCall &c) {
  const PngSizes z = png_sizes_of(c);
  const size_t n = (size_t)c.n, blocks = n * (size_t)z.nblk;
  return align256(n * z.s) + align256(n * z.s * 2) + align256(blocks * kLensStride) + 2 * align256(blocks * 4) +
         align256(blocks * 8) + align256(n * 16) + align256(n * (size_t)z.zwords * 8);
}

int launch_picture_png(mp_ctx *ctx, void *scratch, const float *images, const float *alpha, const PngCall &c,
                       uint8_t *out, int32_t *info, hipStream_t st) {
  static const int dist_base[30] = {1,   2,   3,   4,   5,   7,    9,    13,   17,   25,   33,   49,   65,    97,    129,
                                    193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
  const PngSizes z = png_sizes_of(c);
  PngGeom ge;
  std::memset(&ge, 0, sizeof(ge));
  ge.h = c.h;
  ge.w = c.w;
  ge.format = c.format;
  ge.filter = c.filter;
  ge.unmatte = c.unmatte;
  ge.bpp = png_bpp(c.format);
  ge.stride = 1 + c.w * ge.bpp;
  ge.lo = c.lo;
  ge.scale = c.scale;
  ge.bg = c.background;
  ge.s = z.s;
  ge.nblk = (int)z.nblk;
  ge.capacity = c.capacity;
  ge.zwords = z.zwords;
  // the candidate distances, ascending and without repeats
  const int wanted[kMaxCand] = {1, ge.bpp, 2 * ge.bpp, ge.stride - ge.bpp, ge.stride, ge.stride + ge.bpp, 2 * ge.stride};
  for (int d = 1, last = 0; ge.ncand < kMaxCand;) {
    d = 0;
    for (int i = 0; i < kMaxCand; ++i)
      if (wanted[i] > last && wanted[i] <= 32768 && (d == 0 || wanted[i] < d)) d = wanted[i];
    if (d == 0) break;
    int sym = 29;
    while (dist_base[sym] > d) --sym;
    ge.cand[ge.ncand] = d;
    ge.cand_sym[ge.ncand] = sym;
    ge.cand_ebits[ge.ncand] = sym < 2 ? 0 : (sym - 2) >> 1;
    ge.cand_eval[ge.ncand] = d - dist_base[sym];
    ++ge.ncand;
    last = d;
  }
  for (int l = 0; l < 8; ++l) ge.crck[l] = crc_shift((long long)kPiece << l);
  static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1A, '\n'};
  std::memcpy(ge.head, sig, 8);
  put32(ge.head + 8, 13);
  std::memcpy(ge.head + 12, "IHDR", 4);
  put32(ge.head + 16, (uint32_t)c.w);
  put32(ge.head + 20, (uint32_t)c.h);
  ge.head[24] = c.format == MP_PNG_GRAY16 ? 16 : 8;
  ge.head[25] = c.format == MP_PNG_RGB8 ? 2 : (c.format == MP_PNG_RGBA8 ? 6 : 0);
  put32(ge.head + 29, crc32_host(ge.head + 12, 17));

  const size_t n = (size_t)c.n, blocks = n * (size_t)z.nblk;
  char *p = static_cast<char *>(scratch);
  auto take = [&p](size_t bytes) {
    char *r = p;
    p += align256(bytes);
    return r;
  };
  ge.filt = reinterpret_cast<uint8_t *>(take(n * z.s));
  ge.tok = reinterpret_cast<uint16_t *>(take(n * z.s * 2));
  ge.lens = reinterpret_cast<uint8_t *>(take(blocks * kLensStride));
  ge.blen = reinterpret_cast<int32_t *>(take(blocks * 4));
  ge.boff = reinterpret_cast<int32_t *>(take(blocks * 4));
  ge.adl = reinterpret_cast<uint32_t *>(take(blocks * 8));
  ge.pic = reinterpret_cast<uint32_t *>(take(n * 16));
  ge.zbuf = reinterpret_cast<unsigned long long *>(take(n * (size_t)z.zwords * 8));

  const int wpb = kThreads / kWave;
  hipLaunchKernelGGL(png_filter, dim3((unsigned)((c.h + wpb - 1) / wpb), (unsigned)c.n), dim3(kThreads), 0, st, images,
                     alpha, ge);
  // grid.y is limited to 65535 (the pictures: the caller has checked n); a picture has at most 16385 blocks
  hipLaunchKernelGGL(png_block, dim3((unsigned)z.nblk, (unsigned)c.n), dim3(kThreads), 0, st, ge);
  hipLaunchKernelGGL(png_sizes, dim3((unsigned)c.n), dim3(kThreads), 0, st, ge, info);
  MP_HIP(ctx, hipMemsetAsync(ge.zbuf, 0, n * (size_t)z.zwords * 8, st));
  hipLaunchKernelGGL(png_emit, dim3((unsigned)z.nblk, (unsigned)c.n), dim3(kThreads), 0, st, ge,
                     static_cast<const int32_t *>(info));
  const long long chunks = (z.zwords * 8 + kIdat - 1) / kIdat;
  hipLaunchKernelGGL(png_frame, dim3((unsigned)chunks, (unsigned)c.n), dim3(kThreads), 0, st, ge,
                     static_cast<const int32_t *>(info), out);
  MP_HIP(ctx, hipGetLastError());
  return MP_OK;
}

}  // namespace mp
