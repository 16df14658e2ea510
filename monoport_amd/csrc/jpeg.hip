// Baseline JPEG on the device (mp_picture_u8 / mp_picture_jpeg, include/monoport_hip.h): n float pictures of one size
// -> n JFIF files with restart intervals, all-integer after the 8-bit step and defined bit for bit.
//   picture_u8      four floats per thread: clamp, * 255, + 0.5 as two f32 operations, truncate
//   jpeg_transform  one wavefront per 8x8 block, lane = pixel: 8 bit, colour, 2x2 box (420), the two DCT passes through
//                   LDS, quantise, zig-zag int16 coefficients
//   jpeg_code       one wavefront per block, lane = zig-zag index: the ballot of the non-zeros gives every lane its run
//                   and the EOB position; a lane's symbols fit 59 bits; a wave prefix sum places them in the block's
//                   bit string (LDS, integer OR); the string goes out at a fixed stride with its bit length
//   jpeg_scan       one workgroup per restart interval: exclusive scan of its blocks' bit lengths
//   jpeg_merge      one thread per 64-bit word of an interval's byte string: the blocks that overlap the word, found
//                   by bisection in the scanned offsets, shifted into place; 1-bits pad the last byte; 0xFF bytes are
//                   counted (integer atomicAdd)
//   jpeg_offsets    one workgroup per picture: exclusive scan of bytes + 0xFF count + 2 over its intervals; the total
//                   against the capacity -> info
//   jpeg_emit       one workgroup per interval: the header (interval 0), the stuffed bytes, RSTm or EOI at their final
//                   offsets.  Nothing of a picture that overflowed is written, and every store is bounded by capacity.
// Bit strings are MSB first: bit 63 of word 0 is the first bit of the string.  The intermediates live in the stream's
// scratch arena; a stage reads only what an earlier stage of the same call wrote (no zero fill is assumed).  No float
// atomics, no inline assembly, no host value.
#include "mp_internal.h"

#include <cstring>

namespace mp {

namespace {

constexpr int kWave = 64;
constexpr int kThreads = 256;
constexpr int kBlockWords = 26;     // 64-bit words per block bit string: 1660 bits at most
constexpr int kJpegHeaderMax = 640;

// zig-zag position -> natural index (row * 8 + column)
constexpr uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                 41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
// ITU-T T.81 Annex K.1 in zig-zag order
constexpr uint8_t kBaseLuma[64] = {16, 11, 12, 14, 12,  10, 16,  14,  13,  14,  18,  17,  16, 19, 24,  40,
                                   26, 24, 22, 22, 24,  49, 35,  37,  29,  40,  58,  51,  61, 60, 57,  51,
                                   56, 55, 64, 72, 92,  78, 64,  68,  87,  69,  55,  56,  80, 109, 81, 87,
                                   95, 98, 103, 104, 103, 62, 77, 113, 121, 112, 100, 120, 92, 101, 103, 99};
constexpr uint8_t kBaseChroma[64] = {17, 18, 18, 24, 21, 24, 47, 26, 26, 47, 99, 66, 56, 66, 99, 99, 99, 99, 99, 99, 99, 99,
                                     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
// ITU-T T.81 Annex K.3: codes per length 1..16, then the symbols
struct HuffSpec {
  uint8_t counts[16];
  int n;
  uint8_t symbols[162];
};
constexpr HuffSpec kDcLuma = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, 12, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}};
constexpr HuffSpec kDcChroma = {{0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}, 12, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}};
constexpr HuffSpec kAcLuma = {
    {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125},
    162,
    {1,   2,   3,   0,   4,   17,  5,   18,  33,  49,  65,  6,   19,  81,  97,  7,   34,  113, 20,  50,  129, 145, 161,
     8,   35,  66,  177, 193, 21,  82,  209, 240, 36,  51,  98,  114, 130, 9,   10,  22,  23,  24,  25,  26,  37,  38,
     39,  40,  41,  42,  52,  53,  54,  55,  56,  57,  58,  67,  68,  69,  70,  71,  72,  73,  74,  83,  84,  85,  86,
     87,  88,  89,  90,  99,  100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 131, 132, 133,
     134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170,
     178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214,
     215, 216, 217, 218, 225, 226, 227, 228, 229, 230, 231, 232, 233, 234, 241, 242, 243, 244, 245, 246, 247, 248, 249,
     250}};
constexpr HuffSpec kAcChroma = {
    {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119},
    162,
    {0,   1,   2,   3,   17,  4,   5,   33,  49,  6,   18,  65,  81,  7,   97,  113, 19,  34,  50,  129, 8,   20,  66,
     145, 161, 177, 193, 9,   35,  51,  82,  240, 21,  98,  114, 209, 10,  22,  36,  52,  225, 37,  241, 23,  24,  25,
     26,  38,  39,  40,  41,  42,  53,  54,  55,  56,  57,  58,  67,  68,  69,  70,  71,  72,  73,  74,  83,  84,  85,
     86,  87,  88,  89,  90,  99,  100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 130, 131,
     132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168,
     169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212,
     213, 214, 215, 216, 217, 218, 226, 227, 228, 229, 230, 231, 232, 233, 234, 242, 243, 244, 245, 246, 247, 248, 249,
     250}};

// symbol -> code << 8 | length (length 0: no such symbol), canonical codes of T.81 Annex C, derived at compile time
struct HuffCodes {
  uint32_t e[256];
};
constexpr HuffCodes huff_codes(const HuffSpec &s) {
  HuffCodes t = {};
  uint32_t code = 0;
  int k = 0;
  for (int len = 1; len <= 16; ++len) {
    for (int i = 0; i < s.counts[len - 1]; ++i) {
      t.e[s.symbols[k]] = (code << 8) | (uint32_t)len;
      ++code;
      ++k;
    }
    code <<= 1;
  }
  return t;
}
// the device's copy of kZigzag (a lane indexes it)
__device__ const uint8_t kZigzagDev[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,
                                           12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                                           35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51,
                                           58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
// [0] luminance, [1] chrominance
__device__ const HuffCodes kDcCodes[2] = {huff_codes(kDcLuma), huff_codes(kDcChroma)};
__device__ const HuffCodes kAcCodes[2] = {huff_codes(kAcLuma), huff_codes(kAcChroma)};
// C[u][x] = rint(8192 a(u) cos((2x + 1) u pi / 16)), computed once in float64
__device__ const int kDctDev[64] = {2896, 2896,  2896,  2896,  2896,  2896,  2896,  2896,   //
                                    4017, 3406,  2276,  799,   -799,  -2276, -3406, -4017,  //
                                    3784, 1567,  -1567, -3784, -3784, -1567, 1567,  3784,   //
                                    3406, -799,  -4017, -2276, 2276,  4017,  799,   -3406,  //
                                    2896, -2896, -2896, 2896,  2896,  -2896, -2896, 2896,   //
                                    2276, -4017, 799,   3406,  -3406, -799,  4017,  -2276,  //
                                    1567, -3784, 3784,  -1567, -1567, 3784,  -3784, 1567,   //
                                    799,  -2276, 3406,  -4017, 4017,  -3406, 2276,  -799};

// What every kernel of one call shares: the geometry (host values) and the scratch pointers
struct JpegGeom {
  int h, w;
  int s420;          // 0: 4:4:4, 1: 4:2:0
  int mw, n_mcu;     // MCU columns, MCUs per picture
  int bpm;           // blocks per MCU: 3 or 6
  int nb;            // blocks per picture
  int restart, ni;   // MCUs per interval, intervals per picture
  int header_len;
  long long capacity;
  int16_t *coef;                // [n][nb][64] zig-zag
  unsigned long long *bits;     // [n][nb][kBlockWords]
  int32_t *blen;                // [n][nb] bits of a block
  int32_t *boff;                // [n][nb] bit offset of a block in its interval
  unsigned long long *merged;   // [n][nb][kBlockWords]: interval k's byte string starts at its first block's slot
  int32_t *ibits;               // [n][ni] bits of an interval (before padding)
  int32_t *iff;                 // [n][ni] 0xFF bytes of an interval
  int32_t *ioff;                // [n][ni] offset of an interval's first byte in the file
};
struct JpegTables {
  uint8_t q[2][64];  // natural order: [0] luminance, [1] chrominance
  uint8_t header[kJpegHeaderMax];
};
static_assert(sizeof(JpegGeom) + sizeof(JpegTables) + 256 <= 4096, "mp_picture_jpeg: kernel arguments");

// step 1 of the definition: two separately rounded f32 operations (-ffp-contract=off), NaN -> 0
__device__ __forceinline__ int to_u8(float x) {
  const float t = x > 0.0f ? (x < 1.0f ? x : 1.0f) : 0.0f;
  const float m = t * 255.0f;
  return (int)(m + 0.5f);
}

// four floats per thread: one 16-byte load and one 4-byte store where the caller found both pointers aligned (vec)
__global__ __launch_bounds__(kThreads) void picture_u8(const float *__restrict__ in, uint8_t *__restrict__ out,
                                                       long long n, int vec) {
  const long long i = ((long long)blockIdx.x * kThreads + threadIdx.x) * 4;
  if (i >= n) return;
  if (vec && i + 4 <= n) {
    const float4 v = *reinterpret_cast<const float4 *>(in + i);
    const uint32_t b = (uint32_t)to_u8(v.x) | ((uint32_t)to_u8(v.y) << 8) | ((uint32_t)to_u8(v.z) << 16) |
                       ((uint32_t)to_u8(v.w) << 24);
    *reinterpret_cast<uint32_t *>(out + i) = b;
    return;
  }
  for (long long j = i; j < n && j < i + 4; ++j) out[j] = (uint8_t)to_u8(in[j]);
}

// exclusive scan of one value per thread over a workgroup of kThreads; total: the sum.  lds: kThreads / kWave ints
__device__ __forceinline__ int block_scan(int v, int *lds, int &total) {
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

__device__ __forceinline__ void ycc(const float *__restrict__ img, int h, int w, int y, int x, int &yy, int &cb,
                                    int &cr) {
  y = y < h ? y : h - 1;
  x = x < w ? x : w - 1;
  const float *p = img + ((long long)y * w + x) * 3;
  const int r = to_u8(p[0]), g = to_u8(p[1]), b = to_u8(p[2]);
  yy = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
  cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
  cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
}

__global__ __launch_bounds__(kThreads) void jpeg_transform(const float *__restrict__ images, JpegGeom ge,
                                                           JpegTables tb) {
  __shared__ int s_c[64];
  __shared__ int s_p[kThreads / kWave][64];
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
  if (threadIdx.x < 64) s_c[threadIdx.x] = kDctDev[threadIdx.x];
  __syncthreads();
  const int g = blockIdx.x * (kThreads / kWave) + wv;  // the block, in scan order
  const bool active = g < ge.nb;                       // a whole wave; the idle ones only keep the barriers
  const int pic = blockIdx.y;
  const float *img = images + (long long)pic * ge.h * ge.w * 3;
  const int mcu = g / ge.bpm, k = g - mcu * ge.bpm;
  const int my = mcu / ge.mw, mx = mcu - my * ge.mw;
  const int y = lane >> 3, x = lane & 7;
  int sample = 128, comp = 0;
  if (!active) {
  } else if (!ge.s420) {
    int c[3];
    ycc(img, ge.h, ge.w, my * 8 + y, mx * 8 + x, c[0], c[1], c[2]);
    comp = k;
    sample = k == 0 ? c[0] : (k == 1 ? c[1] : c[2]);
  } else if (k < 4) {
    int c[3];
    ycc(img, ge.h, ge.w, my * 16 + (k >> 1) * 8 + y, mx * 16 + (k & 1) * 8 + x, c[0], c[1], c[2]);
    comp = 0;
    sample = c[0];
  } else {
    int sum = 2;
#pragma unroll
    for (int dy = 0; dy < 2; ++dy) {
#pragma unroll
      for (int dx = 0; dx < 2; ++dx) {
        int c[3];
        ycc(img, ge.h, ge.w, my * 16 + 2 * y + dy, mx * 16 + 2 * x + dx, c[0], c[1], c[2]);
        sum += k == 4 ? c[1] : c[2];
      }
    }
    comp = k - 3;
    sample = sum >> 2;
  }
  int *p = s_p[wv];
  p[lane] = sample - 128;
  __syncthreads();
  // rows: lane = (y, u)
  int a = 1024;
#pragma unroll
  for (int i = 0; i < 8; ++i) a += s_c[x * 8 + i] * p[y * 8 + i];
  a >>= 11;
  __syncthreads();
  p[lane] = a;
  __syncthreads();
  // columns: lane = (v, u)
  int f = 16384;
#pragma unroll
  for (int i = 0; i < 8; ++i) f += s_c[y * 8 + i] * p[i * 8 + x];
  f >>= 15;
  const int q = tb.q[comp > 0][lane];
  const int m = ((f < 0 ? -f : f) + (q >> 1)) / q;
  __syncthreads();
  p[lane] = f < 0 ? -m : m;
  __syncthreads();
  if (active) ge.coef[((long long)pic * ge.nb + g) * 64 + lane] = (int16_t)p[kZigzagDev[lane]];
}

__global__ __launch_bounds__(kThreads) void jpeg_code(JpegGeom ge) {
  __shared__ unsigned long long s_bits[kThreads / kWave][kBlockWords + 1];
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
  const int g = blockIdx.x * (kThreads / kWave) + wv;
  const bool active = g < ge.nb;  // a whole wave; the idle ones only keep the barriers
  const int pic = blockIdx.y;
  const int16_t *coef = ge.coef + (long long)pic * ge.nb * 64;
  const int mcu = g / ge.bpm, k = g - mcu * ge.bpm;
  const int tsel = ge.s420 ? (k >= 4) : (k > 0);
  int v = active ? coef[(long long)g * 64 + lane] : 0;
  if (lane == 0 && active) {
    // the previous block of the same component; 0 at the start of a restart interval
    int prev;
    if (ge.s420 && k > 0 && k < 4)
      prev = g - 1;
    else if (mcu % ge.restart == 0)
      prev = -1;
    else
      prev = ge.s420 ? (k == 0 ? g - 3 : g - 6) : g - 3;
    v -= prev >= 0 ? (int)coef[(long long)prev * 64] : 0;
  }
  const unsigned long long nz = __ballot(v != 0) | 1ull;  // the DC lane counts as a symbol: runs start behind it
  const int last = 63 - __builtin_clzll(nz);
  const int mag = v < 0 ? -v : v;
  const int cat = mag ? 32 - __builtin_clz((unsigned)mag) : 0;
  const unsigned long long vbits = (unsigned long long)((v < 0 ? v - 1 : v) & ((1 << cat) - 1));
  unsigned long long val = 0;
  int n = 0;
  if (lane == 0) {
    const uint32_t e = kDcCodes[tsel].e[cat];
    val = ((unsigned long long)(e >> 8) << cat) | vbits;
    n = (int)(e & 255) + cat;
  } else if (v != 0) {
    const unsigned long long below = nz & ((1ull << lane) - 1);
    const int run = lane - (63 - __builtin_clzll(below)) - 1;
    const uint32_t zrl = kAcCodes[tsel].e[0xF0];
    for (int i = 0; i < (run >> 4); ++i) {
      val = (val << (zrl & 255)) | (zrl >> 8);
      n += (int)(zrl & 255);
    }
    const uint32_t e = kAcCodes[tsel].e[((run & 15) << 4) | cat];
    val = (((val << (e & 255)) | (e >> 8)) << cat) | vbits;
    n += (int)(e & 255) + cat;
  } else if (lane == last + 1) {  // EOB, unless coefficient 63 is non-zero
    const uint32_t e = kAcCodes[tsel].e[0x00];
    val = e >> 8;
    n = (int)(e & 255);
  }
  int inc = n;
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    const int t = __shfl_up(inc, d, kWave);
    if (lane >= d) inc += t;
  }
  const int total = __shfl(inc, kWave - 1, kWave);
  const int pos = inc - n;
  unsigned long long *s = s_bits[wv];
  if (lane <= kBlockWords) s[lane] = 0ull;
  __syncthreads();
  if (n > 0 && pos + n <= kBlockWords * 64) {  // always true: a block is at most 1660 bits
    const int w0 = pos >> 6, sh = pos & 63;
    if (sh + n <= 64) {
      atomicOr(&s[w0], val << (64 - sh - n));
    } else {
      atomicOr(&s[w0], val >> (sh + n - 64));
      atomicOr(&s[w0 + 1], val << (128 - sh - n));
    }
  }
  __syncthreads();
  const long long gb = (long long)pic * ge.nb + g;
  const int nw = (total + 63) >> 6;
  if (active && lane < nw && lane < kBlockWords) ge.bits[gb * kBlockWords + lane] = s[lane];
  if (active && lane == 0) ge.blen[gb] = total < kBlockWords * 64 ? total : kBlockWords * 64;
}

// blocks of interval k of a picture: [first, first + count)
__device__ __forceinline__ void interval_blocks(const JpegGeom &ge, int k, int &first, int &count) {
  const int m0 = k * ge.restart;
  const int m1 = m0 + ge.restart < ge.n_mcu ? m0 + ge.restart : ge.n_mcu;
  first = m0 * ge.bpm;
  count = (m1 - m0) * ge.bpm;
}

__global__ __launch_bounds__(kThreads) void jpeg_scan(JpegGeom ge) {
  __shared__ int s_scan[kThreads / kWave];
  const int k = blockIdx.x, pic = blockIdx.y;
  int first, count;
  interval_blocks(ge, k, first, count);
  const long long base = (long long)pic * ge.nb + first;
  int carry = 0;
  for (int i0 = 0; i0 < count; i0 += kThreads) {  // uniform trip count: block_scan holds barriers
    const int i = i0 + threadIdx.x;
    const int len = i < count ? ge.blen[base + i] : 0;
    int total;
    const int ex = block_scan(len, s_scan, total);
    if (i < count) ge.boff[base + i] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) {
    ge.ibits[(long long)pic * ge.ni + k] = carry;
    ge.iff[(long long)pic * ge.ni + k] = 0;
  }
}

// 64 bits of a block's string from bit r (r may be negative: the string then starts inside the word)
__device__ __forceinline__ unsigned long long block_window(const unsigned long long *__restrict__ b, int nw, int r) {
  if (r < 0) return r > -64 ? (nw > 0 ? b[0] : 0ull) >> (-r) : 0ull;
  const int j = r >> 6, sh = r & 63;
  const unsigned long long hi = j < nw ? b[j] : 0ull;
  if (sh == 0) return hi;
  const unsigned long long lo = j + 1 < nw ? b[j + 1] : 0ull;
  return (hi << sh) | (lo >> (64 - sh));
}

__global__ __launch_bounds__(kThreads) void jpeg_merge(JpegGeom ge, int chunks) {
  const int k = blockIdx.x / chunks, chunk = blockIdx.x - k * chunks, pic = blockIdx.y;
  int first, count;
  interval_blocks(ge, k, first, count);
  const long long base = (long long)pic * ge.nb + first;
  const int32_t *__restrict__ boff = ge.boff + base;
  const int32_t *__restrict__ blen = ge.blen + base;
  const int ibits = ge.ibits[(long long)pic * ge.ni + k];
  const int nbytes = (ibits + 7) >> 3;
  const int nwords = (nbytes + 7) >> 3;  // <= count * kBlockWords: a block is below 1664 - 4 bits
  int ff = 0;
  for (int w = chunk * kThreads + threadIdx.x; w < nwords; w += chunks * kThreads) {
    const int lo_bit = w << 6;
    int lo = 0, hi = count - 1;  // the last block that starts at or before lo_bit (boff[0] == 0)
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (boff[mid] <= lo_bit)
        lo = mid;
      else
        hi = mid - 1;
    }
    unsigned long long acc = 0ull;
    for (int i = lo; i < count; ++i) {
      const int o = boff[i];
      if (o >= lo_bit + 64) break;
      const int len = blen[i];
      acc |= block_window(ge.bits + (base + i) * kBlockWords, (len + 63) >> 6, lo_bit - o);
    }
    const int rem = ibits - lo_bit;  // > 0
    if (rem < 64) acc |= ~0ull >> rem;
    ge.merged[base * kBlockWords + w] = acc;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      ff += (8 * w + j < nbytes) && ((acc >> (56 - 8 * j)) & 255ull) == 255ull;
  }
#pragma unroll
  for (int d = kWave / 2; d > 0; d >>= 1) ff += __shfl_down(ff, d, kWave);
  if ((threadIdx.x & (kWave - 1)) == 0 && ff) atomicAdd(&ge.iff[(long long)pic * ge.ni + k], ff);
}

__global__ __launch_bounds__(kThreads) void jpeg_offsets(JpegGeom ge, int32_t *__restrict__ info) {
  __shared__ int s_scan[kThreads / kWave];
  const int pic = blockIdx.x;
  const long long ib = (long long)pic * ge.ni;
  long long carry = ge.header_len;
  for (int i0 = 0; i0 < ge.ni; i0 += kThreads) {
    const int i = i0 + threadIdx.x;
    const int sz = i < ge.ni ? ((ge.ibits[ib + i] + 7) >> 3) + ge.iff[ib + i] + 2 : 0;  // + RSTm, or EOI behind the last
    int total;
    const int ex = block_scan(sz, s_scan, total);
    if (i < ge.ni) ge.ioff[ib + i] = (int)(carry + ex);
    carry += total;
  }
  if (threadIdx.x == 0) {
    info[2 * pic] = (int)carry;
    info[2 * pic + 1] = carry > ge.capacity ? 1 : 0;
  }
}

__global__ __launch_bounds__(kThreads) void jpeg_emit(JpegGeom ge, JpegTables tb, const int32_t *__restrict__ info,
                                                      uint8_t *__restrict__ out_all) {
  __shared__ int s_scan[kThreads / kWave];
  const int k = blockIdx.x, pic = blockIdx.y;
  if (info[2 * pic + 1]) return;  // uniform: nothing of a picture that does not fit is written
  const long long cap = ge.capacity;
  uint8_t *__restrict__ out = out_all + (long long)pic * cap;
  if (k == 0) {
    for (int i = threadIdx.x; i < ge.header_len; i += kThreads)
      if (i < cap) out[i] = tb.header[i];
  }
  int first, count;
  interval_blocks(ge, k, first, count);
  const unsigned long long *__restrict__ src = ge.merged + ((long long)pic * ge.nb + first) * kBlockWords;
  const long long ii = (long long)pic * ge.ni + k;
  const int nbytes = (ge.ibits[ii] + 7) >> 3;
  const int nwords = (nbytes + 7) >> 3;
  const long long start = ge.ioff[ii];
  int carry = 0;  // 0xFF bytes before this chunk
  for (int w0 = 0; w0 < nwords; w0 += kThreads) {  // uniform trip count
    const int w = w0 + threadIdx.x;
    const unsigned long long word = w < nwords ? src[w] : 0ull;
    int ff = 0;
    if (w < nwords) {
#pragma unroll
      for (int j = 0; j < 8; ++j) ff += (8 * w + j < nbytes) && ((word >> (56 - 8 * j)) & 255ull) == 255ull;
    }
    int total;
    const int ex = block_scan(ff, s_scan, total);
    if (w < nwords) {
      long long pos = start + 8LL * w + carry + ex;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        if (8 * w + j < nbytes) {
          const uint8_t b = (uint8_t)(word >> (56 - 8 * j));
          if (pos >= 0 && pos < cap) out[pos] = b;
          ++pos;
          if (b == 0xFF) {
            if (pos >= 0 && pos < cap) out[pos] = 0;
            ++pos;
          }
        }
      }
    }
    carry += total;
  }
  if (threadIdx.x == 0) {
    const long long pos = start + nbytes + carry;
    if (pos >= 0 && pos + 1 < cap) {
      out[pos] = 0xFF;
      out[pos + 1] = k + 1 < ge.ni ? (uint8_t)(0xD0 + (k & 7)) : (uint8_t)0xD9;
    }
  }
}

void put16(uint8_t *&p, int v) {
  *p++ = (uint8_t)(v >> 8);
  *p++ = (uint8_t)(v & 255);
}

void put_dht(uint8_t *&p, int tc, const HuffSpec &s) {
  *p++ = 0xFF;
  *p++ = 0xC4;
  put16(p, 3 + 16 + s.n);
  *p++ = (uint8_t)tc;
  std::memcpy(p, s.counts, 16);
  p += 16;
  std::memcpy(p, s.symbols, (size_t)s.n);
  p += s.n;
}

struct JpegSizes {
  int mcu, mw, mh, bpm, restart;
  long long n_mcu, nb, ni;
};
JpegSizes jpeg_sizes(int h, int w, int s420, int restart) {
  JpegSizes z;
  z.mcu = s420 ? 16 : 8;
  z.mw = (w + z.mcu - 1) / z.mcu;
  z.mh = (h + z.mcu - 1) / z.mcu;
  z.bpm = s420 ? 6 : 3;
  z.restart = restart ? restart : z.mw;
  z.n_mcu = (long long)z.mw * z.mh;
  z.nb = z.n_mcu * z.bpm;
  z.ni = (z.n_mcu + z.restart - 1) / z.restart;
  return z;
}

constexpr size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

}  // namespace

int launch_picture_u8(mp_ctx *ctx, const float *image, long long n_pixels, uint8_t *out, hipStream_t st) {
  const long long n = 3 * n_pixels;
  if (n == 0) return MP_OK;
  const int vec = ((uintptr_t)image & 15u) == 0 && ((uintptr_t)out & 3u) == 0;
  const long long threads = (n + 3) / 4;
  hipLaunchKernelGGL(picture_u8, dim3((unsigned)((threads + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, image, out,
                     n, vec);
  MP_HIP(ctx, hipGetLastError());
  return MP_OK;
}

int jpeg_header_bytes() { return 629; }

long long jpeg_max_bytes(int h, int w, int s420, int restart) {
  const JpegSizes z = jpeg_sizes(h, w, s420, restart);
  return jpeg_header_bytes() + 2 * (z.nb * kBlockWords * 8) + 2 * z.ni;
}

size_t jpeg_scratch_bytes(int n, int h, int w, int s420, int restart) {
  const JpegSizes z = jpeg_sizes(h, w, s420, restart);
  const size_t blocks = (size_t)n * z.nb, iv = (size_t)n * z.ni;
  return align256(blocks * 64 * sizeof(int16_t)) + 2 * align256(blocks * kBlockWords * 8) +
         2 * align256(blocks * sizeof(int32_t)) + 3 * align256(iv * sizeof(int32_t));
}

int launch_picture_jpeg(mp_ctx *ctx, void *scratch, const float *images, int n, int h, int w, int quality, int s420,
                        int restart, uint8_t *out, long long capacity, int32_t *info, hipStream_t st) {
  const JpegSizes z = jpeg_sizes(h, w, s420, restart);
  JpegGeom ge;
  JpegTables tb;
  std::memset(&ge, 0, sizeof(ge));
  std::memset(&tb, 0, sizeof(tb));
  ge.h = h;
  ge.w = w;
  ge.s420 = s420;
  ge.mw = z.mw;
  ge.n_mcu = (int)z.n_mcu;
  ge.bpm = z.bpm;
  ge.nb = (int)z.nb;
  ge.restart = z.restart;
  ge.ni = (int)z.ni;
  ge.header_len = jpeg_header_bytes();
  ge.capacity = capacity;
  const size_t blocks = (size_t)n * z.nb, iv = (size_t)n * z.ni;
  char *p = static_cast<char *>(scratch);
  auto take = [&p](size_t bytes) {
    char *r = p;
    p += align256(bytes);
    return r;
  };
  ge.coef = reinterpret_cast<int16_t *>(take(blocks * 64 * sizeof(int16_t)));
  ge.bits = reinterpret_cast<unsigned long long *>(take(blocks * kBlockWords * 8));
  ge.merged = reinterpret_cast<unsigned long long *>(take(blocks * kBlockWords * 8));
  ge.blen = reinterpret_cast<int32_t *>(take(blocks * sizeof(int32_t)));
  ge.boff = reinterpret_cast<int32_t *>(take(blocks * sizeof(int32_t)));
  ge.ibits = reinterpret_cast<int32_t *>(take(iv * sizeof(int32_t)));
  ge.iff = reinterpret_cast<int32_t *>(take(iv * sizeof(int32_t)));
  ge.ioff = reinterpret_cast<int32_t *>(take(iv * sizeof(int32_t)));

  // the tables of this quality, scaled as the IJG library scales them (zig-zag order), and the header
  const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
  uint8_t qz[2][64];
  for (int t = 0; t < 2; ++t) {
    const uint8_t *base = t ? kBaseChroma : kBaseLuma;
    for (int i = 0; i < 64; ++i) {
      int v = (base[i] * scale + 50) / 100;
      v = v < 1 ? 1 : (v > 255 ? 255 : v);
      qz[t][i] = (uint8_t)v;
      tb.q[t][kZigzag[i]] = (uint8_t)v;
    }
  }
  uint8_t *hp = tb.header;
  static const uint8_t app0[] = {0xFF, 0xD8, 0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
  std::memcpy(hp, app0, sizeof(app0));
  hp += sizeof(app0);
  for (int t = 0; t < 2; ++t) {
    *hp++ = 0xFF;
    *hp++ = 0xDB;
    put16(hp, 67);
    *hp++ = (uint8_t)t;
    std::memcpy(hp, qz[t], 64);
    hp += 64;
  }
  *hp++ = 0xFF;
  *hp++ = 0xC0;
  put16(hp, 17);
  *hp++ = 8;
  put16(hp, h);
  put16(hp, w);
  const uint8_t comps[] = {3, 1, (uint8_t)(s420 ? 0x22 : 0x11), 0, 2, 0x11, 1, 3, 0x11, 1};
  std::memcpy(hp, comps, sizeof(comps));
  hp += sizeof(comps);
  put_dht(hp, 0x00, kDcLuma);
  put_dht(hp, 0x10, kAcLuma);
  put_dht(hp, 0x01, kDcChroma);
  put_dht(hp, 0x11, kAcChroma);
  *hp++ = 0xFF;
  *hp++ = 0xDD;
  put16(hp, 4);
  put16(hp, z.restart);
  static const uint8_t sos[] = {0xFF, 0xDA, 0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0};
  std::memcpy(hp, sos, sizeof(sos));
  hp += sizeof(sos);
  if (hp - tb.header != ge.header_len)
    return fail(ctx, MP_ERR_HIP, "mp_picture_jpeg: a header of %d bytes", (int)(hp - tb.header));

  const int wpb = kThreads / kWave;
  const dim3 per_block((unsigned)((z.nb + wpb - 1) / wpb), (unsigned)n);
  hipLaunchKernelGGL(jpeg_transform, per_block, dim3(kThreads), 0, st, images, ge, tb);
  hipLaunchKernelGGL(jpeg_code, per_block, dim3(kThreads), 0, st, ge);
  // grid.y is limited to 65535 (the pictures: the caller has checked n); ni reaches 262144 (4096^2, restart 1): on x
  hipLaunchKernelGGL(jpeg_scan, dim3((unsigned)z.ni, (unsigned)n), dim3(kThreads), 0, st, ge);
  // words per interval: expect about 4 per block, stride over the rest (26 per block at most)
  long long chunks = ((long long)z.restart * z.bpm * 4 + kThreads - 1) / kThreads;
  chunks = chunks < 1 ? 1 : (chunks > 64 ? 64 : chunks);
  hipLaunchKernelGGL(jpeg_merge, dim3((unsigned)(chunks * z.ni), (unsigned)n), dim3(kThreads), 0, st, ge, (int)chunks);
  hipLaunchKernelGGL(jpeg_offsets, dim3((unsigned)n), dim3(kThreads), 0, st, ge, info);
  hipLaunchKernelGGL(jpeg_emit, dim3((unsigned)z.ni, (unsigned)n), dim3(kThreads), 0, st, ge, tb,
                     static_cast<const int32_t *>(info), out);
  MP_HIP(ctx, hipGetLastError());
  return MP_OK;
}

}  // namespace mp
