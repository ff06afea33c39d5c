// Baseline JPEG files of RGB pictures in device memory (kgdet_amd/jpeg.py: DeviceJpegEncoder) for gfx950: kgdet_jpeg_encode,
// kgdet_jpeg_write.  The file is DEFINED by jpeg.jpeg_restatement (numpy / Python integers); these kernels are held to it byte
// for byte.  In short: JFIF, SOF0, Y / Cb / Cr sampled 2x2 / 1x1 / 1x1 (an MCU is 16 x 16 pixels, blocks Y00 Y01 Y10 Y11 Cb Cr),
// one interleaved scan; the Annex K.1 tables scaled by the IJG quality rule and the Annex K.3 Huffman tables;
//   samples with four fraction bits: Y = ((19595 R + 38470 G + 7471 B + 2048) >> 12) - 2048, Cb / Cr from the 2 x 2 sums of R,
//   G, B with ONE rounding (>> 14); rows P = (X D^T + 1024) >> 11, columns C = (D P + 32768) >> 16 with D = rint(8192 c(u)
//   cos((2x + 1) u pi / 16)): |X D^T| < 2^26, |P| < 2^15, |D P| < 2^30;
//   level = sign(C) ((|C| + 4 q) / (8 q)); zigzag; DC differences chained over the scan, AC as (run, size) with ZRL and EOB;
//   the stream padded with 1-bits and every 0xFF data byte followed by 0x00.
// Every stage is integer arithmetic, so the bytes do not depend on launch geometry or schedule.  No floating point at all.
//
// Five kernels behind kgdet_jpeg_encode, one behind kgdet_jpeg_write; between them the caller reads the n lengths back once.
//  1. transform  one wave per MCU.  The MCU's 16 x 48 bytes are read coalesced (lane = byte, edge pixels replicated by
//     clamping the pixel index) into LDS; 4 luma samples and one chroma pair per lane; 48 lanes take a row, then a column,
//     of the six blocks (the matrix is compile-time constants); each lane quantises the coefficient of zigzag place `lane` of
//     every block: int16 [MCU][6][64], 128-byte rows.  LDS 768 + 2 x 1 728 bytes.
//  2. measure    one wave per MCU, lane = zigzag place.  A ballot of the non-zero places gives every lane its run, so the lane
//     knows its own code (up to three ZRLs, the symbol, the magnitude bits: at most 59 bits) without a loop; lane 0 codes the
//     DC difference against the previous block of its component, READ from the coefficients, so MCUs are independent; lane
//     63 codes EOB when its place is zero.  The wave's sum is the MCU's bits.
//  3. scan       one workgroup per image: the exclusive scan of the MCU bits (uint64).
//  4. pack       ownership by OUTPUT range: a workgroup owns KGDET_JPEG_RANGE_BYTES bytes of an image's unstuffed stream.  It
//     finds the first MCU that reaches its range by bisection of the scan; its four waves code the overlapping MCUs as in
//     (2), a wave scan places every lane's bits, and the bits are ORed into the range's LDS image (LDS integer OR: any order
//     gives the same words); what falls outside the range is dropped, so boundary MCUs are coded by both neighbours.  The
//     range leaves as 16-byte stores and its 0xFF bytes are counted.  LDS 4 144 bytes.
//  5. scan       one workgroup per image over the ranges' 0xFF counts; writes the file lengths.
//  6. finish     (kgdet_jpeg_write) a workgroup per range: a scan of the 0xFF bytes of its 16-byte pieces places each piece in
//     the file, stuffing zeros inserted; the first range writes the header, the last one EOI.  An image whose file does not
//     fit its capacity is not written at all and flagged.
// Workspace per MCU: 768 (coefficients) + 4 + 8 (bits, scan) bytes, and for the stream the WORST case of 1 248 bytes (6 blocks
// of 22 + 63 x 26 bits), since nothing is read back before the pack: about 2 KiB per 768 bytes of pixels.
// No global atomics, no floating point, plain C++ and vector stores only.
//
// Environment switch (tools/time_jpeg.py; not part of the API):
//   KGDET_JPEG_STOP_AFTER=k   kgdet_jpeg_encode launches only its first k kernels (1 .. 5): the kernels' own times by difference
#include <algorithm>
#include <initializer_list>

#include "common.h"

namespace kgdet {

namespace {

constexpr int kWave = 64;
constexpr int kMaxImages = KGDET_JPEG_MAX_IMAGES;
constexpr int kMaxSide = 8192;
constexpr int kHeader = 623;
constexpr int kRange = KGDET_JPEG_RANGE_BYTES;
constexpr int kRangeBits = 8 * kRange;
constexpr int kMcuWorst = 1248;                     // bytes of an MCU's code at most
constexpr int kPackThreads = 256, kPackWaves = kPackThreads / kWave;
constexpr int kLdsWords = 2 + kRange / 4 + 2;       // two guard words in front (a code starts up to 58 bits early), two behind

typedef unsigned long long u64;
typedef unsigned int u32;
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// ---- the standard's tables (ITU T.81 Annex K.1, K.3) ---------------------------------------------------------------------
constexpr unsigned char kBaseLuma[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,
                                         14, 13, 16, 24, 40,  57,  69,  56,  14, 17, 22, 29, 51,  87,  80,  62,
                                         18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
                                         49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
constexpr unsigned char kBaseChroma[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99,
                                           99, 99, 47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                           99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
constexpr unsigned char kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                       41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                       30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
constexpr unsigned char kDcLumaBits[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
constexpr unsigned char kDcChromaBits[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
constexpr unsigned char kAcLumaBits[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d};
constexpr unsigned char kAcChromaBits[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77};
constexpr char kAcLumaVals[] =
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a43444546"
    "4748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7"
    "b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa";
constexpr char kAcChromaVals[] =
    "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a434445"
    "464748494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5"
    "b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa";
constexpr int kAcVals = 162;
static_assert(sizeof(kAcLumaVals) == 2 * kAcVals + 1 && sizeof(kAcChromaVals) == 2 * kAcVals + 1, "162 AC symbols per table");

constexpr int hex_digit(char c) { return c <= '9' ? c - '0' : c - 'a' + 10; }
constexpr int ac_val(const char *hex, int k) { return hex_digit(hex[2 * k]) * 16 + hex_digit(hex[2 * k + 1]); }

// (length << 16 | code) per symbol, Annex C; [0] luminance, [1] chrominance
struct HuffCodes {
  u32 dc[2][16];
  u32 ac[2][256];
};

constexpr HuffCodes make_codes() {
  HuffCodes h = {};
  for (int t = 0; t < 2; ++t) {
    const unsigned char *db = t ? kDcChromaBits : kDcLumaBits, *ab = t ? kAcChromaBits : kAcLumaBits;
    const char *av = t ? kAcChromaVals : kAcLumaVals;
    u32 code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
      for (int i = 0; i < db[len - 1]; ++i) h.dc[t][k++] = (u32)len << 16 | code++;
      code <<= 1;
    }
    code = 0, k = 0;
    for (int len = 1; len <= 16; ++len) {
      for (int i = 0; i < ab[len - 1]; ++i) h.ac[t][ac_val(av, k++)] = (u32)len << 16 | code++;
      code <<= 1;
    }
  }
  return h;
}

__constant__ const HuffCodes d_codes = make_codes();

// D[u][x] = rint(8192 c(u) cos((2x + 1) u pi / 16))
constexpr int kD[8][8] = {{2896, 2896, 2896, 2896, 2896, 2896, 2896, 2896},    {4017, 3406, 2276, 799, -799, -2276, -3406, -4017},
                          {3784, 1567, -1567, -3784, -3784, -1567, 1567, 3784}, {3406, -799, -4017, -2276, 2276, 4017, 799, -3406},
                          {2896, -2896, -2896, 2896, 2896, -2896, -2896, 2896}, {2276, -4017, 799, 3406, -3406, -799, 4017, -2276},
                          {1567, -3784, 3784, -1567, -1567, 3784, -3784, 1567}, {799, -2276, 3406, -4017, 4017, -3406, 2276, -799}};

struct JpegImage {
  long long src_off;
  int H, W, mw, nm;                                 // MCUs per row, MCUs
};

struct JpegArgs {
  JpegImage img[kMaxImages];
  int mcu0[kMaxImages + 1];                         // first (global) MCU of each image
  int range0[kMaxImages + 1];                       // first (global) range of each image, by the worst case
  int n;
};

struct QuantTables {
  unsigned short q[2][64];                          // natural order
};

struct Header {
  unsigned char b[kHeader + 1];
};

struct OutTable {
  long long off[kMaxImages], cap[kMaxImages];
};

// the workspace: byte offsets of its arrays
struct Layout {
  size_t coef, bits, bitoff, ffcount, ffoff, stream, total;
};

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, kWave);
  return v;
}

__device__ __forceinline__ int wave_inclusive(int v, int lane) {
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    const int o = __shfl_up(v, d, kWave);
    if (lane >= d) v += o;
  }
  return v;
}

// the exclusive scan of `count` values into out[0 .. count] (out[count] = the sum) by one workgroup of 256 threads
__device__ __forceinline__ u64 block_scan(const u32 *__restrict__ in, u64 *__restrict__ out, int count, u32 *s_w) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  u64 carry = 0;
  for (int i0 = 0; i0 < count; i0 += kPackThreads) {
    const int i = i0 + tid;
    const int v = i < count ? (int)in[i] : 0;
    const int incl = wave_inclusive(v, lane);
    if (lane == kWave - 1) s_w[wave] = (u32)incl;
    __syncthreads();
    u32 before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < kPackWaves; ++w) {
      before += w < wave ? s_w[w] : 0u;
      all += s_w[w];
    }
    if (i < count) out[i] = carry + before + (u32)(incl - v);
    carry += all;
    __syncthreads();
  }
  if (tid == 0) out[count] = carry;
  return carry;
}

__device__ __forceinline__ int image_of(const int *first, int n, int g) {
  int im = 0;
  while (im + 1 < n && g >= first[im + 1]) ++im;
  return im;
}

// ---- 1. transform ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kWave) void jpeg_transform_kernel(const JpegArgs args, const QuantTables qt,
                                                               const unsigned char *__restrict__ src, short *__restrict__ coef) {
  __shared__ unsigned char s_px[16][48];
  __shared__ int s_a[6][8][9], s_b[6][8][9];
  const int lane = threadIdx.x, g = blockIdx.x;
  const int im = image_of(args.mcu0, args.n, g);
  const JpegImage &I = args.img[im];
  const int m = g - args.mcu0[im];
  const int my = m / I.mw, mx = m - my * I.mw;
  const unsigned char *__restrict__ img = src + I.src_off;
#pragma unroll
  for (int k = 0; k < 12; ++k) {
    const int idx = lane + kWave * k;
    const int j = idx / 48, b = idx - 48 * j;
    const int p = b / 3, c = b - 3 * p;
    const int y = min(16 * my + j, I.H - 1), x = min(16 * mx + p, I.W - 1);
    s_px[j][b] = img[((long long)y * I.W + x) * 3 + c];
  }
  __syncthreads();
  const int r = lane >> 3, c = lane & 7;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const unsigned char *px = &s_px[8 * (k >> 1) + r][3 * (8 * (k & 1) + c)];
    s_a[k][r][c] = ((19595 * px[0] + 38470 * px[1] + 7471 * px[2] + 2048) >> 12) - 2048;
  }
  {
    const unsigned char *p0 = &s_px[2 * r][6 * c], *p1 = &s_px[2 * r + 1][6 * c];
    const int SR = p0[0] + p0[3] + p1[0] + p1[3], SG = p0[1] + p0[4] + p1[1] + p1[4], SB = p0[2] + p0[5] + p1[2] + p1[5];
    s_a[4][r][c] = (-11058 * SR - 21710 * SG + 32768 * SB + 8192) >> 14;
    s_a[5][r][c] = (32768 * SR - 27439 * SG - 5329 * SB + 8192) >> 14;
  }
  __syncthreads();
  if (lane < 48) {                                  // rows: P[y][u] = (sum_x D[u][x] X[y][x] + 1024) >> 11
    int x[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) x[i] = s_a[r][c][i];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      int t = 1024;
#pragma unroll
      for (int i = 0; i < 8; ++i) t += kD[u][i] * x[i];
      s_b[r][c][u] = t >> 11;
    }
  }
  __syncthreads();
  if (lane < 48) {                                  // columns: C[v][u] = (sum_y D[v][y] P[y][u] + 32768) >> 16
    int p[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) p[i] = s_b[r][i][c];
#pragma unroll
    for (int v = 0; v < 8; ++v) {
      int t = 32768;
#pragma unroll
      for (int i = 0; i < 8; ++i) t += kD[v][i] * p[i];
      s_a[r][v][c] = t >> 16;
    }
  }
  __syncthreads();
  const int nat = kZigzag[lane];
  short *__restrict__ out = coef + (long long)g * 384 + lane;
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const int C = s_a[k][nat >> 3][nat & 7];
    const int q = qt.q[k < 4 ? 0 : 1][nat];
    const int level = (abs(C) + 4 * q) / (8 * q);
    out[64 * k] = (short)(C < 0 ? -level : level);
  }
}

// ---- the code of one block, lane = zigzag place ------------------------------------------------------------------------------
struct LaneCode {
  u64 val;                                          // right-aligned
  int len;                                          // 0 .. 59
};

// v: the lane's level; pred: the previous DC of the component (used by lane 0); t: 0 luminance, 1 chrominance
__device__ __forceinline__ LaneCode code_lane(int lane, int v, int pred, int t) {
  const u64 nz = __ballot(lane > 0 && v != 0);
  const int d = lane == 0 ? v - pred : v;
  const int a = abs(d);
  const int size = a ? 32 - __clz(a) : 0;
  const u32 mag = (u32)(d > 0 ? d : d - 1) & ((1u << size) - 1u);
  LaneCode out;
  out.val = 0, out.len = 0;
  if (lane == 0) {
    const u32 e = d_codes.dc[t][size];
    out.val = (u64)(e & 0xffffu) << size | mag;
    out.len = (int)(e >> 16) + size;
  } else if (v != 0) {
    const u64 below = nz & ((1ull << lane) - 1ull);
    const int prev = below ? 63 - __clzll((long long)below) : 0;
    const int run = lane - 1 - prev;
    const u32 zrl = d_codes.ac[t][0xF0], e = d_codes.ac[t][(run & 15) << 4 | size];
    const int zl = (int)(zrl >> 16), el = (int)(e >> 16);
    for (int i = 0; i < (run >> 4); ++i) {
      out.val = out.val << zl | (zrl & 0xffffu);
      out.len += zl;
    }
    out.val = out.val << (el + size) | (u64)(e & 0xffffu) << size | mag;
    out.len += el + size;
  } else if (lane == kWave - 1) {                   // the block ends in zeros: EOB
    const u32 e = d_codes.ac[t][0];
    out.val = e & 0xffffu;
    out.len = (int)(e >> 16);
  }
  return out;
}

// the DC predictor of block k of (global) MCU g, MCU m of its image
__device__ __forceinline__ int dc_pred(const short *__restrict__ coef, long long g, int m, int k) {
  if (k >= 1 && k <= 3) return coef[(g * 6 + k - 1) * 64];
  if (m == 0) return 0;
  return coef[((g - 1) * 6 + (k == 0 ? 3 : k)) * 64];
}

// ---- 2. measure -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kPackThreads) void jpeg_measure_kernel(const JpegArgs args, int total_mcus,
                                                                    const short *__restrict__ coef, u32 *__restrict__ bits) {
  const int lane = threadIdx.x & 63;
  const int g = (int)blockIdx.x * kPackWaves + ((int)threadIdx.x >> 6);
  if (g >= total_mcus) return;                      // (wave-uniform)
  const int m = g - args.mcu0[image_of(args.mcu0, args.n, g)];
  int sum = 0;
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const int v = coef[((long long)g * 6 + k) * 64 + lane];
    sum += code_lane(lane, v, dc_pred(coef, g, m, k), k < 4 ? 0 : 1).len;
  }
  sum = wave_sum(sum);
  if (lane == 0) bits[g] = (u32)sum;
}

// ---- 3. and 5. the scans --------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kPackThreads) void jpeg_scan_bits_kernel(const JpegArgs args, const u32 *__restrict__ bits,
                                                                      u64 *__restrict__ bitoff) {
  __shared__ u32 s_w[kPackWaves];
  const int im = blockIdx.x;
  block_scan(bits + args.mcu0[im], bitoff + args.mcu0[im] + im, args.img[im].nm, s_w);
}

__global__ __launch_bounds__(kPackThreads) void jpeg_scan_ff_kernel(const JpegArgs args, const u64 *__restrict__ bitoff,
                                                                    const u32 *__restrict__ ffcount, u64 *__restrict__ ffoff,
                                                                    long long *__restrict__ lengths) {
  __shared__ u32 s_w[kPackWaves];
  const int im = blockIdx.x;
  const u64 stream_bytes = (bitoff[args.mcu0[im] + im + args.img[im].nm] + 7) >> 3;
  const int live = (int)((stream_bytes + kRange - 1) / kRange);
  const u64 ff = block_scan(ffcount + args.range0[im], ffoff + args.range0[im] + im, live, s_w);
  if (threadIdx.x == 0) lengths[im] = (long long)(kHeader + stream_bytes + ff + 2);
}

// ---- 4. pack --------------------------------------------------------------------------------------------------------------
// `len` bits of val (right-aligned) at bit `rel` of the range, which may begin before the range or end behind it
__device__ __forceinline__ void put_bits(u32 *s_bits, long long rel, u64 val, int len) {
  if (len == 0 || rel + len <= 0 || rel >= kRangeBits) return;
  const int q = (int)rel + 64;                      // (rel > -len >= -59: q >= 6)
  const int w = q >> 5, b = q & 31;
  const u64 x = val << (64 - len);
  const u64 hi = x >> b;
  const u32 w0 = (u32)(hi >> 32), w1 = (u32)hi, w2 = b ? (u32)((x << (64 - b)) >> 32) : 0u;
  if (w0) atomicOr(&s_bits[w], w0);
  if (w1) atomicOr(&s_bits[w + 1], w1);
  if (w2) atomicOr(&s_bits[w + 2], w2);
}

__global__ __launch_bounds__(kPackThreads) void jpeg_pack_kernel(const JpegArgs args, int total_ranges,
                                                                 const short *__restrict__ coef, const u64 *__restrict__ bitoff,
                                                                 unsigned char *__restrict__ stream, u32 *__restrict__ ffcount) {
  __shared__ __attribute__((aligned(16))) u32 s_bits[kLdsWords + 2];
  __shared__ u32 s_w[kPackWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int gr = blockIdx.x; gr < total_ranges; gr += gridDim.x) {
    const int im = image_of(args.range0, args.n, gr);
    const int nm = args.img[im].nm;
    const u64 *__restrict__ off = bitoff + args.mcu0[im] + im;
    const u64 total = off[nm], stream_bytes = (total + 7) >> 3;
    const u64 start = (u64)(gr - args.range0[im]) * kRange;
    if (start >= stream_bytes) continue;            // (uniform: the ranges of the worst case the stream does not reach)
    const u64 start_bits = 8 * start, end_bits = start_bits + kRangeBits;
    for (int i = tid; i < kLdsWords + 2; i += kPackThreads) s_bits[i] = 0;
    __syncthreads();
    int lo = 0, hi = nm - 1;                        // the last MCU that begins at or before the range's first bit
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (off[mid] <= start_bits) lo = mid; else hi = mid - 1;
    }
    for (int m = lo + wave; m < nm && off[m] < end_bits; m += kPackWaves) {
      const long long g = (long long)args.mcu0[im] + m;
      long long rel = (long long)off[m] - (long long)start_bits;
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        const int v = coef[(g * 6 + k) * 64 + lane];
        const LaneCode c = code_lane(lane, v, dc_pred(coef, g, m, k), k < 4 ? 0 : 1);
        const int incl = wave_inclusive(c.len, lane);
        put_bits(s_bits, rel + (incl - c.len), c.val, c.len);
        rel += __shfl(incl, kWave - 1, kWave);
      }
    }
    if (tid == 0) {                                 // the padding of the last byte, where this range holds it
      const int pad = (int)((0 - total) & 7);
      put_bits(s_bits, (long long)total - (long long)start_bits, (1ull << pad) - 1ull, pad);
    }
    __syncthreads();
    const u64 left = stream_bytes - start;
    const int nb = left < (u64)kRange ? (int)left : kRange;
    int ff = 0;
    if (16 * tid < nb) {
      u32x4 word;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const u32 be = s_bits[2 + 4 * tid + j];
        word[j] = __builtin_bswap32(be);
#pragma unroll
        for (int b = 0; b < 4; ++b)
          ff += (16 * tid + 4 * j + b < nb && ((be >> (24 - 8 * b)) & 255u) == 255u) ? 1 : 0;
      }
      *reinterpret_cast<u32x4 *>(stream + (size_t)gr * kRange + 16 * tid) = word;
    }
    ff = wave_sum(ff);
    if (lane == 0) s_w[wave] = (u32)ff;
    __syncthreads();
    if (tid == 0) ffcount[gr] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
    __syncthreads();
  }
}

// ---- 6. finish ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kPackThreads) void jpeg_finish_kernel(const JpegArgs args, const OutTable ot, const Header hdr,
                                                                   int total_ranges, const u64 *__restrict__ bitoff,
                                                                   const unsigned char *__restrict__ stream,
                                                                   const u64 *__restrict__ ffoff, unsigned char *__restrict__ out,
                                                                   int *__restrict__ status) {
  __shared__ u32 s_w[kPackWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int gr = blockIdx.x; gr < total_ranges; gr += gridDim.x) {
    const int im = image_of(args.range0, args.n, gr);
    const JpegImage &I = args.img[im];
    const u64 stream_bytes = (bitoff[args.mcu0[im] + im + I.nm] + 7) >> 3;
    const int r = gr - args.range0[im];
    const u64 start = (u64)r * kRange;
    if (start >= stream_bytes) continue;
    const int live = (int)((stream_bytes + kRange - 1) / kRange);
    const u64 *__restrict__ ffo = ffoff + args.range0[im] + im;
    const u64 length = kHeader + stream_bytes + ffo[live] + 2;
    const bool fits = length <= (u64)ot.cap[im];
    if (r == 0 && tid == 0) status[im] = fits ? 0 : 1;
    if (!fits) continue;
    unsigned char *__restrict__ file = out + ot.off[im];
    if (r == 0) {
      for (int i = tid; i < kHeader; i += kPackThreads) {
        unsigned char b = hdr.b[i];
        if (i >= 163 && i <= 166) b = (unsigned char)(i == 163 ? I.H >> 8 : i == 164 ? I.H & 255 : i == 165 ? I.W >> 8 : I.W & 255);
        file[i] = b;
      }
    }
    const u64 left = stream_bytes - start;
    const int nb = left < (u64)kRange ? (int)left : kRange;
    u32x4 word = {0u, 0u, 0u, 0u};
    if (16 * tid < nb) word = *reinterpret_cast<const u32x4 *>(stream + (size_t)gr * kRange + 16 * tid);
    int ff = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) ff += (16 * tid + j < nb && ((word[j >> 2] >> (8 * (j & 3))) & 255u) == 255u) ? 1 : 0;
    const int incl = wave_inclusive(ff, lane);
    if (lane == kWave - 1) s_w[wave] = (u32)incl;
    __syncthreads();
    u32 before = 0;
#pragma unroll
    for (int w = 0; w < kPackWaves; ++w) before += w < wave ? s_w[w] : 0u;
    unsigned char *__restrict__ o = file + kHeader + start + ffo[r] + before + (u32)(incl - ff) + 16 * tid;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      if (16 * tid + j < nb) {
        const unsigned char b = (unsigned char)((word[j >> 2] >> (8 * (j & 3))) & 255u);
        *o++ = b;
        if (b == 255) *o++ = 0;
      }
    }
    if (r == live - 1 && tid == 0) {
      file[length - 2] = 0xFF;
      file[length - 1] = 0xD9;
    }
    __syncthreads();
  }
}

// ---- host -----------------------------------------------------------------------------------------------------------------
void quant_tables(int quality, QuantTables &qt) {
  const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
  for (int t = 0; t < 2; ++t)
    for (int i = 0; i < 64; ++i) {
      const int v = ((t ? kBaseChroma[i] : kBaseLuma[i]) * s + 50) / 100;
      qt.q[t][i] = (unsigned short)(v < 1 ? 1 : (v > 255 ? 255 : v));
    }
}

void make_header(const QuantTables &qt, Header &h) {
  unsigned char *p = h.b;
  auto put = [&p](std::initializer_list<int> bytes) {
    for (int b : bytes) *p++ = (unsigned char)b;
  };
  put({0xFF, 0xD8, 0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0});
  for (int t = 0; t < 2; ++t) {
    put({0xFF, 0xDB, 0, 67, t});
    for (int i = 0; i < 64; ++i) *p++ = (unsigned char)qt.q[t][kZigzag[i]];
  }
  put({0xFF, 0xC0, 0, 17, 8, 0, 0, 0, 0, 3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1});      // (H, W: the kernel's)
  for (int k = 0; k < 4; ++k) {
    const int t = k >> 1, ac = k & 1;
    const unsigned char *bits = ac ? (t ? kAcChromaBits : kAcLumaBits) : (t ? kDcChromaBits : kDcLumaBits);
    const int nv = ac ? kAcVals : 12, len = 19 + nv;
    put({0xFF, 0xC4, len >> 8, len & 255, ac << 4 | t});
    for (int i = 0; i < 16; ++i) *p++ = bits[i];
    for (int i = 0; i < nv; ++i) *p++ = (unsigned char)(ac ? ac_val(t ? kAcChromaVals : kAcLumaVals, i) : i);
  }
  put({0xFF, 0xDA, 0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0});
  if (p - h.b != kHeader) abort();
}

bool disjoint(const void *a, uint64_t a_bytes, const void *b, uint64_t b_bytes) {
  return (uintptr_t)a + a_bytes <= (uintptr_t)b || (uintptr_t)b + b_bytes <= (uintptr_t)a;
}

// the table's sizes -> kernel arguments and the workspace's layout; src_bytes < 0: the source offsets are not checked
int plan(const char *what, const int64_t *table, int n, int64_t src_bytes, JpegArgs &args, Layout &L) {
  long long mcus = 0, ranges = 0;
  args = {};
  for (int i = 0; i < n; ++i) {
    const int64_t so = table[4 * i], H = table[4 * i + 2], W = table[4 * i + 3];
    KGDET_CHECK_SHAPE(H >= 1 && H <= kMaxSide && W >= 1 && W <= kMaxSide, "%s: image %d: %lld x %lld (sides 1 .. %d)", what, i,
                      (long long)H, (long long)W, kMaxSide);
    KGDET_CHECK_SHAPE(src_bytes < 0 || (so >= 0 && so <= src_bytes - 3 * H * W),
                      "%s: image %d: offset %lld with %lld bytes outside the buffer", what, i, (long long)so, (long long)(3 * H * W));
    JpegImage &I = args.img[i];
    I.src_off = so, I.H = (int)H, I.W = (int)W;
    I.mw = ceil_div((int)W, 16);
    I.nm = I.mw * ceil_div((int)H, 16);
    args.mcu0[i] = (int)mcus, args.range0[i] = (int)ranges;
    mcus += I.nm;
    ranges += ((long long)I.nm * kMcuWorst + kRange - 1) / kRange;
  }
  for (int i = n; i <= kMaxImages; ++i) args.mcu0[i] = (int)mcus, args.range0[i] = (int)ranges;
  args.n = n;
  L.coef = 0;
  L.bits = align_up((size_t)mcus * 768, 16);
  L.bitoff = align_up(L.bits + (size_t)mcus * 4, 16);
  L.ffcount = align_up(L.bitoff + (size_t)(mcus + n) * 8, 16);
  L.ffoff = align_up(L.ffcount + (size_t)ranges * 4, 16);
  L.stream = align_up(L.ffoff + (size_t)(ranges + n) * 8, 16);
  L.total = L.stream + (size_t)ranges * kRange;
  return KGDET_OK;
}

}  // namespace

}  // namespace kgdet

using namespace kgdet;

extern "C" {

size_t kgdet_jpeg_workspace_bytes(const int64_t *table, int32_t n) {
  if (n < 0 || n > kMaxImages || (n > 0 && !table)) return 0;
  JpegArgs args;
  Layout L;
  if (plan("jpeg_workspace_bytes", table, n, -1, args, L) != KGDET_OK) return 0;
  return L.total;
}

int kgdet_jpeg_encode(const uint8_t *src, int64_t src_bytes, const int64_t *table, int32_t n, int32_t quality, void *workspace,
                      size_t workspace_bytes, int64_t *lengths, void *stream) {
  KGDET_CHECK_SHAPE(n >= 0 && n <= kMaxImages, "jpeg_encode: %d images in one call (0 .. %d)", n, kMaxImages);
  KGDET_CHECK_SHAPE(quality >= 1 && quality <= 100, "jpeg_encode: quality %d (1 .. 100)", quality);
  KGDET_CHECK_SHAPE(src_bytes >= 0, "jpeg_encode: negative size");
  if (n == 0) return KGDET_OK;
  KGDET_CHECK_SHAPE(src && table && workspace && lengths, "jpeg_encode: null pointer");
  KGDET_CHECK_SHAPE(((uintptr_t)workspace & 15u) == 0, "jpeg_encode: the workspace is not 16-byte aligned");
  JpegArgs args;
  Layout L;
  if (int rc = plan("jpeg_encode", table, n, src_bytes, args, L)) return rc;
  if (workspace_bytes < L.total) {
    set_error("jpeg_encode: workspace of %zu bytes, %zu needed", workspace_bytes, L.total);
    return KGDET_E_WORKSPACE;
  }
  KGDET_CHECK_SHAPE(disjoint(src, (uint64_t)src_bytes, workspace, workspace_bytes) &&
                        disjoint(src, (uint64_t)src_bytes, lengths, 8ull * n) && disjoint(workspace, workspace_bytes, lengths, 8ull * n),
                    "jpeg_encode: source, workspace and lengths overlap");
  QuantTables qt;
  quant_tables(quality, qt);
  char *ws = (char *)workspace;
  short *coef = (short *)(ws + L.coef);
  u32 *bits = (u32 *)(ws + L.bits), *ffcount = (u32 *)(ws + L.ffcount);
  u64 *bitoff = (u64 *)(ws + L.bitoff), *ffoff = (u64 *)(ws + L.ffoff);
  unsigned char *bytes = (unsigned char *)(ws + L.stream);
  const int mcus = args.mcu0[n], ranges = args.range0[n];
  const int grid = std::min(ranges, 8 * cu_count());
  hipStream_t s = (hipStream_t)stream;
  const int stop = env_int("KGDET_JPEG_STOP_AFTER", 5);
  hipLaunchKernelGGL(jpeg_transform_kernel, dim3((unsigned)mcus), dim3(kWave), 0, s, args, qt, (const unsigned char *)src, coef);
  KGDET_CHECK_LAUNCH("jpeg_transform_kernel");
  if (stop <= 1) return KGDET_OK;
  hipLaunchKernelGGL(jpeg_measure_kernel, dim3((unsigned)ceil_div(mcus, kPackWaves)), dim3(kPackThreads), 0, s, args, mcus,
                     (const short *)coef, bits);
  KGDET_CHECK_LAUNCH("jpeg_measure_kernel");
  if (stop <= 2) return KGDET_OK;
  hipLaunchKernelGGL(jpeg_scan_bits_kernel, dim3((unsigned)n), dim3(kPackThreads), 0, s, args, (const u32 *)bits, bitoff);
  KGDET_CHECK_LAUNCH("jpeg_scan_bits_kernel");
  if (stop <= 3) return KGDET_OK;
  hipLaunchKernelGGL(jpeg_pack_kernel, dim3((unsigned)grid), dim3(kPackThreads), 0, s, args, ranges, (const short *)coef,
                     (const u64 *)bitoff, bytes, ffcount);
  KGDET_CHECK_LAUNCH("jpeg_pack_kernel");
  if (stop <= 4) return KGDET_OK;
  hipLaunchKernelGGL(jpeg_scan_ff_kernel, dim3((unsigned)n), dim3(kPackThreads), 0, s, args, (const u64 *)bitoff,
                     (const u32 *)ffcount, ffoff, (long long *)lengths);
  KGDET_CHECK_LAUNCH("jpeg_scan_ff_kernel");
  return KGDET_OK;
}

int kgdet_jpeg_write(const int64_t *table, int32_t n, int32_t quality, const void *workspace, size_t workspace_bytes,
                     const int64_t *capacity, uint8_t *out, int64_t out_bytes, int32_t *status, void *stream) {
  KGDET_CHECK_SHAPE(n >= 0 && n <= kMaxImages, "jpeg_write: %d images in one call (0 .. %d)", n, kMaxImages);
  KGDET_CHECK_SHAPE(quality >= 1 && quality <= 100, "jpeg_write: quality %d (1 .. 100)", quality);
  KGDET_CHECK_SHAPE(out_bytes >= 0, "jpeg_write: negative size");
  if (n == 0) return KGDET_OK;
  KGDET_CHECK_SHAPE(table && workspace && capacity && out && status, "jpeg_write: null pointer");
  KGDET_CHECK_SHAPE(((uintptr_t)workspace & 15u) == 0, "jpeg_write: the workspace is not 16-byte aligned");
  JpegArgs args;
  Layout L;
  if (int rc = plan("jpeg_write", table, n, -1, args, L)) return rc;
  if (workspace_bytes < L.total) {
    set_error("jpeg_write: workspace of %zu bytes, %zu needed", workspace_bytes, L.total);
    return KGDET_E_WORKSPACE;
  }
  OutTable ot;
  for (int i = 0; i < n; ++i) {
    ot.off[i] = table[4 * i + 1], ot.cap[i] = capacity[i];
    KGDET_CHECK_SHAPE(ot.off[i] >= 0 && ot.cap[i] >= 0 && ot.off[i] <= out_bytes - ot.cap[i],
                      "jpeg_write: image %d: offset %lld with a capacity of %lld bytes outside the buffer", i, ot.off[i], ot.cap[i]);
    for (int j = 0; j < i; ++j)
      KGDET_CHECK_SHAPE(ot.off[i] + ot.cap[i] <= ot.off[j] || ot.off[j] + ot.cap[j] <= ot.off[i],
                        "jpeg_write: the files of images %d and %d overlap", j, i);
  }
  KGDET_CHECK_SHAPE(disjoint(out, (uint64_t)out_bytes, workspace, workspace_bytes) &&
                        disjoint(out, (uint64_t)out_bytes, status, 4ull * n) && disjoint(workspace, workspace_bytes, status, 4ull * n),
                    "jpeg_write: output, workspace and status overlap");
  QuantTables qt;
  quant_tables(quality, qt);
  Header hdr;
  make_header(qt, hdr);
  const char *ws = (const char *)workspace;
  const int ranges = args.range0[n];
  const int grid = std::min(ranges, 8 * cu_count());
  hipLaunchKernelGGL(jpeg_finish_kernel, dim3((unsigned)grid), dim3(kPackThreads), 0, (hipStream_t)stream, args, ot, hdr, ranges,
                     (const u64 *)(ws + L.bitoff), (const unsigned char *)(ws + L.stream), (const u64 *)(ws + L.ffoff),
                     (unsigned char *)out, (int *)status);
  KGDET_CHECK_LAUNCH("jpeg_finish_kernel");
  return KGDET_OK;
}

}  // extern "C"
