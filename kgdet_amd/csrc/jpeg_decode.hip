// Baseline JPEG files -> RGB pictures in device memory (kgdet_amd/jpeg.py: DeviceJpegDecoder) for gfx950: kgdet_jpeg_decode.
// The picture is DEFINED by jpeg.decode_restatement (numpy / Python integers), itself held to PIL's decoder; these kernels are
// held to it bit for bit.  The host parses the header (jpeg.parse_header); the device gets the scan's bytes and a table block.
//
// Four kernels, all on the caller's stream, no read-back:
//  1. unstuff   a workgroup per image.  The scan ends at the first 0xFF that a byte other than 0x00 follows (a minimum over the
//     lanes' strided searches); EOI has to be that marker.  Then 16 bytes per lane: a byte is dropped when it is the 0x00 behind
//     an 0xFF, a workgroup scan of the kept counts places the rest.  32 bytes of 0xFF follow the stream, so that the decoder's
//     64-bit windows never read what nobody wrote, and read 1-bits behind the end.
//  2. huffman   a workgroup per image, a lane per subsequence of kSub bits, kLanes subsequences at a time.  State = (bit
//     position, block slot of the MCU, zigzag index).  `decode_span` decodes the symbols that START in the lane's subsequence.
//     Lane 0 of a chunk enters with the true state, the others cold; exit[i] -> entry[i + 1] is iterated until a workgroup-wide
//     vote finds no change.  Round k fixes lane k at the latest, so at most (lanes of the chunk) + 1 rounds, whatever the picture
//     (a uniform picture is a periodic stream in which a shifted parse never meets the true one: it takes that many rounds and
//     is decoded all the same).  A lane decodes again only when its entry changed.  Speculative parses write states only; an
//     unmatched code or an index past 63 gives the INVALID state, which equals no valid state.  A lane whose predecessor left
//     INVALID keeps its cold start (a few in a hundred cold parses end so; handed on, each would walk down the chunk a lane per
//     round and cost as many rounds as a uniform picture); on the TRUE parse INVALID is met by the write pass and is the status.
//     Then: an exclusive scan of the completed-block counts, `decode_span<true>` from the now-true entries stores the non-zero
//     coefficients (int16, natural order; block < the frame's count checked at every store); the chunk's last exit is the next
//     chunk's entry.  At the end the checks of the TRUE parse (status) and the inclusive scan of the DC differences.
//     Look-ups in LDS per table: 256 entries for codes up to 8 bits, maxcode / value offset per length for longer ones.
//  3. idct      a thread per block: level * q, libjpeg's islow inverse DCT (13-bit constants; pass 1 down the columns >> 11, pass
//     2 along the rows >> 18, + 128, clamp) in 64-bit integers, since nothing bounds what a file's levels dequantise to;
//     8-byte stores into sample planes padded to whole blocks.
//  4. colour    a lane per 16 destination bytes at DESTINATION alignment (rows of 3 W bytes are not aligned): up to seven
//     pixels, fancy-upsampled chroma read from the planes (L2-resident), one 16-byte store; bytes at the head and the tail.
// Integers only; no global atomics; plain C++ and vector stores.
//
// kgdet_jpeg_decode_stages (tools/time_jpeg_decode.py) is the same call cut short after its first `stages` kernels: the
// kernels' own times by difference.  A call cut short leaves no picture and says so: every status becomes
// KGDET_JPEG_DECODE_STOPPED.  No environment switch.
#include <algorithm>

#include "common.h"

namespace kgdet {

namespace {

constexpr int kWave = 64;
constexpr int kMaxImages = KGDET_JPEG_DECODE_MAX_IMAGES;
constexpr int kMaxSide = 8192;
constexpr int kSub = KGDET_JPEG_DECODE_SUBSEQ_BITS;
constexpr int kLanes = KGDET_JPEG_DECODE_CHUNK_LANES, kWaves = kLanes / kWave;
constexpr int kTableBytes = KGDET_JPEG_DECODE_TABLE_BYTES;
constexpr long long kMaxScanBytes = 1ll << 28;      // 8 * bytes fits 32 bits
constexpr int kStreamPad = 32;
constexpr int kBackThreads = 256;
// camera entry points: the stream a tile of whole restart intervals holds on average, a chunk's worth
constexpr long long kTileBytes = (long long)kLanes * kSub / 8;

typedef unsigned char u8;
typedef unsigned int u32;
typedef unsigned long long u64;
typedef long long i64;
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

__constant__ const u8 d_zigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                      41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                      30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct DecImage {
  i64 scan_off, tab_off, dst_off;                   // inside src, src, out
  i64 stream_off, coef_off, plane_off;              // inside the workspace, 16-byte aligned
  int scan_bytes, H, W, mode;
};

struct DecArgs {
  DecImage img[kMaxImages];
  int n;
};

// what follows from an image's sizes
struct Geometry {
  int mw, mh, bpm, nblocks;                         // MCUs per row, MCU rows, blocks per MCU, blocks
  int pw0, ph0, pw1, ph1;                           // the luma plane's and a chroma plane's padded extent
};

// CAM: the camera entry points' instance, which also knows mode 3 (an MCU 16 wide and 8 high, 4 blocks)
template <bool CAM = false>
__host__ __device__ inline Geometry geometry(int H, int W, int mode) {
  Geometry g;
  if (CAM && mode == KGDET_JPEG_DECODE_422) {
    g.mw = (W + 15) / 16, g.mh = (H + 7) / 8, g.bpm = 4;
    g.nblocks = g.mw * g.mh * g.bpm;
    g.pw0 = g.mw * 16, g.ph0 = g.mh * 8, g.pw1 = g.mw * 8, g.ph1 = g.mh * 8;
    return g;
  }
  const int unit = mode == KGDET_JPEG_DECODE_420 ? 16 : 8;
  g.mw = (W + unit - 1) / unit, g.mh = (H + unit - 1) / unit;
  g.bpm = mode == KGDET_JPEG_DECODE_420 ? 6 : (mode == KGDET_JPEG_DECODE_444 ? 3 : 1);
  g.nblocks = g.mw * g.mh * g.bpm;
  g.pw0 = g.mw * unit, g.ph0 = g.mh * unit;
  g.pw1 = mode == KGDET_JPEG_DECODE_GREY ? 0 : g.mw * 8, g.ph1 = mode == KGDET_JPEG_DECODE_GREY ? 0 : g.mh * 8;
  return g;
}

__device__ __forceinline__ int wave_inclusive(int v, int lane) {
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    const int o = __shfl_up(v, d, kWave);
    if (lane >= d) v += o;
  }
  return v;
}

// exclusive scan of one int per thread over a workgroup of kLanes threads; `total` = the sum.  Two barriers.
__device__ __forceinline__ int block_exclusive(int v, int *s_w, int &total) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int incl = wave_inclusive(v, lane);
  __syncthreads();                                  // (s_w may still be read from the previous use)
  if (lane == kWave - 1) s_w[wave] = incl;
  __syncthreads();
  int before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) {
    const int x = s_w[w];
    before += w < wave ? x : 0;
    all += x;
  }
  total = all;
  return before + incl - v;
}

// ---- 1. unstuff -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kLanes) void jpeg_unstuff_kernel(const DecArgs args, const u8 *__restrict__ src, u8 *__restrict__ ws,
                                                              u32 *__restrict__ lens, int *__restrict__ status) {
  __shared__ u32 s_end;
  __shared__ int s_w[kWaves];
  const int tid = threadIdx.x, im = blockIdx.x;
  const DecImage &I = args.img[im];
  const u8 *__restrict__ in = src + I.scan_off;
  u8 *__restrict__ out = ws + I.stream_off;
  const u32 nbytes = (u32)I.scan_bytes;
  if (tid == 0) s_end = 0xffffffffu;
  __syncthreads();
  for (u32 k = tid; k + 1 < nbytes; k += kLanes) {
    if (in[k] == 0xFF && in[k + 1] != 0) {          // (the lane's first: its smallest)
      atomicMin(&s_end, k);
      break;
    }
  }
  __syncthreads();
  const u32 end = s_end;
  if (end == 0xffffffffu || in[end + 1] != 0xD9) {  // (uniform)
    if (tid == 0) {
      status[im] = end == 0xffffffffu ? KGDET_JPEG_DECODE_NO_MARKER : KGDET_JPEG_DECODE_NOT_EOI;
      lens[im] = 0;
    }
    return;
  }
  u32 carry = 0;
  for (u32 base = 0; base < end; base += 16 * kLanes) {
    const u32 k0 = base + 16 * tid;
    u8 b[16];
    u32 keep = 0;
    int count = 0;
    if (k0 < end) {
      u8 prev = k0 ? in[k0 - 1] : 0;
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const bool live = k0 + j < end;
        b[j] = live ? in[k0 + j] : 0;
        const bool kept = live && !(b[j] == 0 && prev == 0xFF);
        keep |= kept ? 1u << j : 0u;
        count += kept ? 1 : 0;
        prev = b[j];
      }
    }
    int total;
    const int at = block_exclusive(count, s_w, total);
    u8 *o = out + carry + at;
#pragma unroll
    for (int j = 0; j < 16; ++j)
      if (keep >> j & 1u) *o++ = b[j];
    carry += (u32)total;
  }
  if (tid < kStreamPad) out[carry + tid] = 0xFF;
  if (tid == 0) {
    status[im] = 0;
    lens[im] = carry;
  }
}

// ---- 2. huffman -------------------------------------------------------------------------------------------------------------
struct Huff {
  unsigned short lut[256];                          // by the next 8 bits: length << 8 | symbol, 0: no code of up to 8 bits
  int maxcode[17];                                  // the largest code of each length, -1: none
  int valoff[17];                                   // index of a code's value = valoff[length] + code
  u8 vals[256];
};

struct State {
  u32 p, bz;                                        // bit position; slot << 8 | zigzag index
};
constexpr u32 kInvalid = 0xffffffffu;

__device__ __forceinline__ bool same(State a, State b) { return a.p == b.p && a.bz == b.bz; }

// the 32 bits from bit p of the big-endian stream
__device__ __forceinline__ u32 peek(const u32 *__restrict__ words, u32 p) {
  const u32 w = p >> 5;
  const u64 both = (u64)__builtin_bswap32(words[w]) << 32 | __builtin_bswap32(words[w + 1]);
  return (u32)((both << (p & 31)) >> 32);
}

// jpeg.decode_span: the symbols that start in [st.p, limit) of a stream of `total` bits; `done` = blocks completed.  WRITE: the
// non-zero values go to block `blk` + done of `coef` when that is a block of the frame, else `beyond` is set.
template <bool WRITE, bool CAM = false>
__device__ __forceinline__ State decode_span(State st, u32 start, u32 limit, u32 total, const u32 *__restrict__ words,
                                             const Huff *s_h, const u8 *s_tab, const u8 *s_zz, int mode, int bpm, int &done,
                                             short *__restrict__ coef, int blk, int nblocks, bool &beyond) {
  done = 0;
  if (st.p < start || st.p >= limit || st.p >= total) return st;       // (INVALID included: it passes through)
  u32 p = st.p;
  int b = (int)(st.bz >> 8), z = (int)(st.bz & 255u);
  const State invalid = {kInvalid, kInvalid};
  while (p < limit && p < total) {
    const int comp = mode == KGDET_JPEG_DECODE_420 ? max(b - 3, 0) : (CAM && mode == KGDET_JPEG_DECODE_422 ? max(b - 1, 0) : b);
    const Huff &T = s_h[z == 0 ? (s_tab[comp] & 1) : 2 + (s_tab[3 + comp] & 1)];
    const u32 w32 = peek(words, p);
    const u32 w16 = w32 >> 16;
    int len = 0, sym = 0;
    const u32 e = T.lut[w16 >> 8];
    if (e) {
      len = (int)(e >> 8), sym = (int)(e & 255u);
    } else {
      for (int l = 9; l <= 16; ++l) {
        const int code = (int)(w16 >> (16 - l));
        if (code <= T.maxcode[l]) {
          sym = T.vals[min(max(T.valoff[l] + code, 0), 255)];
          len = l;
          break;
        }
      }
    }
    if (len == 0) {
      if (total - p < 16) break;                    // no code fits what is left of the stream
      return invalid;
    }
    int run = 0, s, place = 0;
    if (z == 0) {
      s = sym;
      if (s > 11) return invalid;
    } else {
      run = sym >> 4, s = sym & 15;
      if (s == 0) {
        if (run == 15) {
          if (z + 16 > 63) return invalid;
        } else if (run != 0) {
          return invalid;
        }
      } else if (z + run > 63 || s > 10) {
        return invalid;
      }
      place = z + run;
    }
    if (p + (u32)(len + s) > total) break;          // the symbol would run past the last bit: not taken
    bool ends = false;
    int nz;
    if (z == 0 || s) {
      if (WRITE && s) {
        int v = (int)((w32 >> (32 - len - s)) & ((1u << s) - 1u));
        if (!(v >> (s - 1))) v -= (1 << s) - 1;
        if (blk + done < nblocks)
          coef[(size_t)(blk + done) * 64 + s_zz[place]] = (short)v;
        else
          beyond = true;
      }
      nz = place + 1;
      ends = nz == 64;
    } else if (run == 15) {
      nz = z + 16;
    } else {
      nz = 0, ends = true;
    }
    p += (u32)(len + s);
    if (ends) {
      z = 0;
      b = b + 1 < bpm ? b + 1 : 0;
      ++done;
    } else {
      z = nz;
    }
  }
  State out;
  out.p = p, out.bz = (u32)b << 8 | (u32)z;
  return out;
}

// the look-ups of an image's four Huffman tables, Annex C / F.2.2.3, by the whole workgroup; every index made from the table
// block is clamped.  Ends behind a barrier.  (jpeg_huffman_kernel keeps the same statements in its body: called from there the
// compiler allocates that kernel's registers differently, and the old entry point's code stays instruction for instruction what
// it was.)
__device__ __forceinline__ void build_tables(const u8 *__restrict__ tab, Huff *s_h, u8 *s_tab, u8 *s_zz, int *s_bad) {
  const int tid = threadIdx.x;
  for (int i = tid; i < 4 * 256; i += kLanes) s_h[i >> 8].lut[i & 255] = 0;
  if (tid < 64) s_zz[tid] = d_zigzag[tid];
  if (tid < 6) s_tab[tid] = tab[800 + tid];
  if (tid == 0) *s_bad = 0;
  __syncthreads();
  if (tid < 4) {
    const int ac = tid >> 1, th = tid & 1, nvals = ac ? 256 : 16;
    const u8 *bits = tab + (ac ? 256 : 192) + 16 * th, *vals = tab + (ac ? 288 + 256 * th : 224 + 16 * th);
    Huff &T = s_h[tid];
    int code = 0, k = 0;
    T.maxcode[0] = -1, T.valoff[0] = 0;
    for (int len = 1; len <= 16; ++len) {
      const int count = bits[len - 1];
      T.valoff[len] = k - code;
      for (int i = 0; i < count; ++i, ++code, ++k) {
        if (len <= 8) {
          const int lo = code << (8 - len);
          const unsigned short entry = (unsigned short)(len << 8 | vals[min(k, nvals - 1)]);
          for (int j = 0; j < (1 << (8 - len)); ++j)
            if (lo + j < 256) T.lut[lo + j] = entry;
        }
      }
      T.maxcode[len] = count ? code - 1 : -1;
      code <<= 1;
    }
    for (int i = 0; i < 256; ++i) T.vals[i] = i < nvals ? vals[i] : 0;
  }
  __syncthreads();
}

__global__ __launch_bounds__(kLanes) void jpeg_huffman_kernel(const DecArgs args, const u8 *__restrict__ src, u8 *__restrict__ ws,
                                                              const u32 *__restrict__ lens, u32 *__restrict__ rounds,
                                                              int *__restrict__ status) {
  __shared__ Huff s_h[4];                           // DC 0, DC 1, AC 0, AC 1
  __shared__ u8 s_tab[8], s_zz[64];
  __shared__ u32 s_exit_p[kLanes], s_exit_bz[kLanes];
  __shared__ int s_w[kWaves];
  __shared__ int s_bad;
  const int tid = threadIdx.x, im = blockIdx.x;
  if (status[im] != 0) return;                      // (uniform: the first kernel refused the scan)
  const DecImage &I = args.img[im];
  const Geometry g = geometry(I.H, I.W, I.mode);
  const u8 *__restrict__ tab = src + I.tab_off;
  const u32 *__restrict__ words = (const u32 *)(ws + I.stream_off);
  short *__restrict__ coef = (short *)(ws + I.coef_off);
  const u32 total = 8u * lens[im];
  // the look-ups, Annex C / F.2.2.3; every index made from the table block is clamped
  for (int i = tid; i < 4 * 256; i += kLanes) s_h[i >> 8].lut[i & 255] = 0;
  if (tid < 64) s_zz[tid] = d_zigzag[tid];
  if (tid < 6) s_tab[tid] = tab[800 + tid];
  if (tid == 0) s_bad = 0;
  __syncthreads();
  if (tid < 4) {
    const int ac = tid >> 1, th = tid & 1, nvals = ac ? 256 : 16;
    const u8 *bits = tab + (ac ? 256 : 192) + 16 * th, *vals = tab + (ac ? 288 + 256 * th : 224 + 16 * th);
    Huff &T = s_h[tid];
    int code = 0, k = 0;
    T.maxcode[0] = -1, T.valoff[0] = 0;
    for (int len = 1; len <= 16; ++len) {
      const int count = bits[len - 1];
      T.valoff[len] = k - code;
      for (int i = 0; i < count; ++i, ++code, ++k) {
        if (len <= 8) {
          const int lo = code << (8 - len);
          const unsigned short entry = (unsigned short)(len << 8 | vals[min(k, nvals - 1)]);
          for (int j = 0; j < (1 << (8 - len)); ++j)
            if (lo + j < 256) T.lut[lo + j] = entry;
        }
      }
      T.maxcode[len] = count ? code - 1 : -1;
      code <<= 1;
    }
    for (int i = 0; i < 256; ++i) T.vals[i] = i < nvals ? vals[i] : 0;
  }
  __syncthreads();
  const u32 nsub = (total + kSub - 1) / kSub;
  State chunk_entry = {0u, 0u};
  int blocks = 0;                                   // blocks completed before the chunk
  bool beyond = false;
  int most_rounds = 0;                              // of any chunk (tools/time_jpeg_decode.py reads it)
  for (u32 base = 0; base < nsub; base += kLanes) {
    const int nl = (int)min((u32)kLanes, nsub - base);
    const u32 start = (base + tid) * kSub, limit = start + kSub;
    State entry = {start, 0u}, ex = entry;
    if (tid == 0) entry = chunk_entry;
    bool need = tid < nl;
    int done = 0;
    bool settled = false;
    for (int round = 0; round <= nl; ++round) {
      if (need) {
        ex = decode_span<false>(entry, start, limit, total, words, s_h, s_tab, s_zz, I.mode, g.bpm, done, coef, 0, 0, beyond);
        s_exit_p[tid] = ex.p, s_exit_bz[tid] = ex.bz;
      }
      __syncthreads();
      need = false;
      if (tid > 0 && tid < nl) {
        State in;
        in.p = s_exit_p[tid - 1], in.bz = s_exit_bz[tid - 1];
        if (in.p == kInvalid) in.p = start, in.bz = 0u;               // an invalid parse tells nothing: the cold start again
        need = !same(in, entry);
        entry = in;
      }
      if (!__syncthreads_or(need ? 1 : 0)) {
        settled = true;
        most_rounds = max(most_rounds, round + 1);
        break;
      }
    }
    if (!settled) beyond = true;                    // (cannot happen: round k fixes lane k)
    int all;
    const int first = blocks + block_exclusive(tid < nl ? done : 0, s_w, all);
    if (tid < nl) {
      int again;
      const State wx = decode_span<true>(entry, start, limit, total, words, s_h, s_tab, s_zz, I.mode, g.bpm, again, coef, first,
                                         g.nblocks, beyond);
      if (wx.p == kInvalid) beyond = true;                             // the TRUE parse met an invalid code
      if (!same(wx, ex) || again != done) beyond = true;               // (cannot happen: the fixpoint is the true parse)
    }
    chunk_entry.p = s_exit_p[nl - 1], chunk_entry.bz = s_exit_bz[nl - 1];
    blocks += all;
    __syncthreads();                                // (the exits are read before the next chunk overwrites them)
  }
  if (beyond) s_bad = 1;                            // (an idempotent flag store)
  if (tid == 0) rounds[im] = (u32)most_rounds;
  __syncthreads();
  const bool good = !s_bad && chunk_entry.p != kInvalid && (chunk_entry.bz & 255u) == 0 && blocks == g.nblocks &&
                    chunk_entry.p <= total && total - chunk_entry.p < 8;
  if (!good) {
    if (tid == 0) status[im] = KGDET_JPEG_DECODE_BAD_SCAN;
    return;
  }
  // DC values: the inclusive scan of the differences per component, an MCU per lane; clamped to int16 as the definition says
  const int nm = g.mw * g.mh;
  int carry[3] = {0, 0, 0};
  for (int m0 = 0; m0 < nm; m0 += kLanes) {
    const int m = m0 + tid;
    int d[6] = {0, 0, 0, 0, 0, 0}, sum[3] = {0, 0, 0};
    if (m < nm) {
#pragma unroll
      for (int k = 0; k < 6; ++k)
        if (k < g.bpm) d[k] = coef[((size_t)m * g.bpm + k) * 64];
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const int c = I.mode == KGDET_JPEG_DECODE_420 ? (k < 4 ? 0 : k - 3) : (k < 3 ? k : 0);
      sum[c] += d[k];
    }
    int before[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      int all;
      before[c] = carry[c] + block_exclusive(sum[c], s_w, all);
      carry[c] += all;
    }
    if (m < nm) {
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        if (k < g.bpm) {
          const int c = I.mode == KGDET_JPEG_DECODE_420 ? (k < 4 ? 0 : k - 3) : (k < 3 ? k : 0);
          before[c] += d[k];
          coef[((size_t)m * g.bpm + k) * 64] = (short)min(max(before[c], -32768), 32767);
        }
      }
    }
  }
}

// ---- 1c / 2c. the camera entry points: restart intervals -------------------------------------------------------------------
// kgdet_jpeg_decode_camera (jpeg.decode_restatement(camera=True)): 4:2:2 files (mode 3) and restart intervals.  With an
// interval of R MCUs the scan holds nint = ceil(MCUs / R) pieces between RSTm markers; at every piece's first bit the true
// state is known ((0, 0), predictors 0) and so is the index of its first block, i * R * blocks per MCU.
//  1c. unstuff  as above, and: a restart marker does not end the scan, both its bytes are dropped, and the lane that holds its
//      0xFF writes where the next interval's un-stuffed bytes begin into the image's interval table (its ordinal is the
//      scan of the marker counts, which rides in the high half of the kept counts' scan).  The ordinal fixes the marker's number
//      and must stay below nint - 1; at the end there must be nint - 1 of them: else KGDET_JPEG_DECODE_BAD_RESTART.  Then per
//      interval its length and the exclusive scan of its subsequences, max(1, ceil(bits / kSub)), counted from ITS first bit.
//  2c. huffman  a workgroup per (tile, image); a tile is a run of `per_tile` whole intervals (the host's plan: about a chunk's
//      worth of stream, at most kLanes intervals).  A lane per subsequence of an interval, kLanes at a time; a lane that holds
//      an interval's first subsequence enters with the true state and never takes its predecessor's exit, the others iterate as
//      above, within the interval's own bits.  The block index of a lane is the interval's first block plus the SEGMENTED scan
//      of the completed-block counts (prefix minus the prefix at the interval's first lane, or the blocks carried over from
//      earlier chunks); stores are confined to the interval's own blocks.  The lane of an interval's last subsequence checks its
//      share of blocks and its end.  Then the DC scan of the tile's MCUs, restarting at every interval.  A tile leaves
//      (status, rounds) in the workspace; `verdict` (a workgroup per image) takes the first tile's non-zero status and the most
//      rounds: no atomics on global memory, and the status does not depend on which tile ran first.
struct CamImage {
  i64 table_off, tile_off;                          // inside the workspace: uint32 begin / length / first subsequence [nint + 1] each; uint32 [ntiles][2]
  int interval, nint, per_tile, ntiles;             // R (0: none), intervals, intervals per tile, tiles
};

struct CamArgs {
  CamImage img[kMaxImages];
};

__device__ __forceinline__ int slot_component(int mode, int k) {
  return mode == KGDET_JPEG_DECODE_420 ? (k < 4 ? 0 : k - 3) : (mode == KGDET_JPEG_DECODE_422 ? (k < 2 ? 0 : k - 1) : (k < 3 ? k : 0));
}

__global__ __launch_bounds__(kLanes) void jpeg_unstuff_camera_kernel(const DecArgs args, const CamArgs cam,
                                                                     const u8 *__restrict__ src, u8 *__restrict__ ws,
                                                                     u32 *__restrict__ lens, int *__restrict__ status) {
  __shared__ u32 s_end;
  __shared__ int s_w[kWaves];
  __shared__ int s_bad;
  const int tid = threadIdx.x, im = blockIdx.x;
  const DecImage &I = args.img[im];
  const CamImage &C = cam.img[im];
  const u8 *__restrict__ in = src + I.scan_off;
  u8 *__restrict__ out = ws + I.stream_off;
  u32 *begin = (u32 *)(ws + C.table_off), *length = begin + (C.nint + 1), *first = length + (C.nint + 1);
  const u32 nbytes = (u32)I.scan_bytes;
  const bool rst = C.interval > 0;
  if (tid == 0) s_end = 0xffffffffu, s_bad = 0;
  __syncthreads();
  for (u32 k = tid; k + 1 < nbytes; k += kLanes) {
    if (in[k] == 0xFF) {
      const u8 nx = in[k + 1];
      if (nx != 0 && !(rst && nx >= 0xD0 && nx <= 0xD7)) {
        atomicMin(&s_end, k);
        break;
      }
    }
  }
  __syncthreads();
  const u32 end = s_end;
  if (end == 0xffffffffu || in[end + 1] != 0xD9) {  // (uniform)
    if (tid == 0) {
      status[im] = end == 0xffffffffu ? KGDET_JPEG_DECODE_NO_MARKER : KGDET_JPEG_DECODE_NOT_EOI;
      lens[im] = 0;
    }
    return;
  }
  // before `end` every 0xFF is followed by 0x00 or, with an interval, by RSTm: never by another 0xFF
  u32 carry = 0, markers = 0;
  for (u32 base = 0; base < end; base += 16 * kLanes) {
    const u32 k0 = base + 16 * tid;
    u8 b[17];
    u32 keep = 0, lead = 0;
    int count = 0, nlead = 0;
    if (k0 < end) {
      u8 prev = k0 ? in[k0 - 1] : 0;
#pragma unroll
      for (int j = 0; j < 17; ++j) b[j] = k0 + j <= end ? in[k0 + j] : 0;       // (in[end] is the 0xFF of EOI)
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const bool live = k0 + j < end;
        const bool leads = rst && live && b[j] == 0xFF && b[j + 1] >= 0xD0 && b[j + 1] <= 0xD7;
        const bool follows = prev == 0xFF && (b[j] == 0 || (rst && b[j] >= 0xD0 && b[j] <= 0xD7));
        const bool kept = live && !leads && !follows;
        keep |= kept ? 1u << j : 0u;
        lead |= leads ? 1u << j : 0u;
        count += kept ? 1 : 0;
        nlead += leads ? 1 : 0;
        prev = b[j];
      }
    }
    int total;
    const int at = block_exclusive(count | nlead << 16, s_w, total);            // kept bytes <= 16384 a pass: the halves do not mix
    u8 *o = out + carry + (u32)(at & 0xffff);
    u32 ordinal = markers + (u32)(at >> 16);
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      if (lead >> j & 1u) {
        if (ordinal + 1 < (u32)C.nint) {
          begin[ordinal + 1] = (u32)(o - out);
          if ((u32)(b[j + 1] - 0xD0) != (ordinal & 7u)) s_bad = 1;              // (an idempotent flag store)
        } else {
          s_bad = 1;                                                            // a surplus marker
        }
        ++ordinal;
      }
      if (keep >> j & 1u) *o++ = b[j];
    }
    carry += (u32)(total & 0xffff);
    markers += (u32)(total >> 16);
  }
  if (tid < kStreamPad) out[carry + tid] = 0xFF;
  if (tid == 0) {
    begin[0] = 0, begin[C.nint] = carry;
    if (markers != (u32)(C.nint - 1)) s_bad = 1;
  }
  __syncthreads();
  if (s_bad) {                                      // (uniform)
    if (tid == 0) {
      status[im] = KGDET_JPEG_DECODE_BAD_RESTART;
      lens[im] = 0;
    }
    return;
  }
  u32 subs = 0;
  for (int i0 = 0; i0 <= C.nint; i0 += kLanes) {
    const int i = i0 + tid;
    u32 bytes = 0;
    if (i < C.nint) bytes = begin[i + 1] - begin[i];
    int total;
    const int at = block_exclusive(i < C.nint ? (int)max((bytes + kSub / 8 - 1) / (kSub / 8), 1u) : 0, s_w, total);
    if (i <= C.nint) length[i] = bytes, first[i] = subs + (u32)at;
    subs += (u32)total;
  }
  if (tid == 0) {
    status[im] = 0;
    lens[im] = carry;
  }
}

__global__ __launch_bounds__(kLanes) void jpeg_huffman_camera_kernel(const DecArgs args, const CamArgs cam,
                                                                     const u8 *__restrict__ src, u8 *__restrict__ ws,
                                                                     const int *__restrict__ status) {
  __shared__ Huff s_h[4];                           // DC 0, DC 1, AC 0, AC 1
  __shared__ u8 s_tab[8], s_zz[64];
  __shared__ u32 s_exit_p[kLanes], s_exit_bz[kLanes];
  __shared__ u32 s_first[kLanes + 1];               // the first subsequence of the tile's intervals, and the end
  __shared__ int s_pre[kLanes];                     // the chunk's exclusive scan of the block counts
  __shared__ int s_dc[3][kLanes];
  __shared__ int s_w[kWaves];
  __shared__ int s_bad, s_count, s_carry;
  const int tid = threadIdx.x, im = blockIdx.y, tile = blockIdx.x;
  if (status[im] != 0) return;                      // (uniform: the first kernel refused the scan)
  const CamImage &C = cam.img[im];
  if (tile >= C.ntiles) return;                     // (uniform)
  const DecImage &I = args.img[im];
  const Geometry g = geometry<true>(I.H, I.W, I.mode);
  const u8 *__restrict__ tab = src + I.tab_off;
  const u32 *__restrict__ words = (const u32 *)(ws + I.stream_off);
  short *__restrict__ coef = (short *)(ws + I.coef_off);
  const u32 *__restrict__ begin = (const u32 *)(ws + C.table_off), *__restrict__ length = begin + (C.nint + 1),
                         *__restrict__ first = length + (C.nint + 1);
  u32 *__restrict__ verdict = (u32 *)(ws + C.tile_off) + 2 * tile;
  const int nm = g.mw * g.mh, R = C.interval ? min(C.interval, nm) : nm;        // MCUs of an interval
  const int i0 = tile * C.per_tile, i1 = min(i0 + C.per_tile, C.nint), ni = i1 - i0;      // ni <= kLanes
  build_tables(tab, s_h, s_tab, s_zz, &s_bad);
  if (tid == 0) s_count = 0, s_carry = 0;
  for (int k = tid; k <= ni; k += kLanes) s_first[k] = first[i0 + k];
  __syncthreads();
  const u32 sub0 = s_first[0], sub1 = s_first[ni];
  State chunk_entry = {kInvalid, kInvalid};         // (the tile's first lane holds an interval start)
  int carried = 0;                                  // blocks the interval that runs into this chunk completed in earlier ones
  bool bad_scan = false, bad_count = false;
  int most_rounds = 0;
  for (u32 base = sub0; base < sub1; base += kLanes) {
    const int nl = (int)min((u32)kLanes, sub1 - base);
    const bool live = tid < nl;
    u32 j = 0, start = 0, limit = 0, total = 0;
    int share = 0, blk0 = 0;
    bool tail = false;
    if (live) {
      const u32 l = base + (u32)tid;
      int lo = 0, hi = ni - 1;                      // the interval: the last one that begins at or before subsequence l
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (s_first[mid] <= l)
          lo = mid;
        else
          hi = mid - 1;
      }
      const int itv = i0 + lo;
      j = l - s_first[lo], tail = l + 1 == s_first[lo + 1];
      const u32 at = begin[itv];
      start = 8u * at + j * kSub, limit = start + kSub, total = 8u * (at + length[itv]);
      share = min(R, nm - itv * R) * g.bpm, blk0 = itv * R * g.bpm;
    }
    const bool head = j == 0;
    State entry = {start, 0u}, ex = entry;
    if (tid == 0 && !head) entry = chunk_entry;
    bool need = live;
    int done = 0;
    bool settled = false, beyond = false;
    for (int round = 0; round <= nl; ++round) {
      if (need) {
        ex = decode_span<false, true>(entry, start, limit, total, words, s_h, s_tab, s_zz, I.mode, g.bpm, done, coef, 0, 0, beyond);
        s_exit_p[tid] = ex.p, s_exit_bz[tid] = ex.bz;
      }
      __syncthreads();
      need = false;
      if (tid > 0 && live && !head) {
        State in;
        in.p = s_exit_p[tid - 1], in.bz = s_exit_bz[tid - 1];
        if (in.p == kInvalid) in.p = start, in.bz = 0u;               // an invalid parse tells nothing: the cold start again
        need = !same(in, entry);
        entry = in;
      }
      if (!__syncthreads_or(need ? 1 : 0)) {
        settled = true;
        most_rounds = max(most_rounds, round + 1);
        break;
      }
    }
    if (!settled) bad_scan = true;                  // (cannot happen: round k fixes lane k)
    int all;
    const int pre = block_exclusive(live ? done : 0, s_w, all);
    s_pre[tid] = pre;
    __syncthreads();
    if (live) {
      const int before = j <= (u32)tid ? pre - s_pre[tid - (int)j] : carried + pre;       // blocks of the interval before the lane
      int again;
      const State wx = decode_span<true, true>(entry, start, limit, total, words, s_h, s_tab, s_zz, I.mode, g.bpm, again, coef,
                                               blk0 + before, blk0 + share, beyond);
      if (wx.p == kInvalid) bad_scan = true;                           // the TRUE parse met an invalid code
      if (!same(wx, ex) || again != done) bad_scan = true;             // (cannot happen: the fixpoint is the true parse)
      if (beyond) bad_count = true;                                    // more blocks than the interval's share
      if (tail && !(ex.p != kInvalid && (ex.bz & 255u) == 0 && before + done == share && ex.p <= total && total - ex.p < 8))
        bad_count = true;
      if (tid == nl - 1) s_carry = before + done;
    }
    chunk_entry.p = s_exit_p[nl - 1], chunk_entry.bz = s_exit_bz[nl - 1];
    __syncthreads();                                // (the exits and the scan are read before the next chunk overwrites them)
    carried = s_carry;
  }
  if (bad_scan) s_bad = 1;                          // (idempotent flag stores)
  if (bad_count) s_count = 1;
  __syncthreads();
  const int code = s_bad ? KGDET_JPEG_DECODE_BAD_SCAN
                         : (s_count ? (C.interval ? KGDET_JPEG_DECODE_BAD_RESTART : KGDET_JPEG_DECODE_BAD_SCAN) : 0);
  if (tid == 0) verdict[0] = (u32)code, verdict[1] = (u32)most_rounds;
  if (code) return;                                 // (uniform)
  // DC values of the tile's MCUs: the inclusive scan of the differences per component restarts at every interval
  const int mfirst = i0 * R, mend = min(i1 * R, nm);
  int carry[3] = {0, 0, 0};                         // the sums of the segment that runs into this chunk
  for (int m0 = mfirst; m0 < mend; m0 += kLanes) {
    const int m = m0 + tid;
    int d[6] = {0, 0, 0, 0, 0, 0}, sum[3] = {0, 0, 0};
    if (m < mend) {
#pragma unroll
      for (int k = 0; k < 6; ++k)
        if (k < g.bpm) d[k] = coef[((size_t)m * g.bpm + k) * 64];
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) sum[slot_component(I.mode, k)] += d[k];
    int pre[3], all[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      pre[c] = block_exclusive(sum[c], s_w, all[c]);
      s_dc[c][tid] = pre[c];
    }
    __syncthreads();
    if (m < mend) {
      const int seg = mfirst + (m - mfirst) / R * R;                   // the first MCU of m's interval
      int before[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) before[c] = seg >= m0 ? pre[c] - s_dc[c][seg - m0] : carry[c] + pre[c];
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        if (k < g.bpm) {
          const int c = slot_component(I.mode, k);
          before[c] += d[k];
          coef[((size_t)m * g.bpm + k) * 64] = (short)min(max(before[c], -32768), 32767);
        }
      }
    }
    const int m1 = m0 + kLanes;
    if (m1 < mend) {                                // (uniform)
      const int seg = mfirst + (m1 - mfirst) / R * R;
#pragma unroll
      for (int c = 0; c < 3; ++c) carry[c] = seg >= m1 ? 0 : (seg >= m0 ? all[c] - s_dc[c][seg - m0] : carry[c] + all[c]);
    }
    __syncthreads();                                // (the scans are read before the next chunk overwrites them)
  }
}

// an image's status and rounds from its tiles': the first tile that refused, the most rounds
__global__ __launch_bounds__(kBackThreads) void jpeg_verdict_camera_kernel(const CamArgs cam, const u8 *__restrict__ ws,
                                                                           u32 *__restrict__ rounds, int *__restrict__ status) {
  __shared__ u32 s_tile, s_rounds;
  const int tid = threadIdx.x, im = blockIdx.x;
  if (status[im] != 0) return;                      // (uniform)
  const CamImage &C = cam.img[im];
  const u32 *__restrict__ verdict = (const u32 *)(ws + C.tile_off);
  if (tid == 0) s_tile = 0xffffffffu, s_rounds = 0;
  __syncthreads();
  for (int t = tid; t < C.ntiles; t += kBackThreads) {
    if (verdict[2 * t]) atomicMin(&s_tile, (u32)t);
    atomicMax(&s_rounds, verdict[2 * t + 1]);
  }
  __syncthreads();
  if (tid == 0) {
    rounds[im] = s_rounds;
    if (s_tile != 0xffffffffu) status[im] = (int)verdict[2 * s_tile];
  }
}

// ---- 3. idct ----------------------------------------------------------------------------------------------------------------
// jidctint.c's butterfly on eight values; out[k] before the descale
__device__ __forceinline__ void idct_1d(const i64 *in, i64 *out) {
  i64 z1 = (in[2] + in[6]) * 4433;
  const i64 t2 = z1 - in[6] * 15137, t3 = z1 + in[2] * 6270;
  const i64 t0 = (in[0] + in[4]) * 8192, t1 = (in[0] - in[4]) * 8192;
  const i64 t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  i64 o0 = in[7], o1 = in[5], o2 = in[3], o3 = in[1];
  z1 = o0 + o3;
  i64 z2 = o1 + o2, z3 = o0 + o2, z4 = o1 + o3;
  const i64 z5 = (z3 + z4) * 9633;
  o0 *= 2446, o1 *= 16819, o2 *= 25172, o3 *= 12299;
  z1 *= -7373, z2 *= -20995;
  z3 = z3 * -16069 + z5, z4 = z4 * -3196 + z5;
  o0 += z1 + z3, o1 += z2 + z4, o2 += z2 + z3, o3 += z1 + z4;
  out[0] = t10 + o3, out[7] = t10 - o3;
  out[1] = t11 + o2, out[6] = t11 - o2;
  out[2] = t12 + o1, out[5] = t12 - o1;
  out[3] = t13 + o0, out[4] = t13 - o0;
}

// CAM: the camera entry points' instance, which also maps mode 3's slots (Y left, Y right, Cb, Cr)
template <bool CAM>
__global__ __launch_bounds__(kBackThreads) void jpeg_idct_kernel(const DecArgs args, const u8 *__restrict__ src,
                                                                 u8 *__restrict__ ws, const int *__restrict__ status) {
  __shared__ u8 s_q[3][64];
  const int tid = threadIdx.x, im = blockIdx.y;
  if (status[im] != 0) return;                      // (uniform)
  const DecImage &I = args.img[im];
  const Geometry g = geometry<CAM>(I.H, I.W, I.mode);
  if (tid < 192) s_q[tid >> 6][tid & 63] = src[I.tab_off + tid];
  __syncthreads();
  const short *__restrict__ coef = (const short *)(ws + I.coef_off);
  u8 *__restrict__ planes = ws + I.plane_off;
  const size_t luma_bytes = (size_t)g.pw0 * g.ph0, chroma_bytes = (size_t)g.pw1 * g.ph1;
  for (int blk = (int)blockIdx.x * kBackThreads + tid; blk < g.nblocks; blk += (int)gridDim.x * kBackThreads) {
    const int m = blk / g.bpm, slot = blk - m * g.bpm;
    const int my = m / g.mw, mx = m - my * g.mw;
    int comp, by, bx, pw;
    if (I.mode == KGDET_JPEG_DECODE_420 && slot < 4) {
      comp = 0, by = 2 * my + (slot >> 1), bx = 2 * mx + (slot & 1), pw = g.pw0;
    } else if (CAM && I.mode == KGDET_JPEG_DECODE_422) {
      comp = slot < 2 ? 0 : slot - 1, by = my, bx = slot < 2 ? 2 * mx + slot : mx, pw = slot < 2 ? g.pw0 : g.pw1;
    } else {
      comp = I.mode == KGDET_JPEG_DECODE_420 ? slot - 3 : slot;
      by = my, bx = mx, pw = comp ? g.pw1 : g.pw0;
    }
    u8 *__restrict__ plane = planes + (comp ? luma_bytes + (size_t)(comp - 1) * chroma_bytes : 0);
    short lv[64];
    const u32x4 *__restrict__ rows = (const u32x4 *)(coef + (size_t)blk * 64);
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const u32x4 v = rows[r];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        lv[8 * r + 2 * j] = (short)(v[j] & 0xffffu);
        lv[8 * r + 2 * j + 1] = (short)(v[j] >> 16);
      }
    }
    int mid[64];                                    // after pass 1: |.| < 2^30 for int16 levels and 8-bit table entries
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      i64 in[8], out[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) in[k] = (i64)((int)lv[8 * k + c] * (int)s_q[comp][8 * k + c]);
      idct_1d(in, out);
#pragma unroll
      for (int k = 0; k < 8; ++k) mid[8 * k + c] = (int)((out[k] + 1024) >> 11);
    }
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      i64 in[8], out[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) in[k] = mid[8 * r + k];
      idct_1d(in, out);
      u32x2 packed = {0u, 0u};
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const i64 v = ((out[k] + 131072) >> 18) + 128;
        const u32 byte = (u32)(v < 0 ? 0 : (v > 255 ? 255 : v));
        packed[k >> 2] |= byte << (8 * (k & 3));
      }
      *(u32x2 *)(plane + (size_t)(8 * by + r) * pw + 8 * bx) = packed;
    }
  }
}

// ---- 4. colour --------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int fancy(const u8 *__restrict__ c, int pw, int ch, int cw, int y, int x) {
  const int cy = y >> 1, cx = x >> 1;
  const int ny = (y & 1) ? min(cy + 1, ch - 1) : max(cy - 1, 0);
  const int nx = (x & 1) ? min(cx + 1, cw - 1) : max(cx - 1, 0);
  const u8 *r0 = c + (size_t)cy * pw, *r1 = c + (size_t)ny * pw;
  const int v = 3 * r0[cx] + r1[cx], vn = 3 * r0[nx] + r1[nx];
  return (3 * v + vn + ((x & 1) ? 7 : 8)) >> 4;
}

// libjpeg's h2v1 fancy upsampling of a chroma row of cw real samples; a row of up to two samples is replicated
__device__ __forceinline__ int fancy_h2v1(const u8 *__restrict__ row, int cw, int x) {
  const int cx = x >> 1;
  if (cw <= 2) return row[cx];
  const int nx = (x & 1) ? min(cx + 1, cw - 1) : max(cx - 1, 0);
  return (3 * row[cx] + row[nx] + ((x & 1) ? 2 : 1)) >> 2;
}

__device__ __forceinline__ u32 clamp255(int v) { return (u32)min(max(v, 0), 255); }

template <bool CAM>
__global__ __launch_bounds__(kBackThreads) void jpeg_colour_kernel(const DecArgs args, const u8 *__restrict__ ws,
                                                                   u8 *__restrict__ out, const int *__restrict__ status) {
  const int tid = threadIdx.x, im = blockIdx.y;
  if (status[im] != 0) return;                      // (uniform)
  const DecImage &I = args.img[im];
  const Geometry g = geometry<CAM>(I.H, I.W, I.mode);
  const u8 *__restrict__ py = ws + I.plane_off;
  const u8 *__restrict__ pcb = py + (size_t)g.pw0 * g.ph0, *__restrict__ pcr = pcb + (size_t)g.pw1 * g.ph1;
  u8 *__restrict__ dst = out + I.dst_off;
  const i64 npix = (i64)I.H * I.W, nbytes = 3 * npix;
  const int head = (int)((uintptr_t)dst & 15u);
  const i64 pieces = (head + nbytes + 15) / 16;
  const int ch = (I.H + 1) >> 1, cw = (I.W + 1) >> 1;
  for (i64 piece = (i64)blockIdx.x * kBackThreads + tid; piece < pieces; piece += (i64)gridDim.x * kBackThreads) {
    const i64 lo = 16 * piece - head;               // the piece is bytes [lo, lo + 16) of the picture; lo < 0 in the first one
    const i64 from = lo < 0 ? 0 : lo, to = lo + 16 < nbytes ? lo + 16 : nbytes;
    const i64 pix0 = from / 3;
    int y = (int)(pix0 / I.W), x = (int)(pix0 - (i64)y * I.W);
    u64 w0 = 0, w1 = 0;
#pragma unroll
    for (int j = 0; j < 7; ++j) {
      const i64 pix = pix0 + j;
      if (pix < npix && 3 * pix < to) {
        const int Y = py[(size_t)y * g.pw0 + x];
        u32 rgb[3];
        if (I.mode == KGDET_JPEG_DECODE_GREY) {
          rgb[0] = rgb[1] = rgb[2] = (u32)Y;
        } else {
          int cb, cr;
          if (I.mode == KGDET_JPEG_DECODE_420) {
            cb = fancy(pcb, g.pw1, ch, cw, y, x) - 128, cr = fancy(pcr, g.pw1, ch, cw, y, x) - 128;
          } else if (CAM && I.mode == KGDET_JPEG_DECODE_422) {
            cb = fancy_h2v1(pcb + (size_t)y * g.pw1, cw, x) - 128, cr = fancy_h2v1(pcr + (size_t)y * g.pw1, cw, x) - 128;
          } else {
            cb = pcb[(size_t)y * g.pw1 + x] - 128, cr = pcr[(size_t)y * g.pw1 + x] - 128;
          }
          rgb[0] = clamp255(Y + ((91881 * cr + 32768) >> 16));
          rgb[1] = clamp255(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
          rgb[2] = clamp255(Y + ((116130 * cb + 32768) >> 16));
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const int pos = (int)(3 * pix + c - lo);
          if (pos >= 0 && pos < 8) w0 |= (u64)rgb[c] << (8 * pos);
          if (pos >= 8 && pos < 16) w1 |= (u64)rgb[c] << (8 * (pos - 8));
        }
        if (++x == I.W) x = 0, ++y;
      }
    }
    if (lo >= 0 && lo + 16 <= nbytes) {
      u32x4 v = {(u32)w0, (u32)(w0 >> 32), (u32)w1, (u32)(w1 >> 32)};
      *(u32x4 *)(dst + lo) = v;
    } else {
      for (int pos = (int)(from - lo); pos < (int)(to - lo); ++pos)
        dst[lo + pos] = (u8)((pos < 8 ? w0 >> (8 * pos) : w1 >> (8 * (pos - 8))) & 255u);
    }
  }
}

// ---- host -------------------------------------------------------------------------------------------------------------------
bool disjoint(const void *a, uint64_t a_bytes, const void *b, uint64_t b_bytes) {
  return (uintptr_t)a + a_bytes <= (uintptr_t)b || (uintptr_t)b + b_bytes <= (uintptr_t)a;
}

struct Layout {
  size_t lens, coef, coef_bytes, total;
  int most_tiles;                                   // camera: of any image
};

// the jobs' sizes -> kernel arguments and the workspace's layout: the stream lengths, the streams, the coefficients of all
// images (one run, zeroed by one memset), the planes.  src_bytes / out_bytes < 0: offsets are not checked.  `cam` (the camera
// entry points): mode 3 is taken, `reserved` is the restart interval, and behind the planes follow per image the interval table
// (three uint32 [intervals + 1]) and the tiles' verdicts (two uint32 a tile).  The tile plan: as many whole intervals as hold
// a chunk's worth of the scan's bytes on average, 1 .. kLanes of them.
int plan(const char *what, const kgdet_jpeg_decode_job *jobs, int n, int64_t src_bytes, int64_t out_bytes, DecArgs &args, Layout &L,
         CamArgs *cam = nullptr) {
  args = {};
  args.n = n;
  L.most_tiles = 1;
  for (int i = 0; i < n; ++i) {
    const kgdet_jpeg_decode_job &J = jobs[i];
    KGDET_CHECK_SHAPE(J.H >= 1 && J.H <= kMaxSide && J.W >= 1 && J.W <= kMaxSide, "%s: image %d: %d x %d (sides 1 .. %d)", what, i,
                      J.H, J.W, kMaxSide);
    KGDET_CHECK_SHAPE(J.mode == KGDET_JPEG_DECODE_GREY || J.mode == KGDET_JPEG_DECODE_444 || J.mode == KGDET_JPEG_DECODE_420 ||
                          (cam && J.mode == KGDET_JPEG_DECODE_422),
                      "%s: image %d: mode %d", what, i, J.mode);
    KGDET_CHECK_SHAPE(!cam || (J.reserved >= 0 && J.reserved <= 65535), "%s: image %d: a restart interval of %d MCUs (0 .. 65535)",
                      what, i, J.reserved);
    KGDET_CHECK_SHAPE(J.scan_bytes >= 2 && J.scan_bytes <= kMaxScanBytes, "%s: image %d: a scan of %lld bytes (2 .. 2^28)", what, i,
                      (long long)J.scan_bytes);
    const int64_t pixels = 3ll * J.H * J.W;
    if (src_bytes >= 0) {
      KGDET_CHECK_SHAPE(J.scan_offset >= 0 && J.scan_offset <= src_bytes - J.scan_bytes,
                        "%s: image %d: the scan (offset %lld, %lld bytes) lies outside the source buffer", what, i,
                        (long long)J.scan_offset, (long long)J.scan_bytes);
      KGDET_CHECK_SHAPE(J.tables_offset >= 0 && J.tables_offset <= src_bytes - kTableBytes,
                        "%s: image %d: the table block (offset %lld) lies outside the source buffer", what, i,
                        (long long)J.tables_offset);
    }
    if (out_bytes >= 0) {
      KGDET_CHECK_SHAPE(J.dst_offset >= 0 && J.dst_offset <= out_bytes - pixels,
                        "%s: image %d: the picture (offset %lld, %lld bytes) lies outside the output buffer", what, i,
                        (long long)J.dst_offset, (long long)pixels);
      for (int j = 0; j < i; ++j)
        KGDET_CHECK_SHAPE(J.dst_offset + pixels <= jobs[j].dst_offset ||
                              jobs[j].dst_offset + 3ll * jobs[j].H * jobs[j].W <= J.dst_offset,
                          "%s: the pictures of images %d and %d overlap", what, j, i);
    }
    DecImage &I = args.img[i];
    I.scan_off = J.scan_offset, I.tab_off = J.tables_offset, I.dst_off = J.dst_offset;
    I.scan_bytes = (int)J.scan_bytes, I.H = J.H, I.W = J.W, I.mode = J.mode;
  }
  size_t at = align_up(8 * (size_t)kMaxImages, 16);      // the streams' lengths, the rounds of the fixpoint
  L.lens = 0;
  for (int i = 0; i < n; ++i) {
    args.img[i].stream_off = (i64)at;
    at += align_up((size_t)args.img[i].scan_bytes, 16) + kStreamPad;
  }
  L.coef = at;
  for (int i = 0; i < n; ++i) {
    args.img[i].coef_off = (i64)at;
    at += (size_t)geometry<true>(args.img[i].H, args.img[i].W, args.img[i].mode).nblocks * 128;
  }
  L.coef_bytes = at - L.coef;
  for (int i = 0; i < n; ++i) {
    const Geometry g = geometry<true>(args.img[i].H, args.img[i].W, args.img[i].mode);
    args.img[i].plane_off = (i64)at;
    at += (size_t)g.pw0 * g.ph0 + 2 * (size_t)g.pw1 * g.ph1;
  }
  if (cam) {
    *cam = {};
    for (int i = 0; i < n; ++i) {
      const Geometry g = geometry<true>(args.img[i].H, args.img[i].W, args.img[i].mode);
      CamImage &C = cam->img[i];
      const int nm = g.mw * g.mh;
      C.interval = jobs[i].reserved;
      C.nint = C.interval ? ceil_div(nm, C.interval) : 1;
      C.per_tile = (int)std::min<i64>(std::max<i64>((i64)C.nint * kTileBytes / args.img[i].scan_bytes, 1), kLanes);
      C.ntiles = ceil_div(C.nint, C.per_tile);
      L.most_tiles = std::max(L.most_tiles, C.ntiles);
      at = align_up(at, 16);
      C.table_off = (i64)at;
      at += align_up(12 * ((size_t)C.nint + 1), 16);
      C.tile_off = (i64)at;
      at += align_up(8 * (size_t)C.ntiles, 16);
    }
  }
  L.total = at;
  return KGDET_OK;
}

}  // namespace

}  // namespace kgdet

using namespace kgdet;

extern "C" {

size_t kgdet_jpeg_decode_workspace_bytes(const kgdet_jpeg_decode_job *jobs, int32_t n) {
  if (n < 0 || n > kMaxImages || (n > 0 && !jobs)) return 0;
  DecArgs args;
  Layout L;
  if (plan("jpeg_decode_workspace_bytes", jobs, n, -1, -1, args, L) != KGDET_OK) return 0;
  return L.total;
}

int kgdet_jpeg_decode(const uint8_t *src, int64_t src_bytes, const kgdet_jpeg_decode_job *jobs, int32_t n, void *workspace,
                      size_t workspace_bytes, uint8_t *out, int64_t out_bytes, int32_t *status, void *stream) {
  return kgdet_jpeg_decode_stages(src, src_bytes, jobs, n, workspace, workspace_bytes, out, out_bytes, status, stream, 4);
}

}  // extern "C"

namespace kgdet {
namespace {

// the body of kgdet_jpeg_decode_stages and kgdet_jpeg_decode_camera_stages
int run(bool camera, const uint8_t *src, int64_t src_bytes, const kgdet_jpeg_decode_job *jobs, int32_t n, void *workspace,
        size_t workspace_bytes, uint8_t *out, int64_t out_bytes, int32_t *status, void *stream, int32_t stages) {
  KGDET_CHECK_SHAPE(stages >= 1 && stages <= 4, "jpeg_decode: %d stages (1 .. 4)", stages);
  KGDET_CHECK_SHAPE(n >= 0 && n <= kMaxImages, "jpeg_decode: %d images in one call (0 .. %d)", n, kMaxImages);
  KGDET_CHECK_SHAPE(src_bytes >= 0 && out_bytes >= 0, "jpeg_decode: negative size");
  if (n == 0) return KGDET_OK;
  KGDET_CHECK_SHAPE(src && jobs && workspace && out && status, "jpeg_decode: null pointer");
  KGDET_CHECK_SHAPE(((uintptr_t)workspace & 15u) == 0, "jpeg_decode: the workspace is not 16-byte aligned");
  DecArgs args;
  CamArgs cam;
  Layout L;
  if (int rc = plan(camera ? "jpeg_decode_camera" : "jpeg_decode", jobs, n, src_bytes, out_bytes, args, L, camera ? &cam : nullptr))
    return rc;
  KGDET_CHECK_SHAPE(workspace_bytes >= L.total, "jpeg_decode: workspace of %zu bytes, %zu needed", workspace_bytes, L.total);
  KGDET_CHECK_SHAPE(disjoint(src, (uint64_t)src_bytes, workspace, workspace_bytes) &&
                        disjoint(src, (uint64_t)src_bytes, out, (uint64_t)out_bytes) &&
                        disjoint(src, (uint64_t)src_bytes, status, 4ull * n) &&
                        disjoint(workspace, workspace_bytes, out, (uint64_t)out_bytes) &&
                        disjoint(workspace, workspace_bytes, status, 4ull * n) && disjoint(out, (uint64_t)out_bytes, status, 4ull * n),
                    "jpeg_decode: source, workspace, output and status overlap");
  u8 *ws = (u8 *)workspace;
  u32 *lens = (u32 *)(ws + L.lens);
  hipStream_t s = (hipStream_t)stream;
  const int stop = stages;
  // a call cut short for timing: no image of it may pass for decoded (status bytes 0xFF: KGDET_JPEG_DECODE_STOPPED)
  auto stopped = [&]() -> int {
    KGDET_HIP_TRY(hipMemsetAsync(status, 0xFF, 4 * (size_t)n, s));
    return KGDET_OK;
  };
  if (camera) {
    hipLaunchKernelGGL(jpeg_unstuff_camera_kernel, dim3((unsigned)n), dim3(kLanes), 0, s, args, cam, (const u8 *)src, ws, lens,
                       (int *)status);
    KGDET_CHECK_LAUNCH("jpeg_unstuff_camera_kernel");
  } else {
    hipLaunchKernelGGL(jpeg_unstuff_kernel, dim3((unsigned)n), dim3(kLanes), 0, s, args, (const u8 *)src, ws, lens, (int *)status);
    KGDET_CHECK_LAUNCH("jpeg_unstuff_kernel");
  }
  if (stop <= 1) return stopped();
  KGDET_HIP_TRY(hipMemsetAsync(ws + L.coef, 0, L.coef_bytes, s));
  if (camera) {
    hipLaunchKernelGGL(jpeg_huffman_camera_kernel, dim3((unsigned)L.most_tiles, (unsigned)n), dim3(kLanes), 0, s, args, cam,
                       (const u8 *)src, ws, (const int *)status);
    KGDET_CHECK_LAUNCH("jpeg_huffman_camera_kernel");
    hipLaunchKernelGGL(jpeg_verdict_camera_kernel, dim3((unsigned)n), dim3(kBackThreads), 0, s, cam, (const u8 *)ws,
                       lens + kMaxImages, (int *)status);
    KGDET_CHECK_LAUNCH("jpeg_verdict_camera_kernel");
  } else {
    hipLaunchKernelGGL(jpeg_huffman_kernel, dim3((unsigned)n), dim3(kLanes), 0, s, args, (const u8 *)src, ws, (const u32 *)lens,
                       lens + kMaxImages, (int *)status);
    KGDET_CHECK_LAUNCH("jpeg_huffman_kernel");
  }
  if (stop <= 2) return stopped();
  int most_blocks = 1;
  i64 most_pieces = 1;
  for (int i = 0; i < n; ++i) {
    most_blocks = std::max(most_blocks, geometry<true>(args.img[i].H, args.img[i].W, args.img[i].mode).nblocks);
    most_pieces = std::max(most_pieces, (3ll * args.img[i].H * args.img[i].W + 30) / 16);
  }
  const int cap = std::max(1, 8 * cu_count() / n);
  const dim3 idct_grid((unsigned)std::min(ceil_div(most_blocks, kBackThreads), cap), (unsigned)n);
  if (camera)
    hipLaunchKernelGGL(jpeg_idct_kernel<true>, idct_grid, dim3(kBackThreads), 0, s, args, (const u8 *)src, ws, (const int *)status);
  else
    hipLaunchKernelGGL(jpeg_idct_kernel<false>, idct_grid, dim3(kBackThreads), 0, s, args, (const u8 *)src, ws, (const int *)status);
  KGDET_CHECK_LAUNCH("jpeg_idct_kernel");
  if (stop <= 3) return stopped();
  const dim3 colour_grid((unsigned)std::min<i64>((most_pieces + kBackThreads - 1) / kBackThreads, (i64)cap), (unsigned)n);
  if (camera)
    hipLaunchKernelGGL(jpeg_colour_kernel<true>, colour_grid, dim3(kBackThreads), 0, s, args, (const u8 *)ws, (u8 *)out,
                       (const int *)status);
  else
    hipLaunchKernelGGL(jpeg_colour_kernel<false>, colour_grid, dim3(kBackThreads), 0, s, args, (const u8 *)ws, (u8 *)out,
                       (const int *)status);
  KGDET_CHECK_LAUNCH("jpeg_colour_kernel");
  return KGDET_OK;
}

}  // namespace
}  // namespace kgdet

extern "C" {

int kgdet_jpeg_decode_stages(const uint8_t *src, int64_t src_bytes, const kgdet_jpeg_decode_job *jobs, int32_t n, void *workspace,
                             size_t workspace_bytes, uint8_t *out, int64_t out_bytes, int32_t *status, void *stream,
                             int32_t stages) {
  return run(false, src, src_bytes, jobs, n, workspace, workspace_bytes, out, out_bytes, status, stream, stages);
}

size_t kgdet_jpeg_decode_camera_workspace_bytes(const kgdet_jpeg_decode_job *jobs, int32_t n) {
  if (n < 0 || n > kMaxImages || (n > 0 && !jobs)) return 0;
  DecArgs args;
  CamArgs cam;
  Layout L;
  if (plan("jpeg_decode_camera_workspace_bytes", jobs, n, -1, -1, args, L, &cam) != KGDET_OK) return 0;
  return L.total;
}

int kgdet_jpeg_decode_camera(const uint8_t *src, int64_t src_bytes, const kgdet_jpeg_decode_job *jobs, int32_t n, void *workspace,
                             size_t workspace_bytes, uint8_t *out, int64_t out_bytes, int32_t *status, void *stream) {
  return run(true, src, src_bytes, jobs, n, workspace, workspace_bytes, out, out_bytes, status, stream, 4);
}

int kgdet_jpeg_decode_camera_stages(const uint8_t *src, int64_t src_bytes, const kgdet_jpeg_decode_job *jobs, int32_t n,
                                    void *workspace, size_t workspace_bytes, uint8_t *out, int64_t out_bytes, int32_t *status,
                                    void *stream, int32_t stages) {
  return run(true, src, src_bytes, jobs, n, workspace, workspace_bytes, out, out_bytes, status, stream, stages);
}

}  // extern "C"
