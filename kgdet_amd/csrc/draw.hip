// Detections and landmarks drawn on images (kgdet_amd/visualize.py: DeviceDrawer) for gfx950: kgdet_draw_detections.
// The picture is DEFINED by visualize.draw_restatement (numpy); this kernel is held to it bit for bit.  In short: a row
// [box 4, score, label, count, K x (x, y, v)] is drawn when score > score_thr, its label is an integer in [0, L) and its box is
// finite; coordinates are rint (half to even) of the float32 value clamped to [-8192, 16383]; its layers, bottom to top, are
//   0 box      x0 <= x <= x1, y0 <= y <= y1 and (x < x0 + t or x > x1 - t or y < y0 + t or y > y1 - t)
//   1 contour  the capsule of half-width line_width / 2 around consecutive visible landmarks of the category's range
//   2 landmark the disc (x - cx)^2 + (y - cy)^2 <= radius^2
//   3 label    "name|d.dd" in 5 x 7 glyphs, cells of 6s x 9s pixels, on a box of the class colour above the box's corner
// and a pixel shows the covering primitive with the greatest key 4 r + layer, else its source value.  No blending: the order
// of evaluation does not matter, so the lists below are in no particular order.
//
// Integer ranges of the capsule test (doubled coordinates: X2 = 2 X, so the half-width line_width / 2 is the integer
// line_width): coordinates lie in [-8192, 16383], pixels in [0, 8191], so every component of d = Q2 - P2 is at most 2 * 24575
// and of v = X2 - P2 at most 2 * 16383 + 1 in magnitude.  cross(v, d) is four times twice the area of the triangle P, Q, X,
// whose corners lie in a square of side 24575: |cross| <= 4 * 24575^2 < 2^31.2, its square < 2^62.4; d.d <= 8 * 24575^2 <
// 2^32.2 and R2 = line_width^2 <= 256, so R2 * d.d < 2^40.2; v.d and |v|^2 stay below 2^33.  All of it fits int64.
//
// Shape: ONE WAVE per tile of 64 x 16 pixels (a workgroup of 64 threads: lane = column, 16 pixels per lane, their best keys
// in 16 registers), all control flow wave-uniform, so the only synchronisation is the wave's own barrier around LDS phases.
//  1. The wave walks the image's `count` rows.  The row's head is read by uniform loads; box and label are tested against the
//     tile with scalar arithmetic (a tile wholly inside a box's interior keeps nothing of it).  The landmarks of the
//     category's range are read 64 at a time, one per lane; discs and capsules whose bounding boxes touch the tile are kept:
//     a ballot and a prefix count of the lanes below give every kept primitive its place in the LDS list (no atomics).
//  2. The list holds 256 records of 5 ints (key, four parameters).  When it cannot take another 130 it is evaluated and
//     emptied: a record is read by all lanes at once (an LDS broadcast), its bounding box cut to the tile with scalar
//     arithmetic, and the tile rows it reaches are visited with the lane's column test hoisted out of the row loop.
//  3. The tile's bytes are assembled in LDS: the source bytes of each tile row are copied in (lane = byte, coalesced), covered
//     pixels overwrite theirs, and the row leaves as 16-byte stores at the destination's own 16-byte alignment -- the LDS
//     image of a row starts (destination address mod 16) bytes into its 208-byte slot -- with byte stores for the unaligned
//     head and tail (3 W is rarely a multiple of 4, so every row has its own alignment).
// LDS per workgroup: 5 120 (list) + 3 328 (16 rows x 208 bytes) = 8 448 bytes.  No atomics, no global scratch, no read-back;
// plain C++ and vector stores only.  The source is never written; source and destination buffers may not overlap.
#include "common.h"

#pragma clang fp contract(off)

namespace kgdet {

namespace {

constexpr int kWave = 64;
constexpr int kTileW = 64, kTileH = 16;
constexpr int kCap = 256, kRec = 5;                 // records of the list, ints of a record
constexpr int kSlot = 208;                          // bytes of a tile row's LDS image: 15 (shift) + 192, rounded up to 16
constexpr int kChunks = kSlot / 16;
constexpr int kMaxImages = KGDET_DRAW_MAX_IMAGES;
constexpr int kCoordMin = -8192, kCoordMax = 16383, kMaxSide = 8192;
constexpr int kMaxName = 255;

typedef unsigned long long u64;
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

struct DrawImage {
  long long src_off, dst_off;
  int H, W, block, tiles_x;
};

struct DrawArgs {
  DrawImage img[kMaxImages];
  int tile0[kMaxImages + 1];                        // first (global) tile of each image
  int n;
};

struct DrawStyle {
  float score_thr;
  int t, radius, contour, lw, s, kpt;               // kpt: 0xRRGGBB or -1 (the class colour)
  int L, M, W7, K, name_total;
};

struct Tile {
  int x0, y0, x1, y1;                               // inclusive, cut to the image
};

__device__ __forceinline__ int coord(float v) { return (int)fminf(fmaxf(rintf(v), (float)kCoordMin), (float)kCoordMax); }
__device__ __forceinline__ bool finite(float v) { return fabsf(v) < __builtin_inff(); }
__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }

// the list's records against the lane's column x of the tile: best[i] = the greatest (key << 1 | ink) covering (x, t.y0 + i)
__device__ __forceinline__ void evaluate(const int *s_rec, int n_list, const Tile &t, int x, const DrawStyle &st,
                                         const unsigned char *__restrict__ names, const unsigned char *__restrict__ glyphs,
                                         int (&best)[kTileH]) {
  __syncthreads();
  for (int i = 0; i < n_list; ++i) {
    const int key = uni(s_rec[i * kRec]);
    const int a = uni(s_rec[i * kRec + 1]), b = uni(s_rec[i * kRec + 2]), c = uni(s_rec[i * kRec + 3]),
              d = uni(s_rec[i * kRec + 4]);
    const int key2 = key << 1;
    switch (key & 3) {
      case 0: {                                     // box a, b .. c, d
        const int ylo = max(b, t.y0), yhi = min(d, t.y1);
        const bool inx = x >= a && x <= c && x <= t.x1;
        const bool edge = x < a + st.t || x > c - st.t;
#pragma unroll
        for (int j = 0; j < kTileH; ++j) {
          const int y = t.y0 + j;
          if (y < ylo || y > yhi) continue;
          if (inx && (edge || y < b + st.t || y > d - st.t)) best[j] = max(best[j], key2);
        }
        break;
      }
      case 1: {                                     // capsule P (a, b) -> Q (c, d), doubled coordinates
        const int pad = (st.lw + 1) >> 1;
        const int xlo = max(min(a, c) - pad, t.x0), xhi = min(max(a, c) + pad, t.x1);
        const int ylo = max(min(b, d) - pad, t.y0), yhi = min(max(b, d) + pad, t.y1);
        const bool inx = x >= xlo && x <= xhi;
        const long long dx = 2 * (c - a), dy = 2 * (d - b), R2 = st.lw * st.lw;
        const long long dd = dx * dx + dy * dy;
        const long long vx = 2 * x - 2 * a, wx = 2 * x - 2 * c;
#pragma unroll
        for (int j = 0; j < kTileH; ++j) {
          const int y = t.y0 + j;
          if (y < ylo || y > yhi) continue;
          if (inx) {
            const long long vy = 2 * y - 2 * b, wy = 2 * y - 2 * d;
            const long long dot = vx * dx + vy * dy;
            bool in;
            if (dot <= 0) {
              in = vx * vx + vy * vy <= R2;
            } else if (dot >= dd) {
              in = wx * wx + wy * wy <= R2;
            } else {
              const long long cr = vx * dy - vy * dx;
              const u64 ac = (u64)(cr < 0 ? -cr : cr);
              in = ac * ac <= (u64)(R2 * dd);
            }
            if (in) best[j] = max(best[j], key2);
          }
        }
        break;
      }
      case 2: {                                     // disc around (a, b)
        const int ylo = max(b - st.radius, t.y0), yhi = min(b + st.radius, t.y1);
        const int dx = x - a, r2 = st.radius * st.radius;
        const bool inx = dx >= -st.radius && dx <= st.radius && x <= t.x1;
        const int dx2 = inx ? dx * dx : 0;
#pragma unroll
        for (int j = 0; j < kTileH; ++j) {
          const int y = t.y0 + j;
          if (y < ylo || y > yhi) continue;
          const int dy = y - b;
          if (inx && dx2 + dy * dy <= r2) best[j] = max(best[j], key2);
        }
        break;
      }
      default: {                                    // label: left a, top b, c = name bytes | q << 16, d = the name's offset
        const int nlen = c & 0xffff, q = c >> 16, s = st.s;
        const int wd = (6 * (nlen + 5) + 1) * s, ht = 9 * s;
        const int ylo = max(b, t.y0), yhi = min(b + ht - 1, t.y1);
        const int lx = x - a;
        const bool inx = lx >= 0 && lx < wd && x <= t.x1;
        u64 m7 = 0;                                 // the glyph's seven row masks, row j in bits 8j .. 8j + 4
        int col = 5;
        if (inx) {
          const int g1 = lx / s - 1;
          if (g1 >= 0) {
            const int gi = g1 / 6;
            col = g1 - 6 * gi;
            if (col < 5) {
              int ch;
              if (gi < nlen) {
                ch = names[d + gi];
              } else if (gi == nlen) {
                ch = '|';
              } else {
                const int k = gi - nlen - 1;
                ch = k == 0 ? '0' + q / 100 : k == 1 ? '.' : k == 2 ? '0' + (q / 10) % 10 : '0' + q % 10;
              }
              for (int j = 0; j < 7; ++j) m7 |= (u64)glyphs[ch * 7 + j] << (8 * j);
            }
          }
        }
#pragma unroll
        for (int j = 0; j < kTileH; ++j) {
          const int y = t.y0 + j;
          if (y < ylo || y > yhi) continue;
          if (inx) {
            const int gy = (y - b) / s;
            const int ink = (col < 5 && gy >= 1 && gy <= 7) ? (int)((m7 >> (8 * (gy - 1) + 4 - col)) & 1ull) : 0;
            best[j] = max(best[j], key2 | ink);
          }
        }
        break;
      }
    }
  }
  __syncthreads();
}

__global__ __launch_bounds__(kWave) void draw_detections_kernel(
    const DrawArgs args, const DrawStyle st, const unsigned char *__restrict__ src, unsigned char *__restrict__ dst,
    const float *__restrict__ rows, const unsigned char *__restrict__ colors, const unsigned char *__restrict__ names,
    const int *__restrict__ name_off, const int *__restrict__ ranges, const unsigned char *__restrict__ glyphs) {
  __shared__ int s_rec[kCap * kRec];
  __shared__ __attribute__((aligned(16))) unsigned char s_out[kTileH * kSlot];
  const int lane = threadIdx.x;
  int im = 0;
  while ((int)blockIdx.x >= args.tile0[im + 1]) ++im;
  const DrawImage &I = args.img[im];
  const int H = I.H, W = I.W;
  const int tile = (int)blockIdx.x - args.tile0[im];
  const int ty = tile / I.tiles_x, tx = tile - ty * I.tiles_x;
  Tile t;
  t.x0 = tx * kTileW;
  t.y0 = ty * kTileH;
  t.x1 = min(t.x0 + kTileW - 1, W - 1);
  t.y1 = min(t.y0 + kTileH - 1, H - 1);
  const int x = t.x0 + lane;
  const float *__restrict__ blk = rows + (long long)I.block * st.M * st.W7;
  const float cf = blk[6];
  const int count = !(cf >= 0.0f) ? 0 : (cf >= (float)st.M ? st.M : (int)cf);

  int best[kTileH];
#pragma unroll
  for (int j = 0; j < kTileH; ++j) best[j] = -1;
  int n_list = 0;

  for (int r = 0; r < count; ++r) {
    const float *__restrict__ row = blk + (long long)r * st.W7;
    const float f0 = row[0], f1 = row[1], f2 = row[2], f3 = row[3], score = row[4], lf = row[5];
    if (!(score > st.score_thr && lf == floorf(lf) && lf >= 0.0f && lf < (float)st.L && finite(f0) && finite(f1) && finite(f2) &&
          finite(f3)))
      continue;
    const int lab = (int)lf;
    const int bx0 = coord(f0), by0 = coord(f1), bx1 = coord(f2), by1 = coord(f3);
    if (n_list + 2 > kCap) {
      evaluate(s_rec, n_list, t, x, st, names, glyphs, best);
      n_list = 0;
    }
    // 0: the box, unless it is empty, misses the tile or holds the tile in its interior
    if (bx1 >= bx0 && by1 >= by0 && bx0 <= t.x1 && bx1 >= t.x0 && by0 <= t.y1 && by1 >= t.y0 &&
        !(t.x0 >= bx0 + st.t && t.x1 <= bx1 - st.t && t.y0 >= by0 + st.t && t.y1 <= by1 - st.t)) {
      if (lane == 0) {
        int *rec = s_rec + n_list * kRec;
        rec[0] = 4 * r;
        rec[1] = bx0, rec[2] = by0, rec[3] = bx1, rec[4] = by1;
      }
      n_list += 1;
    }
    // 3: the label
    {
      int noff = name_off[lab], nlen = name_off[lab + 1] - noff;
      noff = min(max(noff, 0), st.name_total);
      nlen = min(min(max(nlen, 0), kMaxName), st.name_total - noff);
      const int wd = (6 * (nlen + 5) + 1) * st.s, ht = 9 * st.s;
      int top = by0 - ht;
      if (top < 0) top = by0;
      if (bx0 <= t.x1 && bx0 + wd - 1 >= t.x0 && top <= t.y1 && top + ht - 1 >= t.y0) {
        const double p = fmin(fmax(rint((double)score * 100.0), 0.0), 999.0);
        if (lane == 0) {
          int *rec = s_rec + n_list * kRec;
          rec[0] = 4 * r + 3;
          rec[1] = bx0, rec[2] = top, rec[3] = nlen | ((int)p << 16), rec[4] = noff;
        }
        n_list += 1;
      }
    }
    // 2 and 1: the landmarks of the category's range, 64 at a time, and the segments between consecutive ones
    int ka = 0, kb = st.K;
    if (ranges != nullptr) {
      ka = min(max(ranges[2 * lab], 0), st.K);
      kb = min(max(ranges[2 * lab + 1], 0), st.K);
    }
    const int rad = st.radius, pad = (st.lw + 1) >> 1;
    for (int k0 = ka; k0 < kb; k0 += kWave) {
      const int k = k0 + lane;
      bool ok = false, ok2 = false;
      int cx = 0, cy = 0, qx = 0, qy = 0;
      if (k < kb) {
        const float px = row[7 + 3 * k], py = row[8 + 3 * k], pv = row[9 + 3 * k];
        ok = pv > 0.0f && finite(px) && finite(py);
        cx = coord(px), cy = coord(py);
        if (st.contour && k + 1 < kb) {
          const float nx = row[10 + 3 * k], ny = row[11 + 3 * k], nv = row[12 + 3 * k];
          ok2 = ok && nv > 0.0f && finite(nx) && finite(ny);
          qx = coord(nx), qy = coord(ny);
        }
      }
      const bool disc = ok && cx + rad >= t.x0 && cx - rad <= t.x1 && cy + rad >= t.y0 && cy - rad <= t.y1;
      const bool seg = ok2 && max(cx, qx) + pad >= t.x0 && min(cx, qx) - pad <= t.x1 && max(cy, qy) + pad >= t.y0 &&
                       min(cy, qy) - pad <= t.y1;
      if (n_list + 2 * kWave > kCap) {
        evaluate(s_rec, n_list, t, x, st, names, glyphs, best);
        n_list = 0;
      }
      const u64 below = (1ull << lane) - 1ull;
      const u64 m_disc = __ballot(disc);
      if (disc) {
        int *rec = s_rec + (n_list + __popcll(m_disc & below)) * kRec;
        rec[0] = 4 * r + 2;
        rec[1] = cx, rec[2] = cy, rec[3] = 0, rec[4] = 0;
      }
      n_list += __popcll(m_disc);
      const u64 m_seg = __ballot(seg);
      if (seg) {
        int *rec = s_rec + (n_list + __popcll(m_seg & below)) * kRec;
        rec[0] = 4 * r + 1;
        rec[1] = cx, rec[2] = cy, rec[3] = qx, rec[4] = qy;
      }
      n_list += __popcll(m_seg);
    }
  }
  evaluate(s_rec, n_list, t, x, st, names, glyphs, best);

  // the tile's bytes: source, then the covered pixels over it, then out
  const int nbytes = 3 * (t.x1 - t.x0 + 1);
  const unsigned char *__restrict__ s_img = src + I.src_off;
  unsigned char *__restrict__ d_img = dst + I.dst_off;
#pragma unroll
  for (int j = 0; j < kTileH; ++j) {
    const int y = t.y0 + j;
    if (y > t.y1) continue;
    const long long at = ((long long)y * W + t.x0) * 3;
    const int shift = (int)((uintptr_t)(d_img + at) & 15u);
    unsigned char *slot = s_out + j * kSlot + shift;
    for (int b = lane; b < nbytes; b += kWave) slot[b] = s_img[at + b];
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < kTileH; ++j) {
    const int y = t.y0 + j;
    if (y > t.y1) continue;
    if (best[j] >= 0 && x <= t.x1) {
      const int key = best[j] >> 1, layer = key & 3;
      const int lab = (int)blk[(long long)(key >> 2) * st.W7 + 5];
      int R = colors[3 * lab], G = colors[3 * lab + 1], B = colors[3 * lab + 2];
      if (layer == 2 && st.kpt >= 0) {
        R = (st.kpt >> 16) & 255, G = (st.kpt >> 8) & 255, B = st.kpt & 255;
      } else if (layer == 3 && (best[j] & 1)) {
        R = G = B = (299 * R + 587 * G + 114 * B >= 128000) ? 0 : 255;
      }
      const long long at = ((long long)y * W + t.x0) * 3;
      const int shift = (int)((uintptr_t)(d_img + at) & 15u);
      unsigned char *px = s_out + j * kSlot + shift + 3 * lane;
      px[0] = (unsigned char)R, px[1] = (unsigned char)G, px[2] = (unsigned char)B;
    }
  }
  __syncthreads();
  // chunk c of row j is s_out[j][16c, 16c + 16) and the destination's aligned 16 bytes at (row address - shift) + 16c
  for (int idx = lane; idx < kTileH * kChunks; idx += kWave) {
    const int j = idx / kChunks, c = idx - j * kChunks;
    const int y = t.y0 + j;
    if (y > t.y1) continue;
    unsigned char *g_row = d_img + ((long long)y * W + t.x0) * 3;
    const int shift = (int)((uintptr_t)g_row & 15u);
    const int end = shift + nbytes, lo = 16 * c;
    if (lo >= end || lo + 16 <= shift) continue;
    const unsigned char *s_row = s_out + j * kSlot;
    unsigned char *g_base = g_row - shift;
    if (lo >= shift && lo + 16 <= end) {
      *reinterpret_cast<u32x4 *>(g_base + lo) = *reinterpret_cast<const u32x4 *>(s_row + lo);
    } else {
      const int b0 = max(lo, shift), b1 = min(lo + 16, end);
      for (int b = b0; b < b1; ++b) g_base[b] = s_row[b];
    }
  }
}

}  // namespace

}  // namespace kgdet

using namespace kgdet;

extern "C" {

int kgdet_draw_detections(const uint8_t *src, int64_t src_bytes, uint8_t *dst, int64_t dst_bytes, const int64_t *table,
                          const int32_t *row_block, int32_t n, const float *rows, int64_t N, int32_t M, int32_t W7,
                          const uint8_t *colors, int32_t L, const uint8_t *name_bytes, const int32_t *name_off,
                          int32_t name_total, const int32_t *ranges, const uint8_t *glyphs, float score_thr, int32_t thickness,
                          int32_t radius, int32_t contour, int32_t line_width, int32_t font_scale, int32_t kpt_color,
                          void *stream) {
  KGDET_CHECK_SHAPE(n >= 0 && n <= kMaxImages, "draw_detections: %d images in one launch (0 .. %d)", n, kMaxImages);
  KGDET_CHECK_SHAPE(M >= 1 && M <= KGDET_DRAW_MAX_ROWS, "draw_detections: %d rows per image (1 .. %d)", M, KGDET_DRAW_MAX_ROWS);
  KGDET_CHECK_SHAPE(W7 >= 10 && (W7 - 7) % 3 == 0 && (W7 - 7) / 3 <= KGDET_DRAW_MAX_K,
                    "draw_detections: rows of %d floats (7 + 3K, K = 1 .. %d)", W7, KGDET_DRAW_MAX_K);
  KGDET_CHECK_SHAPE(L >= 1 && L <= KGDET_DRAW_MAX_LABELS, "draw_detections: %d labels (1 .. %d)", L, KGDET_DRAW_MAX_LABELS);
  KGDET_CHECK_SHAPE(N >= 0 && N < (1ll << 31), "draw_detections: %lld row blocks (0 .. 2^31 - 1)", (long long)N);
  KGDET_CHECK_SHAPE(thickness >= 1 && thickness <= 64 && radius >= 1 && radius <= 64,
                    "draw_detections: thickness %d, radius %d (1 .. 64)", thickness, radius);
  KGDET_CHECK_SHAPE(line_width >= 1 && line_width <= 16, "draw_detections: line_width %d (1 .. 16)", line_width);
  KGDET_CHECK_SHAPE(font_scale >= 1 && font_scale <= 8, "draw_detections: font_scale %d (1 .. 8)", font_scale);
  KGDET_CHECK_SHAPE(kpt_color >= -1 && kpt_color <= 0xffffff, "draw_detections: kpt_color %d (0xRRGGBB or -1)", kpt_color);
  KGDET_CHECK_SHAPE(src_bytes >= 0 && dst_bytes >= 0 && name_total >= 0, "draw_detections: negative size");
  if (n == 0) return KGDET_OK;
  KGDET_CHECK_SHAPE(src && dst && table && row_block && rows && colors && name_bytes && name_off && glyphs,
                    "draw_detections: null pointer");
  KGDET_CHECK_SHAPE((uintptr_t)src + (uint64_t)src_bytes <= (uintptr_t)dst || (uintptr_t)dst + (uint64_t)dst_bytes <= (uintptr_t)src,
                    "draw_detections: source and destination buffers overlap (the call is out of place)");
  DrawArgs args = {};
  long long tiles = 0;
  for (int i = 0; i < n; ++i) {
    const int64_t so = table[4 * i], dof = table[4 * i + 1], H = table[4 * i + 2], W = table[4 * i + 3];
    KGDET_CHECK_SHAPE(H >= 1 && H <= kMaxSide && W >= 1 && W <= kMaxSide, "draw_detections: image %d: %lld x %lld (sides 1 .. %d)",
                      i, (long long)H, (long long)W, kMaxSide);
    const int64_t size = 3 * H * W;
    KGDET_CHECK_SHAPE(so >= 0 && so <= src_bytes - size && dof >= 0 && dof <= dst_bytes - size,
                      "draw_detections: image %d: offsets %lld / %lld with %lld bytes outside the buffers", i, (long long)so,
                      (long long)dof, (long long)size);
    KGDET_CHECK_SHAPE(row_block[i] >= 0 && row_block[i] < N, "draw_detections: image %d: row block %d of %lld", i, row_block[i],
                      (long long)N);
    DrawImage &I = args.img[i];
    I.src_off = so, I.dst_off = dof;
    I.H = (int)H, I.W = (int)W, I.block = row_block[i];
    I.tiles_x = ceil_div((int)W, kTileW);
    args.tile0[i] = (int)tiles;
    tiles += (long long)I.tiles_x * ceil_div((int)H, kTileH);
  }
  for (int i = n; i <= kMaxImages; ++i) args.tile0[i] = (int)tiles;
  args.n = n;
  DrawStyle st;
  st.score_thr = score_thr;
  st.t = thickness, st.radius = radius, st.contour = contour != 0, st.lw = line_width, st.s = font_scale, st.kpt = kpt_color;
  st.L = L, st.M = M, st.W7 = W7, st.K = (W7 - 7) / 3, st.name_total = name_total;
  hipLaunchKernelGGL(draw_detections_kernel, dim3((unsigned)tiles), dim3(kWave), 0, (hipStream_t)stream, args, st,
                     (const unsigned char *)src, (unsigned char *)dst, rows, (const unsigned char *)colors,
                     (const unsigned char *)name_bytes, (const int *)name_off, (const int *)ranges, (const unsigned char *)glyphs);
  KGDET_CHECK_LAUNCH("draw_detections_kernel");
  return KGDET_OK;
}

}  // extern "C"
