// COCO-style evaluation on the device (kgdet_amd/evaluation_device.py) for gfx950: the [D, G] similarity matrix of every
// (image, category) cell -- box IoU or OKS over the 294 DeepFashion2 landmarks -- and the greedy score-ordered matching of
// evaluation.CocoEvaluator._match for every (area range, IoU threshold), each as ONE launch over the dataset's cell table.
//
// Cell table: int32 [C, 4] = (first detection, number of detections, first ground truth, number of ground truths) into the
// packed detection / ground-truth arrays, int64 [C] = offset of the cell's row-major [D, G] block in `sim`.  Detections of a
// cell are already in descending-score order (the host sorts them once).  A cell whose ranges leave the arrays is skipped.
//
// Everything is float64 and contraction is off: box IoU is numpy's value bit for bit, the OKS exponent argument too; `exp`
// is the device library's and the 294 terms are added lane-strided, then across the wave by a fixed xor butterfly, so two
// runs give the same bits.
#include "common.h"

#pragma clang fp contract(off)

namespace kgdet {

namespace {

constexpr int kSimThreads = 256;
constexpr int kWave = 64;

__device__ __forceinline__ bool cell_ok(const int *c, long long ND, long long NG) {
  return c[0] >= 0 && c[1] >= 0 && c[2] >= 0 && c[3] >= 0 && (long long)c[0] + c[1] <= ND && (long long)c[2] + c[3] <= NG;
}

// evaluation.box_iou_xywh, operation by operation
__global__ __launch_bounds__(kSimThreads) void coco_iou_kernel(const int *__restrict__ cells,
                                                               const long long *__restrict__ sim_off, long long ND,
                                                               long long NG, long long sim_size,
                                                               const double *__restrict__ d_box,
                                                               const double *__restrict__ g_box,
                                                               const int *__restrict__ g_crowd, double *__restrict__ sim) {
  const int *c = cells + 4ll * blockIdx.x;
  if (!cell_ok(c, ND, NG)) return;
  const int D = c[1], G = c[3];
  const long long n = (long long)D * G, off = sim_off[blockIdx.x];
  if (n == 0 || off < 0 || off + n > sim_size) return;
  for (long long p = threadIdx.x; p < n; p += kSimThreads) {
    const int di = (int)(p / G), gi = (int)(p - (long long)di * G);
    const double *d = d_box + 4ll * (c[0] + di), *g = g_box + 4ll * (c[2] + gi);
    const double iw = fmin(d[0] + d[2], g[0] + g[2]) - fmax(d[0], g[0]);
    const double ih = fmin(d[1] + d[3], g[1] + g[3]) - fmax(d[1], g[1]);
    const double inter = (iw > 0.0 && ih > 0.0) ? iw * ih : 0.0;
    const double da = d[2] * d[3], ga = g[2] * g[3];
    const double uni = g_crowd[c[2] + gi] ? da : (da + ga) - inter;
    sim[off + p] = inter > 0.0 ? inter / uni : 0.0;
  }
}

// evaluation.oks: one wave per (detection, ground truth) pair, the landmarks across its lanes
__global__ __launch_bounds__(kSimThreads) void coco_oks_kernel(const int *__restrict__ cells,
                                                               const long long *__restrict__ sim_off, long long ND,
                                                               long long NG, long long sim_size,
                                                               const double *__restrict__ d_kxy,    // [ND, K, 2]
                                                               const double *__restrict__ g_kpt,    // [NG, K, 3]
                                                               const double *__restrict__ g_box,
                                                               const double *__restrict__ g_area,
                                                               const int *__restrict__ g_nvis,
                                                               const double *__restrict__ var, int K,
                                                               double *__restrict__ sim) {
  const int *c = cells + 4ll * blockIdx.x;
  if (!cell_ok(c, ND, NG)) return;
  const int D = c[1], G = c[3];
  const long long n = (long long)D * G, off = sim_off[blockIdx.x];
  if (n == 0 || off < 0 || off + n > sim_size) return;
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  for (long long p = wave; p < n; p += kSimThreads / kWave) {      // (p is wave-uniform: the shuffles below see all 64 lanes)
    const int di = (int)(p / G), gi = (int)(p - (long long)di * G);
    const long long dd = c[0] + di, gg = c[2] + gi;
    const double *dk = d_kxy + dd * K * 2, *gk = g_kpt + gg * K * 3;
    const int nvis = g_nvis[gg];
    const double area = g_area[gg] + 2.220446049250313e-16;          // np.spacing(1)
    double acc = 0.0;
    if (nvis > 0) {
      for (int k = lane; k < K; k += kWave) {
        if (!(gk[3 * k + 2] > 0.0)) continue;
        const double dx = dk[2 * k] - gk[3 * k], dy = dk[2 * k + 1] - gk[3 * k + 1];
        const double e = (dx * dx + dy * dy) / var[k] / area / 2.0;
        acc += exp(-e);
      }
    } else {      // no labelled landmark: distance to the doubled ground-truth box
      const double *b = g_box + 4 * gg;
      const double x0 = b[0] - b[2], x1 = b[0] + b[2] * 2.0, y0 = b[1] - b[3], y1 = b[1] + b[3] * 2.0;
      for (int k = lane; k < K; k += kWave) {
        const double xd = dk[2 * k], yd = dk[2 * k + 1];
        const double dx = fmax(0.0, x0 - xd) + fmax(0.0, xd - x1);
        const double dy = fmax(0.0, y0 - yd) + fmax(0.0, yd - y1);
        const double e = (dx * dx + dy * dy) / var[k] / area / 2.0;
        acc += exp(-e);
      }
    }
    for (int m = kWave / 2; m >= 1; m >>= 1) acc += __shfl_xor(acc, m, kWave);
    if (lane == 0) sim[off + p] = acc / (double)(nvis > 0 ? nvis : K);
  }
}

// CocoEvaluator._match: one wave per cell, lane = (area range a, threshold t).  Instead of sorting the ground truths
// regular-first, a detection sweeps the regular ones in order and then -- only when none of them matched, which is the
// reference's `break` -- the ignored ones in order: the same candidates in the same sequence.
__global__ __launch_bounds__(kWave) void coco_match_kernel(const int *__restrict__ cells,
                                                           const long long *__restrict__ sim_off, long long ND,
                                                           long long NG, long long sim_size,
                                                           const double *__restrict__ sim,
                                                           const double *__restrict__ d_area,
                                                           const double *__restrict__ g_area,
                                                           const unsigned char *__restrict__ g_ignore,
                                                           const int *__restrict__ g_crowd,
                                                           const double *__restrict__ area_rng, int A,
                                                           const double *__restrict__ best0, int T,
                                                           int *__restrict__ d_match,               // [ND, A, T]
                                                           unsigned char *__restrict__ d_ignore,    // [ND, A, T]
                                                           unsigned char *__restrict__ g_ignore_out,  // [NG, A]
                                                           unsigned char *__restrict__ g_taken) {   // [NG, A, T] scratch
  const int *c = cells + 4ll * blockIdx.x;
  if (!cell_ok(c, ND, NG)) return;
  const int lane = threadIdx.x, AT = A * T;
  if (lane >= AT) return;
  const int D = c[1], G = c[3], a = lane / T, t = lane - a * T;
  const long long d0 = c[0], g0 = c[2], off = sim_off[blockIdx.x];
  const bool have_sim = D > 0 && G > 0 && off >= 0 && off + (long long)D * G <= sim_size;
  const double lo = area_rng[2 * a], hi = area_rng[2 * a + 1], start = best0[t];
  for (int gi = 0; gi < G; ++gi) {
    const double ga = g_area[g0 + gi];
    const unsigned char ign = (g_ignore[g0 + gi] || ga < lo || ga > hi) ? 1 : 0;
    if (t == 0) g_ignore_out[(g0 + gi) * A + a] = ign;
    g_taken[(g0 + gi) * AT + lane] = ign;          // bit 0: ignored for this area range, bit 1: matched at (a, t)
  }
  for (int di = 0; di < D; ++di) {
    double best = start;
    int m = -1;
    if (have_sim) {
      const double *row = sim + off + (long long)di * G;
      for (int pass = 0; pass < 2; ++pass) {
        if (pass == 1 && m >= 0) break;             // a regular match exists and only ignore regions follow
        for (int gi = 0; gi < G; ++gi) {
          const unsigned char f = g_taken[(g0 + gi) * AT + lane];
          if ((f & 1) != pass) continue;
          if ((f & 2) && !g_crowd[g0 + gi]) continue;
          if (row[gi] < best) continue;
          best = row[gi];
          m = gi;
        }
      }
    }
    const double da = d_area[d0 + di];
    int match = 0;
    unsigned char ign = 0;
    if (m >= 0) {
      const unsigned char f = g_taken[(g0 + m) * AT + lane];
      ign = f & 1;
      g_taken[(g0 + m) * AT + lane] = f | 2;
      match = (int)(g0 + m) + 1;
    } else if (da < lo || da > hi) {
      ign = 1;
    }
    d_match[(d0 + di) * AT + lane] = match;
    d_ignore[(d0 + di) * AT + lane] = ign;
  }
}

}  // namespace

}  // namespace kgdet

using namespace kgdet;

extern "C" {

int kgdet_coco_similarity(int32_t iou_type, const int32_t *cells, const int64_t *sim_off, int32_t C, int64_t ND, int64_t NG,
                          int64_t sim_size, const double *d_box, const double *d_kxy, const double *g_box,
                          const double *g_kpt, const double *g_area, const int32_t *g_crowd, const int32_t *g_nvis,
                          const double *var, int32_t K, double *sim, void *stream) {
  KGDET_CHECK_SHAPE(iou_type == 0 || iou_type == 1, "coco_similarity: iou_type %d (0 = bbox, 1 = keypoints)", iou_type);
  KGDET_CHECK_SHAPE(C >= 0 && ND >= 0 && NG >= 0 && sim_size >= 0, "coco_similarity: negative size");
  KGDET_CHECK_SHAPE(ND < (1ll << 31) && NG < (1ll << 31), "coco_similarity: more than 2^31 - 1 rows (evaluate in chunks)");
  if (C == 0 || sim_size == 0) return KGDET_OK;
  KGDET_CHECK_SHAPE(cells && sim_off && sim && g_box, "coco_similarity: null pointer");
  if (iou_type == 0) {
    KGDET_CHECK_SHAPE(d_box && g_crowd, "coco_similarity: bbox needs d_box and g_crowd");
    hipLaunchKernelGGL(coco_iou_kernel, dim3((unsigned)C), dim3(kSimThreads), 0, (hipStream_t)stream, (const int *)cells,
                       (const long long *)sim_off, (long long)ND, (long long)NG, (long long)sim_size, d_box, g_box,
                       (const int *)g_crowd, sim);
    KGDET_CHECK_LAUNCH("coco_iou_kernel");
  } else {
    KGDET_CHECK_SHAPE(K >= 1, "coco_similarity: K = %d landmarks", K);
    KGDET_CHECK_SHAPE(d_kxy && g_kpt && g_area && g_nvis && var, "coco_similarity: keypoints needs d_kxy, g_kpt, g_area, "
                      "g_nvis and var");
    hipLaunchKernelGGL(coco_oks_kernel, dim3((unsigned)C), dim3(kSimThreads), 0, (hipStream_t)stream, (const int *)cells,
                       (const long long *)sim_off, (long long)ND, (long long)NG, (long long)sim_size, d_kxy, g_kpt, g_box,
                       g_area, (const int *)g_nvis, var, (int)K, sim);
    KGDET_CHECK_LAUNCH("coco_oks_kernel");
  }
  return KGDET_OK;
}

int kgdet_coco_match(const int32_t *cells, const int64_t *sim_off, int32_t C, int64_t ND, int64_t NG, int64_t sim_size,
                     const double *sim, const double *d_area, const double *g_area, const uint8_t *g_ignore,
                     const int32_t *g_crowd, const double *area_rng, int32_t A, const double *best0, int32_t T,
                     int32_t *d_match, uint8_t *d_ignore, uint8_t *g_ignore_out, uint8_t *g_taken, void *stream) {
  KGDET_CHECK_SHAPE(C >= 0 && ND >= 0 && NG >= 0 && sim_size >= 0, "coco_match: negative size");
  KGDET_CHECK_SHAPE(ND < (1ll << 31) && NG < (1ll << 31), "coco_match: more than 2^31 - 1 rows (evaluate in chunks)");
  KGDET_CHECK_SHAPE(A >= 1 && T >= 1 && A * T <= kWave,
                    "coco_match: %d area ranges x %d thresholds (the pairs are the lanes of one wave: at most %d)", A, T, kWave);
  if (C == 0) return KGDET_OK;
  KGDET_CHECK_SHAPE(cells && sim_off && area_rng && best0, "coco_match: null pointer");
  KGDET_CHECK_SHAPE(sim_size == 0 || sim, "coco_match: null similarity matrix");
  KGDET_CHECK_SHAPE(ND == 0 || (d_area && d_match && d_ignore), "coco_match: null detection array");
  KGDET_CHECK_SHAPE(NG == 0 || (g_area && g_ignore && g_crowd && g_ignore_out && g_taken), "coco_match: null ground-truth array");
  hipLaunchKernelGGL(coco_match_kernel, dim3((unsigned)C), dim3(kWave), 0, (hipStream_t)stream, (const int *)cells,
                     (const long long *)sim_off, (long long)ND, (long long)NG, (long long)sim_size, sim, d_area, g_area,
                     (const unsigned char *)g_ignore, (const int *)g_crowd, area_rng, (int)A, best0, (int)T, (int *)d_match,
                     (unsigned char *)d_ignore, (unsigned char *)g_ignore_out, (unsigned char *)g_taken);
  KGDET_CHECK_LAUNCH("coco_match_kernel");
  return KGDET_OK;
}

}  // extern "C"
