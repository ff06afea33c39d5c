// CocoEvaluator.accumulate and the landmark half of pack_test_results on the device (kgdet_amd/evaluation_device.py) for
// gfx950, launched from evaluation only.
//
// kgdet_coco_accumulate: one workgroup per line (category k, area range a, max_dets m, threshold t).  It walks the category's
// score-ordered sequence in tiles of KGDET_COCO_ACC_TILE positions: an integer block scan gives every position its tp / fp
// counts; because tp rises by at most one per position, the position where tp first reaches c is the one whose own flag
// is a true positive, and that position writes precision(c) = c / (fp + c + eps) and its score into the line's workspace.
// Inside a run of equal tp the precision only falls (fp grows; a correctly rounded division is monotone), so the suffix
// maximum of numpy's envelope is the suffix maximum over c of precision(c): a backward tiled max scan over the workspace.
// searchsorted(rc, thr, 'left') is then "the smallest count c with c / n_gt >= thr" (rc takes every count up to the
// total), found by bisection with the same single division.  Integer counts, two float64 divisions, exact max and
// comparisons: the result is numpy's bit for bit, and independent of the schedule.
//
// kgdet_coco_pack_landmarks: one wave per row, the landmarks strided over its lanes, np.round as rint(v * 10^d) / 10^d,
// the extents through a fixed xor butterfly.
#include "common.h"

#pragma clang fp contract(off)

namespace kgdet {

namespace {

constexpr int kWave = 64;
constexpr int kAccThreads = 256;
constexpr int kAccItems = KGDET_COCO_ACC_TILE / kAccThreads;
constexpr int kPackThreads = KGDET_COCO_PACK_ROWS * kWave;
static_assert(kAccItems * kAccThreads == KGDET_COCO_ACC_TILE && kAccItems >= 1, "tile = threads x items");

struct Cnt {
  int sel, tp, fp;
};
__device__ __forceinline__ Cnt operator+(Cnt a, Cnt b) { return Cnt{a.sel + b.sel, a.tp + b.tp, a.fp + b.fp}; }

// exclusive scan of `v` over the block's threads; `total` = the block's sum.  `part` is LDS for one entry per wave.
__device__ __forceinline__ Cnt block_exclusive_scan(Cnt v, Cnt *part, Cnt &total) {
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  Cnt inc = v;
  for (int d = 1; d < kWave; d <<= 1) {
    const int s = __shfl_up(inc.sel, d, kWave), p = __shfl_up(inc.tp, d, kWave), f = __shfl_up(inc.fp, d, kWave);
    if (lane >= d) inc = inc + Cnt{s, p, f};
  }
  if (lane == kWave - 1) part[wave] = inc;
  __syncthreads();
  Cnt base{0, 0, 0};
  total = Cnt{0, 0, 0};
  for (int w = 0; w < kAccThreads / kWave; ++w) {
    const Cnt x = part[w];
    if (w < wave) base = base + x;
    total = total + x;
  }
  __syncthreads();      // (`part` is written again by the next tile)
  return Cnt{base.sel + inc.sel - v.sel, base.tp + inc.tp - v.tp, base.fp + inc.fp - v.fp};
}

__device__ __forceinline__ double max_exact(double a, double b) { return a < b ? b : a; }

__global__ __launch_bounds__(kAccThreads) void coco_count_gt_kernel(const unsigned char *__restrict__ g_ignore,
                                                                    const int *__restrict__ g_cat, long long NG, int A,
                                                                    int *__restrict__ n_gt) {
  __shared__ int part[kAccThreads / kWave];
  const int k = blockIdx.x / A, a = blockIdx.x - k * A;
  int n = 0;
  for (long long g = threadIdx.x; g < NG; g += kAccThreads) n += (g_cat[g] == k && g_ignore[g * A + a] == 0) ? 1 : 0;
  for (int m = kWave / 2; m >= 1; m >>= 1) n += __shfl_xor(n, m, kWave);
  if ((threadIdx.x & (kWave - 1)) == 0) part[threadIdx.x / kWave] = n;
  __syncthreads();
  if (threadIdx.x == 0) {
    int sum = 0;
    for (int w = 0; w < kAccThreads / kWave; ++w) sum += part[w];
    n_gt[blockIdx.x] = sum;
  }
}

__global__ __launch_bounds__(kAccThreads) void coco_accumulate_kernel(
    const int *__restrict__ d_match, const unsigned char *__restrict__ d_ignore, const double *__restrict__ score,
    const int *__restrict__ rank, const long long *__restrict__ order, const long long *__restrict__ cat_cut,
    const int *__restrict__ n_gt, const int *__restrict__ max_dets, const double *__restrict__ rec_thrs, long long ND, int K,
    int A, int T, int M, int R, long long tp_cap, double *__restrict__ precision, double *__restrict__ recall,
    double *__restrict__ scores, double *__restrict__ workspace) {
  __shared__ Cnt part[kAccThreads / kWave];
  __shared__ double s_max[kAccThreads];
  __shared__ double s_score0;
  const int tid = threadIdx.x;
  int line = blockIdx.x;                       // ((k * A + a) * M + m) * T + t: neighbours read the same flag rows
  const int t = line % T;
  line /= T;
  const int m = line % M;
  line /= M;
  const int a = line % A, k = line / A;
  const long long KAM = (long long)K * A * M;
  const long long out0 = ((long long)k * A + a) * M + m;          // + (t * R + r) * KAM  /  + t * KAM
  const int ngt = n_gt[k * A + a];
  if (ngt <= 0) {
    for (int r = tid; r < R; r += kAccThreads) {
      precision[((long long)t * R + r) * KAM + out0] = -1.0;
      scores[((long long)t * R + r) * KAM + out0] = -1.0;
    }
    if (tid == 0) recall[(long long)t * KAM + out0] = -1.0;
    return;
  }
  long long lo = cat_cut[k], hi = cat_cut[k + 1];
  lo = lo < 0 ? 0 : (lo > ND ? ND : lo);
  hi = hi < lo ? lo : (hi > ND ? ND : hi);
  long long cap64 = hi - lo < (long long)ngt ? hi - lo : (long long)ngt;
  if (cap64 > tp_cap) cap64 = tp_cap;
  const int cap = (int)cap64;
  double *ws_p = workspace + 2ll * tp_cap * blockIdx.x, *ws_s = ws_p + tp_cap;
  const int AT = A * T, at = a * T + t, max_det = max_dets[m];
  const double eps = 2.220446049250313e-16;                         // np.spacing(1)
  if (tid == 0) s_score0 = 0.0;

  Cnt run{0, 0, 0};                                                 // block-uniform: the counts before this tile
  for (long long base = lo; base < hi; base += KGDET_COCO_ACC_TILE) {
    const long long p0 = base + (long long)tid * kAccItems;
    long long det[kAccItems];
    unsigned flag[kAccItems];                                       // 1 selected, 2 true positive, 4 false positive
    Cnt mine{0, 0, 0};
#pragma unroll
    for (int i = 0; i < kAccItems; ++i) {
      flag[i] = 0;
      det[i] = 0;
      if (p0 + i < hi) {
        const long long d = order[p0 + i];
        if (d >= 0 && d < ND && rank[d] < max_det) {
          const bool matched = d_match[d * AT + at] != 0, ignored = d_ignore[d * AT + at] != 0;
          flag[i] = 1u | (!ignored && matched ? 2u : 0u) | (!ignored && !matched ? 4u : 0u);
          det[i] = d;
          mine.sel += 1;
          mine.tp += (flag[i] >> 1) & 1;
          mine.fp += (flag[i] >> 2) & 1;
        }
      }
    }
    Cnt total;
    Cnt c = block_exclusive_scan(mine, part, total);
    c = c + run;
#pragma unroll
    for (int i = 0; i < kAccItems; ++i) {
      if (!(flag[i] & 1u)) continue;
      if (c.sel == 0) s_score0 = score[det[i]];                     // (one thread of the block sees sel == 0 selected)
      c.sel += 1;
      if (flag[i] & 4u) c.fp += 1;
      if (flag[i] & 2u) {
        c.tp += 1;
        if (c.tp <= cap) {
          ws_p[c.tp - 1] = (double)c.tp / (((double)c.fp + (double)c.tp) + eps);
          ws_s[c.tp - 1] = score[det[i]];
        }
      }
    }
    run = run + total;
  }
  __syncthreads();                               // the workspace and s_score0 are the whole block's from here on
  const int TP = run.tp < cap ? run.tp : cap;

  // the precision envelope: suffix maximum over the counts, tiles from the back; thread 0 holds the last count of a tile
  double carry = 0.0;                            // (every recorded precision is > 0)
  for (int end = TP; end > 0; end -= kAccThreads) {
    const int idx = end - 1 - tid;
    double v = idx >= 0 ? ws_p[idx] : 0.0;
    s_max[tid] = v;
    __syncthreads();
    for (int d = 1; d < kAccThreads; d <<= 1) {
      const double o = tid >= d ? s_max[tid - d] : 0.0;
      __syncthreads();
      v = max_exact(v, o);
      s_max[tid] = v;
      __syncthreads();
    }
    v = max_exact(v, carry);
    if (idx >= 0) ws_p[idx] = v;
    carry = max_exact(carry, s_max[kAccThreads - 1]);
    __syncthreads();
  }

  const double n = (double)ngt, score0 = s_score0;
  for (int r = tid; r < R; r += kAccThreads) {
    const double thr = rec_thrs[r];
    int c0 = 0, c1 = TP + 1;                     // the smallest count c in [0, TP] with c / n >= thr; TP + 1: none
    while (c0 < c1) {
      const int mid = (c0 + c1) >> 1;
      if ((double)mid / n >= thr) c1 = mid; else c0 = mid + 1;
    }
    double q = 0.0, s = 0.0;
    if (c0 == 0) {                               // position 0, when a position is selected at all
      if (run.sel > 0) {
        q = TP >= 1 ? ws_p[0] : 0.0;
        s = score0;
      }
    } else if (c0 <= TP) {
      q = ws_p[c0 - 1];
      s = ws_s[c0 - 1];
    }
    precision[((long long)t * R + r) * KAM + out0] = q;
    scores[((long long)t * R + r) * KAM + out0] = s;
  }
  if (tid == 0) recall[(long long)t * KAM + out0] = (double)run.tp / n;
}

// numpy's minimum / maximum: a NaN wins
__device__ __forceinline__ double np_min(double a, double b) { return a != a ? a : (b != b ? b : (b < a ? b : a)); }
__device__ __forceinline__ double np_max(double a, double b) { return a != a ? a : (b != b ? b : (a < b ? b : a)); }

__global__ __launch_bounds__(kPackThreads) void coco_pack_landmarks_kernel(const float *__restrict__ src, long long n, int K,
                                                                           double scale, double *__restrict__ kxy,
                                                                           double *__restrict__ bbox,
                                                                           double *__restrict__ area) {
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const long long row = (long long)blockIdx.x * KGDET_COCO_PACK_ROWS + wave;
  if (row >= n) return;                          // (wave-uniform: the shuffles below see all 64 lanes)
  const float *s = src + row * 3 * K;
  double *o = kxy + row * 2 * K;
  const double inf = __builtin_huge_val();
  double x0 = inf, x1 = -inf, y0 = inf, y1 = -inf;
  for (int k = lane; k < K; k += kWave) {
    const double x = rint((double)s[3 * k] * scale) / scale, y = rint((double)s[3 * k + 1] * scale) / scale;
    o[2 * k] = x;
    o[2 * k + 1] = y;
    x0 = np_min(x0, x);
    x1 = np_max(x1, x);
    y0 = np_min(y0, y);
    y1 = np_max(y1, y);
  }
  for (int m = kWave / 2; m >= 1; m >>= 1) {
    x0 = np_min(x0, __shfl_xor(x0, m, kWave));
    x1 = np_max(x1, __shfl_xor(x1, m, kWave));
    y0 = np_min(y0, __shfl_xor(y0, m, kWave));
    y1 = np_max(y1, __shfl_xor(y1, m, kWave));
  }
  if (lane == 0) {
    const double w = x1 - x0, h = y1 - y0;
    bbox[4 * row] = x0;
    bbox[4 * row + 1] = y0;
    bbox[4 * row + 2] = w;
    bbox[4 * row + 3] = h;
    area[row] = w * h;
  }
}

}  // namespace

}  // namespace kgdet

using namespace kgdet;

extern "C" {

int kgdet_coco_count_gt(const uint8_t *g_ignore, const int32_t *g_cat, int64_t NG, int32_t K, int32_t A, int32_t *n_gt,
                        void *stream) {
  KGDET_CHECK_SHAPE(K >= 1 && A >= 1 && A <= kWave && (int64_t)K * A < (1ll << 31),
                    "coco_count_gt: %d categories x %d area ranges", K, A);
  KGDET_CHECK_SHAPE(NG >= 0 && NG < (1ll << 31), "coco_count_gt: %lld ground truths (0 .. 2^31 - 2)", (long long)NG);
  KGDET_CHECK_SHAPE(n_gt && (NG == 0 || (g_ignore && g_cat)), "coco_count_gt: null pointer");
  hipLaunchKernelGGL(coco_count_gt_kernel, dim3((unsigned)(K * A)), dim3(kAccThreads), 0, (hipStream_t)stream,
                     (const unsigned char *)g_ignore, (const int *)g_cat, (long long)NG, (int)A, (int *)n_gt);
  KGDET_CHECK_LAUNCH("coco_count_gt_kernel");
  return KGDET_OK;
}

int kgdet_coco_accumulate(const int32_t *d_match, const uint8_t *d_ignore, const double *score, const int32_t *rank,
                          const int64_t *order, const int64_t *cat_cut, const int32_t *n_gt, const int32_t *max_dets,
                          const double *rec_thrs, int64_t ND, int32_t K, int32_t A, int32_t T, int32_t M, int32_t R,
                          int64_t tp_cap, double *precision, double *recall, double *scores, void *workspace,
                          size_t workspace_bytes, void *stream) {
  KGDET_CHECK_SHAPE(A >= 1 && T >= 1 && A * T <= kWave,
                    "coco_accumulate: %d area ranges x %d thresholds (kgdet_coco_match's lanes: at most %d pairs)", A, T, kWave);
  KGDET_CHECK_SHAPE(K >= 1 && M >= 1 && R >= 1, "coco_accumulate: %d categories, %d max_dets, %d recall thresholds (each >= 1)",
                    K, M, R);
  const int64_t lines = (int64_t)K * A * T;      // (A * T <= 64: no overflow; times M below)
  KGDET_CHECK_SHAPE(lines <= ((1ll << 31) - 1) / M, "coco_accumulate: %d x %d x %d x %d lines (below 2^31)", K, A, M, T);
  KGDET_CHECK_SHAPE(ND >= 0 && ND < (1ll << 31) - 1, "coco_accumulate: %lld detections (0 .. 2^31 - 2)", (long long)ND);
  KGDET_CHECK_SHAPE(tp_cap >= 0 && tp_cap < (1ll << 31), "coco_accumulate: tp_cap %lld (0 .. 2^31 - 1)", (long long)tp_cap);
  KGDET_CHECK_SHAPE(cat_cut && n_gt && max_dets && rec_thrs && precision && recall && scores, "coco_accumulate: null pointer");
  KGDET_CHECK_SHAPE(ND == 0 || (d_match && d_ignore && score && rank && order), "coco_accumulate: null detection array");
  const size_t need = (size_t)16 * (size_t)tp_cap * (size_t)(lines * M);
  if (need > 0 && (workspace == nullptr || workspace_bytes < need)) {
    set_error("coco_accumulate: needs %zu bytes of workspace (16 * tp_cap * K * A * M * T), got %zu", need, workspace_bytes);
    return KGDET_E_WORKSPACE;
  }
  hipLaunchKernelGGL(coco_accumulate_kernel, dim3((unsigned)(lines * M)), dim3(kAccThreads), 0, (hipStream_t)stream,
                     (const int *)d_match, (const unsigned char *)d_ignore, score, (const int *)rank, (const long long *)order,
                     (const long long *)cat_cut, (const int *)n_gt, (const int *)max_dets, rec_thrs, (long long)ND, (int)K,
                     (int)A, (int)T, (int)M, (int)R, (long long)tp_cap, precision, recall, scores, (double *)workspace);
  KGDET_CHECK_LAUNCH("coco_accumulate_kernel");
  return KGDET_OK;
}

int kgdet_coco_pack_landmarks(const float *src, int64_t n, int32_t K, int32_t num_digits, double *kxy, double *bbox,
                              double *area, void *stream) {
  static const double kPow10[16] = {1e0, 1e1, 1e2, 1e3, 1e4, 1e5, 1e6, 1e7, 1e8, 1e9, 1e10, 1e11, 1e12, 1e13, 1e14, 1e15};
  KGDET_CHECK_SHAPE(K >= 1, "coco_pack_landmarks: K = %d landmarks", K);
  KGDET_CHECK_SHAPE(n >= 0 && n < (1ll << 31), "coco_pack_landmarks: %lld rows (0 .. 2^31 - 1)", (long long)n);
  KGDET_CHECK_SHAPE(num_digits >= 0 && num_digits <= 15, "coco_pack_landmarks: num_digits %d (0 .. 15)", num_digits);
  if (n == 0) return KGDET_OK;
  KGDET_CHECK_SHAPE(src && kxy && bbox && area, "coco_pack_landmarks: null pointer");
  const unsigned blocks = (unsigned)((n + KGDET_COCO_PACK_ROWS - 1) / KGDET_COCO_PACK_ROWS);
  hipLaunchKernelGGL(coco_pack_landmarks_kernel, dim3(blocks), dim3(kPackThreads), 0, (hipStream_t)stream, src, (long long)n,
                     (int)K, kPow10[num_digits], kxy, bbox, area);
  KGDET_CHECK_LAUNCH("coco_pack_landmarks_kernel");
  return KGDET_OK;
}

}  // extern "C"
