// pack_test_results on the device (kgdet_amd/evaluation_device.py: pack_device_results) for gfx950: the detections of a whole
// test run stay in the [N, M, 7 + 3K] float32 tensor the detector wrote them into (runner.DeviceResults.rows) and are
// ordered, rounded, cut and gathered here.  Launched from evaluation only.
//
// kgdet_coco_order_dets: one workgroup per image.  The first `count` rows (column 6 of row 0) are read once: xywh and the
// score are rounded like Python's round(v, d) (round_decimal below: exact, no host pass), every row gets its index k in the
// host list's enumeration (label ascending, then row order) and its rank inside its (image, category) cell by counting
// comparisons over the image's rows in LDS -- M is small.  Per cell the kept counts of both cuts are written.
// kgdet_coco_scatter_dets: one workgroup per image again, after the host has scanned the cell counts: every kept row goes
// to start[cell] + rank of either kind; the landmark rows of the keypoints kind are copied by one wave per row.
// Integer arithmetic, single float64 operations without contraction, no float atomics: bit-equal to
// evaluation_device.pack_rows_restatement and independent of the schedule.
#include "common.h"

#pragma clang fp contract(off)

namespace kgdet {

namespace {

constexpr int kWave = 64;
constexpr int kThreads = 256;
constexpr int kVals = 6;        // x, y, w, h, score, area
constexpr int kInfo = 3;        // category index (-1: unknown), k inside the image, rank inside the cell

typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

// Python's round(v, d) for S = 10^d (exact in float64) and |v * S| < 2^40: the exact decimal value of v rounded half to even
// at d digits, then the double nearest to n / S.  p = fl(a * S) and e = a * S - p exactly (one fma), so the position of the
// exact product against the half is known: p - floor(p) is exact, and where it IS one half the sign of e decides.
// *bad is raised for a non-finite value or one at or beyond 2^40 / S.
__device__ __forceinline__ double round_decimal(double v, double S, int *bad) {
  const double a = fabs(v);
  const double p = a * S;
  if (!(p < 1099511627776.0)) {        // 2^40; a NaN lands here too
    *bad += 1;
    return v;
  }
  const double e = fma(a, S, -p);
  const double f = floor(p);
  const double r = p - f;
  double n = f;
  if (r > 0.5 || (r == 0.5 && (e > 0.0 || (e == 0.0 && fmod(f, 2.0) != 0.0)))) n = f + 1.0;
  return copysign(n / S, v);
}

__global__ __launch_bounds__(kThreads) void coco_order_dets_kernel(
    const float *__restrict__ rows, int M, int W, const int *__restrict__ img_slot, const int *__restrict__ cat_of_label, int L,
    int C, long long n_cells, double S, int cut_bbox, int cut_kp, double *__restrict__ vals, int *__restrict__ info,
    int *__restrict__ img_rows, int *__restrict__ cnt_bbox, int *__restrict__ cnt_kp, int *__restrict__ flags) {
  __shared__ double s_score[KGDET_COCO_ORDER_MAX_ROWS];
  __shared__ short s_label[KGDET_COCO_ORDER_MAX_ROWS];
  __shared__ short s_cat[KGDET_COCO_ORDER_MAX_ROWS];
  __shared__ int s_lab_n[KGDET_COCO_ORDER_MAX_LABELS], s_lab_base[KGDET_COCO_ORDER_MAX_LABELS];
  const int tid = threadIdx.x;
  const long long img = blockIdx.x;
  const float *src = rows + img * (long long)M * W;
  const float cf = src[6];
  int bad_value = 0, bad_layout = 0;
  int count = 0;
  if (cf >= 0.0f && cf < (float)(M + 1))
    count = (int)cf;                   // (truncated, as unpack_results reads it)
  else if (tid == 0)
    bad_layout += 1;
  const long long slot = img_slot[img];
  const bool known = slot >= 0 && (slot + 1) * (long long)C <= n_cells;
  for (int l = tid; l < L; l += kThreads) s_lab_n[l] = 0;
  __syncthreads();
  double *v_out = vals + img * (long long)M * kVals;
  int *i_out = info + img * (long long)M * kInfo;
  for (int i = tid; i < count; i += kThreads) {
    const float *r = src + (long long)i * W;
    const float lf = r[5];
    int label = -1, cat = -1;
    if (lf > -1.0f && lf < (float)L) {
      label = (int)lf;
      cat = cat_of_label[label];
      if (cat >= C) cat = -1;
      atomicAdd(&s_lab_n[label], 1);
    }
    s_label[i] = (short)label;
    s_cat[i] = (short)cat;
    double sc = 0.0;
    if (label >= 0) {
      const double x1 = (double)r[0], y1 = (double)r[1], x2 = (double)r[2], y2 = (double)r[3];
      const double x = round_decimal(x1, S, &bad_value), y = round_decimal(y1, S, &bad_value);
      const double w = round_decimal(x2 - x1 + 1.0, S, &bad_value), h = round_decimal(y2 - y1 + 1.0, S, &bad_value);
      sc = round_decimal((double)r[4], S, &bad_value);
      double *o = v_out + (long long)i * kVals;
      o[0] = x;
      o[1] = y;
      o[2] = w;
      o[3] = h;
      o[4] = sc;
      o[5] = w * h;
    }
    s_score[i] = sc;
  }
  __syncthreads();
  if (tid == 0) {
    int run = 0;
    for (int l = 0; l < L; ++l) {
      s_lab_base[l] = run;
      run += s_lab_n[l];
    }
    img_rows[img] = run;
    if (run > 0 && !known) bad_layout += 1;      // detections of an image the ground truth does not hold
  }
  __syncthreads();
  for (int i = tid; i < count; i += kThreads) {
    const int label = s_label[i], cat = s_cat[i];
    int k = -1, rank = -1;
    if (label >= 0) {
      int before = 0;
      for (int j = 0; j < i; ++j) before += s_label[j] == label ? 1 : 0;
      k = s_lab_base[label] + before;
      if (cat >= 0) {
        // rank by descending rounded score, ties by k: a row of the same category is ahead when its score is higher, or equal
        // with a smaller label, or equal in the same label and earlier
        const double sc = s_score[i];
        rank = 0;
        for (int j = 0; j < count; ++j) {
          if (s_cat[j] != cat || j == i) continue;
          const double o = s_score[j];
          const int lj = s_label[j];
          rank += (o > sc || (o == sc && (lj < label || (lj == label && j < i)))) ? 1 : 0;
        }
      }
    }
    int *o = i_out + (long long)i * kInfo;
    o[0] = cat;
    o[1] = k;
    o[2] = rank;
  }
  if (known) {
    for (int c = tid; c < C; c += kThreads) {
      int n = 0;
      for (int j = 0; j < count; ++j) n += s_cat[j] == c ? 1 : 0;
      cnt_bbox[slot * C + c] = n < cut_bbox ? n : cut_bbox;
      cnt_kp[slot * C + c] = n < cut_kp ? n : cut_kp;
    }
  }
  if (bad_value) atomicAdd(&flags[0], bad_value);
  if (bad_layout) atomicAdd(&flags[1], bad_layout);
}

struct KindOut {
  long long n;
  long long *cell, *img_idx, *cat_idx, *id;
  double *score, *bbox, *area;
  float *kxy32;
};

__device__ __forceinline__ void write_row(const KindOut &o, long long pos, long long cell, long long slot, int cat, long long id,
                                          const double *v) {
  o.cell[pos] = cell;
  o.img_idx[pos] = slot;
  o.cat_idx[pos] = cat;
  o.id[pos] = id;
  o.score[pos] = v[4];
  if (o.bbox) {
    o.bbox[4 * pos] = v[0];
    o.bbox[4 * pos + 1] = v[1];
    o.bbox[4 * pos + 2] = v[2];
    o.bbox[4 * pos + 3] = v[3];
  }
  if (o.area) o.area[pos] = v[5];
}

__global__ __launch_bounds__(kThreads) void coco_scatter_dets_kernel(
    const float *__restrict__ rows, int M, int W, int K, const int *__restrict__ img_slot, int C, long long n_cells,
    const double *__restrict__ vals, const int *__restrict__ info, const long long *__restrict__ img_base,
    const long long *__restrict__ start_bbox, const long long *__restrict__ start_kp, int cut_bbox, int cut_kp, KindOut ob,
    KindOut ok, int *__restrict__ flags) {
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const long long img = blockIdx.x;
  const float *src = rows + img * (long long)M * W;
  const float cf = src[6];
  if (!(cf >= 0.0f && cf < (float)(M + 1))) return;      // (counted by the order kernel)
  const int count = (int)cf;
  const long long slot = img_slot[img];
  if (!(slot >= 0 && (slot + 1) * (long long)C <= n_cells)) return;
  const double *v_in = vals + img * (long long)M * kVals;
  const int *i_in = info + img * (long long)M * kInfo;
  const long long base = img_base[img];
  int bad = 0;
  for (int i = tid; i < count; i += kThreads) {
    const int cat = i_in[i * kInfo], k = i_in[i * kInfo + 1], rank = i_in[i * kInfo + 2];
    if (cat < 0 || cat >= C || rank < 0) continue;
    const long long cell = slot * C + cat, id = base + k + 1;
    const double *v = v_in + (long long)i * kVals;
    if (rank < cut_bbox) {
      const long long pos = start_bbox[cell] + rank;
      if (pos >= 0 && pos < ob.n) write_row(ob, pos, cell, slot, cat, id, v); else bad += 1;
    }
    if (rank < cut_kp) {
      const long long pos = start_kp[cell] + rank;
      if (pos >= 0 && pos < ok.n) write_row(ok, pos, cell, slot, cat, id, v); else bad += 1;
    }
  }
  if (bad) atomicAdd(&flags[1], bad);
  if (ok.kxy32 == nullptr) return;
  // the landmark rows: one wave per kept row.  A source row starts 7 floats into a row of W = 7 + 3K floats -- 4-byte
  // aligned only; 16-byte loads at that alignment run at the aligned rate on gfx950 (tools/microbench/unaligned_x4.hip).  A
  // destination row of 3K floats is 8-byte aligned when K is even: 8-byte stores then, 4-byte stores otherwise.
  const int n_f = 3 * K, n4 = (K & 1) ? 0 : n_f / 4;
  for (int i = wave; i < count; i += kThreads / kWave) {
    const int cat = i_in[i * kInfo], rank = i_in[i * kInfo + 2];
    if (cat < 0 || cat >= C || rank < 0 || rank >= cut_kp) continue;      // (wave-uniform)
    const long long pos = start_kp[slot * C + cat] + rank;
    if (pos < 0 || pos >= ok.n) continue;
    const float *s = src + (long long)i * W + 7;
    float *d = ok.kxy32 + pos * n_f;
    for (int q = lane; q < n4; q += kWave) {
      const f32x4u v = *reinterpret_cast<const f32x4u *>(s + 4 * q);
      *reinterpret_cast<f32x2 *>(d + 4 * q) = f32x2{v[0], v[1]};
      *reinterpret_cast<f32x2 *>(d + 4 * q + 2) = f32x2{v[2], v[3]};
    }
    for (int q = 4 * n4 + lane; q < n_f; q += kWave) d[q] = s[q];
  }
}

bool kind_ok(const kgdet_coco_packed_dets *o) {
  return o && o->n >= 0 && (o->n == 0 || (o->cell && o->img_idx && o->cat_idx && o->id && o->score));
}

KindOut kind_of(const kgdet_coco_packed_dets *o) {
  return KindOut{(long long)o->n,        (long long *)o->cell, (long long *)o->img_idx, (long long *)o->cat_idx,
                 (long long *)o->id,     o->score,             o->bbox,                 o->area,
                 o->kxy32};
}

const double kPow10[10] = {1e0, 1e1, 1e2, 1e3, 1e4, 1e5, 1e6, 1e7, 1e8, 1e9};

}  // namespace

}  // namespace kgdet

using namespace kgdet;

extern "C" {

int kgdet_coco_order_dets(const float *rows, int64_t N, int32_t M, int32_t W, const int32_t *img_slot,
                          const int32_t *cat_of_label, int32_t L, int32_t C, int64_t n_cells, int32_t num_digits,
                          int32_t cut_bbox, int32_t cut_kp, double *vals, int32_t *info, int32_t *img_rows, int32_t *cnt_bbox,
                          int32_t *cnt_kp, int32_t *flags, void *stream) {
  KGDET_CHECK_SHAPE(num_digits >= 1 && num_digits <= 9, "coco_order_dets: num_digits %d (1 .. 9)", num_digits);
  KGDET_CHECK_SHAPE(M >= 1 && M <= KGDET_COCO_ORDER_MAX_ROWS, "coco_order_dets: %d rows per image (1 .. %d)", M,
                    KGDET_COCO_ORDER_MAX_ROWS);
  KGDET_CHECK_SHAPE(L >= 1 && L <= KGDET_COCO_ORDER_MAX_LABELS, "coco_order_dets: %d labels (1 .. %d)", L,
                    KGDET_COCO_ORDER_MAX_LABELS);
  KGDET_CHECK_SHAPE(W >= 10 && (W - 7) % 3 == 0, "coco_order_dets: rows of %d floats (7 + 3K, K >= 1)", W);
  KGDET_CHECK_SHAPE(C >= 1 && C < (1 << 15) && n_cells >= 0 && cut_bbox >= 0 && cut_kp >= 0,
                    "coco_order_dets: %d categories (1 .. 32767), %lld cells, cuts %d / %d (each >= 0)", C, (long long)n_cells,
                    cut_bbox, cut_kp);
  KGDET_CHECK_SHAPE(N >= 0 && N < (1ll << 31), "coco_order_dets: %lld images (0 .. 2^31 - 1)", (long long)N);
  if (N == 0) return KGDET_OK;
  KGDET_CHECK_SHAPE(rows && img_slot && cat_of_label && vals && info && img_rows && flags && (n_cells == 0 || (cnt_bbox && cnt_kp)),
                    "coco_order_dets: null pointer");
  hipLaunchKernelGGL(coco_order_dets_kernel, dim3((unsigned)N), dim3(kThreads), 0, (hipStream_t)stream, rows, (int)M, (int)W,
                     (const int *)img_slot, (const int *)cat_of_label, (int)L, (int)C, (long long)n_cells, kPow10[num_digits],
                     (int)cut_bbox, (int)cut_kp, vals, (int *)info, (int *)img_rows, (int *)cnt_bbox, (int *)cnt_kp, (int *)flags);
  KGDET_CHECK_LAUNCH("coco_order_dets_kernel");
  return KGDET_OK;
}

int kgdet_coco_scatter_dets(const float *rows, int64_t N, int32_t M, int32_t W, const int32_t *img_slot, int32_t C,
                            int64_t n_cells, const double *vals, const int32_t *info, const int64_t *img_base,
                            const int64_t *start_bbox, const int64_t *start_kp, int32_t cut_bbox, int32_t cut_kp,
                            const kgdet_coco_packed_dets *out_bbox, const kgdet_coco_packed_dets *out_kp, int32_t *flags,
                            void *stream) {
  KGDET_CHECK_SHAPE(M >= 1 && M <= KGDET_COCO_ORDER_MAX_ROWS, "coco_scatter_dets: %d rows per image (1 .. %d)", M,
                    KGDET_COCO_ORDER_MAX_ROWS);
  KGDET_CHECK_SHAPE(W >= 10 && (W - 7) % 3 == 0, "coco_scatter_dets: rows of %d floats (7 + 3K, K >= 1)", W);
  KGDET_CHECK_SHAPE(C >= 1 && C < (1 << 15) && n_cells >= 0 && cut_bbox >= 0 && cut_kp >= 0,
                    "coco_scatter_dets: %d categories (1 .. 32767), %lld cells, cuts %d / %d (each >= 0)", C, (long long)n_cells,
                    cut_bbox, cut_kp);
  KGDET_CHECK_SHAPE(N >= 0 && N < (1ll << 31), "coco_scatter_dets: %lld images (0 .. 2^31 - 1)", (long long)N);
  KGDET_CHECK_SHAPE(kind_ok(out_bbox) && kind_ok(out_kp), "coco_scatter_dets: an output set is missing, negative or holds a null pointer");
  if (N == 0) return KGDET_OK;
  KGDET_CHECK_SHAPE(rows && img_slot && vals && info && img_base && flags && (n_cells == 0 || (start_bbox && start_kp)),
                    "coco_scatter_dets: null pointer");
  hipLaunchKernelGGL(coco_scatter_dets_kernel, dim3((unsigned)N), dim3(kThreads), 0, (hipStream_t)stream, rows, (int)M, (int)W,
                     (int)((W - 7) / 3), (const int *)img_slot, (int)C, (long long)n_cells, vals, (const int *)info,
                     (const long long *)img_base, (const long long *)start_bbox, (const long long *)start_kp, (int)cut_bbox,
                     (int)cut_kp, kind_of(out_bbox), kind_of(out_kp), (int *)flags);
  KGDET_CHECK_LAUNCH("coco_scatter_dets_kernel");
  return KGDET_OK;
}

}  // extern "C"
