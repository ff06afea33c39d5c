// What the fused loss kernels (head_loss.hip, serial_loss.hip) share.  Device side: the sigmoid focal loss with the float /
// double promotions of csrc/focal.hip, the smooth-L1 row of csrc/smooth_l1.hip, the PointAssigner frame of a gt, the label
// rule, the keypoint targets and the block reduction.  Host side: the descriptor checks, the workspace carve, the row plan.
//
// Contraction.  serial_loss.hip compiles its own code under `#pragma clang fp contract(off)`, head_loss.hip under the compiler's
// default, which fuses a multiply into the add or subtract it feeds; the mode follows the place an expression is WRITTEN, and
// this header is included above that pragma.  So nothing here holds such a multiply: `diff - 0.5f * beta`, the squared
// distance `dx * dx + dy * dy`, the coordinate decodes and `acc += l * w` are written by the caller, in the caller's mode.
#pragma once
#include <float.h>

#include "common.h"

namespace kgdet {

constexpr int kMaxImages = KGDET_HEAD_MAX_IMAGES;
constexpr int kMaxGt = 64;

__device__ __forceinline__ double neg_softplus_d(float x) {  // as csrc/focal.hip
  const int ge = x >= 0;
  return -1. * x * ge - logf((float)(1. + expf((float)(x - 2. * x * ge))));
}

// sigmoid_focal_loss_cuda.cu:24-59 (same promotions as csrc/focal.hip)
__device__ __forceinline__ float focal_fwd(float x, int t, int d, float gamma, float alpha) {
  const float c1 = (t == (d + 1));
  const float c2 = ((t >= 0) & (t != (d + 1)));
  const float zn = (float)(1.0 - alpha), zp = alpha;
  const float p = (float)(1. / (1. + expf(-x)));
  const float term1 = powf((float)(1. - p), gamma) * logf(fmaxf(p, FLT_MIN));
  const float term2 = (float)(powf(p, gamma) * neg_softplus_d(x));
  float l = 0.0f;
  l += -c1 * term1 * zp;
  l += -c2 * term2 * zn;
  return l;
}

// :62-97
__device__ __forceinline__ float focal_bwd(float x, int t, int d, float gamma, float alpha) {
  const float c1 = (t == (d + 1));
  const float c2 = ((t >= 0) & (t != (d + 1)));
  const float zn = (float)(1.0 - alpha), zp = alpha;
  const float p = (float)(1. / (1. + expf(-x)));
  const float term1 = (float)(powf((float)(1. - p), gamma) * (1. - p - (p * gamma * logf(fmaxf(p, FLT_MIN)))));
  const float term2 = (float)(powf(p, gamma) * (neg_softplus_d(x) * (1. - p) * gamma - p));
  float g = 0.0f;
  g += -c1 * term1 * zp;
  g += -c2 * term2 * zn;
  return g;
}

// The smooth-L1 row, csrc/smooth_l1.hip's expressions: x of a decoded coordinate and its target, the forward value of
// diff = |x| (`linear` = diff - 0.5f * beta, written by the caller: see "Contraction"), and the gradient to the RAW map value
// (decoded = raw * stride + centre) under scale = upstream * loss_weight / num_total; weight 0 writes 0.
__device__ __forceinline__ float smooth_l1_x(float pred, float target, float nt) { return pred / nt - target / nt; }
__device__ __forceinline__ float smooth_l1_fwd(float diff, float beta, float linear) {
  return diff < beta ? 0.5f * diff * diff / beta : linear;
}
__device__ __forceinline__ float smooth_l1_bwd(float x, float beta, float w, float scale, float nt, float stride) {
  const float dl = fabsf(x) < beta ? x / beta : (x > 0.0f ? 1.0f : x < 0.0f ? -1.0f : 0.0f);
  return w != 0.0f ? scale * w * dl / nt * stride : 0.0f;
}

// PointAssigner (point_assigner.py:69-71, :93-95): centre and size of a gt, the size clamped at 1e-6; the distance of a
// grid point p is ((p - centre) / size).norm(), whose sum of squares the caller writes (see "Contraction")
struct GtFrame {
  float cx, cy, w, h;
};
__device__ __forceinline__ GtFrame gt_frame(const float *__restrict__ box) {
  return {(box[0] + box[2]) / 2, (box[1] + box[3]) / 2, fmaxf(box[2] - box[0], 1e-6f), fmaxf(box[3] - box[1], 1e-6f)};
}

// a valid extent on a side of `full` grid points: 0 (or anything beyond the side) is the whole side
__host__ __device__ __forceinline__ int extent_of(int v, int full) { return v > 0 && v < full ? v : full; }

// the visible keypoints (visibility != 0) among m = first, first + step, ... < K of one gt's [K, 3] rows: a thread's share
// of kpt_weights.sum(1) / 2
__device__ __forceinline__ int visible_keypoints(const float *__restrict__ gkp, int K, int first, int step) {
  int cnt = 0;
  for (int m = first; m < K; m += step) cnt += gkp[m * 3 + 2] != 0.0f ? 1 : 0;
  return cnt;
}

// point_target_kp.py:140-147: a positive (a > 0: gt a - 1) takes its gt's label (1 without a label table) and pos_weight;
// a negative (a == 0) inside the valid extent label 0 and weight 1; don't-care (a < 0) and (unmap fill) invalid points 0
struct PointLabel {
  int label;
  float weight;
};
__device__ __forceinline__ PointLabel point_label(const int64_t *__restrict__ gt_labels, int a, bool inside, float pos_weight) {
  return {a > 0 ? (gt_labels ? (int)gt_labels[a - 1] : 1) : 0, a > 0 ? pos_weight : ((a == 0 && inside) ? 1.0f : 0.0f)};
}

// One regression row of a point at (px, py): the grid coordinate the raw value is decoded around, the target, and whether
// the row counts at all.  Keypoint channel pairs are (y, x) and the loss pairs them with the (x, y) targets of the gt's
// [K, 3] rows gkp; an invisible keypoint does not count.  (Box channel c: {(c & 1) ? py : px, gbox[c], true}.)
struct RowTarget {
  float centre, target;
  bool on;
};
__device__ __forceinline__ RowTarget keypoint_target(const float *__restrict__ gkp, int c, float px, float py) {
  const int m = c >> 1, is_x = c & 1;
  return {is_x ? px : py, gkp[m * 3 + (is_x ? 0 : 1)], gkp[m * 3 + 2] != 0.0f};
}

// 256 threads = 4 waves: the block's sums of K per-thread accumulators, returned to threads [0, K) (0 elsewhere).  Fixed
// order: the xor tree within a wave, then waves 0 .. 3.  The caller keeps a barrier between two uses in one kernel.
template <int K>
__device__ __forceinline__ float block_sums(const float (&acc)[K]) {
  __shared__ float s_part[4][K];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    float v = acc[k];
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    if (lane == 0) s_part[wave][k] = v;
  }
  __syncthreads();
  return tid < K ? s_part[0][tid] + s_part[1][tid] + s_part[2][tid] + s_part[3][tid] : 0.0f;
}

// ---- host side

// images, channel counts, betas and the per-image ground truth of either descriptor; `counts`: num_gt is looked at (the
// table route keeps it in device memory), and *gmax is the largest
template <class Targets>
int check_targets(const Targets *t, const float *beta, int num_betas, bool counts, int *gmax) {
  KGDET_CHECK_SHAPE(t->B >= 1 && t->B <= kMaxImages, "1..%d images per call", kMaxImages);
  KGDET_CHECK_SHAPE(t->num_classes > 0 && t->num_keypoints > 0, "bad channel counts");
  for (int k = 0; k < num_betas; ++k) KGDET_CHECK_SHAPE(beta[k] > 0.0f, "beta must be positive");
  *gmax = 0;
  for (int b = 0; b < t->B; ++b) {
    KGDET_CHECK_SHAPE(!counts || (t->num_gt[b] >= 1 && t->num_gt[b] <= kMaxGt), "image %d: %d ground-truth boxes (1..%d)",
                      b, t->num_gt[b], kMaxGt);
    KGDET_CHECK_SHAPE(t->gt_bboxes[b] && t->gt_keypoints[b], "null ground-truth pointer");
    if (counts && t->num_gt[b] > *gmax) *gmax = t->num_gt[b];
  }
  return KGDET_OK;
}

// `who` needs the `need` bytes its *_workspace_bytes names (backward: the workspace its forward call filled)
static inline int check_workspace(const char *who, const void *workspace, size_t got, size_t need) {
  if (workspace != nullptr && got >= need) return KGDET_OK;
  set_error("%s_loss: needs %zu bytes of workspace (kgdet_%s_loss_workspace_bytes; backward: the forward call's), got %zu", who,
            need, who, got);
  return KGDET_E_WORKSPACE;
}

// the next 256-byte-aligned array of a workspace, `off` bytes in; base == nullptr: only the size is wanted
template <class T>
T *take(void *base, size_t &off, size_t count) {
  T *p = base ? reinterpret_cast<T *>(static_cast<unsigned char *>(base) + off) : nullptr;
  off += align_up(count * sizeof(T), 256);
  return p;
}

// The loss rows of a 64-point tile are split over *groups workgroups of (the value) rows each -- 4 waves: at least 4 rows --
// so that tiles x groups x images reaches `target` workgroups, enough for the chip.
static inline int rows_per_group(int total_rows, int tiles_times_images, int target, int *groups) {
  int g = ceil_div(target, tiles_times_images);
  if (g > total_rows / 4) g = total_rows / 4 > 0 ? total_rows / 4 : 1;
  const int rows = ceil_div(total_rows, g);
  *groups = ceil_div(total_rows, rows);
  return rows;
}

}  // namespace kgdet
