// Target assignment + the nine losses of the KGDet head as four launches (gfx950).
//
// What it replaces (one pyramid level -- KGDet: stride 32, 25 x 42 = 1050 points per image):
//   PointAssigner.assign ................. mmdet/core/bbox/assigners/point_assigner.py:23-121
//   point_target_kp / _single ............ mmdet/core/anchor/point_target_kp.py:7-169
//   offset_to_pts, loss_single, loss ..... mmdet/models/anchor_heads/reppoints_head_kp3rep_cas_1_assign_once.py:537-665
//   FocalLoss / SmoothL1Loss reductions .. mmdet/models/losses/{focal_loss.py:28-82, smooth_l1_loss.py:8-45, utils.py:7-52},
//                                          ops/sigmoid_focal_loss/src/sigmoid_focal_loss_cuda.cu:24-97
// In torch that is ~650 small launches per step (topk / scatter / where chains per ground truth, six permute + flip +
// decode chains, target tensors of 2100 x 588 built with where(), weight normalisation, the focal weight / sum tail and
// the backward of every one of those nodes): 2.5 ms of a 14.6 ms step, all launch latency.  Here:
//
//   head_assign_select   block (gt, image): distance of every point to the gt centre (normalised by the gt size), the
//                        pos_num nearest by RANK among the ~2 pos_num candidates inside a bounding distance (ties by
//                        point index).
//   head_loss_forward    block (64-point tile, channel group, image): final assignment of its points (sequential over
//                        the gts: `min_dist < assigned_dist`, earlier gt wins ties), then the loss ROWS of its group --
//                        a row = one channel of one prediction map, lanes = points (coalesced NCHW reads): focal
//                        (13 x 3 rows), smooth-L1 boxes (4 x 3) and keypoints (588 x 3) on coordinates decoded in
//                        registers (pred * stride + centre, (y, x) -> (x, y)), targets gathered from the gt tables by
//                        the assigned index, keypoint weights 4 / (2 n_visible).  Nine per-workgroup partial sums.
//   head_loss_finish     one block: positives per image, num_total = sum max(n_pos, 1), partials in fixed order,
//                        loss_k = weight_k * (sum_k / num_total).
//   head_loss_backward   same rows: grad of every prediction map, written in full (zeros where the reference's weight is 0).
//
// No tensor of targets or weights exists; nothing is read by the host.  Deterministic (fixed summation orders).
// The loss rows' arithmetic, the PointAssigner frame of a gt, the reductions and the host-side skeleton are loss_math.h's, shared
// with serial_loss.hip; the rank-based selection, the row enumeration, the decode order and the keypoint weight are this file's.
#include <float.h>

#include "common.h"
#include "loss_math.h"

namespace kgdet {

namespace {

constexpr int kMaxPoints = 4096;

// the assignment of point i of image b from the per-gt selections: point_assigner.py:106-117 (`min_dist <
// assigned_gt_dist[point_index]`, gts in order: the earlier gt keeps a tie)
__device__ __forceinline__ int final_assign(const float *__restrict__ dsel, int b, int gmax, int n_gt, int N, int i) {
  float best = INFINITY;
  int a = 0;
  for (int g = 0; g < n_gt; ++g) {
    const float d = dsel[((long long)b * gmax + g) * N + i];
    if (d < best) { best = d; a = g + 1; }
  }
  return a;
}

// Ground-truth count and valid extent of image b.  TABLE = false: the by-value fields of the descriptor (checked by the host at
// launch).  TABLE = true: row b of a device table [B][4] = (num_gt, valid_h, valid_w, 0) -- the address depends on the workgroup
// alone, so the row is ONE 16-byte uniform (scalar) load per workgroup, not a load per point; the host cannot see its contents, so
// the count is clamped to [0, cap] (the buffers hold cap rows) and the extent to the grid: no content reads outside a buffer.
struct ImageRow {
  int n_gt, vh, vw;
};
template <bool TABLE>
__device__ __forceinline__ ImageRow image_row(const kgdet_head_targets &t, const int32_t *__restrict__ table, int cap, int b) {
  int n, h, w;
  if (TABLE) {
    const int4 row = *reinterpret_cast<const int4 *>(table + 4 * b);
    n = min(max(row.x, 0), cap);
    h = row.y;
    w = row.z;
  } else {
    n = t.num_gt[b];
    h = t.valid_h[b];
    w = t.valid_w[b];
  }
  return {n, extent_of(h, t.H), extent_of(w, t.W)};
}

}  // namespace

// block (g, b), 256 threads.  dsel[b][g][i] = distance if point i is among the pos_num nearest of gt g, else +inf; row stride 64
// (kMaxGt) whatever the images' gt counts, rows g >= num_gt[b] are left unwritten and never read.
// "Among the pos_num nearest" = rank < pos_num under the (distance, point index) order.  Ranks are only needed for the
// points within T = the largest distance inside a ceil(sqrt(pos_num))-sided block of grid points around the centre: that
// block holds >= pos_num points, so every point beyond T has rank >= pos_num, and every point that precedes a candidate
// is a candidate itself -- the all-pairs count runs over ~2 pos_num candidates instead of all H * W points.
// TABLE: the launch is (gt_capacity, B) workgroups and the count comes from the table (image_row).
template <bool TABLE>
__global__ __launch_bounds__(256) void head_assign_select(const kgdet_head_targets t, int pos_num, int gmax,
                                                          float *__restrict__ dsel, const int32_t *__restrict__ table, int cap) {
  extern __shared__ float dist[];                    // [N] distances, then [N] candidate indices
  __shared__ int s_tbits, s_count;
  const int g = blockIdx.x, b = blockIdx.y, N = t.H * t.W, tid = threadIdx.x;
  const ImageRow im = image_row<TABLE>(t, table, cap, b);
  if (g >= im.n_gt) return;
  int *cand = reinterpret_cast<int *>(dist + N);
  const GtFrame gt = gt_frame(t.gt_bboxes[b] + 4 * g);
  if (tid == 0) { s_tbits = 0; s_count = 0; }
  // the image's valid extent (point_target_kp.py:107-118: the assigner only sees the points inside it)
  const int vh = im.vh, vw = im.vw;
  for (int i = tid; i < N; i += 256) {
    const int col = i % t.W, row = i / t.W;
    const float px = (float)col * t.stride, py = (float)row * t.stride;
    const float dx = (px - gt.cx) / gt.w, dy = (py - gt.cy) / gt.h;
    dist[i] = (row < vh && col < vw) ? sqrtf(dx * dx + dy * dy) : INFINITY;
  }
  __syncthreads();
  int side = 1;
  while (side * side < pos_num) ++side;
  float T = FLT_MAX;           // (every valid point is a candidate; invalid ones -- distance +inf -- never are)
  if (side <= vh && side <= vw) {
    const int j0 = min(max((int)floorf(gt.cx / t.stride + 0.5f) - side / 2, 0), vw - side);
    const int i0 = min(max((int)floorf(gt.cy / t.stride + 0.5f) - side / 2, 0), vh - side);
    for (int e = tid; e < side * side; e += 256)
      atomicMax(&s_tbits, __float_as_int(dist[(i0 + e / side) * t.W + j0 + e % side]));   // (distances are >= 0)
    __syncthreads();
    T = __int_as_float(s_tbits);
  }
  for (int i = tid; i < N; i += 256)
    if (dist[i] <= T) cand[atomicAdd(&s_count, 1)] = i;       // (any order: only counts are taken over the list)
  __syncthreads();
  const int M = s_count;
  float *out = dsel + ((long long)b * gmax + g) * N;
  for (int i = tid; i < N; i += 256) out[i] = INFINITY;
  __syncthreads();
  for (int c = tid; c < M; c += 256) {
    const int i = cand[c];
    const float di = dist[i];
    int rank = 0;
    for (int e = 0; e < M; ++e) {
      const int j = cand[e];
      const float dj = dist[j];
      rank += (dj < di || (dj == di && j < i)) ? 1 : 0;
    }
    if (rank < pos_num) out[i] = di;
  }
}

namespace {

// Row enumeration shared by forward and backward: row r of [0, 3 * (C + 4 + 2 K)) -> (stage, kind, channel).
struct Row {
  int stage, kind, c;   // kind 0: cls, 1: bbox, 2: keypoints
};
__device__ __forceinline__ Row row_of(int r, int C, int K2) {
  const int per = C + 4 + K2;
  Row q;
  q.stage = r / per;
  int c = r - q.stage * per;
  if (c < C) { q.kind = 0; q.c = c; }
  else if (c < C + 4) { q.kind = 1; q.c = c - C; }
  else { q.kind = 2; q.c = c - C - 4; }
  return q;
}

}  // namespace

// block (tile of 64 points, channel group, image); 256 threads = 4 waves, lane = point, waves take rows round-robin.
template <bool BACKWARD, bool TABLE>
__global__ __launch_bounds__(256) void head_loss_rows(const kgdet_head_targets t, const kgdet_head_loss_cfg cfg,
                                                      const kgdet_head_maps maps, const float *__restrict__ dsel, int gmax,
                                                      int rows_per_group, float *__restrict__ partial,
                                                      const float *__restrict__ num_total_dev,
                                                      const float *__restrict__ upstream, kgdet_head_maps grads,
                                                      const int32_t *__restrict__ table, int cap) {
  __shared__ int s_nvis[kMaxGt];
  const int N = t.H * t.W, b = blockIdx.z, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i = blockIdx.x * 64 + lane;
  const bool live = i < N;
  const int ic = min(i, N - 1);
  const ImageRow im = image_row<TABLE>(t, table, cap, b);
  const int n_gt = im.n_gt;
  const int K = t.num_keypoints, K2 = 2 * K, C = t.num_classes;
  // visible keypoints per gt (kpt_weights.sum(1) / 2 of KP3:641-644)
  for (int g = wave; g < n_gt; g += 4) {
    int cnt = visible_keypoints(t.gt_keypoints[b] + (long long)g * K * 3, K, lane, 64);
    for (int d = 32; d >= 1; d >>= 1) cnt += __shfl_xor(cnt, d);
    if (lane == 0) s_nvis[g] = cnt;
  }
  __syncthreads();
  const int a = final_assign(dsel, b, gmax, n_gt, N, ic);          // assigned gt (0: none)
  const int nvis = a > 0 ? s_nvis[a - 1] : 0;
  const float px = (float)(ic % t.W) * t.stride, py = (float)(ic / t.W) * t.stride;
  const float *gbox = t.gt_bboxes[b] + 4 * max(a - 1, 0);
  const float *gkp = t.gt_keypoints[b] + (long long)max(a - 1, 0) * K * 3;
  const bool inside = ic / t.W < im.vh && ic % t.W < im.vw;          // (a point outside is never assigned: a == 0)
  const PointLabel lab = point_label(t.gt_labels[b], a, inside, cfg.pos_weight);
  const float kp_w = nvis > 0 ? 1.0f / (float)(2 * nvis) * 4.0f : 0.0f;     // (x 4: KP3:641-644)
  const float nt = cfg.normalize_term;

  float acc[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) acc[k] = 0.f;

  const int total_rows = 3 * (C + 4 + K2);
  const int r_begin = blockIdx.y * rows_per_group, r_end = min(r_begin + rows_per_group, total_rows);
  for (int r = r_begin + wave; r < r_end; r += 4) {
    const Row q = row_of(r, C, K2);
    const int k = q.kind * 3 + q.stage;                              // loss index: cls 0-2, bbox 3-5, kpt 6-8
    if (q.kind == 0) {
      const long long off = ((long long)b * C + q.c) * N + ic;
      const float x = maps.cls[q.stage][off];
      if (!BACKWARD) {
        const float l = focal_fwd(x, lab.label, q.c, cfg.gamma[q.stage], cfg.alpha[q.stage]) * lab.weight;
        if (live) acc[k] += l;
      } else if (live) {
        const float g = upstream[k] * cfg.loss_weight[k] / num_total_dev[0];      // loss = lw * (sum / num_total)
        grads.cls[q.stage][off] = focal_bwd(x, lab.label, q.c, cfg.gamma[q.stage], cfg.alpha[q.stage]) * lab.weight * g;
      }
    } else {
      const float beta = cfg.beta[k - 3];
      float pred_raw, w;
      long long off;
      RowTarget ct;
      if (q.kind == 1) {            // offset_to_pts(y_first=False)
        off = ((long long)b * 4 + q.c) * N + ic;
        pred_raw = maps.bbox[q.stage][off];
        ct = {(q.c & 1) ? py : px, gbox[q.c], true};
        w = a > 0 ? 1.0f : 0.0f;
      } else {
        off = ((long long)b * K2 + q.c) * N + ic;
        pred_raw = maps.kpt[q.stage][off];
        ct = keypoint_target(gkp, q.c, px, py);
        w = (a > 0 && ct.on) ? kp_w : 0.0f;
      }
      const float pred = pred_raw * t.stride + ct.centre;            // offset_to_pts: pred * stride + centre
      const float x = smooth_l1_x(pred, ct.target, nt);
      if (!BACKWARD) {
        const float diff = fabsf(x), l = smooth_l1_fwd(diff, beta, diff - 0.5f * beta);
        if (live && w != 0.0f) acc[k] += l * w;
      } else if (live) {
        const float g = upstream[k] * cfg.loss_weight[k] / num_total_dev[0];
        const float gr = smooth_l1_bwd(x, beta, w, g, nt, t.stride);
        if (q.kind == 1) grads.bbox[q.stage][off] = gr; else grads.kpt[q.stage][off] = gr;
      }
    }
  }
  if (!BACKWARD) {
    const float sum = block_sums(acc);
    const long long wg = ((long long)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    if (tid < 9) partial[wg * 9 + tid] = sum;
  }
}

// one block: n_pos per image -> num_total; partials in fixed order; the nine losses
// (an image whose count is 0 -- the table route only -- has no positives and adds max(0, 1) = 1)
template <bool TABLE>
__global__ __launch_bounds__(256) void head_loss_finish(const kgdet_head_targets t, const kgdet_head_loss_cfg cfg,
                                                        const float *__restrict__ dsel, int gmax,
                                                        const float *__restrict__ partial, int num_partials,
                                                        float *__restrict__ losses, float *__restrict__ num_total_out,
                                                        const int32_t *__restrict__ table, int cap) {
  __shared__ int s_pos[4];
  __shared__ float s_total;
  const int N = t.H * t.W, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float total = 0.f;
  for (int b = 0; b < t.B; ++b) {
    int cnt = 0;
    const int n_gt = image_row<TABLE>(t, table, cap, b).n_gt;
    for (int i = tid; i < N; i += 256) cnt += final_assign(dsel, b, gmax, n_gt, N, i) > 0 ? 1 : 0;
    for (int d = 32; d >= 1; d >>= 1) cnt += __shfl_xor(cnt, d);
    __syncthreads();
    if (lane == 0) s_pos[wave] = cnt;
    __syncthreads();
    total += (float)max(s_pos[0] + s_pos[1] + s_pos[2] + s_pos[3], 1);     // point_target_kp.py:60: max(n_pos, 1) per image
  }
  if (tid == 0) { s_total = total; num_total_out[0] = total; }
  float acc[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) acc[k] = 0.f;
  for (int p = tid; p < num_partials; p += 256)
#pragma unroll
    for (int k = 0; k < 9; ++k) acc[k] += partial[(long long)p * 9 + k];
  const float s = block_sums(acc);                                        // (its barrier publishes s_total)
  if (tid < 9) losses[tid] = cfg.loss_weight[tid] * (s / s_total);        // losses/utils.py:44-48, focal_loss.py:76-82
}

}  // namespace kgdet

using namespace kgdet;

namespace {

// the launch shape and the workspace (the selections of the ABI first) of one descriptor; base == nullptr: for the size alone
struct Plan {
  int N, tiles;          // points per image, its 64-point tiles
  int rows_per_group, groups;
  float *dsel;           // [B][64][N]
  float *partial;        // [B][groups][tiles][9]
  size_t bytes;
};
Plan plan_of(const kgdet_head_targets *t, void *base) {
  Plan p;
  p.N = t->H * t->W;
  p.tiles = ceil_div(p.N, 64);
  p.rows_per_group = rows_per_group(3 * (t->num_classes + 4 + 2 * t->num_keypoints), p.tiles * t->B, 512, &p.groups);
  p.bytes = 0;
  p.dsel = take<float>(base, p.bytes, (size_t)t->B * kMaxGt * p.N);
  p.partial = take<float>(base, p.bytes, (size_t)p.tiles * p.groups * t->B * 9);
  p.bytes += 256;     // (the size the library has always named)
  return p;
}

// by_table: the counts and extents live in device memory (the *_table entry points): the by-value fields are not looked at
int head_check(const kgdet_head_targets *t, const kgdet_head_loss_cfg *cfg, bool by_table, int *gmax) {
  KGDET_CHECK_SHAPE(t && cfg, "null descriptor");
  if (int rc = check_targets(t, cfg->beta, 6, !by_table, gmax)) return rc;
  KGDET_CHECK_SHAPE(t->H > 0 && t->W > 0 && t->H * t->W <= kMaxPoints, "point grid beyond %d points", kMaxPoints);
  KGDET_CHECK_SHAPE(cfg->pos_num >= 1 && cfg->normalize_term > 0.0f, "bad assigner / normaliser");
  KGDET_CHECK_SHAPE(cfg->pos_num <= t->H * t->W, "pos_num beyond the number of points");
  for (int b = 0; b < t->B && !by_table; ++b)
    KGDET_CHECK_SHAPE(t->valid_h[b] >= 0 && t->valid_w[b] >= 0 &&
                          (long long)extent_of(t->valid_h[b], t->H) * extent_of(t->valid_w[b], t->W) >= cfg->pos_num,
                      "image %d: fewer valid points than pos_num", b);
  return KGDET_OK;
}

int head_table_check(const int32_t *table, int32_t gt_capacity) {
  KGDET_CHECK_SHAPE(table != nullptr, "null target table");
  KGDET_CHECK_SHAPE(reinterpret_cast<uintptr_t>(table) % 16 == 0, "the target table must be 16-byte aligned");
  KGDET_CHECK_SHAPE(gt_capacity >= 1 && gt_capacity <= kMaxGt, "gt_capacity %d (1..%d)", gt_capacity, kMaxGt);
  return KGDET_OK;
}

// All four entry points.  `table` == nullptr is the by-value route (select grid = the largest count), else (gt_capacity, B)
// workgroups.  Forward: select, rows, finish, writing `losses` and num_total.  Backward: the rows again, reading num_total and
// `upstream` (the gradients of the nine losses) and writing `grads`.
int head_run(bool backward, const kgdet_head_targets *t, const kgdet_head_loss_cfg *cfg, const kgdet_head_maps *maps,
             const int32_t *table, int32_t gt_capacity, float *losses, const float *upstream, float *num_total,
             const kgdet_head_maps *grads, void *workspace, size_t workspace_bytes, void *stream) {
  const int cap = gt_capacity;
  int gmax = 0;
  if (int rc = head_check(t, cfg, table != nullptr, &gmax)) return rc;
  if (table) gmax = cap;
  KGDET_CHECK_SHAPE(maps && num_total && (backward ? upstream && grads : losses != nullptr), "null pointer");
  for (int s = 0; s < 3; ++s)
    KGDET_CHECK_SHAPE(maps->cls[s] && maps->bbox[s] && maps->kpt[s] &&
                          (!backward || (grads->cls[s] && grads->bbox[s] && grads->kpt[s])),
                      "null map");
  const Plan p = plan_of(t, workspace);
  if (int rc = check_workspace("head", workspace, workspace_bytes, p.bytes)) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (!backward) {
    hipLaunchKernelGGL(table ? head_assign_select<true> : head_assign_select<false>, dim3(gmax, t->B), dim3(256),
                       (size_t)p.N * 2 * sizeof(float), st, *t, cfg->pos_num, kMaxGt, p.dsel, table, cap);
    KGDET_CHECK_LAUNCH("head_assign_select");
  }
  const auto rows = backward ? (table ? head_loss_rows<true, true> : head_loss_rows<true, false>)
                             : (table ? head_loss_rows<false, true> : head_loss_rows<false, false>);
  hipLaunchKernelGGL(rows, dim3(p.tiles, p.groups, t->B), dim3(256), 0, st, *t, *cfg, *maps, (const float *)p.dsel, kMaxGt,
                     p.rows_per_group, backward ? nullptr : p.partial, backward ? (const float *)num_total : nullptr, upstream,
                     backward ? *grads : kgdet_head_maps{}, table, cap);
  KGDET_CHECK_LAUNCH(backward ? "head_loss_rows<backward>" : "head_loss_rows<forward>");
  if (!backward) {
    hipLaunchKernelGGL(table ? head_loss_finish<true> : head_loss_finish<false>, dim3(1), dim3(256), 0, st, *t, *cfg,
                       (const float *)p.dsel, kMaxGt, (const float *)p.partial, p.tiles * p.groups * t->B, losses, num_total,
                       table, cap);
    KGDET_CHECK_LAUNCH("head_loss_finish");
  }
  return KGDET_OK;
}

}  // namespace

extern "C" {

size_t kgdet_head_loss_workspace_bytes(const kgdet_head_targets *t) {
  return t ? plan_of(t, nullptr).bytes : 0;
}

int kgdet_head_loss_forward(const kgdet_head_targets *t, const kgdet_head_loss_cfg *cfg, const kgdet_head_maps *maps,
                            float *losses, float *num_total, void *workspace, size_t workspace_bytes, void *stream) {
  return head_run(false, t, cfg, maps, nullptr, 0, losses, nullptr, num_total, nullptr, workspace, workspace_bytes, stream);
}

// (the backward calls only read num_total and the workspace)
int kgdet_head_loss_backward(const kgdet_head_targets *t, const kgdet_head_loss_cfg *cfg, const kgdet_head_maps *maps,
                             const float *grad_losses, const float *num_total, const kgdet_head_maps *grads,
                             const void *workspace, size_t workspace_bytes, void *stream) {
  return head_run(true, t, cfg, maps, nullptr, 0, nullptr, grad_losses, const_cast<float *>(num_total), grads,
                  const_cast<void *>(workspace), workspace_bytes, stream);
}

int kgdet_head_loss_forward_table(const kgdet_head_targets *t, const kgdet_head_loss_cfg *cfg, const kgdet_head_maps *maps,
                                  const int32_t *table, int32_t gt_capacity, float *losses, float *num_total, void *workspace,
                                  size_t workspace_bytes, void *stream) {
  if (int rc = head_table_check(table, gt_capacity)) return rc;
  return head_run(false, t, cfg, maps, table, gt_capacity, losses, nullptr, num_total, nullptr, workspace, workspace_bytes, stream);
}

int kgdet_head_loss_backward_table(const kgdet_head_targets *t, const kgdet_head_loss_cfg *cfg, const kgdet_head_maps *maps,
                                   const int32_t *table, int32_t gt_capacity, const float *grad_losses, const float *num_total,
                                   const kgdet_head_maps *grads, const void *workspace, size_t workspace_bytes, void *stream) {
  if (int rc = head_table_check(table, gt_capacity)) return rc;
  return head_run(true, t, cfg, maps, table, gt_capacity, nullptr, grad_losses, const_cast<float *>(num_total), grads,
                  const_cast<void *>(workspace), workspace_bytes, stream);
}

}  // extern "C"
