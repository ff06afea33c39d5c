// Target assignment + the five loss families of the serial / parallel two-stage heads over the whole pyramid (gfx950):
// five launches forward, one backward, whatever the number of levels, images and ground truths.
//
// What it replaces (five levels -- config 5: 100 x 168 ... 7 x 11 = 22 400 points per image):
//   offset_to_pts, loss_single, loss ...... mmdet/models/anchor_heads/reppoints_head_kp_serial.py:400-611 (the parallel head's are
//                                           the same code): decode, the init boxes handed to the refine assigner, five losses per level
//   PointAssigner.assign .................. mmdet/core/bbox/assigners/point_assigner.py:23-121 (init stage)
//   MaxIoUAssigner.assign_wrt_overlaps .... mmdet/core/bbox/assigners/max_iou_assigner.py:47-153 (refine stage, gt_max_assign_all)
//   bbox_overlaps ......................... mmdet/core/bbox/geometry.py:4-63 (+1 convention)
//   point_target_kp / _single ............. mmdet/core/anchor/point_target_kp.py:7-182 (targets, weights, images_to_levels, unmap)
//   FocalLoss / SmoothL1Loss reductions ... as csrc/head_loss.hip
// The boxes come in as maps (the head's points2bbox of the raw reppoints, stride units): the moment transform and its
// backward stay with the existing op, and the kernels do not depend on transform_method.
//
//   serial_init_select    block (gt, image): the gt's level, then pos_num rounds of "the nearest valid point of that level
//                         after the previous one" under the (distance, point index) order -- no per-point table; also the
//                         gt's visible-keypoint count, and the reset of its IoU maximum.
//   serial_refine_iou     thread = point, block (256-point tile of a level, image): IoU of the point's init box
//                         (centre + box * stride) with every gt; best IoU / gt, the threshold rule; per-gt maximum over the
//                         valid points: wave max, LDS, then one integer atomicMax on the bits of the non-negative IoU per
//                         gt and block (order-independent).
//   serial_assign_finish  same tiles: every gt whose maximum reaches min_pos_iou takes every valid point at exactly that
//                         IoU (recomputed by the same code: the same bits), the last gt winning; one more block per image
//                         scatters the init selections (nearest gt, the earliest on a tie).
//   serial_loss_rows      block (64-point tile of a level, channel group, image); a row = one channel of one map, lanes =
//                         points (coalesced NCHW reads): focal (C rows), smooth-L1 boxes (4 + 4) and keypoints (2 K + 2 K)
//                         on coordinates decoded in registers.  Forward skips the regression rows of a tile without a
//                         positive; backward writes their zeros without reading.
//   serial_loss_finish    one block: the tiles' positive counts (left by serial_loss_rows) per image and stage -> num_total;
//                         partials in fixed order per level.
//
// No tensor of targets or weights exists; nothing is read by the host.  Deterministic (fixed summation orders).
// The loss rows' arithmetic, the PointAssigner frame of a gt, the reductions and the host-side skeleton are loss_math.h's, shared
// with head_loss.hip; the selection rounds, the IoU assigner, the row enumeration, the decode order and the keypoint weight
// are this file's.
#include <float.h>

#include "common.h"
#include "loss_math.h"

// every operation below is one IEEE rounding: the IoU and the image-space box are then the bits an uncontracted float32
// evaluation (the torch chain) forms, and the second pass over the IoU meets the first pass's maximum exactly
#pragma clang fp contract(off)

namespace kgdet {

namespace {

constexpr int kMaxLevels = KGDET_SERIAL_MAX_LEVELS;
constexpr int kMaxPosNum = 64;
constexpr int kMaxLevelPoints = 32768;
constexpr int kFamilies = 5;   // cls, bbox_init, bbox_refine, kpt_init, kpt_refine

// the launch shape and the workspace (the three tables of the ABI first) of one descriptor; base == nullptr: for the size alone
struct Plan {
  int N;               // points per image
  int tiles64, tiles256;
  int rows_per_group, groups;
  int *a_init, *a_ref;
  float *best_iou;
  int *sel_idx;        // [B][64][pos_num] point index within the image (-1: none)
  float *sel_dist;     // [B][64][pos_num]
  int *gt_max;         // [B][64] bits of the gt's maximum IoU over the image's valid points
  int *nvis;           // [B][64] visible keypoints of the gt
  float *partial;      // [B][groups][tiles64][5]
  int *counts;         // [B][tiles64][2] positives of the tile's points: init, refine
  size_t bytes;
};

Plan plan_of(const kgdet_serial_targets *t, int pos_num, void *base) {
  Plan p = {};
  for (int l = 0; l < t->L; ++l) {
    const int n = t->H[l] * t->W[l];
    p.N += n;
    p.tiles64 += ceil_div(n, 64);
    p.tiles256 += ceil_div(n, 256);
  }
  p.rows_per_group = rows_per_group(t->num_classes + 8 + 4 * t->num_keypoints, p.tiles64 * t->B, 2048, &p.groups);
  const size_t BN = (size_t)t->B * p.N, BG = (size_t)t->B * kMaxGt;
  p.a_init = take<int>(base, p.bytes, BN);
  p.a_ref = take<int>(base, p.bytes, BN);
  p.best_iou = take<float>(base, p.bytes, BN);
  p.sel_idx = take<int>(base, p.bytes, BG * pos_num);
  p.sel_dist = take<float>(base, p.bytes, BG * pos_num);
  p.gt_max = take<int>(base, p.bytes, BG);
  p.nvis = take<int>(base, p.bytes, BG);
  p.partial = take<float>(base, p.bytes, (size_t)t->B * p.groups * p.tiles64 * kFamilies);
  p.counts = take<int>(base, p.bytes, (size_t)t->B * p.tiles64 * 2);
  return p;
}

// tile -> (level, first point of the tile within the level, offset of the level within the image)
struct Place {
  int l, first, level_off, Nl;
};
__device__ __forceinline__ Place place_of(const kgdet_serial_targets &t, int tile, int tile_points) {
  Place q = {0, 0, 0, 0};
  int off = 0;
  for (int l = 0; l < t.L; ++l) {
    const int n = t.H[l] * t.W[l], tiles = (n + tile_points - 1) / tile_points;
    if (tile < tiles || l == t.L - 1) {
      q.l = l; q.first = tile * tile_points; q.level_off = off; q.Nl = n;
      return q;
    }
    tile -= tiles;
    off += n;
  }
  return q;
}

// geometry.py bbox_overlaps(gt, box), mode 'iou', in its order of operations
__device__ __forceinline__ float iou_of(const float *__restrict__ g, float x1, float y1, float x2, float y2) {
  const float ew = fmaxf(fminf(g[2], x2) - fmaxf(g[0], x1) + 1.0f, 0.0f);
  const float eh = fmaxf(fminf(g[3], y2) - fmaxf(g[1], y1) + 1.0f, 0.0f);
  const float shared = ew * eh;
  const float area1 = (g[2] - g[0] + 1.0f) * (g[3] - g[1] + 1.0f);
  const float area2 = (x2 - x1 + 1.0f) * (y2 - y1 + 1.0f);
  return shared / (area1 + area2 - shared);
}

struct PointBox {
  float x1, y1, x2, y2;
  bool valid;
};
// the init box of point i of level q.l in image coordinates: centre + box * stride
__device__ __forceinline__ PointBox point_box(const kgdet_serial_targets &t, const kgdet_serial_maps &maps, const Place &q, int b,
                                              int i) {
  const int W = t.W[q.l], row = i / W, col = i - row * W;
  const float s = t.stride[q.l], px = (float)col * s, py = (float)row * s;
  const float *m = maps.box_init[q.l] + (long long)b * 4 * q.Nl + i;
  PointBox p;
  p.x1 = px + m[0] * s;
  p.y1 = py + m[q.Nl] * s;
  p.x2 = px + m[2 * (long long)q.Nl] * s;
  p.y2 = py + m[3 * (long long)q.Nl] * s;
  p.valid = row < extent_of(t.valid_h[b][q.l], t.H[q.l]) && col < extent_of(t.valid_w[b][q.l], W);
  return p;
}

}  // namespace

// block (g, b), 256 threads
__global__ __launch_bounds__(256) void serial_init_select(const kgdet_serial_targets t, int pos_num, float scale,
                                                          int *__restrict__ sel_idx, float *__restrict__ sel_dist,
                                                          int *__restrict__ gt_max, int *__restrict__ nvis) {
  __shared__ unsigned long long s_key[4];
  __shared__ int s_cnt;
  const int g = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (g >= t.num_gt[b]) return;
  if (tid == 0) s_cnt = 0;
  __syncthreads();
  // visible keypoints (kpt_weights.sum(1) / 2 of reppoints_head_kp_serial.py loss_single)
  const int K = t.num_keypoints;
  const int cnt = visible_keypoints(t.gt_keypoints[b] + (long long)g * K * 3, K, tid, 256);
  if (cnt) atomicAdd(&s_cnt, cnt);
  const GtFrame gt = gt_frame(t.gt_bboxes[b] + 4 * g);
  // point_assigner.py: the level of the gt
  const int lowest = (int)log2f(t.stride[0]);
  int l = (int)((log2f(gt.w / scale) + log2f(gt.h / scale)) / 2) - lowest;
  l = min(max(l, 0), t.L - 1);
  int level_off = 0;
  for (int k = 0; k < l; ++k) level_off += t.H[k] * t.W[k];
  const int W = t.W[l], Nl = t.H[l] * W;
  const int vh = extent_of(t.valid_h[b][l], t.H[l]), vw = extent_of(t.valid_w[b][l], W);
  const float s = t.stride[l];
  const long long out = ((long long)b * kMaxGt + g) * pos_num;
  unsigned long long prev = 0;
  for (int r = 0; r < pos_num; ++r) {
    unsigned long long best = ~0ull;
    for (int i = tid; i < Nl; i += 256) {
      const int row = i / W, col = i - row * W;
      if (row >= vh || col >= vw) continue;
      const float dx = ((float)col * s - gt.cx) / gt.w, dy = ((float)row * s - gt.cy) / gt.h;
      const float d = sqrtf(dx * dx + dy * dy);
      const unsigned long long key = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)i;   // (distances are >= 0)
      if ((r == 0 || key > prev) && key < best) best = key;
    }
    for (int m = 32; m >= 1; m >>= 1) {
      const unsigned long long o = __shfl_xor(best, m);
      best = o < best ? o : best;
    }
    __syncthreads();
    if (lane == 0) s_key[wave] = best;
    __syncthreads();
    best = s_key[0];
    for (int k = 1; k < 4; ++k) best = s_key[k] < best ? s_key[k] : best;
    if (tid == 0) {
      const bool none = best == ~0ull;
      sel_idx[out + r] = none ? -1 : level_off + (int)(best & 0xffffffffu);
      sel_dist[out + r] = none ? INFINITY : __uint_as_float((unsigned)(best >> 32));
    }
    prev = best;
  }
  if (tid == 0) {
    nvis[b * kMaxGt + g] = s_cnt;      // (every atomicAdd precedes the rounds' barriers)
    gt_max[b * kMaxGt + g] = 0;        // bits of 0.0f: an IoU is never below it
  }
}

// block (256-point tile, image), thread = point
__global__ __launch_bounds__(256) void serial_refine_iou(const kgdet_serial_targets t, const kgdet_serial_loss_cfg cfg,
                                                         const kgdet_serial_maps maps, int N, int *__restrict__ a_init,
                                                         int *__restrict__ a_ref, float *__restrict__ best_iou,
                                                         int *__restrict__ gt_max) {
  __shared__ int s_max[kMaxGt];
  const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
  const Place q = place_of(t, blockIdx.x, 256);
  const int i = q.first + tid, n_gt = t.num_gt[b];
  const bool live = i < q.Nl;
  if (tid < kMaxGt) s_max[tid] = 0;
  __syncthreads();
  const PointBox p = point_box(t, maps, q, b, min(i, q.Nl - 1));
  const bool counted = live && p.valid;
  float best = -INFINITY;
  int bg = 0;
  for (int g = 0; g < n_gt; ++g) {
    const float v = iou_of(t.gt_bboxes[b] + 4 * g, p.x1, p.y1, p.x2, p.y2);
    if (v > best) { best = v; bg = g; }                      // (the lowest gt keeps equal values)
    int m = counted ? __float_as_int(v) : 0;                 // (non-negative floats order as their bits)
    for (int d = 32; d >= 1; d >>= 1) m = max(m, __shfl_xor(m, d));
    if (lane == 0) atomicMax(&s_max[g], m);
  }
  if (live) {
    // max_iou_assigner.py: -1, then 0 inside the negative range, then gt + 1 from pos_iou_thr on
    int a = -1;
    if (best >= cfg.neg_lo && best < cfg.neg_hi) a = 0;
    if (best >= cfg.pos_iou_thr) a = bg + 1;
    const long long n = (long long)b * N + q.level_off + i;
    a_ref[n] = p.valid ? a : 0;
    best_iou[n] = p.valid ? best : -2.0f;
    a_init[n] = 0;
  }
  __syncthreads();
  if (tid < n_gt) atomicMax(&gt_max[b * kMaxGt + tid], s_max[tid]);
}

// blocks [0, tiles256): the gt-max step of their points; block tiles256: the init scatter of the image
__global__ __launch_bounds__(256) void serial_assign_finish(const kgdet_serial_targets t, const kgdet_serial_loss_cfg cfg,
                                                            const kgdet_serial_maps maps, int N, int tiles256,
                                                            const int *__restrict__ sel_idx, const float *__restrict__ sel_dist,
                                                            const int *__restrict__ gt_max, int *__restrict__ a_init,
                                                            int *__restrict__ a_ref) {
  const int b = blockIdx.y, tid = threadIdx.x, n_gt = t.num_gt[b];
  if ((int)blockIdx.x == tiles256) {
    // point_assigner.py: `min_dist < assigned_gt_dist[point_index]`, gts in order: the nearest, the earliest on a tie
    // (all pairs of the image's E = num_gt * pos_num selections in one workgroup: 2 .. 64 for the configs' pos_num = 1, 4096^2
    //  comparisons at both limits -- stated in the header)
    const int E = n_gt * cfg.pos_num;
    const int *idx = sel_idx + (long long)b * kMaxGt * cfg.pos_num;
    const float *dist = sel_dist + (long long)b * kMaxGt * cfg.pos_num;
    for (int e = tid; e < E; e += 256) {
      const int n = idx[e];
      if (n < 0 || n >= N) continue;
      const float d = dist[e];
      bool wins = true;
      for (int o = 0; o < E; ++o)
        if (idx[o] == n && (dist[o] < d || (dist[o] == d && o / cfg.pos_num < e / cfg.pos_num))) wins = false;
      if (wins) a_init[(long long)b * N + n] = e / cfg.pos_num + 1;
    }
    return;
  }
  const Place q = place_of(t, blockIdx.x, 256);
  const int i = q.first + tid;
  if (i >= q.Nl) return;
  const PointBox p = point_box(t, maps, q, b, i);
  if (!p.valid) return;
  int last = 0;
  for (int g = 0; g < n_gt; ++g) {
    const float top = __int_as_float(gt_max[b * kMaxGt + g]);
    if (top >= cfg.min_pos_iou && iou_of(t.gt_bboxes[b] + 4 * g, p.x1, p.y1, p.x2, p.y2) == top) last = g + 1;
  }
  if (last > 0) a_ref[(long long)b * N + q.level_off + i] = last;
}

// block (tile of 64 points of one level, channel group, image); 256 threads = 4 waves, lane = point, waves take rows
// round-robin.  Rows: [0, C) cls, 4 bbox_init, 4 bbox_refine, 2 K kpt_init, 2 K kpt_refine.
template <bool BACKWARD>
__global__ __launch_bounds__(256) void serial_loss_rows(const kgdet_serial_targets t, const kgdet_serial_loss_cfg cfg,
                                                        const kgdet_serial_maps maps, int N, int rows_per_group,
                                                        const int *__restrict__ a_init, const int *__restrict__ a_ref,
                                                        const int *__restrict__ nvis, float *__restrict__ partial,
                                                        int *__restrict__ counts,
                                                        const float *__restrict__ num_total, const float *__restrict__ upstream,
                                                        kgdet_serial_maps grads) {
  const int b = blockIdx.z, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const Place q = place_of(t, blockIdx.x, 64);
  const int l = q.l, Nl = q.Nl, i = q.first + lane;
  const bool live = i < Nl;
  const int ic = min(i, Nl - 1);
  const int K = t.num_keypoints, K2 = 2 * K, C = t.num_classes;
  const int W = t.W[l], row = ic / W, col = ic - row * W;
  const float s = t.stride[l], px = (float)col * s, py = (float)row * s;
  const long long n = (long long)b * N + q.level_off + ic;
  // (clamped: a workspace that no forward call filled must not index beyond the ground-truth tables)
  const int n_gt = t.num_gt[b];
  const int ai = live ? min(max(a_init[n], 0), n_gt) : 0, ar = live ? min(max(a_ref[n], -1), n_gt) : 0;
  const bool inside = row < extent_of(t.valid_h[b][l], t.H[l]) && col < extent_of(t.valid_w[b][l], W);
  const PointLabel lab = point_label(t.gt_labels[b], ar, inside, cfg.pos_weight);
  const unsigned long long pos_i = __ballot(ai > 0), pos_r = __ballot(ar > 0);
  const bool any_i = pos_i != 0, any_r = pos_r != 0;
  if (!BACKWARD && blockIdx.y == 0 && tid == 0) {        // the tile's positives, for num_total (serial_loss_finish)
    int *c = counts + ((long long)b * gridDim.x + blockIdx.x) * 2;
    c[0] = __popcll(pos_i);
    c[1] = __popcll(pos_r);
  }
  const float nt = cfg.point_base_scale * s;

  float acc[kFamilies];
#pragma unroll
  for (int k = 0; k < kFamilies; ++k) acc[k] = 0.f;

  const int rows = C + 8 + 2 * K2;
  const int r_begin = blockIdx.y * rows_per_group, r_end = min(r_begin + rows_per_group, rows);
  for (int r = r_begin + wave; r < r_end; r += 4) {
    if (r < C) {
      const long long off = ((long long)b * C + r) * Nl + ic;
      const float x = maps.cls[l][off];
      if (!BACKWARD) {
        const float v = focal_fwd(x, lab.label, r, cfg.gamma, cfg.alpha) * lab.weight;
        if (live) acc[0] += v;
      } else if (live) {
        const float g = upstream[0 * t.L + l] * cfg.loss_weight[0] / num_total[1];      // loss = lw * (sum / num_total)
        grads.cls[l][off] = focal_bwd(x, lab.label, r, cfg.gamma, cfg.alpha) * lab.weight * g;
      }
      continue;
    }
    int c = r - C, k;              // family k: 1 bbox_init, 2 bbox_refine, 3 kpt_init, 4 kpt_refine
    if (c < 8) { k = 1 + (c >> 2); c &= 3; }
    else { c -= 8; k = 3 + (c >= K2); c -= (k - 3) * K2; }
    const bool init = (k == 1 || k == 3), box = k < 3;
    const int a = init ? ai : ar;
    const long long off = ((long long)b * (box ? 4 : K2) + c) * Nl + ic;
    float *const *src = k == 1 ? maps.box_init : k == 2 ? maps.box_refine : k == 3 ? maps.kpt_init : maps.kpt_refine;
    float *const *dst = k == 1 ? grads.box_init : k == 2 ? grads.box_refine : k == 3 ? grads.kpt_init : grads.kpt_refine;
    if (!(init ? any_i : any_r)) {                       // a tile without a positive of the stage: weight 0 throughout
      if (BACKWARD && live) dst[l][off] = 0.0f;
      continue;
    }
    const float pred_raw = src[l][off];
    const int gi = max(a - 1, 0), nv = (a > 0 && !box) ? nvis[b * kMaxGt + gi] : 0;
    const RowTarget ct = box ? RowTarget{(c & 1) ? py : px, t.gt_bboxes[b][4 * gi + c], true}
                             : keypoint_target(t.gt_keypoints[b] + (long long)gi * K * 3, c, px, py);
    // (no x 4 on the keypoint weight here: reppoints_head_kp_serial.py)
    const float w = box ? (a > 0 ? 1.0f : 0.0f) : ((nv > 0 && ct.on) ? 1.0f / (float)(2 * nv) : 0.0f);
    // boxes: centre + box * stride as the assigner saw it; keypoints: pred * stride + centre (offset_to_pts) -- the same sum
    const float pred = ct.centre + pred_raw * s;
    const float x = smooth_l1_x(pred, ct.target, nt);
    const float beta = cfg.beta[k - 1];
    if (!BACKWARD) {
      const float diff = fabsf(x), v = smooth_l1_fwd(diff, beta, diff - 0.5f * beta);
      if (live && w != 0.0f) acc[k] += v * w;
    } else if (live) {
      const float g = upstream[k * t.L + l] * cfg.loss_weight[k] / num_total[init ? 0 : 1];
      dst[l][off] = smooth_l1_bwd(x, beta, w, g, nt, s);
    }
  }
  if (!BACKWARD) {
    const float sum = block_sums(acc);
    const long long wg = ((long long)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    if (tid < kFamilies) partial[wg * kFamilies + tid] = sum;
  }
}

// one block: positives per image and stage -> num_total[2]; partials in fixed order per level; 5 * L losses
__global__ __launch_bounds__(256) void serial_loss_finish(const kgdet_serial_targets t, const kgdet_serial_loss_cfg cfg,
                                                          int tiles64, int groups, const int *__restrict__ counts,
                                                          const float *__restrict__ partial,
                                                          float *__restrict__ losses, float *__restrict__ num_total_out) {
  __shared__ int s_pos[4][2];
  __shared__ float s_total[2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float total_i = 0.f, total_r = 0.f;
  for (int b = 0; b < t.B; ++b) {
    int ci = 0, cr = 0;
    for (int i = tid; i < tiles64; i += 256) {
      ci += counts[((long long)b * tiles64 + i) * 2];
      cr += counts[((long long)b * tiles64 + i) * 2 + 1];
    }
    for (int d = 32; d >= 1; d >>= 1) { ci += __shfl_xor(ci, d); cr += __shfl_xor(cr, d); }
    __syncthreads();
    if (lane == 0) { s_pos[wave][0] = ci; s_pos[wave][1] = cr; }
    __syncthreads();
    // point_target_kp.py: max(n_pos, 1) per image
    total_i += (float)max(s_pos[0][0] + s_pos[1][0] + s_pos[2][0] + s_pos[3][0], 1);
    total_r += (float)max(s_pos[0][1] + s_pos[1][1] + s_pos[2][1] + s_pos[3][1], 1);
  }
  if (tid == 0) {
    s_total[0] = num_total_out[0] = total_i;
    s_total[1] = num_total_out[1] = total_r;
  }
  int tile0 = 0;
  for (int l = 0; l < t.L; ++l) {
    const int tl = (t.H[l] * t.W[l] + 63) / 64, count = t.B * groups * tl;
    float acc[kFamilies];
#pragma unroll
    for (int k = 0; k < kFamilies; ++k) acc[k] = 0.f;
    for (int p = tid; p < count; p += 256) {
      const long long wg = (long long)(p / tl) * tiles64 + tile0 + p % tl;      // (image, group) major, the level's tiles
#pragma unroll
      for (int k = 0; k < kFamilies; ++k) acc[k] += partial[wg * kFamilies + k];
    }
    __syncthreads();                                       // (the previous level's sums have been read; s_total is written)
    const float sum = block_sums(acc);
    if (tid < kFamilies) {
      const bool init = tid == 1 || tid == 3;
      losses[tid * t.L + l] = cfg.loss_weight[tid] * (sum / s_total[init ? 0 : 1]);    // losses/utils.py, focal_loss.py
    }
    tile0 += tl;
  }
}

}  // namespace kgdet

using namespace kgdet;

namespace {

int serial_check(const kgdet_serial_targets *t, const kgdet_serial_loss_cfg *cfg, int *gmax) {
  KGDET_CHECK_SHAPE(t && cfg, "null descriptor");
  KGDET_CHECK_SHAPE(t->L >= 1 && t->L <= kMaxLevels, "1..%d pyramid levels", kMaxLevels);
  if (int rc = check_targets(t, cfg->beta, 4, true, gmax)) return rc;
  KGDET_CHECK_SHAPE(cfg->pos_num >= 1 && cfg->pos_num <= kMaxPosNum, "pos_num 1..%d", kMaxPosNum);
  KGDET_CHECK_SHAPE(cfg->scale > 0.0f && cfg->point_base_scale > 0.0f, "bad assigner scale / normaliser");
  for (int l = 0; l < t->L; ++l) {
    KGDET_CHECK_SHAPE(t->H[l] > 0 && t->W[l] > 0 && (long long)t->H[l] * t->W[l] <= kMaxLevelPoints,
                      "level %d: point grid beyond %d points", l, kMaxLevelPoints);
    int e = 0;
    const float m = frexpf(t->stride[l], &e);
    KGDET_CHECK_SHAPE(t->stride[l] >= 1.0f && m == 0.5f && (l == 0 || t->stride[l] == 2.0f * t->stride[l - 1]),
                      "strides must be consecutive powers of two");
    for (int b = 0; b < t->B; ++b)
      KGDET_CHECK_SHAPE(t->valid_h[b][l] >= 0 && t->valid_w[b][l] >= 0 &&
                            (long long)extent_of(t->valid_h[b][l], t->H[l]) * extent_of(t->valid_w[b][l], t->W[l]) >= cfg->pos_num,
                        "image %d, level %d: fewer valid points than pos_num", b, l);
  }
  return KGDET_OK;
}

int serial_maps_check(const kgdet_serial_targets *t, const kgdet_serial_maps *m, const char *what) {
  KGDET_CHECK_SHAPE(m, "null %s descriptor", what);
  for (int l = 0; l < t->L; ++l)
    KGDET_CHECK_SHAPE(m->cls[l] && m->box_init[l] && m->box_refine[l] && m->kpt_init[l] && m->kpt_refine[l], "null %s (level %d)",
                      what, l);
  return KGDET_OK;
}

// Both entry points.  Forward: select, IoU, assign, rows, finish, writing `losses` and num_total.  Backward: the rows again,
// reading num_total and `upstream` (the gradients of the 5 * L losses) and writing `grads`.
int serial_run(bool backward, const kgdet_serial_targets *t, const kgdet_serial_loss_cfg *cfg, const kgdet_serial_maps *maps,
               float *losses, const float *upstream, float *num_total, const kgdet_serial_maps *grads, void *workspace,
               size_t workspace_bytes, void *stream) {
  int gmax = 0;
  if (int rc = serial_check(t, cfg, &gmax)) return rc;
  if (int rc = serial_maps_check(t, maps, "prediction map")) return rc;
  if (backward)
    if (int rc = serial_maps_check(t, grads, "gradient map")) return rc;
  KGDET_CHECK_SHAPE(num_total && (backward ? upstream != nullptr : losses != nullptr), "null pointer");
  const Plan p = plan_of(t, cfg->pos_num, workspace);
  if (int rc = check_workspace("serial", workspace, workspace_bytes, p.bytes)) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (!backward) {
    hipLaunchKernelGGL(serial_init_select, dim3(gmax, t->B), dim3(256), 0, st, *t, cfg->pos_num, cfg->scale, p.sel_idx,
                       p.sel_dist, p.gt_max, p.nvis);
    KGDET_CHECK_LAUNCH("serial_init_select");
    hipLaunchKernelGGL(serial_refine_iou, dim3(p.tiles256, t->B), dim3(256), 0, st, *t, *cfg, *maps, p.N, p.a_init, p.a_ref,
                       p.best_iou, p.gt_max);
    KGDET_CHECK_LAUNCH("serial_refine_iou");
    hipLaunchKernelGGL(serial_assign_finish, dim3(p.tiles256 + 1, t->B), dim3(256), 0, st, *t, *cfg, *maps, p.N, p.tiles256,
                       (const int *)p.sel_idx, (const float *)p.sel_dist, (const int *)p.gt_max, p.a_init, p.a_ref);
    KGDET_CHECK_LAUNCH("serial_assign_finish");
  }
  hipLaunchKernelGGL(backward ? serial_loss_rows<true> : serial_loss_rows<false>, dim3(p.tiles64, p.groups, t->B),
                     dim3(256), 0, st, *t, *cfg, *maps, p.N, p.rows_per_group, (const int *)p.a_init, (const int *)p.a_ref,
                     (const int *)p.nvis, backward ? nullptr : p.partial, backward ? nullptr : p.counts,
                     backward ? (const float *)num_total : nullptr, upstream,
                     backward ? *grads : kgdet_serial_maps{});
  KGDET_CHECK_LAUNCH(backward ? "serial_loss_rows<backward>" : "serial_loss_rows<forward>");
  if (!backward) {
    hipLaunchKernelGGL(serial_loss_finish, dim3(1), dim3(256), 0, st, *t, *cfg, p.tiles64, p.groups, (const int *)p.counts,
                       (const float *)p.partial, losses, num_total);
    KGDET_CHECK_LAUNCH("serial_loss_finish");
  }
  return KGDET_OK;
}

}  // namespace

extern "C" {

size_t kgdet_serial_loss_workspace_bytes(const kgdet_serial_targets *t, const kgdet_serial_loss_cfg *cfg) {
  int gmax = 0;
  if (serial_check(t, cfg, &gmax)) return 0;
  return plan_of(t, cfg->pos_num, nullptr).bytes;
}

int kgdet_serial_loss_forward(const kgdet_serial_targets *t, const kgdet_serial_loss_cfg *cfg, const kgdet_serial_maps *maps,
                              float *losses, float *num_total, void *workspace, size_t workspace_bytes, void *stream) {
  return serial_run(false, t, cfg, maps, losses, nullptr, num_total, nullptr, workspace, workspace_bytes, stream);
}

// (the backward call only reads num_total and the workspace)
int kgdet_serial_loss_backward(const kgdet_serial_targets *t, const kgdet_serial_loss_cfg *cfg, const kgdet_serial_maps *maps,
                               const float *grad_losses, const float *num_total, const kgdet_serial_maps *grads,
                               const void *workspace, size_t workspace_bytes, void *stream) {
  return serial_run(true, t, cfg, maps, nullptr, grad_losses, const_cast<float *>(num_total), grads,
                    const_cast<void *>(workspace), workspace_bytes, stream);
}

}  // extern "C"
