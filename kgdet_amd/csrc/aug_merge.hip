// Test-time augmentation merge (RepPointsDetectorKp.aug_test, kgdet_amd/detector.py) for gfx950: every augmentation's
// decoded candidates mapped back to the original image frame and concatenated, in one launch per image.
//
// Per augmentation a (img_shape width w, scalar scale_factor s), row by row in augmentation order:
//   flip:  x1' = (w - x2) - 1, x2' = (w - x1) - 1 (y unchanged); each landmark x' = (w - x) - 1 and the landmarks are
//          GATHERED: out slot k takes input slot perm[k] (perm = flip_indices[0::2] // 2; the Python callers only pass
//          involutions, for which a scatter would give the same -- the C ABI takes any permutation and gathers)
//   then:  box coordinates and landmark x / y times (1 / s) -- torch on the GPU divides by a python float as x * (1 / s)
//          with the reciprocal taken in double and rounded to fp32 once, so the detector's restatement gives these bits on
//          GPU tensors; on CPU tensors it divides truly and may differ in the last bit (both within 2 * 2^-24 |x / s| of
//          the quotient); visibility and scores are copied bit for bit.
// Contraction is off: every expression is rounded in the order written, as torch evaluates it op by op.
//
// Work split: one workgroup per tile of kTileRows rows of ONE augmentation.  The tile's landmark rows (K * 3 floats each,
// contiguous in the source and in the output) are staged through LDS: dwordx4 reads of the source range, the
// permutation gathered from LDS, dwordx4 writes of the output range (scalar only for the head / tail floats before / after
// a 16-byte boundary: a row is 3528 bytes for K = 294, so an odd row offset leaves the range 8-byte aligned).  Boxes and
// score rows are tiny next to the landmarks (16 + 56 bytes against 3528 per row) and are copied with dword accesses.
#include "common.h"

#pragma clang fp contract(off)

namespace kgdet {

namespace {

constexpr int kAugThreads = 256;
constexpr int kTileRows = 8;
constexpr int kAugMaxK = 1024;      // landmarks per row: the permutation lives in LDS
constexpr int kAugTileFloats = 8192;  // 32 KiB of LDS stage: 8 rows of 294 landmarks, at least 2 rows of kAugMaxK
constexpr int kAugMaxSegs = 16;

struct AugArgs {
  const float *boxes[kAugMaxSegs];
  const float *scores[kAugMaxSegs];
  const float *kpts[kAugMaxSegs];
  int row0[kAugMaxSegs + 1];        // first output row of each augmentation
  int tile0[kAugMaxSegs + 1];       // first tile (workgroup) of each augmentation
  float img_w[kAugMaxSegs];
  float inv[kAugMaxSegs];           // (float)(1.0 / scale), rounded on the host
  int flip[kAugMaxSegs];
  int A;
};

__device__ __forceinline__ float map_kpt(float v, int c, bool flip, float w, float inv) {
  if (c == 2) return v;
  if (c == 0 && flip) v = (w - v) - 1.0f;
  return v * inv;
}

// floats [0, len) of src (global) -> dst (LDS); dwordx4 for every 16-byte-aligned group
__device__ __forceinline__ void stage_in(const float *__restrict__ src, int len, float *dst) {
  const int head = min(len, (int)(((16 - ((uintptr_t)src & 15)) & 15) >> 2));
  const int body = (len - head) >> 2;
  for (int i = threadIdx.x; i < head; i += kAugThreads) dst[i] = src[i];
  const float4 *s4 = reinterpret_cast<const float4 *>(src + head);
  for (int q = threadIdx.x; q < body; q += kAugThreads) {
    const float4 v = s4[q];
    float *d = dst + head + 4 * q;
    d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
  }
  for (int i = head + 4 * body + threadIdx.x; i < len; i += kAugThreads) dst[i] = src[i];
}

__global__ __launch_bounds__(kAugThreads) void aug_merge_kernel(const AugArgs args, int S, int K,
                                                                const int *__restrict__ perm,
                                                                float *__restrict__ out_boxes,
                                                                float *__restrict__ out_scores,
                                                                float *__restrict__ out_kpts) {
  __shared__ int sperm[kAugMaxK];
  __shared__ float tile[kAugTileFloats];
  const int tid = threadIdx.x, t = blockIdx.x;
  int a = 0;
  while (t >= args.tile0[a + 1]) ++a;        // (an empty augmentation owns no tile)
  const int n = args.row0[a + 1] - args.row0[a];
  const int r0 = (t - args.tile0[a]) * kTileRows;
  const int rows = min(kTileRows, n - r0);
  const int orow = args.row0[a] + r0;
  const bool flip = args.flip[a] != 0;
  const float w = args.img_w[a], inv = args.inv[a];

  // boxes
  const float *bsrc = args.boxes[a] + (long long)r0 * 4;
  float *bdst = out_boxes + (long long)orow * 4;
  for (int i = tid; i < rows * 4; i += kAugThreads) {
    const int c = i & 3;
    float v;
    if (flip && (c & 1) == 0) v = (w - bsrc[i ^ 2]) - 1.0f;   // x1 <- x2, x2 <- x1
    else v = bsrc[i];
    bdst[i] = v * inv;
  }
  // scores: copied
  const float *ssrc = args.scores[a] + (long long)r0 * S;
  float *sdst = out_scores + (long long)orow * S;
  for (int i = tid; i < rows * S; i += kAugThreads) sdst[i] = ssrc[i];

  // landmarks: the tile's rows through LDS in chunks of whole rows that fit
  const int KF = K * 3;
  const int chunk_rows = min(rows, kAugTileFloats / KF);
  if (flip)
    for (int i = tid; i < K; i += kAugThreads) sperm[i] = perm[i];
  for (int c0 = 0; c0 < rows; c0 += chunk_rows) {
    const int cr = min(chunk_rows, rows - c0);
    const int len = cr * KF;
    __syncthreads();                                          // (previous chunk's readers done; sperm written)
    stage_in(args.kpts[a] + (long long)(r0 + c0) * KF, len, tile);
    __syncthreads();
    float *dst = out_kpts + (long long)(orow + c0) * KF;
    const int head = min(len, (int)(((16 - ((uintptr_t)dst & 15)) & 15) >> 2));
    const int body = (len - head) >> 2;
    auto value = [&](int e) {                                 // output float e of the chunk
      const int lr = e / KF, wi = e - lr * KF, j = wi / 3, c = wi - 3 * j;
      const int src = lr * KF + (flip ? sperm[j] : j) * 3 + c;
      return map_kpt(tile[src], c, flip, w, inv);
    };
    for (int i = tid; i < head; i += kAugThreads) dst[i] = value(i);
    float4 *d4 = reinterpret_cast<float4 *>(dst + head);
    for (int q = tid; q < body; q += kAugThreads) {
      const int e = head + 4 * q;
      d4[q] = make_float4(value(e), value(e + 1), value(e + 2), value(e + 3));
    }
    for (int i = head + 4 * body + tid; i < len; i += kAugThreads) dst[i] = value(i);
  }
}

}  // namespace

}  // namespace kgdet

using namespace kgdet;

extern "C" {

int kgdet_aug_merge(const kgdet_aug_segment *segs, int32_t A, int32_t score_stride, int32_t K, const int32_t *kpt_perm,
                    float *out_boxes, float *out_scores, float *out_kpts, void *stream) {
  if (A > kAugMaxSegs) {
    set_error("aug_merge: %d augmentations (limit %d)", A, kAugMaxSegs);
    return KGDET_E_UNSUPPORTED;
  }
  KGDET_CHECK_SHAPE(A >= 1 && segs, "aug_merge: need 1..%d segments", kAugMaxSegs);
  KGDET_CHECK_SHAPE(score_stride >= 1 && K >= 1 && K <= kAugMaxK, "aug_merge: bad sizes (1 <= K <= %d)", kAugMaxK);
  AugArgs args = {};
  long long rows = 0, tiles = 0;
  bool any_flip = false;
  for (int a = 0; a < A; ++a) {
    const kgdet_aug_segment &s = segs[a];
    KGDET_CHECK_SHAPE(s.n >= 0, "aug_merge: negative row count");
    KGDET_CHECK_SHAPE(s.n == 0 || (s.boxes && s.scores && s.kpts), "aug_merge: null pointer");
    KGDET_CHECK_SHAPE(s.scale > 0.0, "aug_merge: scale_factor must be positive");
    args.boxes[a] = s.boxes; args.scores[a] = s.scores; args.kpts[a] = s.kpts;
    args.row0[a] = (int)rows; args.tile0[a] = (int)tiles;
    args.img_w[a] = s.img_w;
    args.inv[a] = (float)(1.0 / s.scale);
    args.flip[a] = s.flip ? 1 : 0;
    any_flip = any_flip || (s.flip && s.n > 0);
    rows += s.n;
    tiles += (s.n + kTileRows - 1) / kTileRows;
  }
  args.row0[A] = (int)rows; args.tile0[A] = (int)tiles;
  args.A = A;
  KGDET_CHECK_SHAPE(rows * K * 3 < (1ll << 31) && rows * score_stride < (1ll << 31), "aug_merge: too many rows");
  if (tiles == 0) return KGDET_OK;
  KGDET_CHECK_SHAPE(out_boxes && out_scores && out_kpts, "aug_merge: null pointer");
  KGDET_CHECK_SHAPE(!any_flip || kpt_perm, "aug_merge: a flipped augmentation needs the landmark permutation");
  hipLaunchKernelGGL(aug_merge_kernel, dim3((unsigned)tiles), dim3(kAugThreads), 0, (hipStream_t)stream, args,
                     score_stride, K, (const int *)kpt_perm, out_boxes, out_scores, out_kpts);
  KGDET_CHECK_LAUNCH("aug_merge_kernel");
  return KGDET_OK;
}

}  // extern "C"
