// Image preprocessing (datasets.ImageTransform on the device) for gfx950: a batch of raw uint8 HWC images ->
// the detector's float32 [3, out_h, out_w] input slots in ONE launch: bilinear resize (half-pixel centres, edge-clamped, no
// antialias), quantisation to a grey level, normalisation, optional horizontal flip, zero padding.
//
// The arithmetic is the one of kgdet_amd/preprocess.py::image_transform_restatement, bit for bit.  Per output pixel, with d
// its index in the UN-flipped resized image (a flipped job writes column new_w - 1 - d):
//   src = max(scale * (d + 0.5f) - 0.5f, 0)         (multiply and subtract rounded separately)
//   i0 = min((int)src, n - 1), i1 = i0 + (i0 < n - 1), l1 = src - i0, l0 = 1 - l1       (the min never binds: it keeps a
//                                                                   read inside the source whatever the scale holds)
//   v = ly0 * (lx0 * a + lx1 * b) + ly1 * (lx0 * c + lx1 * d)      (every product and sum rounded to fp32 on its own)
//   q = (uint8) clamp(rintf(v), 0, 255)             (half to even);  out = norm_lut[channel][q]
// Contraction is off: an FMA would change the bits.
//
// Work split: a capped grid strides over (slot rows x jobs); one workgroup takes one output row at a time (the row's y taps
// are uniform), one thread produces 4 consecutive x for all three channel planes and stores them as one dwordx4 per plane
// wherever the destination row allows (the groups are laid on the row's 16-byte grid; the head / tail groups and rows of a
// destination whose planes are not 16-byte congruent store dwords).  Rows below new_h and columns right of new_w are
// written as zeros without touching the source.  The two source rows are read straight through the cache (byte loads):
// neighbouring lanes share lines, the next output row re-reads the same or the adjacent source row from L1 / L2, and a
// staged row segment would have a length that depends on the job's scale.  The 3 KiB normalisation table sits in LDS.
#include "common.h"

#pragma clang fp contract(off)

namespace kgdet {

namespace {

constexpr int kPreThreads = 256;
constexpr int kPreMaxJobs = KGDET_PREPROC_MAX_JOBS;
constexpr int kPreMaxBlocks = 2048;       // 256 CUs x 8 workgroups: the memory-bound grid cap
constexpr int kPreMaxExtent = 1 << 20;    // per source / output side: (d + 0.5f) and the taps are exact far beyond it

struct PreArgs {
  kgdet_preproc_job job[kPreMaxJobs];
  int row0[kPreMaxJobs + 1];              // first (global) row of each job's slot
  int n;
};

struct Tap {
  int i0, i1;
  float l0, l1;
};

__device__ __forceinline__ Tap make_tap(int d, float scale, int n) {
  const float src = fmaxf(scale * ((float)d + 0.5f) - 0.5f, 0.0f);
  Tap t;
  t.i0 = (int)fminf(src, (float)(n - 1));             // == min((int)src, n - 1), without an out-of-range conversion
  t.i1 = t.i0 + (t.i0 < n - 1 ? 1 : 0);
  t.l1 = src - (float)t.i0;
  t.l0 = 1.0f - t.l1;
  return t;
}

__global__ __launch_bounds__(kPreThreads) void image_preprocess_kernel(const PreArgs args,
                                                                       const float *__restrict__ norm_lut,
                                                                       int reverse_channels) {
  __shared__ float lut[3 * 256];
  const int tid = threadIdx.x;
  for (int i = tid; i < 3 * 256; i += kPreThreads) lut[i] = norm_lut[i];
  __syncthreads();

  const int total = args.row0[args.n];
  int j = 0;
  for (int r = blockIdx.x; r < total; r += gridDim.x) {
    while (r >= args.row0[j + 1]) ++j;                       // (r only grows: j never steps back)
    const kgdet_preproc_job &J = args.job[j];
    const int y = r - args.row0[j];
    const int new_w = J.new_w, out_w = J.out_w, src_w = J.src_w;
    const long long cs = J.dst_channel_stride;
    float *__restrict__ row = J.dst + (long long)y * J.dst_row_stride;
    const bool live_row = y < J.new_h;
    const bool flip = J.flip != 0;
    const float scale_x = J.scale_x;
    Tap ty = {0, 0, 0.0f, 0.0f};
    if (live_row) ty = make_tap(y, J.scale_y, J.src_h);
    const uint8_t *__restrict__ s0 = J.src + (long long)ty.i0 * J.src_row_bytes;
    const uint8_t *__restrict__ s1 = J.src + (long long)ty.i1 * J.src_row_bytes;

    // groups of 4 x on the row's 16-byte grid: group g covers [start + 4g, start + 4g + 4), start in {-3 .. 0}
    const bool vec = (cs & 3) == 0;
    const int head = vec ? (int)(((16 - ((uintptr_t)row & 15)) & 15) >> 2) : 0;
    const int start = head ? head - 4 : 0;
    const int groups = (out_w - start + 3) >> 2;
    for (int g = tid; g < groups; g += kPreThreads) {
      const int x0 = start + 4 * g;
      float v[3][4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int x = x0 + k;
        if (live_row && x >= 0 && x < new_w) {
          const Tap tx = make_tap(flip ? new_w - 1 - x : x, scale_x, src_w);
          const uint8_t *p00 = s0 + 3 * tx.i0, *p01 = s0 + 3 * tx.i1;
          const uint8_t *p10 = s1 + 3 * tx.i0, *p11 = s1 + 3 * tx.i1;
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const int sc = reverse_channels ? 2 - c : c;
            const float top = tx.l0 * (float)p00[sc] + tx.l1 * (float)p01[sc];
            const float bot = tx.l0 * (float)p10[sc] + tx.l1 * (float)p11[sc];
            const float val = ty.l0 * top + ty.l1 * bot;
            const int q = (int)fminf(fmaxf(rintf(val), 0.0f), 255.0f);
            v[c][k] = lut[c * 256 + q];
          }
        } else {
          v[0][k] = 0.0f; v[1][k] = 0.0f; v[2][k] = 0.0f;
        }
      }
      if (vec && x0 >= 0 && x0 + 4 <= out_w) {
#pragma unroll
        for (int c = 0; c < 3; ++c)
          *reinterpret_cast<float4 *>(row + c * cs + x0) = make_float4(v[c][0], v[c][1], v[c][2], v[c][3]);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int x = x0 + k;
          if (x >= 0 && x < out_w) {
#pragma unroll
            for (int c = 0; c < 3; ++c) row[c * cs + x] = v[c][k];
          }
        }
      }
    }
  }
}

}  // namespace

}  // namespace kgdet

using namespace kgdet;

extern "C" {

int kgdet_image_preprocess(const kgdet_preproc_job *jobs, int32_t n_jobs, const float *norm_lut,
                           int32_t reverse_channels, void *stream) {
  KGDET_CHECK_SHAPE(n_jobs >= 0, "image_preprocess: negative job count");
  if (n_jobs == 0) return KGDET_OK;
  if (n_jobs > kPreMaxJobs) {
    set_error("image_preprocess: %d jobs in one launch (limit %d)", n_jobs, kPreMaxJobs);
    return KGDET_E_UNSUPPORTED;
  }
  KGDET_CHECK_SHAPE(jobs && norm_lut, "image_preprocess: null pointer");
  PreArgs args = {};
  long long rows = 0;
  for (int j = 0; j < n_jobs; ++j) {
    const kgdet_preproc_job &J = jobs[j];
    KGDET_CHECK_SHAPE(J.src && J.dst, "image_preprocess: job %d: null pointer", j);
    KGDET_CHECK_SHAPE(((uintptr_t)J.dst & 3) == 0, "image_preprocess: job %d: dst is not 4-byte aligned", j);
    KGDET_CHECK_SHAPE(J.src_h >= 1 && J.src_w >= 1 && J.src_h <= kPreMaxExtent && J.src_w <= kPreMaxExtent,
                      "image_preprocess: job %d: source size %d x %d outside 1..%d", j, J.src_h, J.src_w, kPreMaxExtent);
    KGDET_CHECK_SHAPE((long long)J.src_row_bytes >= 3ll * J.src_w,
                      "image_preprocess: job %d: source row pitch %d below 3 * %d", j, J.src_row_bytes, J.src_w);
    KGDET_CHECK_SHAPE(J.new_h >= 1 && J.new_w >= 1, "image_preprocess: job %d: resized size %d x %d must be positive", j,
                      J.new_h, J.new_w);
    KGDET_CHECK_SHAPE(J.out_h >= J.new_h && J.out_w >= J.new_w && J.out_h <= kPreMaxExtent && J.out_w <= kPreMaxExtent,
                      "image_preprocess: job %d: slot %d x %d must hold the resized %d x %d (and stay below %d)", j,
                      J.out_h, J.out_w, J.new_h, J.new_w, kPreMaxExtent);
    KGDET_CHECK_SHAPE(J.dst_row_stride >= J.out_w, "image_preprocess: job %d: row stride %d below the slot width %d", j,
                      J.dst_row_stride, J.out_w);
    KGDET_CHECK_SHAPE(J.dst_channel_stride >= (long long)(J.out_h - 1) * J.dst_row_stride + J.out_w,
                      "image_preprocess: job %d: channel stride %lld does not hold a %d x %d plane", j,
                      (long long)J.dst_channel_stride, J.out_h, J.out_w);
    KGDET_CHECK_SHAPE(J.scale_y > 0.0f && J.scale_x > 0.0f && J.scale_y <= (float)kPreMaxExtent &&
                          J.scale_x <= (float)kPreMaxExtent,
                      "image_preprocess: job %d: scales must be positive and finite", j);
    args.job[j] = J;
    args.row0[j] = (int)rows;
    rows += J.out_h;
  }
  KGDET_CHECK_SHAPE(rows < (1ll << 31), "image_preprocess: too many rows");
  args.row0[n_jobs] = (int)rows;
  args.n = n_jobs;
  const unsigned grid = (unsigned)(rows < kPreMaxBlocks ? rows : kPreMaxBlocks);
  hipLaunchKernelGGL(image_preprocess_kernel, dim3(grid), dim3(kPreThreads), 0, (hipStream_t)stream, args, norm_lut,
                     (int)(reverse_channels != 0));
  KGDET_CHECK_LAUNCH("image_preprocess_kernel");
  return KGDET_OK;
}

}  // extern "C"
