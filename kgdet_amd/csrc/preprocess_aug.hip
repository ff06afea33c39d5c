// Image preprocessing under train-time extra_aug for gfx950: the launch of preprocess.hip with photometric distortion on
// every source pixel and an expand / crop window in front of the resize.  A batch of raw uint8 HWC images -> the detector's
// float32 [3, out_h, out_w] input slots in ONE launch.
//
// The arithmetic is the one of kgdet_amd/preprocess.py::image_transform_restatement_aug, bit for bit, written out in
// include/kgdet_hip.h: the image is float32 from the first step (no grey-level quantisation, no table), every operation is
// rounded to fp32 on its own, the divisions are the compiler's correctly rounded ones.  Contraction is off: an FMA would
// change the bits.
//
// Work split: preprocess.hip's -- a capped grid strides over (slot rows x jobs), one workgroup per output row, one thread
// per 4 consecutive x of all three planes, dwordx4 stores on the row's 16-byte grid with scalar head and tail, zeros beyond
// new_h / new_w without touching the source.
//
// Where the distortion is computed.  STAGED (the default under KGDET_AUG_COLOUR): the two source rows of an output row have
// row-uniform y taps, so the workgroup distorts the part of them the window can reach ONCE into LDS (2 rows x kStageMax pixels
// x 3 floats = 36 KiB) and the x taps read from there.  PER TAP (four distortions per output pixel, about twelve per source
// pixel at a 1.7x upscale): jobs whose reachable row segment is wider than kStageMax, and jobs without a colour stage, whose
// taps are the plain byte loads of preprocess.hip.  Both give the same bits: the same expression on the same pixel.
//
// Environment (A/B measurement, not part of the API):
//   KGDET_PREPROC_AUG_STAGE=0   every job per tap (tools/time_augment.py measures both variants with it; read per call)
#include "common.h"

#pragma clang fp contract(off)

namespace kgdet {

namespace {

constexpr int kAugThreads = 256;
constexpr int kAugMaxJobs = KGDET_PREPROC_AUG_MAX_JOBS;
constexpr int kAugMaxBlocks = 2048;       // 256 CUs x 8 workgroups, as preprocess.hip
constexpr int kAugMaxExtent = 1 << 20;    // per source / virtual / output side, and per offset
constexpr float kAugMaxNumber = 65536.0f; // |delta|, |alpha|, |sat|: keeps every intermediate finite
constexpr int kStageMax = 1536;           // pixels per staged row segment
constexpr float kAugMaxHue = 720.0f;      // h in [-720, 1080] before the wrap: the sector loops make at most 3 trips
constexpr unsigned kAugKnownFlags = KGDET_AUG_COLOUR | KGDET_AUG_BRIGHTNESS | KGDET_AUG_CONTRAST | KGDET_AUG_CONTRAST_FIRST |
                                    KGDET_AUG_SATURATION | KGDET_AUG_HUE | KGDET_AUG_PERMUTE;
constexpr float kHsvEps = 1.1920928955078125e-07f;      // 2^-23
constexpr float kHueToSector = (float)(6.0 / 360.0);    // the constant rounded once

struct AugArgs {
  kgdet_preproc_aug_job job[kAugMaxJobs];
  int row0[kAugMaxJobs + 1];              // first (global) row of each job's slot
  int n;
  float mean[3], std[3];
};
static_assert(sizeof(AugArgs) < 4096 - 64, "the by-value argument block must stay under the kernel-argument limit");

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

struct Px {
  float c[3];                             // raw channel order (r, g, b)
};

// steps 1-8 of the header on one source pixel
__device__ __forceinline__ Px distort(float r, float g, float b, unsigned flags, float delta, float alpha, float sat,
                                      float hue, int perm) {
  if (flags & KGDET_AUG_BRIGHTNESS) { r = r + delta; g = g + delta; b = b + delta; }
  const bool contrast = (flags & KGDET_AUG_CONTRAST) != 0, first = (flags & KGDET_AUG_CONTRAST_FIRST) != 0;
  if (contrast && first) { r = r * alpha; g = g * alpha; b = b * alpha; }
  // to HSV
  float v = g > r ? g : r;
  v = b > v ? b : v;
  float vmin = g < r ? g : r;
  vmin = b < vmin ? b : vmin;
  const float diff = v - vmin;
  float s = diff / (fabsf(v) + kHsvEps);
  const float d = 60.0f / (diff + kHsvEps);
  float h;
  if (v == r) h = (g - b) * d;
  else if (v == g) h = (b - r) * d + 120.0f;
  else h = (r - g) * d + 240.0f;
  if (h < 0.0f) h = h + 360.0f;
  if (flags & KGDET_AUG_SATURATION) s = s * sat;
  if (flags & KGDET_AUG_HUE) {
    h = h + hue;
    if (h > 360.0f) h = h - 360.0f;
    if (h < 0.0f) h = h + 360.0f;
  }
  // to RGB
  if (s == 0.0f) {
    r = v; g = v; b = v;
  } else {
    h = h * kHueToSector;
    // `while h < 0: h += 6` / `while h >= 6: h -= 6`: h lies in [-12, 18] here (|hue| <= 720 is checked by the host
    // side), so 3 trips end either loop; the trip count is bounded so that no input can keep a wave spinning
    for (int i = 0; i < 4 && h < 0.0f; ++i) h = h + 6.0f;
    for (int i = 0; i < 4 && h >= 6.0f; ++i) h = h - 6.0f;
    float k = floorf(h);
    float f = h - k;
    int sector = (int)k;
    if (!(sector >= 0 && sector < 6)) { sector = 0; f = 0.0f; }
    const float t1 = v * (1.0f - s);
    const float t2 = v * (1.0f - s * f);
    const float t3 = v * (1.0f - s * (1.0f - f));
    switch (sector) {                      // (b, g, r) = t[(1,3,0), (1,0,2), (3,0,1), (0,2,1), (0,1,3), (2,1,0)]
      case 0: b = t1; g = t3; r = v; break;
      case 1: b = t1; g = v; r = t2; break;
      case 2: b = t3; g = v; r = t1; break;
      case 3: b = v; g = t2; r = t1; break;
      case 4: b = v; g = t1; r = t3; break;
      default: b = t2; g = t1; r = v; break;
    }
  }
  if (contrast && !first) { r = r * alpha; g = g * alpha; b = b * alpha; }
  Px o;
  if (flags & KGDET_AUG_PERMUTE) {
    const int q0 = perm & 3, q1 = (perm >> 2) & 3, q2 = (perm >> 4) & 3;
    o.c[0] = q0 == 0 ? r : (q0 == 1 ? g : b);
    o.c[1] = q1 == 0 ? r : (q1 == 1 ? g : b);
    o.c[2] = q2 == 0 ? r : (q2 == 1 ? g : b);
  } else {
    o.c[0] = r; o.c[1] = g; o.c[2] = b;
  }
  return o;
}

__global__ __launch_bounds__(kAugThreads) void image_preprocess_aug_kernel(const AugArgs args, int reverse_channels,
                                                                           int stage_on) {
  __shared__ float stage[2][kStageMax * 3];
  const int tid = threadIdx.x;
  const int total = args.row0[args.n];
  int j = 0;
  for (int r = blockIdx.x; r < total; r += gridDim.x) {
    while (r >= args.row0[j + 1]) ++j;                       // (r only grows: j never steps back)
    const kgdet_preproc_aug_job &J = args.job[j];
    const int y = r - args.row0[j];
    const int new_w = J.new_w, out_w = J.out_w, src_w = J.src_w, vw = J.vw, ox = J.ox;
    const long long cs = J.dst_channel_stride;
    float *__restrict__ row = J.dst + (long long)y * J.dst_row_stride;
    const bool live_row = y < J.new_h;
    const bool flip = J.flip != 0;
    const float scale_x = J.scale_x;
    const unsigned flags = J.flags;
    const float delta = J.delta, alpha = J.alpha, sat = J.sat, hue = J.hue;
    const int perm = J.perm;
    Px fill;
    fill.c[0] = J.fill[0]; fill.c[1] = J.fill[1]; fill.c[2] = J.fill[2];
    Tap ty = {0, 0, 0.0f, 0.0f};
    if (live_row) ty = make_tap(y, J.scale_y, J.vh);
    // the two tapped rows of V in raw coordinates; a row outside the raw image is all fill and is never read
    const int ry0 = ty.i0 - J.oy, ry1 = ty.i1 - J.oy;
    const bool in0 = live_row && ry0 >= 0 && ry0 < J.src_h, in1 = live_row && ry1 >= 0 && ry1 < J.src_h;
    const uint8_t *__restrict__ s0 = J.src + (long long)(in0 ? ry0 : 0) * J.src_row_bytes;
    const uint8_t *__restrict__ s1 = J.src + (long long)(in1 ? ry1 : 0) * J.src_row_bytes;

    // the raw columns V's columns can reach: [lo, hi); every x tap that lands inside the raw image lands in there
    const int lo = ox < 0 ? -ox : 0, hi = vw - ox < src_w ? vw - ox : src_w;
    const bool staged = stage_on && (flags & KGDET_AUG_COLOUR) && hi - lo <= kStageMax;       // (uniform over the job)
    const float *__restrict__ st0 = stage[0];
    const float *__restrict__ st1 = (in1 && in0 && ry1 == ry0) ? stage[0] : stage[1];
    if (staged) {
      __syncthreads();                                       // the previous row's taps have been read
      if (in0 || in1) {
        const bool second = in1 && !(in0 && ry1 == ry0);
        for (int i = tid; i < hi - lo; i += kAugThreads) {
          if (in0) {
            const uint8_t *p = s0 + 3 * (lo + i);
            const Px o = distort((float)p[0], (float)p[1], (float)p[2], flags, delta, alpha, sat, hue, perm);
            stage[0][3 * i] = o.c[0]; stage[0][3 * i + 1] = o.c[1]; stage[0][3 * i + 2] = o.c[2];
          }
          if (second) {
            const uint8_t *p = s1 + 3 * (lo + i);
            const Px o = distort((float)p[0], (float)p[1], (float)p[2], flags, delta, alpha, sat, hue, perm);
            stage[1][3 * i] = o.c[0]; stage[1][3 * i + 1] = o.c[1]; stage[1][3 * i + 2] = o.c[2];
          }
        }
      }
      __syncthreads();
    }

    auto tap = [&](const uint8_t *__restrict__ s, const float *__restrict__ st, bool row_in, int rx) -> Px {
      if (!(row_in && rx >= 0 && rx < src_w)) return fill;
      if (staged) {
        const float *q = st + 3 * (rx - lo);
        Px o;
        o.c[0] = q[0]; o.c[1] = q[1]; o.c[2] = q[2];
        return o;
      }
      const uint8_t *p = s + 3 * rx;
      const float pr = (float)p[0], pg = (float)p[1], pb = (float)p[2];
      if (!(flags & KGDET_AUG_COLOUR)) {
        Px o;
        o.c[0] = pr; o.c[1] = pg; o.c[2] = pb;
        return o;
      }
      return distort(pr, pg, pb, flags, delta, alpha, sat, hue, perm);
    };

    // groups of 4 x on the row's 16-byte grid: group g covers [start + 4g, start + 4g + 4), start in {-3 .. 0}
    const bool vec = (cs & 3) == 0;
    const int head = vec ? (int)(((16 - ((uintptr_t)row & 15)) & 15) >> 2) : 0;
    const int start = head ? head - 4 : 0;
    const int groups = (out_w - start + 3) >> 2;
    for (int g = tid; g < groups; g += kAugThreads) {
      const int x0 = start + 4 * g;
      float v[3][4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int x = x0 + k;
        if (live_row && x >= 0 && x < new_w) {
          const Tap tx = make_tap(flip ? new_w - 1 - x : x, scale_x, vw);
          const int rx0 = tx.i0 - ox, rx1 = tx.i1 - ox;
          const Px p00 = tap(s0, st0, in0, rx0), p01 = tap(s0, st0, in0, rx1);
          const Px p10 = tap(s1, st1, in1, rx0), p11 = tap(s1, st1, in1, rx1);
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const int sc = reverse_channels ? 2 - c : c;
            const float top = tx.l0 * p00.c[sc] + tx.l1 * p01.c[sc];
            const float bot = tx.l0 * p10.c[sc] + tx.l1 * p11.c[sc];
            const float val = ty.l0 * top + ty.l1 * bot;
            v[c][k] = (val - args.mean[c]) / args.std[c];
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

bool bounded(float x, float limit) { return x >= -limit && x <= limit; }   // false for a NaN

}  // namespace

}  // namespace kgdet

using namespace kgdet;

extern "C" {

int kgdet_image_preprocess_aug(const kgdet_preproc_aug_job *jobs, int32_t n_jobs, const float *mean, const float *std,
                               int32_t reverse_channels, void *stream) {
  KGDET_CHECK_SHAPE(n_jobs >= 0, "image_preprocess_aug: negative job count");
  if (n_jobs == 0) return KGDET_OK;
  if (n_jobs > kAugMaxJobs) {
    set_error("image_preprocess_aug: %d jobs in one launch (limit %d)", n_jobs, kAugMaxJobs);
    return KGDET_E_UNSUPPORTED;
  }
  KGDET_CHECK_SHAPE(jobs && mean && std, "image_preprocess_aug: null pointer");
  AugArgs args = {};
  long long rows = 0;
  for (int j = 0; j < n_jobs; ++j) {
    const kgdet_preproc_aug_job &J = jobs[j];
    KGDET_CHECK_SHAPE(J.src && J.dst, "image_preprocess_aug: job %d: null pointer", j);
    KGDET_CHECK_SHAPE(((uintptr_t)J.dst & 3) == 0, "image_preprocess_aug: job %d: dst is not 4-byte aligned", j);
    KGDET_CHECK_SHAPE(J.src_h >= 1 && J.src_w >= 1 && J.src_h <= kAugMaxExtent && J.src_w <= kAugMaxExtent,
                      "image_preprocess_aug: job %d: source size %d x %d outside 1..%d", j, J.src_h, J.src_w, kAugMaxExtent);
    KGDET_CHECK_SHAPE((long long)J.src_row_bytes >= 3ll * J.src_w,
                      "image_preprocess_aug: job %d: source row pitch %d below 3 * %d", j, J.src_row_bytes, J.src_w);
    KGDET_CHECK_SHAPE(J.vh >= 1 && J.vw >= 1 && J.vh <= kAugMaxExtent && J.vw <= kAugMaxExtent,
                      "image_preprocess_aug: job %d: window size %d x %d outside 1..%d", j, J.vh, J.vw, kAugMaxExtent);
    KGDET_CHECK_SHAPE(J.oy >= -kAugMaxExtent && J.oy <= kAugMaxExtent && J.ox >= -kAugMaxExtent && J.ox <= kAugMaxExtent,
                      "image_preprocess_aug: job %d: window offset (%d, %d) beyond +-%d", j, J.oy, J.ox, kAugMaxExtent);
    KGDET_CHECK_SHAPE(J.new_h >= 1 && J.new_w >= 1, "image_preprocess_aug: job %d: resized size %d x %d must be positive", j,
                      J.new_h, J.new_w);
    KGDET_CHECK_SHAPE(J.out_h >= J.new_h && J.out_w >= J.new_w && J.out_h <= kAugMaxExtent && J.out_w <= kAugMaxExtent,
                      "image_preprocess_aug: job %d: slot %d x %d must hold the resized %d x %d (and stay below %d)", j,
                      J.out_h, J.out_w, J.new_h, J.new_w, kAugMaxExtent);
    KGDET_CHECK_SHAPE(J.dst_row_stride >= J.out_w, "image_preprocess_aug: job %d: row stride %d below the slot width %d", j,
                      J.dst_row_stride, J.out_w);
    KGDET_CHECK_SHAPE(J.dst_channel_stride >= (long long)(J.out_h - 1) * J.dst_row_stride + J.out_w,
                      "image_preprocess_aug: job %d: channel stride %lld does not hold a %d x %d plane", j,
                      (long long)J.dst_channel_stride, J.out_h, J.out_w);
    KGDET_CHECK_SHAPE(J.scale_y > 0.0f && J.scale_x > 0.0f && J.scale_y <= (float)kAugMaxExtent &&
                          J.scale_x <= (float)kAugMaxExtent,
                      "image_preprocess_aug: job %d: scales must be positive and finite", j);
    KGDET_CHECK_SHAPE((J.flags & ~kAugKnownFlags) == 0, "image_preprocess_aug: job %d: unknown flag bits 0x%x", j, J.flags);
    KGDET_CHECK_SHAPE((J.flags & KGDET_AUG_COLOUR) || J.flags == 0,
                      "image_preprocess_aug: job %d: colour stages 0x%x without KGDET_AUG_COLOUR", j, J.flags);
    if (J.flags & KGDET_AUG_COLOUR) {
      KGDET_CHECK_SHAPE(!(J.flags & KGDET_AUG_BRIGHTNESS) || bounded(J.delta, kAugMaxNumber),
                        "image_preprocess_aug: job %d: brightness delta %g not within +-%g", j, J.delta, kAugMaxNumber);
      KGDET_CHECK_SHAPE(!(J.flags & KGDET_AUG_CONTRAST) || bounded(J.alpha, kAugMaxNumber),
                        "image_preprocess_aug: job %d: contrast factor %g not within +-%g", j, J.alpha, kAugMaxNumber);
      KGDET_CHECK_SHAPE(!(J.flags & KGDET_AUG_SATURATION) || bounded(J.sat, kAugMaxNumber),
                        "image_preprocess_aug: job %d: saturation factor %g not within +-%g", j, J.sat, kAugMaxNumber);
      KGDET_CHECK_SHAPE(!(J.flags & KGDET_AUG_HUE) || bounded(J.hue, kAugMaxHue),
                        "image_preprocess_aug: job %d: hue delta %g not within +-%g", j, J.hue, kAugMaxHue);
      if (J.flags & KGDET_AUG_PERMUTE) {
        const int q0 = J.perm & 3, q1 = (J.perm >> 2) & 3, q2 = (J.perm >> 4) & 3;
        KGDET_CHECK_SHAPE((J.perm >> 6) == 0 && q0 < 3 && q1 < 3 && q2 < 3 && q0 != q1 && q0 != q2 && q1 != q2,
                          "image_preprocess_aug: job %d: perm 0x%x is not a permutation of (0, 1, 2)", j, J.perm);
      }
    }
    args.job[j] = J;
    args.row0[j] = (int)rows;
    rows += J.out_h;
  }
  KGDET_CHECK_SHAPE(rows < (1ll << 31), "image_preprocess_aug: too many rows");
  args.row0[n_jobs] = (int)rows;
  args.n = n_jobs;
  for (int c = 0; c < 3; ++c) {
    args.mean[c] = mean[c];
    args.std[c] = std[c];
  }
  const unsigned grid = (unsigned)(rows < kAugMaxBlocks ? rows : kAugMaxBlocks);
  const int stage_on = env_int("KGDET_PREPROC_AUG_STAGE", 1) != 0;   // A/B switch
  hipLaunchKernelGGL(image_preprocess_aug_kernel, dim3(grid), dim3(kAugThreads), 0, (hipStream_t)stream, args,
                     (int)(reverse_channels != 0), stage_on);
  KGDET_CHECK_LAUNCH("image_preprocess_aug_kernel");
  return KGDET_OK;
}

}  // extern "C"
