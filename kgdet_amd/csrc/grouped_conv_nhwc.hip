// Grouped 3x3 convolution (padding 1, dilation 1, stride 1 or 2) on channels-last bf16 activations: the ResNeXt bottleneck's
// conv2 at bf16 inference (include/kgdet_hip.h kgdet_gconv3x3_nhwc_bf16).  x [B, H, W, C], w [C][3][3][cpg] (the channels-last
// storage of a [C, cpg, 3, 3] tensor), y [B, Ho, Wo, C], cpg in {4, 8, 16, 32}, C % 8 == 0.
//
// Arithmetic: bf16 products exact in fp32, fp32 accumulation on the MFMA, then y = bf16(S) (raw) or
// y = bf16([relu](fp32(bf16(S)) + bias[c])) -- the roundings of F.conv2d followed by kgdet_bias_act (csrc/conv_nhwc.hip states
// the same for its own sum).  No atomics, no workspace: the same inputs give the same bits.
//
// Tile plan: a workgroup (4 waves) owns a slab of 64 consecutive channels (whole groups) and walks output tiles of TH x 16
// pixels (TH = 8 at stride 1, 4 at stride 2) with a stride of gridDim.x: as many trips as keep the launch at 4096 workgroups or
// fewer.  Per tile the input halo -- ((TH - 1) s + 3) x (15 s + 3) pixels x 128 bytes -- is staged in LDS with 16-byte loads,
// zero-filled where it leaves the map or the channel count (no divergent taps), and the loads of the NEXT tile are issued into
// registers before the current one is multiplied.
// A wave owns 16 output channels of the slab: mfma_f32_16x16x32_bf16 with the output channels as rows (A = the weights, in
// registers for the whole walk) and 16 pixels of one output row as columns (B = 16-byte LDS reads), so a lane ends with four
// consecutive channels of one pixel.
//   cpg 32: K step = one tap x the group's 32 channels, 9 steps; the group's two halves of 16 outputs sit in two waves.
//   cpg 16: K step = two taps x 16 channels, 5 steps, the tenth tap slot zero on both sides.
//   cpg 8, 4: two / four neighbouring groups form one 16-channel block with a block-diagonal weight (zeros across groups)
//     and run as cpg 16: 5 MFMAs per 16 pixels x 16 channels, fewer than one group per MFMA would take (6 and 8), and one
//     fragment path.  The price: a non-finite activation reaches the other groups of its 16-channel block (0 x inf).
// Results go through an LDS tile and leave as 16-byte channel-contiguous stores, 128 bytes per pixel and workgroup.
#include "common.h"

namespace kgdet {
namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;
constexpr int kSlab = 64;         // channels per workgroup
constexpr int kPix = 144;         // LDS bytes per pixel: 128 of channels + 16, so that neighbouring pixels spread over the banks
constexpr int kTW = 16;           // output pixels of a row per tile = the MFMA's columns
constexpr int kTargetGroups = 4096;   // workgroups of a launch, at most: each keeps its weights for its whole walk

template <int CPG, int S>
__global__ __launch_bounds__(kThreads) void gconv3x3_nhwc(const __bf16 *__restrict__ x, const __bf16 *__restrict__ w,
                                                          const float *__restrict__ bias, __bf16 *__restrict__ y,
                                                          long long ntiles, int tiles_y, int tiles_x, int C, int H, int W, int Ho,
                                                          int Wo, int epilogue, int relu) {
  constexpr int TH = S == 1 ? 8 : 4;
  constexpr int IH = (TH - 1) * S + 3, IW = (kTW - 1) * S + 3;      // the halo tile
  constexpr int NIN = IH * IW * 8, NLD = (NIN + kThreads - 1) / kThreads;   // its 16-byte pieces, and per thread
  constexpr int NST = TH * kTW * 8 / kThreads;                       // 16-byte pieces of the output tile per thread
  constexpr int STEPS = CPG == 32 ? 9 : 5;
  __shared__ __attribute__((aligned(16))) unsigned char lin[IH * IW * kPix];
  __shared__ __attribute__((aligned(16))) unsigned char lout[TH * kTW * kPix];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, p = lane & 15, q = lane >> 4;
  const int slab0 = blockIdx.y * kSlab;

  // ---- the wave's weights as A fragments: row p = output channel slab0 + 16 wave + p, k = 8 q + j --------------------------
  bf16x8 wf[STEPS];
  int boff[STEPS];           // byte offset of the lane's B fragment inside the halo tile, the pixel's own offset aside
  bool bzero[STEPS];         // the tenth tap slot
  {
    const int co = slab0 + 16 * wave + p;
#pragma unroll
    for (int s = 0; s < STEPS; ++s) {
      const int tap = CPG == 32 ? s : 2 * s + (q >> 1);
      const int chunk = CPG == 32 ? q : (q & 1);      // which 8 channels of the wave's input block
      bf16x8 v = {};
      if (co < C && tap < 9) {
        const __bf16 *wp = w + ((long long)co * 9 + tap) * CPG;
        if (CPG >= 16) {
          v = *reinterpret_cast<const bf16x8 *>(wp + 8 * chunk);
        } else if (CPG == 8) {
          if ((p >> 3) == chunk) v = *reinterpret_cast<const bf16x8 *>(wp);
        } else if ((p >> 3) == chunk) {
          const bf16x4 h = *reinterpret_cast<const bf16x4 *>(wp);
          const __bf16 z = (__bf16)0.0f;
          const bf16x8 lo = {h[0], h[1], h[2], h[3], z, z, z, z}, hi = {z, z, z, z, h[0], h[1], h[2], h[3]};
          v = ((p >> 2) & 1) ? hi : lo;
        }
      }
      wf[s] = v;
      const int t = tap < 9 ? tap : 8;
      boff[s] = ((t / 3) * IW + t % 3) * kPix + (CPG == 32 ? (wave >> 1) * 64 : wave * 32) + chunk * 16;
      bzero[s] = tap >= 9;
    }
  }
  // the lane's results: channels slab0 + 16 wave + 4 q + (0..3) of pixel p
  f32x4 bv = {0.f, 0.f, 0.f, 0.f};
  {
    const int c4 = slab0 + 16 * wave + 4 * q;
    if (bias && c4 < C) bv = *reinterpret_cast<const f32x4 *>(bias + c4);
  }

  bf16x8 pre[NLD];
  auto fetch = [&](long long t) {
    const long long b = t / ((long long)tiles_y * tiles_x);
    const int r = (int)(t - b * tiles_y * tiles_x), ty = r / tiles_x, tx = r - ty * tiles_x;
    const int iy0 = ty * TH * S - 1, ix0 = tx * kTW * S - 1;
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      const int idx = tid + i * kThreads, px = idx >> 3, ch = slab0 + (idx & 7) * 8;
      const int iy = iy0 + px / IW, ix = ix0 + px % IW;
      bf16x8 v = {};
      if (idx < NIN && iy >= 0 && iy < H && ix >= 0 && ix < W && ch < C)
        v = *reinterpret_cast<const bf16x8 *>(x + ((b * H + iy) * W + ix) * C + ch);
      pre[i] = v;
    }
  };

  long long t = blockIdx.x;
  if (t >= ntiles) return;
  fetch(t);
  for (; t < ntiles; t += gridDim.x) {
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      const int idx = tid + i * kThreads;
      if (idx < NIN) *reinterpret_cast<bf16x8 *>(lin + (idx >> 3) * kPix + (idx & 7) * 16) = pre[i];
    }
    __syncthreads();
    if (t + gridDim.x < ntiles) fetch(t + gridDim.x);

#pragma unroll
    for (int m0 = 0; m0 < TH; m0 += 4) {
      f32x4 acc[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < STEPS; ++s) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          bf16x8 bf = *reinterpret_cast<const bf16x8 *>(lin + ((m0 + j) * S * IW + p * S) * kPix + boff[s]);
          if (bzero[s]) bf = bf16x8{};
          acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[s], bf, acc[j], 0, 0, 0);
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        bf16x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float f = acc[j][e];
          if (epilogue) {
            f = (float)(__bf16)f + bv[e];
            if (relu) f = fmaxf(f, 0.0f);
          }
          o[e] = (__bf16)f;
        }
        *reinterpret_cast<bf16x4 *>(lout + ((m0 + j) * kTW + p) * kPix + wave * 32 + q * 8) = o;
      }
    }
    __syncthreads();

    {
      const long long b = t / ((long long)tiles_y * tiles_x);
      const int r = (int)(t - b * tiles_y * tiles_x), ty = r / tiles_x, tx = r - ty * tiles_x;
#pragma unroll
      for (int i = 0; i < NST; ++i) {
        const int idx = tid + i * kThreads, px = idx >> 3, ch = slab0 + (idx & 7) * 8;
        const int oy = ty * TH + px / kTW, ox = tx * kTW + px % kTW;
        if (oy < Ho && ox < Wo && ch < C)
          *reinterpret_cast<bf16x8 *>(y + ((b * Ho + oy) * Wo + ox) * C + ch) =
              *reinterpret_cast<const bf16x8 *>(lout + px * kPix + (idx & 7) * 16);
      }
    }
    // (the next trip writes `lin` -- every wave is past its reads, the barrier above -- and `lout` only after its own barrier)
  }
}

inline bool overlaps(const void *a, size_t na, const void *b, size_t nb) {
  const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
  return a && b && na && nb && pa < pb + nb && pb < pa + na;
}

inline bool aligned16(const void *ptr) { return ((uintptr_t)ptr & 15) == 0; }

template <int CPG, int S>
void launch(const void *x, const void *w, const float *bias, void *y, int64_t B, int C, int H, int W, int Ho, int Wo, int relu,
            hipStream_t stream) {
  constexpr int TH = S == 1 ? 8 : 4;
  const int tiles_y = (Ho + TH - 1) / TH, tiles_x = (Wo + kTW - 1) / kTW, slabs = (C + kSlab - 1) / kSlab;
  const long long ntiles = (long long)B * tiles_y * tiles_x;
  // every workgroup of a slab takes the same number of trips (the last one may be short): 336 tiles on 256 workgroups would leave
  // 176 of them idle for the second half of the launch
  const long long want = kTargetGroups / slabs > 0 ? kTargetGroups / slabs : 1;
  const long long trips = (ntiles + want - 1) / want;
  const dim3 grid((unsigned)((ntiles + trips - 1) / trips), (unsigned)slabs);
  hipLaunchKernelGGL((gconv3x3_nhwc<CPG, S>), grid, dim3(kThreads), 0, stream, (const __bf16 *)x, (const __bf16 *)w, bias,
                     (__bf16 *)y, ntiles, tiles_y, tiles_x, C, H, W, Ho, Wo, (bias || relu) ? 1 : 0, relu);
}

}  // namespace
}  // namespace kgdet

using namespace kgdet;

extern "C" int kgdet_gconv3x3_nhwc_bf16(const void *x, const void *w, const float *bias, void *y, int64_t B, int32_t C,
                                        int32_t cpg, int32_t H, int32_t W, int32_t stride, int32_t relu, void *stream) {
  KGDET_CHECK_SHAPE(B >= 1 && C >= 1 && H >= 1 && W >= 1 && (cpg == 4 || cpg == 8 || cpg == 16 || cpg == 32) && C % cpg == 0 &&
                        C % 8 == 0 && (stride == 1 || stride == 2),
                    "gconv3x3_nhwc_bf16: cpg in {4, 8, 16, 32}, C %% cpg == 0, C %% 8 == 0, stride 1 or 2, sizes >= 1");
  KGDET_CHECK_SHAPE(x && w && y, "gconv3x3_nhwc_bf16: null pointer");
  KGDET_CHECK_SHAPE(aligned16(x) && aligned16(w) && aligned16(bias) && aligned16(y), "gconv3x3_nhwc_bf16: pointers must be 16-byte aligned");
  KGDET_CHECK_SHAPE(H <= (1 << 30) && W <= (1 << 30) && (C + kSlab - 1) / kSlab <= 65535 && B <= (1LL << 31),
                    "gconv3x3_nhwc_bf16: too large (H, W <= 2^30, C <= 64 * 65535, B <= 2^31)");
  const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
  const size_t nx = (size_t)B * H * W * C * 2, ny = (size_t)B * Ho * Wo * C * 2, nw = (size_t)C * cpg * 18;
  KGDET_CHECK_SHAPE(!overlaps(y, ny, x, nx) && !overlaps(y, ny, w, nw) && !overlaps(y, ny, bias, (size_t)C * 4),
                    "gconv3x3_nhwc_bf16: y overlaps an operand");
  const hipStream_t st = (hipStream_t)stream;
  const int r = relu ? 1 : 0;
#define KGDET_GCONV_CASE(CPG)                                                     \
  case CPG:                                                                       \
    if (stride == 1) launch<CPG, 1>(x, w, bias, y, B, C, H, W, Ho, Wo, r, st);    \
    else launch<CPG, 2>(x, w, bias, y, B, C, H, W, Ho, Wo, r, st);                \
    break;
  switch (cpg) {
    KGDET_GCONV_CASE(4)
    KGDET_GCONV_CASE(8)
    KGDET_GCONV_CASE(16)
    KGDET_GCONV_CASE(32)
  }
#undef KGDET_GCONV_CASE
  KGDET_CHECK_LAUNCH("gconv3x3_nhwc_bf16");
  return KGDET_OK;
}
