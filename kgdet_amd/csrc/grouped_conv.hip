// Grouped 3x3 convolution (padding 1, dilation 1, stride 1 or 2) for the ResNeXt bottleneck's conv2: forward with the
// bias + ReLU inference epilogue, grad_input, grad_weight (include/kgdet_hip.h kgdet_gconv3x3_*).  fp32 NCHW, cpg in
// {4, 8, 16, 32} channels per group.
//
// Arithmetic: plain fp32 operands, one fp32 FMA chain per result (K = 9 * cpg is 36 .. 288: a group is too narrow for the
// split-MFMA GEMMs and the f32 MFMA runs at the vector FMA rate, MI355X guide).  No atomics: grad_weight keeps one partial
// sum per workgroup in the workspace and a second kernel adds them in index order, so every call returns the same bits.
//
// forward / grad_input (one kernel template, gconv_apply): a thread owns a strip of 4 consecutive pixels of one row for a block
// of OCB channels of one group; per reduction channel it loads the rows of the other map that the strip's taps reach once and
// runs the 9 taps on registers.  The group and the channel block come from blockIdx.y: the block's weights are staged in LDS
// once and read as broadcasts.  grad_input at stride 2: a strip starts at a multiple of 4, so the parity of every
// (pixel, tap) pair is known at compile time -- only the taps that reach a grad_y column are compiled in; rows are tested.
//
// grad_weight (gconv_grad_weight): a workgroup owns 4 output channels x 1 input channel x 9 taps of one group and one chunk of
// the B * Ho * Wo pixels; each lane walks the chunk with a stride of the workgroup, 36 sums in registers, then a fixed shuffle
// tree per wave and a fixed-order sum of the four waves.
#include "common.h"

namespace kgdet {
namespace {

constexpr int kThreads = 256;
constexpr int kStrip = 4;         // pixels of a row per thread (forward / grad_input)
constexpr int kWgradOC = 4;       // output channels per workgroup (grad_weight)
constexpr int kWgradMaxChunks = 128;
constexpr int kWgradPixelsPerLane = 32;

// BWD = false: out = y [B, C, Ho, Wo] from in = x [B, C, Hi, Wi] (Hi, Wi the convolution's input map)
// BWD = true:  out = grad_x [B, C, Ho, Wo] (Ho, Wo the convolution's INPUT map) from in = grad_y [B, C, Hi, Wi]
template <int CPG, int S, int OCB, bool BWD>
__global__ __launch_bounds__(kThreads) void gconv_apply(const float *__restrict__ in, const float *__restrict__ w,
                                                        const float *__restrict__ bias, float *__restrict__ out, int C, int Hi,
                                                        int Wi, int Ho, int Wo, int strips, int relu) {
  constexpr int kBlocks = CPG / OCB;
  // columns of `in` a strip reaches: forward 3 * S + 3 from S * x0 - 1; backward stride 1: 6 from x0 - 1, stride 2: 3 from x0 / 2
  constexpr int NV = BWD ? (S == 1 ? 6 : 3) : ((kStrip - 1) * S + 3);
  const int g = blockIdx.y / kBlocks, cb = (blockIdx.y % kBlocks) * OCB;
  const long long b = blockIdx.z;
  const float *w_g = w + (long long)g * CPG * CPG * 9;
  // the block's weights, [reduction channel][output channel of the block][tap], staged once: every lane of a wave reads the
  // same word (an LDS broadcast), where scalar loads from global memory had to be waited for in every pass of the loop below
  __shared__ float ws[CPG * OCB * 9];
  for (int i = threadIdx.x; i < CPG * OCB * 9; i += kThreads) {
    const int r = i / (OCB * 9), o = (i - r * OCB * 9) / 9, t = i % 9;
    // forward: w[g CPG + cb + o][r][tap]; backward: w[g CPG + r][cb + o][tap]
    ws[i] = BWD ? w_g[(r * CPG + cb + o) * 9 + t] : w_g[((cb + o) * CPG + r) * 9 + t];
  }
  __syncthreads();
  const int sid = blockIdx.x * kThreads + threadIdx.x;
  if (sid >= Ho * strips) return;
  const int oy = sid / strips, x0 = (sid - oy * strips) * kStrip;
  const int col0 = BWD ? (S == 1 ? x0 - 1 : x0 / 2) : S * x0 - 1;
  const float *in_g = in + (b * C + (long long)g * CPG) * Hi * Wi;

  float acc[OCB][kStrip];
#pragma unroll
  for (int o = 0; o < OCB; ++o)
#pragma unroll
    for (int j = 0; j < kStrip; ++j) acc[o][j] = 0.f;

#pragma unroll 1
  for (int r = 0; r < CPG; ++r) {       // the reduction channel of the group: input channel (forward), output channel (backward)
    const float *plane = in_g + (long long)r * Hi * Wi;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
      int row;
      if (BWD) {
        const int t = oy + 1 - ky;      // = S * (row of grad_y)
        if (t < 0 || (S == 2 && (t & 1))) continue;
        row = t / S;
      } else {
        row = oy * S - 1 + ky;
      }
      if (row < 0 || row >= Hi) continue;
      float v[NV];
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int col = col0 + i;
        v[i] = (col >= 0 && col < Wi) ? plane[(long long)row * Wi + col] : 0.f;
      }
#pragma unroll
      for (int o = 0; o < OCB; ++o) {
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          const float wv = ws[(r * OCB + o) * 9 + ky * 3 + kx];
#pragma unroll
          for (int j = 0; j < kStrip; ++j) {
            if (BWD) {
              const int t = j + 1 - kx;           // S * (column of grad_y) - x0
              if (S == 2 && (t & 1)) continue;    // (t = -1 is odd: never divided)
              acc[o][j] = fmaf(v[S == 1 ? t + 1 : t / 2], wv, acc[o][j]);
            } else {
              acc[o][j] = fmaf(v[S * j + kx], wv, acc[o][j]);
            }
          }
        }
      }
    }
  }

  float *out_g = out + ((b * C + (long long)g * CPG + cb) * Ho + oy) * Wo;
#pragma unroll
  for (int o = 0; o < OCB; ++o) {
    const float bv = bias ? bias[g * CPG + cb + o] : 0.f;
#pragma unroll
    for (int j = 0; j < kStrip; ++j) {
      if (x0 + j < Wo) {
        float r = acc[o][j];
        if (bias) r += bv;
        if (relu) r = fmaxf(r, 0.f);
        out_g[(long long)o * Ho * Wo + x0 + j] = r;
      }
    }
  }
}

// partial[(((g CPG + oc) CPG + c) 9 + tap) P + chunk] = the sum over the chunk's pixels of grad_y[b, g CPG + oc, oy, ox]
// x[b, g CPG + c, S oy - 1 + ky, S ox - 1 + kx]
template <int CPG, int S>
__global__ __launch_bounds__(kThreads) void gconv_grad_weight(const float *__restrict__ gy, const float *__restrict__ x,
                                                              float *__restrict__ partial, int C, int H, int W, int Ho, int Wo,
                                                              long long npix, long long chunk, int P) {
  constexpr int kOB = CPG / kWgradOC;
  __shared__ float red[kThreads / 64][kWgradOC * 9];
  const int g = blockIdx.y / (CPG * kOB), rem = blockIdx.y % (CPG * kOB);
  const int c = rem / kOB, ob = (rem % kOB) * kWgradOC;
  const long long q0 = (long long)blockIdx.x * chunk;
  const long long q1 = q0 + chunk < npix ? q0 + chunk : npix;
  const int HoWo = Ho * Wo;

  float acc[kWgradOC][9];
#pragma unroll
  for (int o = 0; o < kWgradOC; ++o)
#pragma unroll
    for (int t = 0; t < 9; ++t) acc[o][t] = 0.f;

  for (long long q = q0 + threadIdx.x; q < q1; q += kThreads) {
    const long long b = q / HoWo;
    const int r = (int)(q - b * HoWo), oy = r / Wo, ox = r - oy * Wo;
    const float *xp = x + (b * C + (long long)g * CPG + c) * H * W;
    float xv[9];
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const int iy = oy * S - 1 + ky, ix = ox * S - 1 + kx;
        xv[ky * 3 + kx] = (iy >= 0 && iy < H && ix >= 0 && ix < W) ? xp[(long long)iy * W + ix] : 0.f;
      }
    const float *gp = gy + (b * C + (long long)g * CPG + ob) * HoWo + r;
#pragma unroll
    for (int o = 0; o < kWgradOC; ++o) {
      const float gv = gp[(long long)o * HoWo];
#pragma unroll
      for (int t = 0; t < 9; ++t) acc[o][t] = fmaf(gv, xv[t], acc[o][t]);
    }
  }

  // the lanes of a wave in a fixed tree, then the four waves in index order
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int o = 0; o < kWgradOC; ++o)
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      float s = acc[o][t];
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) s += __shfl_down(s, d, 64);
      if (lane == 0) red[wave][o * 9 + t] = s;
    }
  __syncthreads();
  if (threadIdx.x < kWgradOC * 9) {
    float s = red[0][threadIdx.x];
#pragma unroll
    for (int v = 1; v < kThreads / 64; ++v) s += red[v][threadIdx.x];
    const int o = threadIdx.x / 9, t = threadIdx.x - o * 9;
    const long long idx = (((long long)g * CPG + ob + o) * CPG + c) * 9 + t;
    partial[idx * P + blockIdx.x] = s;
  }
}

__global__ __launch_bounds__(kThreads) void gconv_grad_weight_sum(const float *__restrict__ partial, float *__restrict__ gw,
                                                                  long long n, int P) {
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  float s = partial[i * P];
  for (int p = 1; p < P; ++p) s += partial[i * P + p];
  gw[i] = s;
}

inline bool overlaps(const void *a, size_t na, const void *b, size_t nb) {
  const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
  return a && b && na && nb && pa < pb + nb && pb < pa + na;
}

inline bool envelope(int64_t B, int32_t C, int32_t cpg, int32_t H, int32_t W, int32_t stride) {
  return B >= 1 && C >= 1 && H >= 1 && W >= 1 && (cpg == 4 || cpg == 8 || cpg == 16 || cpg == 32) && C % cpg == 0 &&
         (stride == 1 || stride == 2);
}

int wgrad_chunks(long long npix) {
  long long P = npix / ((long long)kThreads * kWgradPixelsPerLane);
  return (int)(P < 1 ? 1 : (P > kWgradMaxChunks ? kWgradMaxChunks : P));
}

template <int CPG, int S, bool BWD>
void launch_apply(const float *in, const float *w, const float *bias, float *out, int64_t B, int C, int Hi, int Wi, int Ho,
                  int Wo, int relu, hipStream_t stream) {
  constexpr int OCB = CPG == 4 ? 4 : 8;
  const int strips = (Wo + kStrip - 1) / kStrip;
  const long long threads = (long long)Ho * strips;
  const dim3 grid((unsigned)((threads + kThreads - 1) / kThreads), (unsigned)(C / CPG * (CPG / OCB)), (unsigned)B);
  hipLaunchKernelGGL((gconv_apply<CPG, S, OCB, BWD>), grid, dim3(kThreads), 0, stream, in, w, bias, out, C, Hi, Wi, Ho, Wo,
                     strips, relu);
}

template <bool BWD>
void dispatch_apply(int cpg, int stride, const float *in, const float *w, const float *bias, float *out, int64_t B, int C, int Hi,
                    int Wi, int Ho, int Wo, int relu, hipStream_t stream) {
#define KGDET_GCONV_CASE(CPG)                                                                         \
  case CPG:                                                                                           \
    if (stride == 1) launch_apply<CPG, 1, BWD>(in, w, bias, out, B, C, Hi, Wi, Ho, Wo, relu, stream); \
    else launch_apply<CPG, 2, BWD>(in, w, bias, out, B, C, Hi, Wi, Ho, Wo, relu, stream);             \
    break;
  switch (cpg) {
    KGDET_GCONV_CASE(4)
    KGDET_GCONV_CASE(8)
    KGDET_GCONV_CASE(16)
    KGDET_GCONV_CASE(32)
  }
#undef KGDET_GCONV_CASE
}

// the grid limits of a launch: blockIdx.y = groups x channel blocks, blockIdx.z = B
inline bool grid_ok(int64_t B, long long y_blocks, long long map) {
  return B <= 65535 && y_blocks <= 65535 && map < (1LL << 31);
}

}  // namespace
}  // namespace kgdet

using namespace kgdet;

extern "C" int kgdet_gconv3x3_forward(const float *x, const float *w, const float *bias, float *y, int64_t B, int32_t C,
                                      int32_t cpg, int32_t H, int32_t W, int32_t stride, int32_t relu, void *stream) {
  KGDET_CHECK_SHAPE(envelope(B, C, cpg, H, W, stride), "gconv3x3_forward: cpg in {4, 8, 16, 32}, C %% cpg == 0, stride 1 or 2, sizes >= 1");
  KGDET_CHECK_SHAPE(x && w && y, "gconv3x3_forward: null pointer");
  const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
  const size_t nx = (size_t)B * C * H * W * 4, ny = (size_t)B * C * Ho * Wo * 4, nw = (size_t)C * cpg * 36;
  KGDET_CHECK_SHAPE(!overlaps(y, ny, x, nx) && !overlaps(y, ny, w, nw) && !overlaps(y, ny, bias, (size_t)C * 4),
                    "gconv3x3_forward: y overlaps an operand");
  KGDET_CHECK_SHAPE(grid_ok(B, (long long)C / cpg * (cpg / (cpg == 4 ? 4 : 8)), (long long)H * W), "gconv3x3_forward: too large");
  dispatch_apply<false>(cpg, stride, x, w, bias, y, B, C, H, W, Ho, Wo, relu ? 1 : 0, (hipStream_t)stream);
  KGDET_CHECK_LAUNCH("gconv3x3_forward");
  return KGDET_OK;
}

extern "C" int kgdet_gconv3x3_grad_input(const float *grad_y, const float *w, float *grad_x, int64_t B, int32_t C, int32_t cpg,
                                         int32_t H, int32_t W, int32_t stride, void *stream) {
  KGDET_CHECK_SHAPE(envelope(B, C, cpg, H, W, stride), "gconv3x3_grad_input: cpg in {4, 8, 16, 32}, C %% cpg == 0, stride 1 or 2, sizes >= 1");
  KGDET_CHECK_SHAPE(grad_y && w && grad_x, "gconv3x3_grad_input: null pointer");
  const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
  const size_t nx = (size_t)B * C * H * W * 4, ny = (size_t)B * C * Ho * Wo * 4, nw = (size_t)C * cpg * 36;
  KGDET_CHECK_SHAPE(!overlaps(grad_x, nx, grad_y, ny) && !overlaps(grad_x, nx, w, nw), "gconv3x3_grad_input: grad_x overlaps an operand");
  KGDET_CHECK_SHAPE(grid_ok(B, (long long)C / cpg * (cpg / (cpg == 4 ? 4 : 8)), (long long)H * W), "gconv3x3_grad_input: too large");
  dispatch_apply<true>(cpg, stride, grad_y, w, nullptr, grad_x, B, C, Ho, Wo, H, W, 0, (hipStream_t)stream);
  KGDET_CHECK_LAUNCH("gconv3x3_grad_input");
  return KGDET_OK;
}

extern "C" size_t kgdet_gconv3x3_workspace_bytes(int64_t B, int32_t C, int32_t cpg, int32_t H, int32_t W, int32_t stride) {
  if (!envelope(B, C, cpg, H, W, stride)) return 0;
  const long long npix = (long long)B * ((H - 1) / stride + 1) * ((W - 1) / stride + 1);
  return (size_t)C * cpg * 9 * wgrad_chunks(npix) * sizeof(float);
}

extern "C" int kgdet_gconv3x3_grad_weight(const float *grad_y, const float *x, float *grad_w, int64_t B, int32_t C, int32_t cpg,
                                          int32_t H, int32_t W, int32_t stride, void *workspace, size_t workspace_bytes,
                                          void *stream) {
  KGDET_CHECK_SHAPE(envelope(B, C, cpg, H, W, stride), "gconv3x3_grad_weight: cpg in {4, 8, 16, 32}, C %% cpg == 0, stride 1 or 2, sizes >= 1");
  KGDET_CHECK_SHAPE(grad_y && x && grad_w && workspace, "gconv3x3_grad_weight: null pointer");
  const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
  const size_t nx = (size_t)B * C * H * W * 4, ny = (size_t)B * C * Ho * Wo * 4, nw = (size_t)C * cpg * 36;
  const size_t need = kgdet_gconv3x3_workspace_bytes(B, C, cpg, H, W, stride);
  KGDET_CHECK_SHAPE(!overlaps(grad_w, nw, grad_y, ny) && !overlaps(grad_w, nw, x, nx) && !overlaps(workspace, need, grad_y, ny) &&
                        !overlaps(workspace, need, x, nx) && !overlaps(workspace, need, grad_w, nw),
                    "gconv3x3_grad_weight: grad_w or the workspace overlaps an operand");
  const long long y_blocks = (long long)C * (cpg / kWgradOC);
  KGDET_CHECK_SHAPE(y_blocks <= 65535 && (long long)H * W < (1LL << 31), "gconv3x3_grad_weight: too large");
  if (workspace_bytes < need) {
    set_error("gconv3x3_grad_weight: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    return KGDET_E_WORKSPACE;
  }
  const long long npix = (long long)B * Ho * Wo;
  const int P = wgrad_chunks(npix);
  const long long chunk = (npix + P - 1) / P;
  const dim3 grid((unsigned)P, (unsigned)y_blocks);
  float *partial = (float *)workspace;
  hipStream_t st = (hipStream_t)stream;
#define KGDET_GCONV_CASE(CPG)                                                                                                   \
  case CPG:                                                                                                                     \
    if (stride == 1)                                                                                                            \
      hipLaunchKernelGGL((gconv_grad_weight<CPG, 1>), grid, dim3(kThreads), 0, st, grad_y, x, partial, C, H, W, Ho, Wo, npix, chunk, P); \
    else                                                                                                                        \
      hipLaunchKernelGGL((gconv_grad_weight<CPG, 2>), grid, dim3(kThreads), 0, st, grad_y, x, partial, C, H, W, Ho, Wo, npix, chunk, P); \
    break;
  switch (cpg) {
    KGDET_GCONV_CASE(4)
    KGDET_GCONV_CASE(8)
    KGDET_GCONV_CASE(16)
    KGDET_GCONV_CASE(32)
  }
#undef KGDET_GCONV_CASE
  KGDET_CHECK_LAUNCH("gconv3x3_grad_weight");
  const long long n = (long long)C * cpg * 9;
  hipLaunchKernelGGL(gconv_grad_weight_sum, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, partial,
                     grad_w, n, P);
  KGDET_CHECK_LAUNCH("gconv3x3_grad_weight_sum");
  return KGDET_OK;
}
