// Dense convolutions, forward side: forward and grad_input of the 1x1 and 3x3 convolutions, the 7x7 stem and the weight
// packers, with their launchers (arithmetic and tile constants: dense_common.h; weight gradients: dense_grad_weight.hip).
//
//   forward      y[b] (O x HoWo) = W (O x C*taps) . patches(x[b])          A = packed W
//   grad_input   gx[b] (C x HW)  = W^T, taps mirrored . patches(gy[b])     A = packed W^T (stride 1: the forward kernels)
//
//   1x1 (stride 1 | 2), 3x3 stride 2 forward     conv_nn<1 | 9, 4 | 5 waves along the pixels>
//   3x3 stride 1 forward and grad_input          conv3x3_patch4<4, 5>, <4, 4>, <2, 4> (64-row halves)
//   3x3 stride 2 grad_input                      conv3x3_s2_grad_input
//   7x7 stride 2 stem                            stem_conv7x7_s2
//   K-split closing pass                         conv1x1_sum | conv1x1_sum_epilogue (| kgdet_bias_act on an odd pixel count)
//
// conv_nn: 128 x 128 (or 160) output tile, 8 (10) waves as 2 (M) x 4 (5) (N); reduction in stages of (16 channels, tap).
//   A stage = 8 KB of the pre-split weight image [part][khalf][128 rows][8 bf16] (one 16-byte load per thread);
//   B stage = 16 activation rows x 128 pixels: a thread owns (pixel, 4 channels), dword loads coalesced along pixels
//   (tap shift = address offset, tap validity = bit of a per-thread mask, stride 2 = input index mapping), split on the
//   fly, 8-byte LDS writes.  Four stages of loads in flight; the main loop has no guarded loads (counted vmcnt); one
//   barrier per stage; XCD-contiguous tile order; K-split + deterministic sum below 200 tiles; optional epilogue (bias,
//   residual, ReLU, gate) in the store.
// plan_nn chooses kernel, pixel tiling and K split once per call; the workspace query and the launch both read it.
//
// Environment overrides (read once per process; driven by tools/time_conv3x3.py and tools/time_one_1x1.py, not part of the API):
//   KGDET_CONV_KS=n       K parts of every launch instead of plan_nn's rule
//   KGDET_CONV_TX=n       conv3x3_patch4: tile width (128-pixel tiles of n x 128 / n)
//   KGDET_CONV_NW=4|5     conv_nn: waves along the pixels
//   KGDET_CONV_HALVES=0|1 conv3x3_patch4: never / always the 64-row half workgroups
#include "dense_common.h"

namespace kgdet {

// Operand image of a [O, C, T] weight (T = 1 or 9 taps): stages ordered (chunk of 16 reduction channels, tap),
// image[mt][k16 * T + t][part][khalf][128][8].
//   transpose = 0 (forward):    rows = O, reduction = C:  A[o][(c, t)] = w[o][c][t]
//   transpose = 1 (grad_input): rows = C, reduction = O:  A[c][(o, t)] = w[o][c][T - 1 - t]   (taps mirrored)
// gridDim.y == 2: block row 0 writes the forward image to img, row 1 the grad_input image to img_t (one launch per
// convolution and step instead of two).
__global__ __launch_bounds__(256) void conv1x1_pack(const float *__restrict__ w, int O, int C, int T, int transpose,
                                                    unsigned char *__restrict__ img, unsigned char *__restrict__ img_t,
                                                    int f16_forward) {
  if (gridDim.y == 2) {
    transpose = blockIdx.y;
    img = blockIdx.y ? img_t : img;
  }
  const bool f16 = f16_forward && !transpose;     // only the forward image (activations x weights) takes fp16 parts
  f16_saturate_on();
  const int M = transpose ? C : O, K = transpose ? O : C;
  const int k16s = (K + kTK - 1) / kTK;     // (a 1x1 weight's reduction may end inside a chunk: zeros up to its end)
  const long long total = (long long)((M + kTM - 1) / kTM) * k16s * T * 2 * kTM;   // (mt, k16, t, khalf, row)
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += gridDim.x * 256LL) {
    const int row = (int)(i % kTM);
    const int khalf = (int)((i / kTM) & 1);
    const long long st = i / (2 * kTM);           // stage index (mt, k16, t)
    const int t = (int)(st % T);
    const int k16 = (int)((st / T) % k16s), mt = (int)(st / ((long long)T * k16s));
    const int m = mt * kTM + row, k0 = k16 * kTK + khalf * 8;
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const long long o = transpose ? k0 + j : m, ch = transpose ? m : k0 + j;
      v[j] = (m < M && k0 + j < K) ? w[(o * C + ch) * T + (transpose ? T - 1 - t : t)] : 0.0f;
    }
    bf16x8 hi, lo;
    if (f16) {
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] *= kF16WeightScale;
      split8_t<true>(v, hi, lo);
    } else {
      split8(v, hi, lo);
    }
    unsigned char *dst = img + st * kStage + khalf * (kTM * 16) + row * 16;
    *reinterpret_cast<bf16x8 *>(dst) = hi;
    *reinterpret_cast<bf16x8 *>(dst + kPart) = lo;
  }
}

// Both operand images of MANY weights in one launch (training re-packs every weight every step: 60 launches of a few
// microseconds each).  desc[i] = {w, img, img_t, (O << 32) | C, (T << 32) | first block, scale}; block b works on descriptor
// i with first_block[i] <= b < first_block[i + 1], one 256-item slice of each image.  scale (or 0): float [O], the images
// are those of w[o] * scale[o] -- a frozen-statistics BatchNorm behind the convolution folded into its weight
// (kgdet_amd/backbone.py _ConvBNActFold).
constexpr int kPackDescWords = 6;
__global__ __launch_bounds__(256) void conv1x1_pack_multi(const long long *__restrict__ desc, int n) {
  int lo = 0, hi = n - 1;   // uniform binary search
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if ((int)(desc[mid * kPackDescWords + 4] & 0xffffffffLL) <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
  }
  const long long *d = desc + lo * kPackDescWords;
  const float *w = reinterpret_cast<const float *>(d[0]);
  const float *scale = reinterpret_cast<const float *>(d[5]);
  const int O = (int)(d[3] >> 32), C = (int)(d[3] & 0xffffffffLL), T = (int)((d[4] >> 32) & 0xffff);
  const bool f16_forward = (d[4] >> 62) & 1;     // forward image in fp16 parts
  f16_saturate_on();
  const long long i = (long long)((int)blockIdx.x - (int)(d[4] & 0xffffffffLL)) * 256 + threadIdx.x;
#pragma unroll
  for (int transpose = 0; transpose < 2; ++transpose) {
    unsigned char *img = reinterpret_cast<unsigned char *>(d[1 + transpose]);
    const int M = transpose ? C : O, K = transpose ? O : C;
    const int k16s = (K + kTK - 1) / kTK;
    const long long total = (long long)((M + kTM - 1) / kTM) * k16s * T * 2 * kTM;
    if (!transpose && T == 9) {
      // forward image of a 3x3 weight: a lane's row is an output channel, whose 8 channels x 9 taps are 72 CONTIGUOUS floats
      // (16-byte aligned: C % 16 == 0) -- one thread reads them once (18 float4) and writes the nine taps' items, instead of
      // nine threads each picking 8 floats 36 bytes apart out of the same 288 bytes
      if (i >= total / 9) continue;
      const int row = (int)(i % kTM), khalf = (int)((i / kTM) & 1);
      const long long s2 = i / (2 * kTM);             // (mt, k16)
      const int k16 = (int)(s2 % k16s), mt = (int)(s2 / k16s);
      const int m = mt * kTM + row, k0 = k16 * kTK + khalf * 8;
      float r[72];
      const f32x4 *src = reinterpret_cast<const f32x4 *>(w + ((long long)min(m, M - 1) * C + k0) * 9);
#pragma unroll
      for (int q = 0; q < 18; ++q) {
        const f32x4 u = src[q];
        r[4 * q] = u[0]; r[4 * q + 1] = u[1]; r[4 * q + 2] = u[2]; r[4 * q + 3] = u[3];
      }
      const float sc9 = (scale && m < M) ? scale[m] : 1.0f;
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = m < M ? r[j * 9 + t] * sc9 : 0.0f;
        bf16x8 hi8, lo8;
        if (f16_forward) {
#pragma unroll
          for (int j = 0; j < 8; ++j) v[j] *= kF16WeightScale;
          split8_t<true>(v, hi8, lo8);
        } else {
          split8(v, hi8, lo8);
        }
        unsigned char *dst = img + (s2 * 9 + t) * kStage + khalf * (kTM * 16) + row * 16;
        *reinterpret_cast<bf16x8 *>(dst) = hi8;
        *reinterpret_cast<bf16x8 *>(dst + kPart) = lo8;
      }
      continue;
    }
    if (i >= total) continue;
    const int row = (int)(i % kTM);
    const int khalf = (int)((i / kTM) & 1);
    const long long st = i / (2 * kTM);
    const int t = (int)(st % T);
    const int k16 = (int)((st / T) % k16s), mt = (int)(st / ((long long)T * k16s));
    const int m = mt * kTM + row, k0 = k16 * kTK + khalf * 8;
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const long long o = transpose ? k0 + j : m, ch = transpose ? m : k0 + j;
      v[j] = (m < M && k0 + j < K) ? w[(o * C + ch) * T + (transpose ? T - 1 - t : t)] : 0.0f;
      if (scale && m < M && k0 + j < K) v[j] *= scale[o];
    }
    bf16x8 hi8, lo8;
    if (f16_forward && !transpose) {
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] *= kF16WeightScale;
      split8_t<true>(v, hi8, lo8);
    } else {
      split8(v, hi8, lo8);
    }
    unsigned char *dst = img + st * kStage + khalf * (kTM * 16) + row * 16;
    *reinterpret_cast<bf16x8 *>(dst) = hi8;
    *reinterpret_cast<bf16x8 *>(dst + kPart) = lo8;
  }
}

// y[b][m][p] = sum_{k, t} A[m][(k, t)] * x[b][k][p + shift(t)]  (zero outside the image): a TAPS = 1 (1x1) or 9 (3x3,
// stride 1, padding 1) convolution as an implicit GEMM.  A as packed image, x [B, K, H*W], y [B, M, H*W].
// 512 threads: 8 waves as 2 (M) x 4 (N), 64 x 32 outputs each -- two waves per SIMD, so one wave's MFMAs cover the
// other's loads / conversions even when a problem has only ~1 tile per CU.  B stage: thread (pixel, k quarter) loads
// 4 channels of its pixel (dword loads, coalesced along pixels; the tap's shift is an address offset, its validity a
// bit of a per-thread mask computed once), splits, writes 8 bytes per part.  A stage: one 16-byte load per thread.
// ksplit > 1: workgroup (tile, part) reduces stages [part * per, ...) and writes y-shaped partial `part` of `y`
// (= a [ksplit][B, M, N] buffer); conv1x1_sum adds the parts.  Used when a problem has too few tiles for 256 CUs.
constexpr int kPF = 4;          // stages of global loads in flight per thread

// NW = 4 | 5 waves along the pixels: tiles of 128 or 160 pixels (640 threads).  A CU finishes a tile at a fixed rate whatever
// shares it (see conv3x3_patch4), so what counts is the number of tiles the fullest CU draws: [2, 128, 100 x 168] is 264 tiles of
// 128 pixels (sixteen CUs draw two) but 210 of 160.
template <int TAPS, int NW = 4, bool F16 = false>
__global__ __launch_bounds__(128 * NW) void conv_nn(const unsigned char *__restrict__ img,
                                                      const float *__restrict__ x, float *__restrict__ y, int M, int K,
                                                      int H, int W, int n_mt, int n_nt, int tiles, int ksplit,
                                                      long long part_stride, int Hin, int Win, int stride,
                                                      const float *__restrict__ bias,
                                                      const float *__restrict__ residual, int relu,
    const float *__restrict__ gate = nullptr) {
  // bias [M] / residual [B, M, H, W] / relu: inference epilogue y = [relu](acc + bias[m] [+ residual]) (ksplit == 1)
  // H x W: the OUTPUT map; Hin x Win: the input map; stride 1 (Hin = H, Win = W) or 2 (H = ceil(Hin / 2), ...)
  constexpr int TN = 32 * NW, kPartB = 2 * TN * 16, kBuf = kStage + 2 * kPartB;   // B part: [khalf][TN][8 bf16]
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * kBuf];   // [buf][A (kStage) | B (hi, lo)]
  if constexpr (F16) f16_saturate_on();
  const int unit = xcd_tile(blockIdx.x, tiles * ksplit);
  if (unit >= tiles * ksplit) return;
  // unit order: the K parts and the m tiles of one (image, pixel tile) adjacent -> they share it through one L2
  const int part = unit % ksplit, tile = unit / ksplit;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave & 1, wn = wave >> 1;
  const int n_local = tid % TN, kq = tid / TN;   // pixel column, quarter of the stage's 16 channels
  const int N = H * W;
  const int S = TAPS * ((K + kTK - 1) / kTK), per = (S + ksplit - 1) / ksplit;
  const int s_begin = part * per, s_end = max(s_begin, min(S, s_begin + per));
  const int stages = s_end - s_begin;
  struct Regs {
    f32x4 a;
    float v[4];
    unsigned live;
  };
  const int mt = tile % n_mt, nt = (tile / n_mt) % n_nt, b = tile / (n_mt * n_nt);
  const int n0 = nt * TN;
  const int p = min(n0 + n_local, N - 1);   // columns past the end re-read the last one: never stored
  unsigned ok = 1u;                          // bit t: tap t of this pixel lies inside the image
  if (TAPS == 9) {
    const int h = (p / W) * stride, w = (p - (p / W) * W) * stride;
    ok = 0u;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int hh = h + t / 3 - 1, ww = w + t % 3 - 1;
      ok |= (hh >= 0 && hh < Hin && ww >= 0 && ww < Win) ? (1u << t) : 0u;
    }
  }
  const int Nin = Hin * Win;
  const int pin = stride == 1 ? p : (p / W) * stride * Win + (p - (p / W) * W) * stride;   // input pixel of tap (0, 0)
  const float *xb = x + (long long)b * K * Nin + pin;
  const unsigned char *ai = img + (long long)mt * S * kStage + (tid & 511) * 16;   // (NW = 5: waves 8, 9 duplicate 0, 1 -- loads stay unconditional)

  f32x16 acc[2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][r] = 0.0f;

  auto issue = [&](int s, Regs &R) {   // clamped: unconditional loads keep hipcc's vmcnt counting exact
    const int sc = s_begin + min(s, stages - 1);
    R.a = *reinterpret_cast<const f32x4 *>(ai + (long long)sc * kStage);
    const int c16 = sc / TAPS, t = sc - c16 * TAPS;
    int shift = 0;
    R.live = 1u;
    if (TAPS == 9) {
      R.live = (ok >> t) & 1u;
      shift = R.live ? (t / 3 - 1) * Win + (t % 3 - 1) : 0;
    }
    const float *xp = xb + (long long)(c16 * kTK + kq * 4) * Nin + shift;
    if (TAPS == 1 && (K & (kTK - 1)) && c16 == K / kTK) {
      // the last chunk of a reduction that is not a multiple of 16 (the head's 588-channel key-point maps): channels past the end
      // re-read the last one -- their weights are the image's zero padding (wave-uniform branch)
#pragma unroll
      for (int j = 0; j < 4; ++j) R.v[j] = xb[(long long)min(c16 * kTK + kq * 4 + j, K - 1) * Nin];
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) R.v[j] = xp[(long long)j * Nin];
    }
  };
  auto commit = [&](int buf, const Regs &R) {
    unsigned char *As = smem + buf * kBuf, *Bs = As + kStage;
    *reinterpret_cast<f32x4 *>(As + (tid & 511) * 16) = R.a;
    uint2 hi, lo;
    split_pair_t<F16>(R.live ? R.v[0] : 0.0f, R.live ? R.v[1] : 0.0f, hi.x, lo.x);
    split_pair_t<F16>(R.live ? R.v[2] : 0.0f, R.live ? R.v[3] : 0.0f, hi.y, lo.y);
    unsigned char *dst = Bs + (kq >> 1) * (TN * 16) + n_local * 16 + (kq & 1) * 8;
    *reinterpret_cast<uint2 *>(dst) = hi;
    *reinterpret_cast<uint2 *>(dst + kPartB) = lo;
  };
  auto multiply = [&](int buf) {   // wave (wm, wn): rows wm*64 .. +63, columns wn*32 .. +31
    const unsigned char *A = smem + buf * kBuf + (lane >> 5) * (kTM * 16) + (wm * 64 + (lane & 31)) * 16;
    const unsigned char *Bp = smem + buf * kBuf + kStage + (lane >> 5) * (TN * 16) + (wn * 32 + (lane & 31)) * 16;
    bf16x8 a[2][2], bb[2];
#pragma unroll
    for (int pt = 0; pt < 2; ++pt) {
      a[pt][0] = *reinterpret_cast<const bf16x8 *>(A + pt * kPart);
      a[pt][1] = *reinterpret_cast<const bf16x8 *>(A + pt * kPart + 32 * 16);
      bb[pt] = *reinterpret_cast<const bf16x8 *>(Bp + pt * kPartB);
    }
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) {   // small terms first
      acc[mi] = mfma_t<F16>(a[1][mi], bb[0], acc[mi]);
      acc[mi] = mfma_t<F16>(a[0][mi], bb[1], acc[mi]);
      acc[mi] = mfma_t<F16>(a[0][mi], bb[0], acc[mi]);
    }
  };
  {
    Regs R[kPF];
#pragma unroll
    for (int i = 0; i < kPF; ++i) issue(i, R[i]);
    commit(0, R[0]);
    // stage s: set s % kPF was committed one body ago and is free -> loads of stage s + kPF; set (s+1) % kPF is
    // converted into the other LDS buffer while stage s is multiplied.  The main loop runs whole groups of kPF
    // bodies with NO condition around the loads (clamped addresses instead): only then does hipcc keep counted
    // s_waitcnt vmcnt(N) across the back edge -- with guarded bodies it drained the queue (vmcnt(0)) every trip.
    const int full = stages / kPF * kPF;
    for (int s0 = 0; s0 < full; s0 += kPF) {
#pragma unroll
      for (int u = 0; u < kPF; ++u) {
        const int s = s0 + u;
        __syncthreads();
        issue(s + kPF, R[u]);
        multiply(s & 1);
        commit((s + 1) & 1, R[(u + 1) % kPF]);   // past the last stage: a clamped duplicate nobody reads
      }
    }
#pragma unroll
    for (int u = 0; u < kPF - 1; ++u) {   // tail: stages full .. stages-1 are already in R[u]; no loads
      const int s = full + u;
      if (s < stages) {
        __syncthreads();
        multiply(s & 1);
        if (s + 1 < stages) commit((s + 1) & 1, R[u + 1]);
      }
    }
  }

  // store: lane holds column (lane & 31) of 16 rows per 32 x 32 block -> 128-byte row segments per half wave
  float *yb = y + (long long)part * part_stride + (long long)b * M * N;
  const int n = n0 + wn * 32 + (lane & 31);
  if constexpr (F16) {
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mi][r] *= 1.0f / kF16WeightScale;
  }
  if (bias || residual) {   // epilogue operands first, all loads in flight at once (clamped addresses, no branches)
    const int nc = min(n, N - 1);
    float add[2][16];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = min(mt * kTM + wm * 64 + mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5), M - 1);
        float v = bias ? bias[m] : 0.0f;
        if (residual) v += residual[((long long)b * M + m) * N + nc];
        add[mi][r] = v;
      }
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mi][r] += add[mi][r];
  }
  if (gate) {   // y *= [gate > 0]: the backward of the ReLU that produced this convolution's input (gate = that input), see
                // kgdet_conv_apply_gated_fmt -- the consumer of y no longer takes a masking pass over it.  (Requesting the 32
                // values before the reduction loop was measured slower: tools/experiments/README.md)
    const int nc = min(n, N - 1);
    float gv[2][16];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = min(mt * kTM + wm * 64 + mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5), M - 1);
        gv[mi][r] = gate[((long long)b * M + m) * N + nc];
      }
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mi][r] = gv[mi][r] > 0.0f ? acc[mi][r] : 0.0f;
  }
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int m = mt * kTM + wm * 64 + mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
      if (m < M && n < N) yb[(long long)m * N + n] = relu ? fmaxf(acc[mi][r], 0.0f) : acc[mi][r];
    }
}

// conv3x3_patch4: 3x3, stride 1, padding 1 with the input PATCH of a tile staged once per 16-channel chunk (conv_nn<9>
// loads, splits and writes the shifted tile once per (chunk, tap): nine times the loads, conversions and address
// arithmetic -- and with two waves per SIMD the instruction count, not MFMA / LDS / HBM, is what bounds it).
// Tile = TY x TX output pixels (TY * TX <= 128 or 160, chosen by the host to fit the map: plan_nn), patch = (TY + 2) x
// (TX + 2) <= 256 pixels, zero outside the image, split once, stored [part][khalf][256][8 bf16]; a tap is an LDS address
// offset.  Four waves per workgroup: wave w owns rows 32 w .. 32 w + 31 of the 128-row tile and ALL pixels of the tile.
// Its A fragments (32 rows x 16 channels, hi + lo = 2 KB per stage) come straight from the packed image in L2 into
// registers -- the image is stored in fragment order -- three stages ahead; only the input patch lives in LDS: no A
// staging, no A commit, 8 LDS fragment reads for 12 MFMAs, and ONE barrier per chunk of nine stages (the patch swap).
// 32 KB of LDS and 4 waves per workgroup: two to three workgroups share a CU, so a launch with slightly more tiles than
// CUs (272 for [2, 128, 100, 168]) does not wait for a CU that drew two large workgroups.  (The 8-wave kernel this
// replaced, with A staged through LDS and a phase trace, left the library with the A/B switch that selected it:
// tools/experiments/README.md.)
// WAVES = 4: the whole 128-row tile; WAVES = 2: a 64-row half of it (twice the workgroups, each with its own copy of the
// patch) -- for launches whose tile count is just above the CU count, where workgroups this small spread evenly.
// NB = 4 | 5 blocks of 32 pixels per tile: a tile of up to 160 pixels (e.g. 4 x 34) lets [2, *, 100, 168] take 250 tiles --
// one per CU -- where 128-pixel tiles need 272: a CU finishes a tile in ~28 us whatever shares it, so the 16 CUs that drew
// two set the time (51 us).
constexpr int kPatchMax = 256;
constexpr int kPatchPart = 2 * kPatchMax * 16;   // bytes of one part of a B patch: [khalf][256][8 bf16]
constexpr int kPatchBuf = 2 * kPatchPart;        // hi + lo
template <int WAVES, int NB, bool F16 = false>
__global__ __launch_bounds__(64 * WAVES) void conv3x3_patch4(const unsigned char *__restrict__ img,
                                                             const float *__restrict__ x, float *__restrict__ y, int M,
                                                             int K, int H, int W, int n_mt, int tiles_x, int n_nt,
                                                             int tiles, int ksplit, long long part_stride, int TX, int TY,
                                                             const float *__restrict__ bias,
                                                             const float *__restrict__ residual, int relu,
    const float *__restrict__ gate = nullptr) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * kPatchBuf];
  if constexpr (F16) f16_saturate_on();
  constexpr int HALVES = 4 / WAVES, THREADS = 64 * WAVES, PXT = kPatchMax / THREADS;   // patch pixels per thread
  const int unit0 = xcd_tile(blockIdx.x, tiles * ksplit * HALVES);
  if (unit0 >= tiles * ksplit * HALVES) return;
  const int half = unit0 % HALVES, unit = unit0 / HALVES;
  const int part = unit % ksplit, tile = unit / ksplit;
  const int tid = threadIdx.x, lane = tid & 63, wave = (tid >> 6) + half * WAVES;
  const int N = H * W;
  const int chunks_all = K / kTK, per = (chunks_all + ksplit - 1) / ksplit;
  const int c_begin = part * per, c_end = max(c_begin, min(chunks_all, c_begin + per));
  const int chunks = c_end - c_begin, stages = chunks * 9;
  const int mt = tile % n_mt, nt = (tile / n_mt) % n_nt, b = tile / (n_mt * n_nt);
  const int y0 = (nt / tiles_x) * TY, x0 = (nt % tiles_x) * TX;
  const int PW = TX + 2, PP = PW * (TY + 2);

  if (mt * kTM + half * 64 >= M) return;   // (a 64-row half beyond the last output channel)
  // B patch: thread -> PXT patch pixels, all 16 channels of the chunk
  bool p_live[PXT];
  int p_off[PXT];
#pragma unroll
  for (int i = 0; i < PXT; ++i) {
    const int pp = tid + i * THREADS;
    const int ppy = pp / PW, ppx = pp - ppy * PW;
    const int iy = y0 - 1 + ppy, ix = x0 - 1 + ppx;
    p_live[i] = pp < PP && iy >= 0 && iy < H && ix >= 0 && ix < W;
    p_off[i] = p_live[i] ? iy * W + ix : 0;
  }
  const float *xb = x + (long long)b * K * N;
  unsigned char *b_dst = smem + tid * 16;

  // this lane's four output pixels (one per 32-pixel block) and their patch addresses (tap (-1, -1))
  int b_rd[NB], o_n[NB];
  bool o_live[NB];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    const int qq = nb * 32 + (lane & 31), q = min(qq, TX * TY - 1);
    const int py = q / TX, px = q - py * TX;
    b_rd[nb] = ((lane >> 5) * kPatchMax + py * PW + px) * 16;
    o_live[nb] = qq < TX * TY && y0 + py < H && x0 + px < W;
    o_n[nb] = o_live[nb] ? (y0 + py) * W + x0 + px : 0;
  }
  const int row_pitch = PW * 16;
  const unsigned char *ag = img + ((long long)mt * chunks_all + min(c_begin, chunks_all - 1)) * 9 * kStage +
                            (lane >> 5) * (kTM * 16) + (wave * 32 + (lane & 31)) * 16;

  f32x16 acc[NB];
#pragma unroll
  for (int i = 0; i < NB; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][r] = 0.0f;

  float bv[PXT][16];
  auto issue_b = [&](int ci) {   // chunk ci of this part (clamped: unconditional loads)
    const float *xp = xb + (long long)min(c_begin + min(ci, chunks - 1), chunks_all - 1) * kTK * N;
#pragma unroll
    for (int i = 0; i < PXT; ++i)
#pragma unroll
      for (int j = 0; j < 16; ++j) bv[i][j] = xp[(long long)j * N + p_off[i]];
  };
  auto commit_b = [&](int buf) {
    // (anchor: pure arithmetic floats freely through hipcc's instruction selection; without it the conversion -- and the
    // wait for the loads it consumes -- lands right behind the loads, at the head of the chunk)
#pragma unroll
    for (int i = 0; i < PXT; ++i)
#pragma unroll
      for (int j = 0; j < 16; ++j) asm volatile("" : "+v"(bv[i][j]));
#pragma unroll
    for (int i = 0; i < PXT; ++i)
#pragma unroll
      for (int kh = 0; kh < 2; ++kh) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = p_live[i] ? bv[i][kh * 8 + j] : 0.0f;
        bf16x8 hi, lo;
        split8_t<F16>(v, hi, lo);
        unsigned char *d = b_dst + i * THREADS * 16 + buf * kPatchBuf + kh * (kPatchMax * 16);
        *reinterpret_cast<bf16x8 *>(d) = hi;
        *reinterpret_cast<bf16x8 *>(d + kPatchPart) = lo;
      }
  };
  bf16x8 AR[3][2];
  auto issue_a = [&](int s, bf16x8 (&r)[2]) {
    const unsigned char *p = ag + (long long)max(min(s, stages - 1), 0) * kStage;
    r[0] = *reinterpret_cast<const bf16x8 *>(p);
    r[1] = *reinterpret_cast<const bf16x8 *>(p + kPart);
  };

  issue_b(0);
#pragma unroll
  for (int j = 0; j < 3; ++j) issue_a(j, AR[j]);
  commit_b(0);
  for (int ci = 0; ci < chunks; ++ci) {
    issue_b(ci + 1);
    __syncthreads();   // patch ci is complete; every wave is done with patch ci - 1
    const unsigned char *bbuf = smem + (ci & 1) * kPatchBuf;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int s = ci * 9 + t;
      const unsigned char *bt = bbuf + (t / 3) * row_pitch + (t % 3) * 16;
      bf16x8 bf[NB][2];
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
        bf[nb][0] = *reinterpret_cast<const bf16x8 *>(bt + b_rd[nb]);
        bf[nb][1] = *reinterpret_cast<const bf16x8 *>(bt + b_rd[nb] + kPatchPart);
      }
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) acc[nb] = mfma_t<F16>(AR[t % 3][1], bf[nb][0], acc[nb]);
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) acc[nb] = mfma_t<F16>(AR[t % 3][0], bf[nb][1], acc[nb]);
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) acc[nb] = mfma_t<F16>(AR[t % 3][0], bf[nb][0], acc[nb]);
      __builtin_amdgcn_sched_barrier(0);
      issue_a(s + 3, AR[t % 3]);
      if (t == 6) commit_b((ci + 1) & 1);   // the next chunk's patch (the barrier above freed that buffer)
      __builtin_amdgcn_sched_barrier(0);
    }
  }

  // store: lane holds pixel (lane & 31) of each 32-pixel block, rows 32 w + (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
  float *yb = y + (long long)part * part_stride + (long long)b * M * N;
  const int m0 = mt * kTM + wave * 32 + 4 * (lane >> 5);
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    if constexpr (F16) {
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[nb][r] *= 1.0f / kF16WeightScale;
    }
    if (bias || residual) {
      float add[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = min(m0 + (r & 3) + 8 * (r >> 2), M - 1);
        float v = bias ? bias[m] : 0.0f;
        if (residual) v += residual[((long long)b * M + m) * N + o_n[nb]];
        add[r] = v;
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[nb][r] += add[r];
    }
    if (gate) {   // (as conv_nn)
      float gv[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) gv[r] = gate[((long long)b * M + min(m0 + (r & 3) + 8 * (r >> 2), M - 1)) * N + o_n[nb]];
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[nb][r] = gv[r] > 0.0f ? acc[nb][r] : 0.0f;
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int m = m0 + (r & 3) + 8 * (r >> 2);
      if (m < M && o_live[nb]) yb[(long long)m * N + o_n[nb]] = relu ? fmaxf(acc[nb][r], 0.0f) : acc[nb][r];
    }
  }
}

// grad_input of the 3x3 STRIDE-2 (padding 1) convolution on the patch machinery.  Output pixel (2i + pa, 2j + qa) receives only the
// taps with ky = 1 (pa = 0) or ky in {0, 2} (pa = 1) -- likewise in x -- each from gy(i + dy, j + dx), dy, dx in {0, 1}:
//   gx[c, 2i+pa, 2j+qa] = sum_o sum_(ky, kx of that parity class) w[o, c, ky, kx] * gy[o, i + (pa + 1 - ky) / 2, j + (qa + 1 - kx) / 2]
// So a tile of gy pixels owns four accumulator sets (the four parity classes of its 2 x 2 output blocks) and the nine taps
// are the nine stages of a chunk as in conv3x3_patch4, each adding into its class: one patch per chunk serves all classes,
// the weight fragments come from the ordinary transposed image (block 8 - (3 ky + kx): its taps are mirrored), and a lane
// stores 2 x 2 adjacent outputs.  64 gy pixels per tile (2 blocks of 32), 4 waves = 128 rows.  (MIOpen's fp32 implicit GEMM
// for this gradient runs at ~100 TFLOP/s plus two layout transposes.)
__global__ __launch_bounds__(256) void conv3x3_s2_grad_input(const unsigned char *__restrict__ img_t,
                                                             const float *__restrict__ gy, float *__restrict__ gx, int M,
                                                             int K, int H, int W, int Hin, int Win, int n_mt, int tiles_x,
                                                             int n_nt, int tiles, int TX, int TY) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * kPatchBuf];
  constexpr int NB = 2;
  const int tile = xcd_tile(blockIdx.x, tiles);
  if (tile >= tiles) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int N = H * W;
  const int chunks = K / kTK, stages = chunks * 9;
  const int mt = tile % n_mt, nt = (tile / n_mt) % n_nt, b = tile / (n_mt * n_nt);
  const int y0 = (nt / tiles_x) * TY, x0 = (nt % tiles_x) * TX;
  const int PW = TX + 2, PP = PW * (TY + 2);

  const int pp = tid;
  const int ppy = pp / PW, ppx = pp - ppy * PW;
  const int iy = y0 - 1 + ppy, ix = x0 - 1 + ppx;
  const bool p_live = pp < PP && iy >= 0 && iy < H && ix >= 0 && ix < W;
  const float *xb = gy + (long long)b * K * N + (p_live ? iy * W + ix : 0);
  unsigned char *b_dst = smem + pp * 16;

  int b_rd[NB], o_y[NB], o_x[NB];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    const int qq = nb * 32 + (lane & 31), q = min(qq, TX * TY - 1);
    const int py = q / TX, px = q - py * TX;
    b_rd[nb] = ((lane >> 5) * kPatchMax + py * PW + px) * 16;
    const bool live = qq < TX * TY && y0 + py < H && x0 + px < W;
    o_y[nb] = live ? 2 * (y0 + py) : Hin;     // (dead lanes: every output row fails the bound test)
    o_x[nb] = 2 * (x0 + px);
  }
  const int row_pitch = PW * 16;
  const unsigned char *ag = img_t + (long long)mt * stages * kStage + (lane >> 5) * (kTM * 16) + (wave * 32 + (lane & 31)) * 16;

  f32x16 acc[4][NB];   // [2 pa + qa][pixel block]
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int i = 0; i < NB; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[c][i][r] = 0.0f;

  float bv[16];
  auto issue_b = [&](int ci) {
    const float *xp = xb + (long long)min(ci, chunks - 1) * kTK * N;
#pragma unroll
    for (int j = 0; j < 16; ++j) bv[j] = xp[(long long)j * N];
  };
  auto commit_b = [&](int buf) {
#pragma unroll
    for (int j = 0; j < 16; ++j) asm volatile("" : "+v"(bv[j]));
#pragma unroll
    for (int kh = 0; kh < 2; ++kh) {
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = p_live ? bv[kh * 8 + j] : 0.0f;
      bf16x8 hi, lo;
      split8(v, hi, lo);
      *reinterpret_cast<bf16x8 *>(b_dst + buf * kPatchBuf + kh * (kPatchMax * 16)) = hi;
      *reinterpret_cast<bf16x8 *>(b_dst + buf * kPatchBuf + kh * (kPatchMax * 16) + kPatchPart) = lo;
    }
  };
  // stage t of a chunk = tap (ky, kx) = (t / 3, t % 3): image block 8 - t
  bf16x8 AR[3][2];
  auto issue_a = [&](int s, bf16x8 (&r)[2]) {
    const int sc = min(s, stages - 1), ci = sc / 9, t = sc - ci * 9;
    const unsigned char *p = ag + (long long)(ci * 9 + 8 - t) * kStage;
    r[0] = *reinterpret_cast<const bf16x8 *>(p);
    r[1] = *reinterpret_cast<const bf16x8 *>(p + kPart);
  };

  issue_b(0);
#pragma unroll
  for (int j = 0; j < 3; ++j) issue_a(j, AR[j]);
  commit_b(0);
  for (int ci = 0; ci < chunks; ++ci) {
    issue_b(ci + 1);
    __syncthreads();
    const unsigned char *bbuf = smem + (ci & 1) * kPatchBuf;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      constexpr int kDummy = 0;
      const int ky = t / 3, kx = t % 3;
      const int cls = 2 * (ky != 1) + (kx != 1), dy = ky == 0, dx = kx == 0;
      const unsigned char *bt = bbuf + (1 + dy) * row_pitch + (1 + dx) * 16;
      bf16x8 bf[NB][2];
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
        bf[nb][0] = *reinterpret_cast<const bf16x8 *>(bt + b_rd[nb]);
        bf[nb][1] = *reinterpret_cast<const bf16x8 *>(bt + b_rd[nb] + kPatchPart);
      }
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) acc[cls][nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(AR[t % 3][1], bf[nb][0], acc[cls][nb], 0, 0, 0);
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) acc[cls][nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(AR[t % 3][0], bf[nb][1], acc[cls][nb], 0, 0, 0);
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) acc[cls][nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(AR[t % 3][0], bf[nb][0], acc[cls][nb], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
      issue_a(ci * 9 + t + 3, AR[t % 3]);
      if (t == 6) commit_b((ci + 1) & 1);
      __builtin_amdgcn_sched_barrier(0);
      (void)kDummy;
    }
  }

  // store: rows 32 w + (r & 3) + 8 (r >> 2) + 4 (lane >> 5); a lane owns the 2 x 2 outputs of its gy pixel
  const long long Nin = (long long)Hin * Win;
  float *xo = gx + (long long)b * M * Nin;
  const int m0 = mt * kTM + wave * 32 + 4 * (lane >> 5);
#pragma unroll
  for (int nb = 0; nb < NB; ++nb)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int m = m0 + (r & 3) + 8 * (r >> 2);
      if (m >= M) continue;
      float *row = xo + (long long)m * Nin;
#pragma unroll
      for (int pa = 0; pa < 2; ++pa) {
        const int oy = o_y[nb] + pa;
        if (oy >= Hin) continue;
#pragma unroll
        for (int qa = 0; qa < 2; ++qa)
          if (o_x[nb] + qa < Win) row[(long long)oy * Win + o_x[nb] + qa] = acc[2 * pa + qa][nb][r];
      }
    }
}

// The stem: 7x7, stride 2, padding 3, 3 -> 64 channels (mmdet/models/backbones/resnet.py:487-488) as an implicit GEMM with
// K = 147 (c, ky, kx) padded to 160 = ten stages of 16.  A tile of 8 x 16 output pixels needs a 21 x 37 x 3 input patch
// (9.3 KB, fp32, in LDS, zero outside the image).  Each lane builds ITS OWN B fragment -- pixel lane & 31, k half lane >> 5 --
// by gathering 8 patch values through a 160-entry offset table and splitting them, so the activations are never staged as
// an operand image; A fragments (64 rows: two 32-row blocks) come straight from the packed weight image in L2.  4 waves,
// wave w = pixels 32 w .. 32 w + 31 of the tile, all 64 rows.  (MIOpen's fp32 Winograd-type kernel for this layer: 220 us.)
constexpr int kStemTY = 8, kStemTX = 16, kStemPH = 2 * kStemTY + 5, kStemPW = 2 * kStemTX + 5, kStemK = 160;

template <bool F16>
__global__ __launch_bounds__(256) void stem_conv7x7_s2(const unsigned char *__restrict__ img, const float *__restrict__ x,
                                                       float *__restrict__ y, int H, int W, int Ho, int Wo, int tiles_x,
                                                       int tiles_per_image) {
  __shared__ float patch[3 * kStemPH * kStemPW];
  __shared__ int koff[kStemK];
  if constexpr (F16) f16_saturate_on();
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x / tiles_per_image, nt = blockIdx.x - b * tiles_per_image;
  const int oy0 = (nt / tiles_x) * kStemTY, ox0 = (nt % tiles_x) * kStemTX;
  const int iy0 = 2 * oy0 - 3, ix0 = 2 * ox0 - 3;
  const float *xb = x + (long long)b * 3 * H * W;
  for (int i = tid; i < 3 * kStemPH * kStemPW; i += 256) {
    const int c = i / (kStemPH * kStemPW), r = i - c * (kStemPH * kStemPW), py = r / kStemPW, px = r - py * kStemPW;
    const int iy = iy0 + py, ix = ix0 + px;
    patch[i] = (iy >= 0 && iy < H && ix >= 0 && ix < W) ? xb[((long long)c * H + iy) * W + ix] : 0.0f;
  }
  if (tid < kStemK) {
    const int c = tid / 49, r = tid - c * 49, ky = r / 7, kx = r - ky * 7;
    koff[tid] = tid < 147 ? c * (kStemPH * kStemPW) + ky * kStemPW + kx : 0;   // (k >= 147: zero weights)
  }
  __syncthreads();
  const int q = wave * 32 + (lane & 31), py = q / kStemTX, px = q - py * kStemTX;
  const float *pbase = patch + (2 * py) * kStemPW + 2 * px;
  const int kh = (lane >> 5) * 8;
  const unsigned char *ag = img + (lane >> 5) * (kTM * 16) + (lane & 31) * 16;
  f32x16 acc[2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][r] = 0.0f;
#pragma unroll
  for (int s = 0; s < kStemK / kTK; ++s) {
    bf16x8 a[2][2];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) {
      a[0][mi] = *reinterpret_cast<const bf16x8 *>(ag + (long long)s * kStage + mi * 32 * 16);
      a[1][mi] = *reinterpret_cast<const bf16x8 *>(ag + (long long)s * kStage + kPart + mi * 32 * 16);
    }
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = pbase[koff[s * kTK + kh + j]];
    bf16x8 bhi, blo;
    split8_t<F16>(v, bhi, blo);
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) {   // small terms first
      acc[mi] = mfma_t<F16>(a[1][mi], bhi, acc[mi]);
      acc[mi] = mfma_t<F16>(a[0][mi], blo, acc[mi]);
      acc[mi] = mfma_t<F16>(a[0][mi], bhi, acc[mi]);
    }
  }
  const int oy = oy0 + py, ox = ox0 + px;
  if (oy < Ho && ox < Wo) {
    float *yb = y + (long long)b * 64 * Ho * Wo + (long long)oy * Wo + ox;
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        yb[(long long)m * Ho * Wo] = F16 ? acc[mi][r] * (1.0f / kF16WeightScale) : acc[mi][r];
      }
  }
}

// the same sum with the convolution's epilogue in its store: out = [relu](sum + bias[channel] [+ residual]), channel =
// (i / HW) % M (a K-split problem is small; the separate epilogue pass it used to take cost a launch, ~5 us of a step each)
__global__ __launch_bounds__(256) void conv1x1_sum_epilogue(const float *__restrict__ parts, float *__restrict__ out,
                                                            long long n, long long stride, int count,
                                                            const float *__restrict__ bias, const float *__restrict__ residual,
                                                            int relu, int M, long long HW,
                                                            const float *__restrict__ gate = nullptr) {
  for (long long i = (blockIdx.x * 256LL + threadIdx.x) * 2; i < n; i += gridDim.x * 512LL) {   // (HW is even: both in one plane)
    f32x2 s = {0.0f, 0.0f};
    int k = 0;
    for (; k + 4 <= count; k += 4) {      // (a K split has at most eight parts) four loads in flight, added in slot order
      f32x2 v[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = *reinterpret_cast<const f32x2 *>(parts + (long long)(k + e) * stride + i);
#pragma unroll
      for (int e = 0; e < 4; ++e) s += v[e];
    }
    for (; k < count; ++k) s += *reinterpret_cast<const f32x2 *>(parts + (long long)k * stride + i);
    if (bias) {
      const float b = bias[(i / HW) % M];
      s[0] += b; s[1] += b;
    }
    if (residual) s += *reinterpret_cast<const f32x2 *>(residual + i);
    if (relu) { s[0] = fmaxf(s[0], 0.0f); s[1] = fmaxf(s[1], 0.0f); }
    if (gate) {
      const f32x2 gv = *reinterpret_cast<const f32x2 *>(gate + i);
      s[0] = gv[0] > 0.0f ? s[0] : 0.0f; s[1] = gv[1] > 0.0f ? s[1] : 0.0f;
    }
    *reinterpret_cast<f32x2 *>(out + i) = s;
  }
}

namespace {

// 16-byte items of one operand image = threads of a pack launch: (row tile, 16-channel chunk, tap, k half, row); an item is
// stored twice (hi, lo)
long long pack_items(int M, int K, int taps) { return (long long)ceil_div(M, kTM) * ceil_div(K, kTK) * taps * 2 * kTM; }
// blocks of a launch that packs the forward and the grad_input image of an [O, C, taps] weight
long long pack_both_blocks(int O, int C, int taps) {
  const long long t0 = pack_items(O, C, taps), t1 = pack_items(C, O, taps);
  return ((t0 > t1 ? t0 : t1) + 255) / 256;
}

// the bf16 or the fp16 instantiation of a kernel, same launch shape and arguments
template <typename Kernel, typename... Args>
void launch_fmt(bool f16, Kernel bf16_kernel, Kernel f16_kernel, unsigned grid, unsigned block, void *stream, Args... args) {
  hipLaunchKernelGGL(f16 ? f16_kernel : bf16_kernel, dim3(grid), dim3(block), 0, (hipStream_t)stream, args...);
}

// K parts of the NN kernel: only when the tiles alone leave most CUs idle
int nn_ksplit(long long tiles, int stages) {
  if (tiles >= 200) return 1;
  int k = (int)((384 + tiles - 1) / tiles);
  const int most = stages / 8;                        // at least 8 stages per part
  if (k > most) k = most;
  if (k > 8) k = 8;
  return k < 1 ? 1 : k;
}

// conv3x3_patch4 (3x3, stride 1) or conv_nn (everything else), the pixel tiling and the K split of one convolution: the
// workspace query and the launch both read it from here
struct NNPlan {
  bool patch, halves;       // halves: conv3x3_patch4<2, 4>, a workgroup per 64-row half of a tile
  int TX, TY, NB, NW, tiles_x, n_nt, ks;
  long long tiles;
};
NNPlan plan_nn(long long B, int M, int K, int H, int W, int taps, int stride) {
  NNPlan p;
  const int Ho = (H + stride - 1) / stride, Wo = (W + stride - 1) / stride;
  const int n_mt = (M + kTM - 1) / kTM;
  p.patch = taps == 9 && stride == 1;
  p.TX = p.TY = p.tiles_x = 0;
  p.NB = p.NW = 4;
  p.n_nt = (int)(((long long)Ho * Wo + kTN - 1) / kTN);
  if (p.patch) {
    // the tile shape with the fewest tiles (ties: the smaller patch); TX >= 8 keeps the stores in >= 32-byte runs.  8 x 16
    // fits every map, so there always is one.
    long long best = -1;
    for (int cap = 128; cap <= (M > 64 ? 160 : 128); cap += 32)   // (M <= 64: the 64-row variant, 4 blocks)
      for (int tx = 8; tx <= 126 && tx <= (W + 7) / 8 * 8; ++tx) {
        const int ty = cap / tx;
        if (ty < 1 || (tx + 2) * (ty + 2) > kPatchMax) continue;
        const long long n = (long long)((H + ty - 1) / ty) * ((W + tx - 1) / tx);
        // time ~ rounds over the 256 CUs x blocks per tile (one CU, one tile at a time: see conv3x3_patch4); below one round
        // and in the many-round regime the tile count itself decides
        const long long units = n * n_mt * B;
        const long long rounds = units <= 256 ? 256 : units <= 512 ? 512 : units;
        const long long cost = (rounds * (cap / 32)) * 4096 + n * 8 + (cap == 160) * 4 + ((tx + 2) * (ty + 2) > 230);
        if (best < 0 || cost < best) { best = cost; p.TX = tx; p.TY = ty; p.NB = cap / 32; }
      }
    static const int force_tx = env_int("KGDET_CONV_TX", 0);
    if (force_tx > 0 && (force_tx + 2) * (128 / force_tx + 2) <= kPatchMax) { p.TX = force_tx; p.TY = 128 / force_tx; p.NB = 4; }
    p.tiles_x = (W + p.TX - 1) / p.TX;
    p.n_nt = p.tiles_x * ((H + p.TY - 1) / p.TY);
  } else {
    // conv_nn: 128- or 160-pixel tiles by the number of tiles the fullest of the 256 CUs draws (x the tile's width); only where
    // no K split is needed anyway, and only for a clear win
    static const int force_nw = env_int("KGDET_CONV_NW", 0);
    const long long hw = (long long)Ho * Wo;
    const long long u4 = (long long)n_mt * ((hw + 127) / 128) * B, u5 = (long long)n_mt * ((hw + 159) / 160) * B;
    const long long c4 = ((u4 + 255) / 256) * 4, c5 = ((u5 + 255) / 256) * 5;
    if (force_nw == 5 || (force_nw == 0 && u4 >= 200 && u5 >= 200 && c5 * 10 <= c4 * 9)) {
      p.NW = 5;
      p.n_nt = (int)((hw + 159) / 160);
    }
  }
  p.tiles = (long long)n_mt * p.n_nt * B;
  p.ks = nn_ksplit(p.tiles, taps * ((K + kTK - 1) / kTK));
  if (p.patch && p.tiles < 200) {
    // conv3x3_patch4: parts of whole chunks (>= 2 each), chosen by rounds over the CUs x chunks per part (+ the partials to add)
    const int chunks = K / kTK;
    double best = 1e30;
    p.ks = 1;
    for (int ks = 1; ks <= 8 && ks * 2 <= chunks; ++ks) {
      // (a chunk of a tile is ~3.5 us of a CU; a partial is written and read once: ~0.114 chunk times per MB of output)
      const double out_mb = (double)B * M * Ho * Wo * 4e-6;
      const double cost = (double)((p.tiles * ks + 255) / 256) * ((chunks + ks - 1) / ks) + 0.114 * out_mb * ks;
      if (cost < best) { best = cost; p.ks = ks; }
    }
  }
  static const int force_ks = env_int("KGDET_CONV_KS", 0);
  if (force_ks > 0) p.ks = force_ks;
  // conv3x3_patch4 with fewer than ~1.6 whole-tile workgroups per CU: 64-row halves (twice the workgroups) spread evenly over the
  // CUs ... and M <= 64 (layer 1): the second half has no rows and leaves at once instead of multiplying zeros.  (The 160-pixel
  // tiles have no half variant.)
  static const int force_halves = env_int("KGDET_CONV_HALVES", -1);
  p.halves = p.patch && p.NB == 4 &&
             (force_halves >= 0 ? force_halves != 0 : ((p.ks == 1 && p.tiles > 256 && p.tiles < 400) || M <= 64));
  return p;
}

// which pass closes a launch of `ks` parts on HW output pixels per plane (kgdet_conv_apply_plan reports these numbers)
enum NNCloser { kCloseStore = 0, kCloseSumEpilogue = 1, kCloseSumBiasAct = 2, kCloseSum = 3 };
NNCloser nn_closer(int ks, long long HW, bool epilogue) {
  if (ks <= 1) return kCloseStore;
  if (!epilogue) return kCloseSum;
  return HW % 2 == 0 ? kCloseSumEpilogue : kCloseSumBiasAct;
}

}  // namespace

}  // namespace kgdet

using namespace kgdet;

extern "C" size_t kgdet_conv_packed_bytes(int32_t M, int32_t K, int32_t taps) {
  if (M <= 0 || K <= 0 || (taps == 9 && K % kTK) || (taps != 1 && taps != 9)) return 0;
  return (size_t)pack_items(M, K, taps) * 32;
}

extern "C" int kgdet_conv_pack_fmt(const float *w, int32_t O, int32_t C, int32_t taps, int32_t transpose, void *packed,
                                   int32_t operand_format, void *stream) {
  // weight [O, C, taps]; transpose = 0: rows O, reduction C (forward); 1: rows C, reduction O, taps mirrored (grad_input)
  const int M = transpose ? C : O, K = transpose ? O : C;
  KGDET_CHECK_SHAPE(taps == 1 || taps == 9, "taps must be 1 (1x1) or 9 (3x3)");
  KGDET_CHECK_SHAPE(O > 0 && C > 0 && (taps == 1 || K % kTK == 0), "reduction length %d is not a multiple of 16", K);
  KGDET_CHECK_SHAPE(w && packed, "null pointer");
  const long long blocks = (pack_items(M, K, taps) + 255) / 256;
  hipLaunchKernelGGL(conv1x1_pack, dim3((unsigned)(blocks > 65535 ? 65535 : blocks)), dim3(256), 0, (hipStream_t)stream, w,
                     O, C, taps, transpose, (unsigned char *)packed, (unsigned char *)nullptr, operand_format == 1 ? 1 : 0);
  KGDET_CHECK_LAUNCH("conv_pack");
  return KGDET_OK;
}

extern "C" int kgdet_conv_pack(const float *w, int32_t O, int32_t C, int32_t taps, int32_t transpose, void *packed,
                               void *stream) {
  return kgdet_conv_pack_fmt(w, O, C, taps, transpose, packed, 0, stream);
}

extern "C" int kgdet_conv_pack_both_fmt(const float *w, int32_t O, int32_t C, int32_t taps, void *packed, void *packed_t,
                                        int32_t forward_format, void *stream) {
  KGDET_CHECK_SHAPE(taps == 1 || taps == 9, "taps must be 1 (1x1) or 9 (3x3)");
  KGDET_CHECK_SHAPE(O > 0 && C > 0 && (taps == 1 || (O % kTK == 0 && C % kTK == 0)), "O and C must be multiples of 16");
  KGDET_CHECK_SHAPE(w && packed && packed_t, "null pointer");
  const long long blocks = pack_both_blocks(O, C, taps);
  hipLaunchKernelGGL(conv1x1_pack, dim3((unsigned)(blocks > 32768 ? 32768 : blocks), 2), dim3(256), 0,
                     (hipStream_t)stream, w, O, C, taps, 0, (unsigned char *)packed, (unsigned char *)packed_t,
                     forward_format == 1 ? 1 : 0);
  KGDET_CHECK_LAUNCH("conv_pack_both");
  return KGDET_OK;
}

extern "C" int kgdet_conv_pack_both(const float *w, int32_t O, int32_t C, int32_t taps, void *packed, void *packed_t,
                                    void *stream) {
  return kgdet_conv_pack_both_fmt(w, O, C, taps, packed, packed_t, 0, stream);
}

extern "C" int64_t kgdet_conv_pack_blocks(int32_t O, int32_t C, int32_t taps) {
  if (O <= 0 || C <= 0 || (taps == 9 && (O % kTK || C % kTK)) || (taps != 1 && taps != 9)) return 0;
  return pack_both_blocks(O, C, taps);
}

extern "C" int kgdet_conv_pack_multi(const int64_t *desc_dev, int32_t n, int64_t total_blocks, void *stream) {
  KGDET_CHECK_SHAPE(desc_dev && n > 0 && total_blocks > 0 && total_blocks < (1LL << 31), "bad descriptor table");
  hipLaunchKernelGGL(conv1x1_pack_multi, dim3((unsigned)total_blocks), dim3(256), 0, (hipStream_t)stream,
                     (const long long *)desc_dev, n);
  KGDET_CHECK_LAUNCH("conv_pack_multi");
  return KGDET_OK;
}

// H, W below are the INPUT map; the output map is ceil(H / stride) x ceil(W / stride) (1x1: padding 0, 3x3: padding 1)
extern "C" size_t kgdet_conv_apply_workspace_bytes(int64_t B, int32_t M, int32_t K, int32_t H, int32_t W,
                                                    int32_t taps, int32_t stride) {
  if (B <= 0 || M <= 0 || K <= 0 || H <= 0 || W <= 0 || (taps == 9 && K % kTK) || stride < 1 || stride > 2) return 0;
  const long long HW = (long long)((H + stride - 1) / stride) * ((W + stride - 1) / stride);
  const int ks = plan_nn(B, M, K, H, W, taps, stride).ks;
  return ks > 1 ? (size_t)ks * B * M * HW * sizeof(float) : 0;
}

extern "C" int kgdet_conv_apply_plan(int64_t B, int32_t M, int32_t K, int32_t H, int32_t W, int32_t taps, int32_t stride,
                                     int32_t out[KGDET_CONV_APPLY_PLAN_WORDS]) {
  KGDET_CHECK_SHAPE(out, "null pointer");
  KGDET_CHECK_SHAPE(B > 0 && M > 0 && K > 0 && H > 0 && W > 0 && (long long)H * W < (1LL << 30), "bad sizes");
  KGDET_CHECK_SHAPE(taps == 1 || taps == 9, "taps must be 1 (1x1) or 9 (3x3)");
  KGDET_CHECK_SHAPE(stride == 1 || stride == 2, "stride must be 1 or 2");
  KGDET_CHECK_SHAPE(taps == 1 || K % kTK == 0, "reduction length %d is not a multiple of 16", K);
  const NNPlan p = plan_nn(B, M, K, H, W, taps, stride);
  KGDET_CHECK_SHAPE(p.tiles < (1LL << 28), "too many tiles");
  const long long HW = (long long)((H + stride - 1) / stride) * ((W + stride - 1) / stride);
  const int32_t words[KGDET_CONV_APPLY_PLAN_WORDS] = {
      p.patch, p.TX, p.TY, p.NB, p.NW, p.ks, p.halves, (int32_t)p.tiles, p.n_nt, nn_closer(p.ks, HW, true), nn_closer(p.ks, HW, false)};
  for (int i = 0; i < KGDET_CONV_APPLY_PLAN_WORDS; ++i) out[i] = words[i];
  return KGDET_OK;
}

extern "C" int kgdet_conv_apply_epilogue_fmt(const void *packed, const float *x, float *y, const float *bias,
                                             const float *residual, int32_t relu, int64_t B, int32_t M, int32_t K,
                                             int32_t H, int32_t W, int32_t taps, int32_t stride, int32_t operand_format,
                                             void *workspace, size_t workspace_bytes, void *stream) {
  return kgdet_conv_apply_gated_fmt(packed, x, y, bias, residual, relu, nullptr, B, M, K, H, W, taps, stride, operand_format,
                                    workspace, workspace_bytes, stream);
}

// ... and `gate` [B, M, Ho, Wo] (or NULL): y = [gate > 0] * ([relu](conv + bias [+ residual])).  In the backward of
// `z = relu(...); u = conv(z)` the gradient of z is conv_grad_input(grad_u) [+ the identity branch's gradient = `residual`], and
// the node that produced z masks it with [z > 0] first thing: with gate = z (this convolution's own forward input) the mask rides
// on this kernel's store and that node's pass over the activation (read gradient, read z, write masked gradient) is not taken.
extern "C" int kgdet_conv_apply_gated_fmt(const void *packed, const float *x, float *y, const float *bias,
                                          const float *residual, int32_t relu, const float *gate, int64_t B, int32_t M,
                                          int32_t K, int32_t H, int32_t W, int32_t taps, int32_t stride,
                                          int32_t operand_format, void *workspace, size_t workspace_bytes, void *stream) {
  const bool f16 = operand_format == 1;      // the image and the on-the-fly split of x in fp16 parts (forward operands)
  KGDET_CHECK_SHAPE(B >= 0 && M > 0 && K > 0 && H >= 0 && W >= 0 && (long long)H * W < (1LL << 30), "bad sizes");
  KGDET_CHECK_SHAPE(taps == 1 || taps == 9, "taps must be 1 (1x1) or 9 (3x3)");
  KGDET_CHECK_SHAPE(stride == 1 || stride == 2, "stride must be 1 or 2");
  KGDET_CHECK_SHAPE(taps == 1 || K % kTK == 0, "reduction length %d is not a multiple of 16", K);
  const int Ho = (H + stride - 1) / stride, Wo = (W + stride - 1) / stride;
  const long long HW = (long long)Ho * Wo;
  if (B * HW == 0) return KGDET_OK;
  KGDET_CHECK_SHAPE(packed && x && y, "null pointer");
  const NNPlan plan = plan_nn(B, M, K, H, W, taps, stride);
  const int n_mt = (M + kTM - 1) / kTM, n_nt = plan.n_nt;
  const long long tiles = plan.tiles;
  KGDET_CHECK_SHAPE(tiles < (1LL << 28), "too many tiles");
  const int ks = plan.ks;
  const long long part_stride = B * M * HW;
  if (ks > 1) {
    KGDET_CHECK_SHAPE(workspace && workspace_bytes >= (size_t)ks * part_stride * sizeof(float), "workspace too small");
    KGDET_CHECK_SHAPE(part_stride % 2 == 0, "B*M*Ho*Wo must be even");
    KGDET_CHECK_SHAPE(!gate || HW % 2 == 0, "a gated K-split convolution needs an even pixel count");
  }
  const unsigned grid = (unsigned)((tiles * ks + 7) / 8) * 8;
  // one part: the kernel stores y with the epilogue; K parts: it stores raw partials and the closing pass below applies it
  float *dst = ks > 1 ? (float *)workspace : y;
  const float *k_bias = ks > 1 ? nullptr : bias, *k_residual = ks > 1 ? nullptr : residual, *k_gate = ks > 1 ? nullptr : gate;
  const int k_relu = ks > 1 ? 0 : relu;
  const unsigned char *img = (const unsigned char *)packed;
  if (plan.patch) {
    auto launch = [&](auto bf16_kernel, auto f16_kernel, unsigned g, unsigned threads) {
      launch_fmt(f16, bf16_kernel, f16_kernel, g, threads, stream, img, x, dst, M, K, H, W, n_mt, plan.tiles_x, n_nt, (int)tiles,
                 ks, part_stride, plan.TX, plan.TY, k_bias, k_residual, k_relu, k_gate);
    };
    if (plan.NB == 5)
      launch(conv3x3_patch4<4, 5, false>, conv3x3_patch4<4, 5, true>, grid, 256);
    else if (plan.halves)
      launch(conv3x3_patch4<2, 4, false>, conv3x3_patch4<2, 4, true>, (unsigned)((tiles * ks * 2 + 7) / 8) * 8, 128);
    else
      launch(conv3x3_patch4<4, 4, false>, conv3x3_patch4<4, 4, true>, grid, 256);
  } else {
    auto launch = [&](auto bf16_kernel, auto f16_kernel, unsigned threads) {
      launch_fmt(f16, bf16_kernel, f16_kernel, grid, threads, stream, img, x, dst, M, K, Ho, Wo, n_mt, n_nt, (int)tiles, ks,
                 part_stride, H, W, stride, k_bias, k_residual, k_relu, k_gate);
    };
    if (taps == 1 && plan.NW == 5)
      launch(conv_nn<1, 5, false>, conv_nn<1, 5, true>, 640);
    else if (taps == 1)
      launch(conv_nn<1, 4, false>, conv_nn<1, 4, true>, 512);
    else if (plan.NW == 5)
      launch(conv_nn<9, 5, false>, conv_nn<9, 5, true>, 640);
    else
      launch(conv_nn<9, 4, false>, conv_nn<9, 4, true>, 512);
  }
  KGDET_CHECK_LAUNCH("conv_nn");
  if (ks > 1) {
    const long long blocks = (part_stride / 2 + 255) / 256;
    const NNCloser closer = nn_closer(ks, HW, bias || residual || relu || gate);
    if (closer == kCloseSumEpilogue)   // the epilogue in the sum's store
      hipLaunchKernelGGL(conv1x1_sum_epilogue, dim3((unsigned)(blocks > 2048 ? 2048 : blocks)), dim3(256), 0,
                         (hipStream_t)stream, (const float *)workspace, y, part_stride, part_stride, ks, bias, residual, relu,
                         M, (long long)HW, gate);
    else
      hipLaunchKernelGGL(conv1x1_sum, dim3((unsigned)(blocks > 2048 ? 2048 : blocks)), dim3(256), 0, (hipStream_t)stream,
                         (const float *)workspace, y, part_stride, part_stride, ks);
    KGDET_CHECK_LAUNCH("conv1x1_sum");
    if (closer == kCloseSumBiasAct) return kgdet_bias_act(y, bias, residual, B, M, HW, 0, relu, 0, stream);
  }
  return KGDET_OK;
}

extern "C" int kgdet_conv_apply_epilogue(const void *packed, const float *x, float *y, const float *bias,
                                         const float *residual, int32_t relu, int64_t B, int32_t M, int32_t K,
                                         int32_t H, int32_t W, int32_t taps, int32_t stride, void *workspace,
                                         size_t workspace_bytes, void *stream) {
  return kgdet_conv_apply_epilogue_fmt(packed, x, y, bias, residual, relu, B, M, K, H, W, taps, stride, 0, workspace,
                                       workspace_bytes, stream);
}

extern "C" int kgdet_conv3x3_s2_grad_input(const void *packed_t, const float *grad_y, float *grad_x, int64_t B, int32_t C,
                                           int32_t O, int32_t Hin, int32_t Win, void *stream) {
  // packed_t: kgdet_conv_pack(w, O, C, 9, transpose = 1) of the forward weight [O, C, 3, 3]; grad_y [B, O, ceil(Hin/2), ceil(Win/2)]
  KGDET_CHECK_SHAPE(B >= 0 && C > 0 && O > 0 && Hin > 0 && Win > 0 && O % kTK == 0, "bad sizes (O must be a multiple of 16)");
  if (B == 0) return KGDET_OK;
  KGDET_CHECK_SHAPE(packed_t && grad_y && grad_x, "null pointer");
  const int H = (Hin + 1) / 2, W = (Win + 1) / 2;
  // 64-pixel tiles of the grad_y map: the shape with the fewest tiles whose patch fits
  int TX = 0, TY = 0;
  long long best = -1;
  for (int tx = 8; tx <= 64; ++tx) {
    const int ty = 64 / tx;
    if (ty < 1 || (tx + 2) * (ty + 2) > kPatchMax) continue;
    const long long n = (long long)((H + ty - 1) / ty) * ((W + tx - 1) / tx);
    const long long cost = n * 1024 + (tx + 2) * (ty + 2);
    if (best < 0 || cost < best) { best = cost; TX = tx; TY = ty; }
  }
  const int n_mt = (C + kTM - 1) / kTM, tiles_x = (W + TX - 1) / TX, n_nt = tiles_x * ((H + TY - 1) / TY);
  const long long tiles = (long long)n_mt * n_nt * B;
  KGDET_CHECK_SHAPE(tiles < (1LL << 28), "too many tiles");
  hipLaunchKernelGGL(conv3x3_s2_grad_input, dim3((unsigned)((tiles + 7) / 8 * 8)), dim3(256), 0, (hipStream_t)stream,
                     (const unsigned char *)packed_t, grad_y, grad_x, C, O, H, W, Hin, Win, n_mt, tiles_x, n_nt, (int)tiles, TX, TY);
  KGDET_CHECK_LAUNCH("conv3x3_s2_grad_input");
  return KGDET_OK;
}

extern "C" int kgdet_stem_conv7x7_s2_fmt(const void *packed, const float *x, float *y, int64_t B, int32_t H, int32_t W,
                                         int32_t operand_format, void *stream) {
  // packed: kgdet_conv_pack of the [64, 3, 7, 7] weight flattened to [64, 147] and zero-padded to [64, 160] (taps = 1,
  // transpose = 0); x [B, 3, H, W] -> y [B, 64, (H - 1) / 2 + 1, (W - 1) / 2 + 1]
  KGDET_CHECK_SHAPE(B >= 0 && H > 0 && W > 0, "bad sizes");
  if (B == 0) return KGDET_OK;
  KGDET_CHECK_SHAPE(packed && x && y, "null pointer");
  const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
  const int tiles_x = (Wo + kStemTX - 1) / kStemTX, tiles_per_image = tiles_x * ((Ho + kStemTY - 1) / kStemTY);
  KGDET_CHECK_SHAPE((long long)B * tiles_per_image < (1LL << 31), "too many tiles");
  launch_fmt(operand_format == 1, stem_conv7x7_s2<false>, stem_conv7x7_s2<true>, (unsigned)(B * tiles_per_image), 256, stream,
             (const unsigned char *)packed, x, y, H, W, Ho, Wo, tiles_x, tiles_per_image);
  KGDET_CHECK_LAUNCH("stem_conv7x7_s2");
  return KGDET_OK;
}

extern "C" int kgdet_stem_conv7x7_s2(const void *packed, const float *x, float *y, int64_t B, int32_t H, int32_t W,
                                     void *stream) {
  return kgdet_stem_conv7x7_s2_fmt(packed, x, y, B, H, W, 0, stream);
}

extern "C" int kgdet_conv_apply(const void *packed, const float *x, float *y, int64_t B, int32_t M, int32_t K, int32_t H,
                                int32_t W, int32_t taps, int32_t stride, void *workspace, size_t workspace_bytes,
                                void *stream) {
  return kgdet_conv_apply_epilogue(packed, x, y, nullptr, nullptr, 0, B, M, K, H, W, taps, stride, workspace,
                                   workspace_bytes, stream);
}
