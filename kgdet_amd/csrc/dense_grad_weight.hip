// Dense convolutions, weight-gradient side: grad_weight of the 1x1 and 3x3 (stride 1 | 2) convolutions with their launchers
// (arithmetic and tile constants: dense_common.h; forward and grad_input: dense_forward.hip).
//
//   grad_weight  gW (O x C*taps) = sum_b gy[b] (O x HW) . patches(x[b])^T
//
// Both operands are activations with the reduction (pixels) contiguous.  The pixel range of the batch is cut into `splits`
// runs; one workgroup per (128 x 128 tile of gW, run) writes a partial, and a closing pass adds the partials in fixed order:
//   product       conv_ntp<1 | 9, aligned | unaligned>  producer / consumer waves, any map, operands read in place
//                 conv_nt8<1 | 9>                       eight symmetric waves, rows of W % 4 == 0 (others: pad_rows2 copies)
//   closing pass  conv1x1_sum (1x1) | conv3x3_wsum (3x3: (tap, channel) -> (channel, tap)) | conv_wsum_fold<T9> (with the
//                 parameter gradients of a BatchNorm folded into the convolution)
//   stride 2      conv_s2_gather9 gathers the nine strided views of x, then the 1x1 problem with 9 C columns
// plan_gw chooses kernel, split count and workspace layout once per call; the three size queries and the five entry points
// all go through plan_gw and launch_gw.  This file reads no environment variable.
#include "dense_common.h"

namespace kgdet {

// Weight gradient of a convolution whose BatchNorm is folded into it (kgdet_amd/backbone.py _ConvBNActFold), the split sum and
// the BatchNorm parameter gradients in ONE pass: workgroup o adds the row's partials G[o][.] (slot order), forms
// dot = <w[o], G[o]>, stores grad_w[o] = s[o] * G[o], and adds the row's BatchNorm partials: grad_beta[o] = sum g,
// grad_gamma[o] = (dot - mean[o] * grad_beta[o]) / sqrt(var[o] + eps)   (csrc/bn_act.hip bn_fold_finish_kernel as the sum's
// epilogue: a launch less per convolution and step).  T9: the partials' columns are (tap, channel), grad_w's (channel, tap).
struct ConvFoldArgs {
  const float *w, *s, *mean, *var, *bn_partial;
  float *grad_beta, *grad_gamma;
  float eps;
  int P;
};
// Launch shape (round 5): ONE workgroup per output channel with as many threads as the row has columns (up to 1024), every
// thread one or two columns, a column's partials requested in batches of 16 -- a row's 16-38 MB / O of partials arrive in one or
// two memory round trips instead of the ~9 dependent ones of the 256-thread form (7.6 / 15.6 us per launch for the 1x1 / 3x3
// problems of the backbone, i.e. 1-2 TB/s on data that sits in the Infinity Cache).  T9: the (tap, channel) -> (channel, tap)
// transposition goes through LDS (the row, <= 18 KB), so that grad_w is stored and w is read in whole lines instead of 4-byte
// pieces 36 bytes apart.
template <bool T9>
__global__ __launch_bounds__(1024) void conv_wsum_fold(const float *__restrict__ parts, float *__restrict__ out, int C,
                                                       long long stride, int count, const ConvFoldArgs f) {
  extern __shared__ float row_s[];       // T9: the summed row in grad_w's column order
  __shared__ float red[2][16];
  const int o = blockIdx.x, CK = T9 ? 9 * C : C;
  const int nthr = blockDim.x, tid = threadIdx.x;
  const float so = f.s[o];
  const float *wr = f.w + (long long)o * CK;
  const float *pr = parts + (long long)o * CK;
  float *gr = out + (long long)o * CK;
  float dot = 0.0f, sb = 0.0f;
  for (int q = tid; q < CK; q += nthr) {                  // the partials' columns (coalesced reads); every column in slot order
    float g0 = 0.0f;
    int k = 0;
    for (; k + 16 <= count; k += 16) {
      float v[16];
#pragma unroll
      for (int e = 0; e < 16; ++e) v[e] = pr[(long long)(k + e) * stride + q];
#pragma unroll
      for (int e = 0; e < 16; ++e) g0 += v[e];
    }
    if (k + 8 <= count) {
      float v[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = pr[(long long)(k + e) * stride + q];
#pragma unroll
      for (int e = 0; e < 8; ++e) g0 += v[e];
      k += 8;
    }
    for (; k < count; ++k) g0 += pr[(long long)k * stride + q];
    if constexpr (T9) {
      row_s[(q % C) * 9 + q / C] = g0;                    // partial column (tap, channel) -> grad_w column (channel, tap)
    } else {
      dot += wr[q] * g0;
      gr[q] = g0 * so;
    }
  }
  if constexpr (T9) {
    __syncthreads();
    for (int j = tid; j < CK; j += nthr) {
      const float g0 = row_s[j];
      dot += wr[j] * g0;
      gr[j] = g0 * so;
    }
  }
  for (int k = tid; k < f.P; k += nthr) sb += f.bn_partial[(long long)o * f.P + k];
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) { dot += __shfl_xor(dot, d); sb += __shfl_xor(sb, d); }
  if ((tid & 63) == 0) { red[0][tid >> 6] = sb; red[1][tid >> 6] = dot; }
  __syncthreads();
  if (tid == 0) {
    float b = 0.0f, d = 0.0f;
    for (int w = 0; w < (nthr >> 6); ++w) { b += red[0][w]; d += red[1][w]; }     // wave order: fixed
    if (f.grad_beta) f.grad_beta[o] = b;
    if (f.grad_gamma) f.grad_gamma[o] = (d - f.mean[o] * b) / sqrtf(f.var[o] + f.eps);
  }
}

// 3x3 grad_weight: out[o][c][t] = sum_s parts[s][o][t * C + c]  (the NT kernel's columns are (tap, channel))
__global__ __launch_bounds__(256) void conv3x3_wsum(const float *__restrict__ parts, float *__restrict__ out, int O, int C,
                                                    int count) {
  const long long n = (long long)O * C * 9;
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < n; i += gridDim.x * 256LL) {
    const int o = (int)(i / (9 * C)), rem = (int)(i - (long long)o * 9 * C), t = rem / C, ch = rem - t * C;
    float s = 0.0f;
    int k = 0;
    for (; k + 8 <= count; k += 8) {   // eight loads in flight, added in slot order
      float v[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = parts[(long long)(k + e) * n + i];
#pragma unroll
      for (int e = 0; e < 8; ++e) s += v[e];
    }
    for (; k < count; ++k) s += parts[(long long)k * n + i];
    out[((long long)o * C + ch) * 9 + t] = s;
  }
}

// grad_weight kernels write partial[split][m][n] (natural [M, N] layout) = sum over the split's pixels (and images) of
// a[b][m][px] * bm[b][n][px]; a [B, M, L], bm [B, N, L], L contiguous.  The B * ceil(L / 16) stages are cut into `splits`
// runs of `per` stages; a stage never straddles two images (the tail of an image is zero-filled); conv1x1_sum /
// conv3x3_wsum add the partials in fixed order.
// conv_nt8: grad_weight with 512 threads (8 waves as 2 x 4, 64 x 32 outputs each, two per SIMD) for maps with
// H*W % 4 == 0.  A thread owns (row, 4-pixel quarter of the stage): one 16-byte load per operand (TAPS == 9 with a
// column shift: two aligned loads + a static selection), 8-byte LDS writes.  
constexpr int kNT8Threads = 512;

template <int TAPS, int DX>
__device__ __forceinline__ void conv_nt8_body(const float *__restrict__ a, const float *__restrict__ bm,
                                              float *__restrict__ partial, int M, int N, int L, int B, int n_mt, int n_nt,
                                              int stages_per_image, int per, int H, int W, int Cin, int unit,
                                              unsigned char *smem, float *__restrict__ row_sums, int rs_stride) {
  const int tile = unit % (n_mt * n_nt), split = unit / (n_mt * n_nt);
  const int mt = tile % n_mt, nt = tile / n_mt;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave & 1, wn = wave >> 1;
  const int row = tid >> 2, q = tid & 3;
  // row_sums[m * rs_stride + split] = sum over the split's pixels of a[., m, .] (the BatchNorm beta gradient of a folded
  // convolution whose output gradient arrived already masked: kgdet_conv*_grad_weight_fold with bn_partial == NULL) -- written by
  // the first column tile of every (row tile, split); the values pass through this thread's registers anyway
  const bool rs_on = row_sums != nullptr && nt == 0;
  float rs = 0.0f;
  const int total = B * stages_per_image;
  const int s_begin = split * per, s_end = min(total, s_begin + per);
  const int am = min(mt * kTM + row, M - 1);
  const bool a_real = mt * kTM + row < M;
  const int tap = TAPS == 9 ? (nt * kTN) / Cin : 0;
  const int dy = TAPS == 9 ? tap / 3 - 1 : 0;
  constexpr int dx = DX, off = dx < 0 ? -4 : 0, sh = dx - off;
  constexpr int NB = (TAPS == 9 && dx != 0) ? 8 : 4;                   // floats of bm a thread loads per stage
  const int bcols = TAPS == 9 ? Cin : N;
  const int bn_raw = TAPS == 9 ? nt * kTN - tap * Cin + row : nt * kTN + row;
  const int bn = min(bn_raw, bcols - 1);
  const bool b_real = bn_raw < bcols;
  const float inv_w = 1.0f / (float)W;

  f32x16 acc[2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][r] = 0.0f;

  struct Regs {
    f32x4 va;
    float vb[NB];
    int p0;
  };
  auto issue = [&](int s, Regs &R) {
    const int sc = min(s, s_end - 1);
    const int img = sc / stages_per_image, st = sc - img * stages_per_image;
    const int p0 = st * kTK + q * 4;
    R.p0 = p0;
    const float *ap = a + ((long long)img * M + am) * L, *bp = bm + ((long long)img * bcols + bn) * L;
    R.va = *reinterpret_cast<const f32x4 *>(ap + min(p0, L - 4));
    const int base = p0 + dy * W + off;
#pragma unroll
    for (int k = 0; k < NB / 4; ++k) {   // clamped chunks hold wrong pixels only where the tap is outside the image
      const f32x4 w = *reinterpret_cast<const f32x4 *>(bp + min(max(base + 4 * k, 0), L - 4));
#pragma unroll
      for (int e = 0; e < 4; ++e) R.vb[4 * k + e] = w[e];
    }
  };
  auto commit = [&](int buf, const Regs &R, bool real = true) {   // real: not the clamped duplicate past the last stage
    unsigned char *As = smem + buf * 2 * kStage, *Bs = As + kStage;
    const bool in_img = R.p0 < L;       // L % 4 == 0: a chunk is entirely inside or outside the image
    bool row_ok = in_img && b_real;
    int w0 = 0;
    if (TAPS == 9) {
      const int h = (int)(((float)R.p0 + 0.5f) * inv_w);
      w0 = R.p0 - h * W;
      row_ok = row_ok && h + dy >= 0 && h + dy < H;
    }
    float fa[4], fb[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      fa[i] = (in_img && a_real) ? R.va[i] : 0.0f;
      const int col = w0 + i + dx;
      const bool ok = TAPS == 9 ? (row_ok && col >= 0 && col < W) : row_ok;
      fb[i] = ok ? R.vb[i + (TAPS == 9 ? sh : 0)] : 0.0f;
    }
    if (rs_on && real) rs += (fa[0] + fa[1]) + (fa[2] + fa[3]);
    uint2 ahi, alo, bhi, blo;
    split_pair(fa[0], fa[1], ahi.x, alo.x);
    split_pair(fa[2], fa[3], ahi.y, alo.y);
    split_pair(fb[0], fb[1], bhi.x, blo.x);
    split_pair(fb[2], fb[3], bhi.y, blo.y);
    const int o = (q >> 1) * (kTM * 16) + row * 16 + (q & 1) * 8;
    *reinterpret_cast<uint2 *>(As + o) = ahi;
    *reinterpret_cast<uint2 *>(As + kPart + o) = alo;
    *reinterpret_cast<uint2 *>(Bs + o) = bhi;
    *reinterpret_cast<uint2 *>(Bs + kPart + o) = blo;
  };
  auto multiply = [&](int buf) {   // wave (wm, wn): rows wm*64 .. +63, columns wn*32 .. +31
    const unsigned char *A = smem + buf * 2 * kStage + (lane >> 5) * (kTM * 16) + (wm * 64 + (lane & 31)) * 16;
    const unsigned char *Bp = smem + buf * 2 * kStage + kStage + (lane >> 5) * (kTN * 16) + (wn * 32 + (lane & 31)) * 16;
    bf16x8 fa[2][2], fb[2];
#pragma unroll
    for (int pt = 0; pt < 2; ++pt) {
      fa[pt][0] = *reinterpret_cast<const bf16x8 *>(A + pt * kPart);
      fa[pt][1] = *reinterpret_cast<const bf16x8 *>(A + pt * kPart + 32 * 16);
      fb[pt] = *reinterpret_cast<const bf16x8 *>(Bp + pt * kPart);
    }
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) {
      acc[mi] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[1][mi], fb[0], acc[mi], 0, 0, 0);
      acc[mi] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[0][mi], fb[1], acc[mi], 0, 0, 0);
      acc[mi] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[0][mi], fb[0], acc[mi], 0, 0, 0);
    }
  };
  constexpr int PF = 4;
  const int n = s_end - s_begin;
  if (n > 0) {
    Regs R[PF];
#pragma unroll
    for (int i = 0; i < PF; ++i) issue(s_begin + i, R[i]);
    commit(0, R[0]);
    const int full = n / PF * PF;   // unguarded bodies in the main loop, load-free tail (see conv_nn)
    for (int j0 = 0; j0 < full; j0 += PF) {
#pragma unroll
      for (int u = 0; u < PF; ++u) {
        const int j = j0 + u;
        __syncthreads();
        issue(s_begin + j + PF, R[u]);
        multiply(j & 1);
        commit((j + 1) & 1, R[(u + 1) % PF], j + 1 < n);
      }
    }
#pragma unroll
    for (int u = 0; u < PF - 1; ++u) {
      const int j = full + u;
      if (j < n) {
        __syncthreads();
        multiply(j & 1);
        if (j + 1 < n) commit((j + 1) & 1, R[u + 1]);
      }
    }
  }
  float *out = partial + (long long)split * M * N;
  const int nn = nt * kTN + wn * 32 + (lane & 31);
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int m = mt * kTM + wm * 64 + mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
      if (m < M && nn < N) out[(long long)m * N + nn] = acc[mi][r];
    }
  if (rs_on) {     // the row's four quarters sit in adjacent lanes: fixed order
    rs += __shfl_xor(rs, 1);
    rs += __shfl_xor(rs, 2);
    if (q == 0 && a_real) row_sums[(long long)(mt * kTM + row) * rs_stride + split] = rs;
  }
}

// units = tiles x splits (> 0): the launch holds ceil(units / 8) * 8 workgroups and workgroup b takes unit xcd_tile(b, units) --
// the tiles of one split (same pixels of both operands; for TAPS == 9 the nine taps re-read the same x rows) run on ONE XCD
// and share its L2 instead of fetching the rows once per XCD.
template <int TAPS>
__global__ __launch_bounds__(kNT8Threads) void conv_nt8(const float *__restrict__ a, const float *__restrict__ bm,
                                                       float *__restrict__ partial, int M, int N, int L, int B, int n_mt,
                                                       int n_nt, int stages_per_image, int per, int H, int W, int Cin,
                                                       int units, float *__restrict__ row_sums = nullptr, int rs_stride = 0) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * 2 * kStage];
  const int unit = units > 0 ? xcd_tile(blockIdx.x, units) : (int)blockIdx.x;
  if (units > 0 && unit >= units) return;
  if (TAPS == 9) {
    const int tile = unit % (n_mt * n_nt), nt = tile / n_mt;
    const int dx = ((nt * kTN) / Cin) % 3 - 1;   // uniform: one tap per tile
    if (dx < 0) conv_nt8_body<TAPS, -1>(a, bm, partial, M, N, L, B, n_mt, n_nt, stages_per_image, per, H, W, Cin, unit, smem, row_sums, rs_stride);
    else if (dx == 0) conv_nt8_body<TAPS, 0>(a, bm, partial, M, N, L, B, n_mt, n_nt, stages_per_image, per, H, W, Cin, unit, smem, row_sums, rs_stride);
    else conv_nt8_body<TAPS, 1>(a, bm, partial, M, N, L, B, n_mt, n_nt, stages_per_image, per, H, W, Cin, unit, smem, row_sums, rs_stride);
  } else {
    conv_nt8_body<TAPS, 0>(a, bm, partial, M, N, L, B, n_mt, n_nt, stages_per_image, per, H, W, Cin, unit, smem, row_sums, rs_stride);
  }
}

// conv_ntp (round 4): the same grad_weight tile (128 x 128 outputs, partial[split][m][n]) with the work of a stage divided
// between PRODUCER and CONSUMER waves instead of done by every wave in turn.  Counters of conv_nt8 on a 3x3, 256 -> 256,
// 50 x 84 problem (gpurun, rocprofv3 --pmc): the MFMA pipe busy 25 % of the kernel, ~76 vector instructions per wave and
// 16-pixel stage for 6 MFMAs (index arithmetic, boundary selects, hi / lo split), vector ALU busy 46 %, the loads served by L2
// in ~185 cycles, 33 MB fetched for 66 MB of operands -- not a bandwidth problem: eight waves that all convert, then all
// multiply, between two barriers per 16 pixels, with both waves of a SIMD in the same phase at the same time.
//   * stage = 32 pixels (a full 128-byte line of every operand row), two LDS stages, ONE barrier per stage;
//   * 4 producer waves: thread = (row of a 32-row pass, 16-byte piece of the 128-byte row segment) -- 8 lanes read one
//     contiguous row segment --, four passes for the 128 rows of each operand, loads two stages ahead in registers;
//     boundary masks of the 3x3 taps once per stage and thread (the four passes share the pixels), none for the grad_y
//     operand (rows beyond M / N are clamped duplicates whose outputs are not stored; pixels beyond the image multiply a
//     zeroed x), image / stage counters advanced incrementally instead of divided out;
//   * 4 consumer waves: 64 x 64 outputs each (four accumulator blocks), per 16 pixels 8 fragment reads for 12 MFMAs
//     (conv_nt8: 6 for 6), products ordered so that consecutive MFMAs never share an accumulator;
//   * LDS: the four (16-pixel step, k half) blocks of a stage start 16 banks apart (kPKH = 2048 + 64 bytes): the producers'
//     8-byte stores of one instruction (8 pieces x 4 rows per half wave) fall on 64 different banks.
constexpr int kPK = 32;                         // pixels per stage
constexpr int kPKH = kTM * 16 + 64;             // [128 rows][8 bf16] + the bank offset
constexpr int kPKS = 2 * kPKH;                  // one 16-pixel MFMA step: two k halves
constexpr int kPPart = 2 * kPKS;                // one part (hi / lo) of one operand's stage
constexpr int kPOperand = 2 * kPPart;
constexpr int kPStage = 2 * kPOperand;          // A + B = 33792 bytes
constexpr int kPCons = 4;                       // consumer waves, 64 x 64 outputs each (eight of 64 x 32: tools/experiments/README.md)
constexpr int kPNI = 2;                         // 32-column blocks per consumer wave
constexpr int kPThreads = kPCons * 64 + 256;
constexpr int kPLds = 2 * kPStage;       // (a request padded beyond 80 KB -- never two workgroups on a CU -- changed nothing)

template <int TAPS, bool PRODUCER, bool ALIGNED>
__device__ __forceinline__ void conv_ntp_role(const float *__restrict__ a, const float *__restrict__ bm,
                                              float *__restrict__ partial, int M, int N, int L, int B, int n_mt, int n_nt,
                                              int stages_per_image, int per, int H, int W, int Cin, int unit,
                                              unsigned char *smem, float *__restrict__ row_sums, int rs_stride) {
  const int tile = unit % (n_mt * n_nt), split = unit / (n_mt * n_nt);
  const int mt = tile % n_mt, nt = tile / n_mt;
  const int total = B * stages_per_image;
  const int s_begin = split * per, s_end = min(total, s_begin + per);
  const int n = s_end - s_begin;
  const int wtid = threadIdx.x, tid = PRODUCER ? wtid - kPCons * 64 : wtid;
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);

  if constexpr (PRODUCER) {
    // 16-byte global loads need 4-byte alignment only on this part (tools/microbench/unaligned_x4.hip: same rate at every
    // shift), so a tap is a shift of the load ADDRESS -- no aligned pair + selection, any map width, any pixel count: the
    // zero-padded copies of rounds 2-3 (pad_rows2 for maps with W % 4 != 0) are gone for this kernel.
    typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));
    const int rp = tid >> 3, q = tid & 7;
    const int tap = TAPS == 9 ? (nt * kTN) / Cin : 0;
    const int dy = TAPS == 9 ? tap / 3 - 1 : 0, dx = TAPS == 9 ? tap % 3 - 1 : 0;
    const int shift = dy * W + dx;                                      // of the flat pixel index
    const int bcols = TAPS == 9 ? Cin : N;
    const int bn0 = TAPS == 9 ? nt * kTN - tap * Cin : nt * kTN;
    int a_off[4], b_off[4];                                             // element offsets of the four rows inside one image
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      a_off[k] = min(mt * kTM + rp + 32 * k, M - 1) * L;
      b_off[k] = min(bn0 + rp + 32 * k, bcols - 1) * L;
    }
    const float inv_w = 1.0f / (float)W;
    // LDS byte offset of this thread's piece inside an operand part: pixels 4q .. 4q + 3 = step q >> 2, k half (q >> 1) & 1
    const int lds_o = (q >> 2) * kPKS + ((q >> 1) & 1) * kPKH + rp * 16 + (q & 1) * 8;

    struct Regs {
      f32x4 va[4], vb[4];
      int p0;
    };
    int img = s_begin / stages_per_image, st = s_begin - img * stages_per_image;   // of the NEXT stage to be issued
    int issued = s_begin;
    const bool rs_on = row_sums != nullptr && nt == 0;      // (as conv_nt8_body: per-row sums of the grad_y operand)
    float rs[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    auto issue = [&](Regs &R) __attribute__((always_inline)) {
      // (past the end of the range: the last stage again -- the loads stay unconditional, nothing is committed from them)
      const int p0 = st * kPK + q * 4;
      R.p0 = p0;
      const float *ai = a + (long long)img * M * L, *bi = bm + (long long)img * bcols * L;
      // a piece that lies inside the image is ONE (4-byte aligned) 16-byte load; the few pieces that straddle the image's first /
      // last pixel under a tap, and the ragged last piece of an image with L % 4 != 0, load their in-range pixels one by one
      const int base = p0 + shift;
      if (p0 <= L - 4 && base >= 0 && base <= L - 4) {
        // (scalar image base + zero-extended 32-bit byte offset: the load's own addressing mode, no 64-bit vector arithmetic)
        const char *ab = reinterpret_cast<const char *>(ai), *bb = reinterpret_cast<const char *>(bi);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const f32x4u ua = *reinterpret_cast<const f32x4u *>(ab + (size_t)((unsigned)(a_off[k] + p0) * 4u));
          const f32x4u ub = *reinterpret_cast<const f32x4u *>(bb + (size_t)((unsigned)(b_off[k] + base) * 4u));
          R.va[k] = f32x4{ua[0], ua[1], ua[2], ua[3]};
          R.vb[k] = f32x4{ub[0], ub[1], ub[2], ub[3]};
        }
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            R.va[k][i] = p0 + i < L ? ai[a_off[k] + p0 + i] : 0.0f;
            R.vb[k][i] = (base + i >= 0 && base + i < L) ? bi[b_off[k] + base + i] : 0.0f;
          }
      }
      if (issued + 1 < s_end) {
        ++issued;
        if (++st == stages_per_image) { st = 0; ++img; }
      }
    };
    auto commit = [&](int buf, const Regs &R) __attribute__((always_inline)) {
      unsigned char *As = smem + buf * kPStage + lds_o, *Bs = As + kPOperand;
      const int p0 = R.p0;
      bool ok[4];
      if constexpr (ALIGNED) {
        // W % 4 == 0 (and so L % 4 == 0): a piece lies inside one row and entirely inside or outside the image -- one row test
        // for the four pixels, a column test for the one pixel a +-1 tap can push out (each vector instruction beside the MFMA
        // wave of its SIMD costs that wave ~10 cycles: the per-pixel form below is ~40 instructions per stage)
        bool row_ok = p0 < L;
        int w0 = 0;
        if (TAPS == 9) {
          const int h0 = (int)(((float)p0 + 0.5f) * inv_w);
          w0 = p0 - h0 * W;
          row_ok = row_ok && (unsigned)(h0 + dy) < (unsigned)H;
        }
        ok[0] = row_ok && (TAPS == 1 || dx >= 0 || w0 > 0);
        ok[1] = ok[2] = row_ok;
        ok[3] = row_ok && (TAPS == 1 || dx <= 0 || w0 + 4 < W);
      } else {
        const int h0 = TAPS == 9 ? (int)(((float)p0 + 0.5f) * inv_w) : 0;
        const int w0 = p0 - h0 * W;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          bool v = p0 + i < L;
          if (TAPS == 9) {
            const bool wrap = w0 + i >= W;                              // (W >= 4: a piece touches at most two rows)
            const int h = h0 + (wrap ? 1 : 0) + dy, w = w0 + i - (wrap ? W : 0) + dx;
            v = v && h >= 0 && h < H && w >= 0 && w < W;
          }
          ok[i] = v;
        }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        f32x4 fa = R.va[k], fb = R.vb[k];
        if (rs_on) rs[k] += (p0 < L) ? (fa[0] + fa[1]) + (fa[2] + fa[3]) : 0.0f;   // (beyond L - 4 the loads zero-filled the rest)
#pragma unroll
        for (int i = 0; i < 4; ++i) fb[i] = ok[i] ? fb[i] : 0.0f;       // pixels outside the image multiply a zero
        uint2 ahi, alo, bhi, blo;
        split_pair(fa[0], fa[1], ahi.x, alo.x);
        split_pair(fa[2], fa[3], ahi.y, alo.y);
        split_pair(fb[0], fb[1], bhi.x, blo.x);
        split_pair(fb[2], fb[3], bhi.y, blo.y);
        *reinterpret_cast<uint2 *>(As + k * 32 * 16) = ahi;
        *reinterpret_cast<uint2 *>(As + kPPart + k * 32 * 16) = alo;
        *reinterpret_cast<uint2 *>(Bs + k * 32 * 16) = bhi;
        *reinterpret_cast<uint2 *>(Bs + kPPart + k * 32 * 16) = blo;
      }
    };
    if (n > 0) {
      Regs R0, R1;
      issue(R0);
      issue(R1);
      commit(0, R0);
      issue(R0);
      __syncthreads();
      for (int j = 0; j < n; j += 2) {
        if (j + 1 < n) commit(1, R1);       // stage j + 1
        issue(R1);                          // stage j + 3
        __syncthreads();
        if (j + 1 < n) {
          if (j + 2 < n) commit(0, R0);     // stage j + 2
          issue(R0);                        // stage j + 4
          __syncthreads();
        }
      }
    }
    if (rs_on) {    // the eight pieces of a row segment sit in adjacent lanes: fixed order
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float v = rs[k];
        v += __shfl_xor(v, 1);
        v += __shfl_xor(v, 2);
        v += __shfl_xor(v, 4);
        const int m = mt * kTM + rp + 32 * k;
        if (q == 0 && m < M) row_sums[(long long)m * rs_stride + split] = v;
      }
    }
  } else {
    const int wm = wave & 1, wn = wave >> 1;           // rows wm * 64 .. + 63, columns wn * 32 * kPNI .. + 32 * kPNI - 1
    f32x16 acc[2][kPNI];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int ni = 0; ni < kPNI; ++ni)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.0f;
    const int fo = (lane >> 5) * kPKH + (lane & 31) * 16;
    auto multiply = [&](int buf) __attribute__((always_inline)) {
      const unsigned char *A = smem + buf * kPStage + fo + wm * 64 * 16;
      const unsigned char *Bp = smem + buf * kPStage + kPOperand + fo + wn * (32 * kPNI) * 16;
      bf16x8 fa[2][2][2], fb[2][2][kPNI];     // [step][part][block]
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int pt = 0; pt < 2; ++pt) {
#pragma unroll
          for (int i = 0; i < 2; ++i) fa[ks][pt][i] = *reinterpret_cast<const bf16x8 *>(A + ks * kPKS + pt * kPPart + i * 32 * 16);
#pragma unroll
          for (int i = 0; i < kPNI; ++i) fb[ks][pt][i] = *reinterpret_cast<const bf16x8 *>(Bp + ks * kPKS + pt * kPPart + i * 32 * 16);
        }
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        // small terms first; the other accumulators' MFMAs between two on the same one
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
          for (int ni = 0; ni < kPNI; ++ni)
            acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[ks][1][mi], fb[ks][0][ni], acc[mi][ni], 0, 0, 0);
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
          for (int ni = 0; ni < kPNI; ++ni)
            acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[ks][0][mi], fb[ks][1][ni], acc[mi][ni], 0, 0, 0);
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
          for (int ni = 0; ni < kPNI; ++ni)
            acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[ks][0][mi], fb[ks][0][ni], acc[mi][ni], 0, 0, 0);
      }
    };
    if (n > 0) {
      __syncthreads();
      for (int j = 0; j < n; j += 2) {
        multiply(0);
        __syncthreads();
        if (j + 1 < n) {
          multiply(1);
          __syncthreads();
        }
      }
    }
    float *out = partial + (long long)split * M * N;
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int ni = 0; ni < kPNI; ++ni) {
        const int nn = nt * kTN + wn * (32 * kPNI) + ni * 32 + (lane & 31);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int m = mt * kTM + wm * 64 + mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
          if (m < M && nn < N) out[(long long)m * N + nn] = acc[mi][ni][r];
        }
      }
  }
}

template <int TAPS, bool ALIGNED>
__global__ __launch_bounds__(kPThreads, 1) void conv_ntp(const float *__restrict__ a, const float *__restrict__ bm,
                                                         float *__restrict__ partial, int M, int N, int L, int B, int n_mt,
                                                         int n_nt, int stages_per_image, int per, int H, int W, int Cin,
                                                         int units, float *__restrict__ row_sums = nullptr, int rs_stride = 0) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int unit = units > 0 ? xcd_tile(blockIdx.x, units) : (int)blockIdx.x;      // (as conv_nt8)
  if (units > 0 && unit >= units) return;
  if (threadIdx.x >= kPCons * 64)
    conv_ntp_role<TAPS, true, ALIGNED>(a, bm, partial, M, N, L, B, n_mt, n_nt, stages_per_image, per, H, W, Cin, unit, smem, row_sums, rs_stride);
  else
    conv_ntp_role<TAPS, false, ALIGNED>(a, bm, partial, M, N, L, B, n_mt, n_nt, stages_per_image, per, H, W, Cin, unit, smem, row_sums, rs_stride);
}

}  // namespace kgdet

// (pad_rows2 and conv_s2_gather9 sit outside the namespace: the names the recorded profiles carry)

// rows of W floats -> rows of Wp floats, zero tail, for two tensors in one launch (blockIdx.y: 0 = a, 1 = b)
__global__ __launch_bounds__(256) void pad_rows2(const float *__restrict__ a, float *__restrict__ ap, long long rows_a,
                                                 const float *__restrict__ b, float *__restrict__ bp, long long rows_b, int W,
                                                 int Wp) {
  const float *src = blockIdx.y ? b : a;
  float *dst = blockIdx.y ? bp : ap;
  const long long n = (blockIdx.y ? rows_b : rows_a) * Wp;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const long long r = i / Wp;
    const int c = (int)(i - r * Wp);
    dst[i] = c < W ? src[r * W + c] : 0.0f;
  }
}

// ---- 3x3 stride-2 padding-1 weight gradient (the bottleneck's conv2 at the head of layers 2-4; the FPN's extra levels) -------------
// grad_w[o][c][ky][kx] = sum_{b, oy, ox} grad_y[b][o][oy][ox] * x[b][c][2 oy + ky - 1][2 ox + kx - 1].  The nine strided views of x are
// gathered once into col [B][(tap, channel)][Ho * Wo] (zero outside the image: 9/4 of x's bytes), and the product over the pixels is the
// 1x1 weight-gradient GEMM with 9 C columns -- conv_nt8<1> / conv_ntp<1>, K split, partials added in slot order by conv3x3_wsum, which
// also turns the (tap, channel) columns into grad_w's (channel, tap) order.  Replaces MIOpen's fp32 `igemm_wrw` + its layout transposes
// (366 us per KGDet step for three convolutions), the last vendor kernels of the training step.
__global__ __launch_bounds__(256) void conv_s2_gather9(const float *__restrict__ x, float *__restrict__ col, int C, int H, int W,
                                                       int Ho, int Wo, long long rows) {
  const int HWo = Ho * Wo;
  const long long total = rows * HWo;           // rows = B * C
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const long long r = i / HWo;                // b * C + c
    const int p = (int)(i - r * HWo), oy = p / Wo, ox = p - oy * Wo;
    const long long b = r / C;
    const int c = (int)(r - b * C);
    const float *xp = x + r * (long long)H * W;
    float *cp = col + (b * 9 * C + c) * (long long)HWo + p;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int yy = 2 * oy + t / 3 - 1, xx = 2 * ox + t % 3 - 1;
      cp[(long long)t * C * HWo] = (yy >= 0 && yy < H && xx >= 0 && xx < W) ? xp[(long long)yy * W + xx] : 0.0f;
    }
  }
}

namespace kgdet {

namespace {

// measured on MI355X (tools/bench_conv1x1_wgrad.py): one workgroup per CU with >= 32 stages each beats finer cuts --
// every extra split is another [M, N] partial written and re-read
int nt_splits(int tiles, int total_stages) {
  // Rounds over the 256 CUs decide: a CU works through a tile's stages at a fixed rate whatever shares it (the chip sits at
  // its 1.4 kW limit in these kernels), so 261 workgroups take two rounds where 252 slightly longer ones take one (3x3,
  // 128 channels: 107 -> 86 us).  Time ~ ceil(tiles * s / 256) / s; ties go to the finer split.
  const int most = (total_stages + 31) / 32;
  double best = 1e30;
  const int s_max = 2 * ((256 + tiles - 1) / tiles) < 128 ? 2 * ((256 + tiles - 1) / tiles) : 128;
  for (int s = 1; s <= s_max; ++s) {
    const double t = (double)((tiles * s + 255) / 256) / s;
    if (t < best) best = t;
  }
  // among the best: the coarsest split that still fills 7/8 of the CUs (fewer partials to add), else the finest
  int splits = 0;
  for (int s = 1; s <= s_max && !splits; ++s)
    if ((double)((tiles * s + 255) / 256) / s <= best * (1.0 + 1e-9) && tiles * s >= 224 && tiles * s <= 256) splits = s;
  for (int s = s_max; s >= 1 && !splits; --s)
    if ((double)((tiles * s + 255) / 256) / s <= best * (1.0 + 1e-9)) splits = s;
  if (splits > most) splits = most;
  if (splits > 128) splits = 128;
  return splits < 1 ? 1 : splits;
}

// threads of conv_wsum_fold for a row of `cols` columns: one column per thread up to 1024 (whole waves)
int fold_threads(int cols) {
  const int t = (cols + 63) / 64 * 64;
  return t < 64 ? 64 : (t > 1024 ? 1024 : t);
}

// Kernel, split count and workspace layout of one weight gradient; the size queries and the launch both read them here.
// grad_y [B, O, H, W], x [B, C, H, W] (a 1x1 problem: H = 1, W = its pixel count).  Which kernel:
//   conv_ntp (measured, tools/bench_conv3x3_wgrad.py / bench_conv1x1_wgrad.py, with the sum pass: 3x3 10-13 % faster than
//     conv_nt8, 1x1 3-5 % slower -- ~17 long stages per workgroup, fill and drain weigh more than the leaner stage) takes the 3x3
//     problems, and every map whose rows (1x1: pixel count) are not a multiple of 4 floats (25 x 42, 13 x 21, 7 x 11), which it
//     reads in place through 4-byte aligned 16-byte loads;
//   conv_nt8 takes the aligned 1x1 problems and whatever conv_ntp's index arithmetic does not cover: rows or maps of fewer than
//     four pixels, 3x3 maps beyond 2^21 pixels, operands beyond 2^30 elements per image.  Its 16-byte row pieces need W % 4 == 0:
//     other maps go through zero-padded copies of both operands (pad_rows2; zero grad_y pixels contribute nothing, and x's zeros
//     are what the out-of-range taps read anyway).
// Workspace = [split partials | padded operand copies | per-row sums of grad_y, [O][splits], for the folded variant called without
// bn_partial], each region 256-byte aligned.  The split count is that of the padded size on every route, and the copies' region
// is reserved for every unaligned map, also where conv_ntp reads in place (known slack: DESIGN.md).
struct GWPlan {
  int n_mt, n_nt, tiles, splits;
  bool use_ntp, padded;       // padded: conv_nt8 on pad_rows2's copies; otherwise the operands are read in place
  long long W, Wp, L, Lp;     // row length and pixel count, true and with the rows padded to a multiple of 4
  int spi, per;               // stages per image / per split of the chosen kernel (conv_ntp: 32 pixels, conv_nt8: 16)
  size_t copies_at, rows_at, bytes;   // byte offsets of the second and third region (the partials start at 0), and the total
};
GWPlan plan_gw(long long B, int O, int C, long long H, long long W, int taps) {
  GWPlan p;
  p.W = W;
  p.Wp = (W + 3) & ~3LL;
  p.L = H * W;
  p.Lp = H * p.Wp;
  p.n_mt = (O + kTM - 1) / kTM;
  p.n_nt = taps == 9 ? 9 * C / kTN : (C + kTN - 1) / kTN;     // (3x3: C % 128 == 0, a column tile lies inside one tap)
  p.tiles = p.n_mt * p.n_nt;
  p.splits = nt_splits(p.tiles, (int)(B * ((p.Lp + kTK - 1) / kTK)));
  const long long widest = O > C ? O : C;
  // (3x3, H * W <= 2^21: conv_ntp derives a stage's row as (int)((p0 + 0.5f) * (1.0f / W)) -- exact while p0 < 2^24 and the
  //  product's rounding error stays below half a row; larger maps take conv_nt8, which counts rows)
  p.use_ntp = taps == 9 ? W >= 4 && p.L >= 4 && p.L <= (1LL << 21) && widest * p.Lp < (1LL << 30)
                        : W % 4 != 0 && W >= 4 && widest * p.L < (1LL << 30);
  p.padded = W % 4 != 0 && !p.use_ntp;
  const long long stage = p.use_ntp ? kPK : kTK, len = p.use_ntp ? p.L : p.Lp;
  p.spi = (int)((len + stage - 1) / stage);
  p.per = (int)((B * p.spi + p.splits - 1) / p.splits);
  p.bytes = (size_t)p.splits * O * C * taps * sizeof(float);
  p.copies_at = align_up(p.bytes, 256);
  if (p.Wp != W) p.bytes = p.copies_at + (size_t)B * (O + C) * p.Lp * sizeof(float);
  p.rows_at = align_up(p.bytes, 256);
  p.bytes = p.rows_at + (size_t)p.splits * O * sizeof(float);
  return p;
}

// pad_rows2 (plan.padded), the product kernel, and the pass that adds the partials in slot order: conv_wsum_fold (`fold`),
// conv3x3_wsum (columns in (tap, channel) order: a 3x3 problem, or wsum_C > 0 -- the stride-2 route, whose 1x1 problem has the
// columns (tap, channel) of a 3x3 weight with wsum_C channels) or conv1x1_sum
int launch_gw(const GWPlan &p, int taps, const float *grad_y, const float *x, float *grad_w, long long B, int O, int C, int H,
              void *workspace, void *stream, const ConvFoldArgs *fold, int wsum_C) {
  unsigned char *ws = static_cast<unsigned char *>(workspace);
  const hipStream_t st = (hipStream_t)stream;
  float *partials = reinterpret_cast<float *>(ws);
  // the folded variant without bn_partial: the kernels below also write the per-row sums of grad_y (one slot per split)
  float *row_sums = (fold && !fold->bn_partial) ? reinterpret_cast<float *>(ws + p.rows_at) : nullptr;
  if (p.padded) {
    float *gyp = reinterpret_cast<float *>(ws + p.copies_at), *xp = gyp + (size_t)B * O * p.Lp;
    const long long rows_a = B * O * H, rows_b = B * C * H;
    const long long blocks = ((rows_a > rows_b ? rows_a : rows_b) * p.Wp + 255) / 256;
    hipLaunchKernelGGL(pad_rows2, dim3((unsigned)(blocks > 4096 ? 4096 : blocks), 2), dim3(256), 0, st, grad_y, gyp, rows_a, x,
                       xp, rows_b, (int)p.W, (int)p.Wp);
    KGDET_CHECK_LAUNCH("pad_rows2");
    grad_y = gyp;
    x = xp;
  }
  const int cols = taps * C, units = p.tiles * p.splits, grid = (units + 7) / 8 * 8, Cin = taps == 9 ? C : 0;
  if (p.use_ntp) {
    if (int rc = allow_lds<conv_ntp<1, false>, conv_ntp<1, true>, conv_ntp<9, false>, conv_ntp<9, true>>(kPLds)) return rc;
    const bool aligned = p.W % 4 == 0;
    const auto kernel = taps == 9 ? (aligned ? conv_ntp<9, true> : conv_ntp<9, false>)
                                  : (aligned ? conv_ntp<1, true> : conv_ntp<1, false>);
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(kPThreads), kPLds, st, grad_y, x, partials, O, cols, (int)p.L, (int)B, p.n_mt,
                       p.n_nt, p.spi, p.per, H, (int)p.W, Cin, units, row_sums, p.splits);
    KGDET_CHECK_LAUNCH(taps == 9 ? "conv_ntp<9>" : "conv_ntp<1>");
  } else {
    hipLaunchKernelGGL(taps == 9 ? conv_nt8<9> : conv_nt8<1>, dim3(grid), dim3(kNT8Threads), 0, st, grad_y, x, partials, O, cols,
                       (int)p.Lp, (int)B, p.n_mt, p.n_nt, p.spi, p.per, H, (int)p.Wp, Cin, units, row_sums, p.splits);
    KGDET_CHECK_LAUNCH(taps == 9 ? "conv_nt8<9>" : "conv_nt8<1>");
  }
  const long long n = (long long)O * cols;
  if (fold) {
    ConvFoldArgs f = *fold;
    if (row_sums) { f.bn_partial = row_sums; f.P = p.splits; }
    if (taps == 9)
      hipLaunchKernelGGL(conv_wsum_fold<true>, dim3(O), dim3(fold_threads(cols)), (size_t)cols * sizeof(float), st, partials,
                         grad_w, C, n, p.splits, f);
    else
      hipLaunchKernelGGL(conv_wsum_fold<false>, dim3(O), dim3(fold_threads(cols)), 0, st, partials, grad_w, C, n, p.splits, f);
    KGDET_CHECK_LAUNCH("conv_wsum_fold");
  } else if (taps == 9 || wsum_C > 0) {
    const long long blocks = (n + 255) / 256;
    hipLaunchKernelGGL(conv3x3_wsum, dim3((unsigned)(blocks > 4096 ? 4096 : blocks)), dim3(256), 0, st, partials, grad_w, O,
                       taps == 9 ? C : wsum_C, p.splits);
    KGDET_CHECK_LAUNCH("conv3x3_wsum");
  } else {
    const long long blocks = (n / 2 + 255) / 256;
    hipLaunchKernelGGL(conv1x1_sum, dim3((unsigned)(blocks > 2048 ? 2048 : blocks)), dim3(256), 0, st, partials, grad_w, n, n,
                       p.splits);
    KGDET_CHECK_LAUNCH("conv1x1_sum");
  }
  return KGDET_OK;
}

// the checks of the five entry points, then plan and launch.  taps == 1: H = 1, W = the pixel count
int grad_weight(int taps, const float *grad_y, const float *x, float *grad_w, int64_t B, int32_t O, int32_t C, int32_t H,
                int64_t W, void *workspace, size_t workspace_bytes, void *stream, const ConvFoldArgs *fold, int wsum_C = 0) {
  if (taps == 9) {
    KGDET_CHECK_SHAPE(B > 0 && O > 0 && C > 0 && H > 0 && W > 0 && (long long)H * (W + 3) < (1LL << 23), "bad sizes");
    if (C % kTN != 0) {
      set_error("conv3x3_grad_weight needs C %% 128 == 0 (C=%d)", C);
      return KGDET_E_UNSUPPORTED;
    }
  } else {
    KGDET_CHECK_SHAPE(B > 0 && O > 0 && C > 0 && W > 0 && W < (1LL << 30), "bad sizes");
  }
  KGDET_CHECK_SHAPE(grad_y && x && grad_w && workspace, "null pointer");
  const GWPlan plan = plan_gw(B, O, C, H, W, taps);
  KGDET_CHECK_SHAPE(workspace_bytes >= plan.bytes, "workspace too small");
  KGDET_CHECK_SHAPE(taps == 9 || ((long long)O * C) % 2 == 0, "O*C must be even");
  return launch_gw(plan, taps, grad_y, x, grad_w, B, O, C, H, workspace, stream, fold, wsum_C);
}

int fold_args(ConvFoldArgs &f, const float *w, const float *s, const float *mean, const float *var, float eps,
              const float *bn_partial, int32_t P, float *grad_beta, float *grad_gamma) {
  KGDET_CHECK_SHAPE(w && s && mean && var && ((bn_partial && P > 0) || (!bn_partial && P == 0)),
                    "null pointer (folded BatchNorm arguments; bn_partial == NULL goes with P == 0)");
  f.w = w; f.s = s; f.mean = mean; f.var = var; f.bn_partial = bn_partial; f.grad_beta = grad_beta; f.grad_gamma = grad_gamma;
  f.eps = eps; f.P = P;
  return KGDET_OK;
}

// the stride-2 route's gathered copy of x (see conv_s2_gather9) at the head of its workspace
size_t conv3x3_s2_col_bytes(int64_t B, int32_t C, int32_t H, int32_t W) {
  const long long HWo = (long long)((H + 1) / 2) * ((W + 1) / 2);
  return align_up((size_t)B * 9 * C * HWo * sizeof(float), 256);
}

}  // namespace

}  // namespace kgdet

using namespace kgdet;

extern "C" size_t kgdet_conv1x1_grad_weight_workspace_bytes(int64_t B, int32_t O, int32_t C, int64_t HW) {
  if (B <= 0 || O <= 0 || C <= 0 || HW <= 0) return 0;
  return plan_gw(B, O, C, 1, HW, 1).bytes;
}

extern "C" size_t kgdet_conv3x3_grad_weight_workspace_bytes(int64_t B, int32_t O, int32_t C, int32_t H, int32_t W) {
  if (B <= 0 || O <= 0 || C <= 0 || H <= 0 || W <= 0) return 0;
  return plan_gw(B, O, C, H, W, 9).bytes;
}

extern "C" int kgdet_conv_grad_weight_plan(int64_t B, int32_t O, int32_t C, int32_t H, int64_t W, int32_t taps,
                                           int32_t out[KGDET_CONV_GRAD_WEIGHT_PLAN_WORDS]) {
  // the checks of grad_weight() above (taps == 1: H = 1, W = the pixel count)
  KGDET_CHECK_SHAPE(out, "null pointer");
  KGDET_CHECK_SHAPE(taps == 1 || taps == 9, "taps must be 1 (1x1) or 9 (3x3)");
  if (taps == 9) {
    KGDET_CHECK_SHAPE(B > 0 && O > 0 && C > 0 && H > 0 && W > 0 && (long long)H * (W + 3) < (1LL << 23), "bad sizes");
    if (C % kTN != 0) {
      set_error("conv3x3_grad_weight needs C %% 128 == 0 (C=%d)", C);
      return KGDET_E_UNSUPPORTED;
    }
  } else {
    KGDET_CHECK_SHAPE(B > 0 && O > 0 && C > 0 && H == 1 && W > 0 && W < (1LL << 30), "bad sizes");
  }
  const GWPlan p = plan_gw(B, O, C, H, W, taps);
  KGDET_CHECK_SHAPE(p.bytes < ((size_t)1 << 39), "workspace beyond what the report can express");
  const int32_t words[KGDET_CONV_GRAD_WEIGHT_PLAN_WORDS] = {
      p.use_ntp, p.padded, p.W % 4 == 0, p.splits, p.spi, p.per, 0, (int32_t)(p.copies_at >> 8), (int32_t)(p.rows_at >> 8),
      p.tiles};
  for (int i = 0; i < KGDET_CONV_GRAD_WEIGHT_PLAN_WORDS; ++i) out[i] = words[i];
  return KGDET_OK;
}

extern "C" size_t kgdet_conv3x3_s2_grad_weight_workspace_bytes(int64_t B, int32_t O, int32_t C, int32_t H, int32_t W) {
  if (B <= 0 || O <= 0 || C <= 0 || H <= 0 || W <= 0) return 0;
  const long long HWo = (long long)((H + 1) / 2) * ((W + 1) / 2);
  return conv3x3_s2_col_bytes(B, C, H, W) + plan_gw(B, O, 9 * C, 1, HWo, 1).bytes;
}

extern "C" int kgdet_conv1x1_grad_weight(const float *grad_y, const float *x, float *grad_w, int64_t B, int32_t O,
                                         int32_t C, int64_t HW, void *workspace, size_t workspace_bytes,
                                         void *stream) {
  return grad_weight(1, grad_y, x, grad_w, B, O, C, 1, HW, workspace, workspace_bytes, stream, nullptr);
}

extern "C" int kgdet_conv1x1_grad_weight_fold(const float *grad_y, const float *x, float *grad_w, int64_t B, int32_t O,
                                              int32_t C, int64_t HW, void *workspace, size_t workspace_bytes, const float *w,
                                              const float *s, const float *mean, const float *var, float eps,
                                              const float *bn_partial, int32_t P, float *grad_beta, float *grad_gamma,
                                              void *stream) {
  ConvFoldArgs f;
  if (int rc = fold_args(f, w, s, mean, var, eps, bn_partial, P, grad_beta, grad_gamma)) return rc;
  return grad_weight(1, grad_y, x, grad_w, B, O, C, 1, HW, workspace, workspace_bytes, stream, &f);
}

extern "C" int kgdet_conv3x3_grad_weight(const float *grad_y, const float *x, float *grad_w, int64_t B, int32_t O,
                                         int32_t C, int32_t H, int32_t W, void *workspace, size_t workspace_bytes,
                                         void *stream) {
  return grad_weight(9, grad_y, x, grad_w, B, O, C, H, W, workspace, workspace_bytes, stream, nullptr);
}

extern "C" int kgdet_conv3x3_grad_weight_fold(const float *grad_y, const float *x, float *grad_w, int64_t B, int32_t O,
                                              int32_t C, int32_t H, int32_t W, void *workspace, size_t workspace_bytes,
                                              const float *w, const float *s, const float *mean, const float *var, float eps,
                                              const float *bn_partial, int32_t P, float *grad_beta, float *grad_gamma,
                                              void *stream) {
  ConvFoldArgs f;
  if (int rc = fold_args(f, w, s, mean, var, eps, bn_partial, P, grad_beta, grad_gamma)) return rc;
  return grad_weight(9, grad_y, x, grad_w, B, O, C, H, W, workspace, workspace_bytes, stream, &f);
}

extern "C" int kgdet_conv3x3_s2_grad_weight(const float *grad_y, const float *x, float *grad_w, int64_t B, int32_t O, int32_t C,
                                            int32_t H, int32_t W, void *workspace, size_t workspace_bytes, void *stream) {
  // x [B, C, H, W], grad_y [B, O, ceil(H/2), ceil(W/2)], grad_w [O, C, 3, 3]
  KGDET_CHECK_SHAPE(B > 0 && O > 0 && C > 0 && H > 0 && W > 0 && (long long)9 * C * ((H + 1) / 2) * ((W + 1) / 2) < (1LL << 30), "bad sizes");
  KGDET_CHECK_SHAPE(grad_y && x && grad_w && workspace, "null pointer");
  KGDET_CHECK_SHAPE(workspace_bytes >= kgdet_conv3x3_s2_grad_weight_workspace_bytes(B, O, C, H, W), "workspace too small");
  KGDET_CHECK_SHAPE(((long long)O * C) % 2 == 0, "O*C must be even");
  const int Ho = (H + 1) / 2, Wo = (W + 1) / 2;
  float *col = static_cast<float *>(workspace);
  const long long total = (long long)B * C * Ho * Wo;
  const long long blocks = (total + 255) / 256;
  hipLaunchKernelGGL(conv_s2_gather9, dim3((unsigned)(blocks > 16384 ? 16384 : blocks)), dim3(256), 0, (hipStream_t)stream, x, col, C,
                     H, W, Ho, Wo, (long long)B * C);
  KGDET_CHECK_LAUNCH("conv_s2_gather9");
  const size_t cb = conv3x3_s2_col_bytes(B, C, H, W);
  return grad_weight(1, grad_y, col, grad_w, B, O, 9 * C, 1, (long long)Ho * Wo, static_cast<unsigned char *>(workspace) + cb,
                     workspace_bytes - cb, stream, nullptr, C);
}
