// What the two halves of the dense convolutions share (dense_forward.hip: forward, grad_input, the stem and the weight
// packers; dense_grad_weight.hip: the weight gradients): the operand split, the tile constants and the sum of partials.
//
// All of them are NCHW, fp32 in / fp32 out, computed as bf16 (forward operands: fp16) hi/lo-split MFMA GEMMs for gfx950.
// The ResNet-50 bottleneck (mmdet/models/backbones/resnet.py:142-186, 231-262) is two 1x1 convolutions around a 3x3; with
// the reference's fp32 arithmetic MIOpen runs them at 60-110 TFLOP/s (MI355X fp32 MFMA peak 157; its strided fp32 kernels
// at 15-20).  A 1x1 convolution at these shapes has ~50 flop per byte of fp32 activation traffic, i.e. it sits at ~400
// TFLOP/s on the HBM roofline, and a 3x3 is nine times denser: the matrix pipe, not memory, is what fp32 MFMA leaves on the
// table.  Same arithmetic as the deformable kernels (dcn_forward_plane.hip): every fp32 operand v = hi + lo with
// hi = bf16(v), lo = bf16(v - hi); a product is a_lo*b_hi + a_hi*b_lo + a_hi*b_hi on v_mfma_f32_32x32x16_bf16 with fp32
// accumulation -- ~5e-6 of the output scale (fp32 kernels: ~7e-7) at a third of the bf16 rate.
//
// Everything here has internal linkage: each of the two files compiles its own copy.
#pragma once
#include "common.h"

namespace kgdet {

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

constexpr int kTM = 128, kTN = 128, kTK = 16;
constexpr int kPart = 2 * kTM * 16;          // bytes of one part of one operand stage: [khalf][128][8 bf16]
constexpr int kStage = 2 * kPart;            // hi + lo

// hi = bf16(v), lo = bf16(v - hi) for a PAIR of values: one v_cvt_pk_bf16_f32 for the two hi parts, their float values
// back by a shift and a mask of that dword, one packed subtraction, one v_cvt_pk_bf16_f32 for the lo parts -- 5
// instructions per pair where scalar conversions take 7-8.  These kernels split operands on the fly beside their MFMAs,
// and a SIMD issues both through one port (tools/microbench/mfma_valu.hip): every VALU instruction costs MFMA time.
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void split_pair(float v0, float v1, unsigned &hi, unsigned &lo) {
  const f32x2 v = {v0, v1};
  hi = __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2));
  const f32x2 hf = {__uint_as_float(hi << 16), __uint_as_float(hi & 0xffff0000u)};
  lo = __builtin_bit_cast(unsigned, __builtin_convertvector(v - hf, bf16x2));
}
__device__ __forceinline__ void split8(const float (&v)[8], bf16x8 &hi, bf16x8 &lo) {
  typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
  u32x4 h, l;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    unsigned a, b;
    split_pair(v[2 * i], v[2 * i + 1], a, b);
    h[i] = a;
    l[i] = b;
  }
  hi = __builtin_bit_cast(bf16x8, h);
  lo = __builtin_bit_cast(bf16x8, l);
}

// FORWARD operands (activations x weights) can be split into two fp16 parts instead of two bf16 parts: 22 mantissa bits
// instead of 16 at the same MFMA rate (v_mfma_f32_32x32x16_f16) and the same five conversion instructions per pair
// (v_cvt_pkrtz_f16_f32: the truncation is exact for the hi part's remainder and leaves <= 2^-21 after the lo part).
// Round 3 (tests/golden/make_step_golden.py): against a float64 evaluation of the training step the bf16 split left
// 1.4e-3 on gradient norms and 1.2e-2 on single gradient elements of the classification tower -- all of it from the
// FORWARD features' 5e-6..9e-6 (tools/step_vs_f64.py KGDET_EXP=fwd_exact: 7e-6 with an fp32 forward and the split backward).
// Activations and weights sit inside fp16's range; gradients do not (1e-8 and below), so grad_input / grad_weight
// operands stay bf16 (8 exponent bits).  Values beyond 65504 saturate, below 6e-8 vanish.
// fp16's normal range ends at 6.1e-5: the lo part of a weight of 0.03 (7e-6) would be subnormal and keep ~7 of its 11 bits.
// The pack kernels therefore store fp16-format weights scaled by kF16WeightScale = 2^8 (exact; weights up to 255 in
// magnitude) and the fp16 kernels multiply their accumulators by 2^-8 before the epilogue (exact as well).
// The lower end of that: a weight below ~5e-4 (2^-11) has a subnormal lo part again, an absolute 2^-33 per weight -- a whole ROW of
// such weights (a BatchNorm fold scale near zero) is accurate to 1e-6 of the tensor's scale but not of its own (include/kgdet_hip.h;
// measured on the restated split by tests/test_dense_refs.py).
constexpr float kF16WeightScale = 256.0f;
// "Values beyond 65504 saturate" is made true by the MODE register's FP16_OVFL bit (bit 23: an overflowed FP16 VALU result
// is clamped to +/-MAX_FP16, true infinities stay): set once at the top of every kernel that produces fp16 parts, no
// instruction per element.  Without it v_cvt_pk_f16_f32 rounds |v| > 65504 to inf, hi = inf, lo = v - inf = -inf, and the
// MFMA sum inf + (-inf) is NaN for the whole output channel (round-3 ADVICE; a folded BatchNorm scale gamma / sqrt(var + eps)
// of a channel with a tiny running variance reaches that through w * s * 2^8).  With it: hi = 65504, lo = f16(v - 65504):
// an 11-bit representation up to 131008 (measured on the GPU: 2e-4 of the output scale) and clamped beyond -- finite; the
// fp32-class envelope still ends at 65504 (tests/test_gpu_backbone.py::test_fp16_forward_parts_saturate_instead_of_nan).
// Nothing here enforces the envelope; kgdet_amd/numerics.py checks the weights against it with range_scan.hip (checkpoint load,
// end of epoch) and routes a layer that leaves it to bf16 parts (policy KGDET_ENVELOPE; include/kgdet_hip.h).
__device__ __forceinline__ void f16_saturate_on() {
  __builtin_amdgcn_s_setreg(1 /*HW_REG_MODE*/ | (23 << 6) /*offset*/ | (0 << 11) /*size - 1*/, 1u);
}
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
template <bool F16>
__device__ __forceinline__ void split_pair_t(float v0, float v1, unsigned &hi, unsigned &lo) {
  if constexpr (!F16) {
    split_pair(v0, v1, hi, lo);
  } else {
    // both parts rounded to nearest even (v_cvt_pk_f16_f32 on gfx950); the remainder v - hi is exact in fp32.  Truncated
    // parts (v_cvt_pkrtz_f16_f32) have the sign of v, so the dropped lo * lo term always had the sign of the product: a
    // bias of -6e-8 per layer that grew to -1.4e-6 (both truncated) / -3e-7 (hi truncated) of the rms over the backbone
    const f32x2 v = {v0, v1};
    hi = __builtin_bit_cast(unsigned, __builtin_convertvector(v, f16x2));
    const f32x2 hf = __builtin_convertvector(__builtin_bit_cast(f16x2, hi), f32x2);
    const f32x2 r = v - hf;
    lo = __builtin_bit_cast(unsigned, __builtin_convertvector(r, f16x2));
  }
}
template <bool F16>
__device__ __forceinline__ void split8_t(const float (&v)[8], bf16x8 &hi, bf16x8 &lo) {
  typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
  u32x4 h, l;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    unsigned a, b;
    split_pair_t<F16>(v[2 * i], v[2 * i + 1], a, b);
    h[i] = a;
    l[i] = b;
  }
  hi = __builtin_bit_cast(bf16x8, h);
  lo = __builtin_bit_cast(bf16x8, l);
}
// (bf16x8 is the 16-byte container of either format)
template <bool F16>
__device__ __forceinline__ f32x16 mfma_t(bf16x8 a, bf16x8 b, f32x16 c) {
  if constexpr (F16)
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}

// workgroup b of G -> tile index: the tiles are cut into 8 contiguous runs, one per XCD (block b runs on XCD b % 8)
__device__ __forceinline__ int xcd_tile(int b, int tiles) {
  const int per = (tiles + 7) / 8;
  return (b & 7) * per + (b >> 3);
}

}  // namespace

// out[i] = sum_s parts[s][i], s ascending (deterministic); n a multiple of 2.  Adds the K-split partials of the forward
// kernels and the split partials of the 1x1 weight gradient.
static __global__ __launch_bounds__(256) void conv1x1_sum(const float *__restrict__ parts, float *__restrict__ out,
                                                   long long n, long long stride, int count) {
  for (long long i = (blockIdx.x * 256LL + threadIdx.x) * 2; i < n; i += gridDim.x * 512LL) {
    f32x2 s = {0.0f, 0.0f};
    int k = 0;
    for (; k + 8 <= count; k += 8) {      // eight loads in flight, added in slot order
      f32x2 v[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = *reinterpret_cast<const f32x2 *>(parts + (long long)(k + e) * stride + i);
#pragma unroll
      for (int e = 0; e < 8; ++e) s += v[e];
    }
    for (; k + 2 <= count; k += 2) {
      const f32x2 v0 = *reinterpret_cast<const f32x2 *>(parts + (long long)k * stride + i);
      const f32x2 v1 = *reinterpret_cast<const f32x2 *>(parts + (long long)(k + 1) * stride + i);
      s = (s + v0) + v1;
    }
    for (; k < count; ++k) s += *reinterpret_cast<const f32x2 *>(parts + (long long)k * stride + i);
    *reinterpret_cast<f32x2 *>(out + i) = s;
  }
}

}  // namespace kgdet
