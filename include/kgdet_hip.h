/*
 * kgdet_hip.h -- C ABI of libkgdet_hip.so, the MI355X (gfx950) implementation of KGDet's hot
 * operators.  Plain pointers and sizes only; every pointer named "device" is HBM memory on the
 * current HIP device, `stream` is a hipStream_t passed as void* (NULL = the null stream).
 *
 * Each entry point replaces one native function that the reference's Python wrappers bind
 * through pybind11 (R = mmdetection/mmdet/ops in the reference tree); the reference interface
 * it stands in for is cited next to it.  Conventions kept from the reference: the caller
 * allocates outputs and gradient buffers, the library writes in place; float32, dense NCHW.
 * Differences (not observable by callers): kernels run on the given stream instead of the
 * legacy default stream, scratch comes from a caller-provided workspace instead of per-call
 * at::zeros, and failures are reported (status code + kgdet_last_error()) instead of printf.
 *
 * Return value: 0 on success, non-zero on error (see KGDET_E_*).
 */
#ifndef KGDET_HIP_H_
#define KGDET_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KGDET_OK 0
#define KGDET_E_SHAPE 1     /* shape/argument check failed (reference: AT_CHECK -> RuntimeError) */
#define KGDET_E_WORKSPACE 2 /* workspace too small */
#define KGDET_E_HIP 3       /* 1x1 convolution, stride 1, float32 NCHW, as bf16 hi/lo-split MFMA GEMMs (fp32-level accuracy) -- the conv1 / conv3 /
 * stride-1 downsample convolutions of the bottleneck, mmdet/models/backbones/resnet.py:142-186, which the reference
 * runs through cuDNN / MIOpen.  No reference native entry point.
 *   taps = 1: 1x1;  taps = 9: 3x3 with stride 1, padding 1, dilation 1 (conv2 of the bottleneck) as an implicit GEMM.
 *   kgdet_conv_pack: weight [O, C, taps] -> operand image; transpose = 0 for the forward (y = W * x), 1 for
 *                       grad_input (gx = W^T * gy, taps mirrored); the reduction length (C resp. O) a multiple of 16.
 *   kgdet_conv_apply: y[b] (M x HoWo) = A (M x K*taps) . patches(x[b]) with A = the packed image; x [B, K, H, W],
 *                       y [B, M, ceil(H / stride), ceil(W / stride)]; stride 1 or 2 (forward only: the transposed
 *                       image gives grad_input for stride 1).
 *   kgdet_conv1x1_grad_weight: grad_w [O, C] = sum_b grad_y[b] (O x HW) . x[b]^T (HW x C); HW even; deterministic
 *                       (per-chunk partial tiles added in fixed order); workspace from the _workspace_bytes query. */
size_t kgdet_conv_packed_bytes(int32_t M, int32_t K, int32_t taps);
int kgdet_conv_pack(const float *w, int32_t O, int32_t C, int32_t taps, int32_t transpose, void *packed, void *stream);
/* operand_format of the *_fmt entry points: 0 = two bf16 parts per fp32 value (16 mantissa bits; every gradient operand),
 * 1 = two fp16 parts (22 bits, fp32-class results at the same MFMA rate) for FORWARD operands.  Envelope of format 1: weights up
 * to 255 in magnitude (the image stores them scaled by 2^8 so that their lo parts stay normal; the kernels scale the
 * accumulators back) and, for an output channel to keep that accuracy against ITS OWN scale, down to ~5e-4 (2^-11): below, the lo
 * part of w * 2^8 is an fp16 subnormal with a quantum of 2^-24, i.e. an absolute 2^-33 per weight -- a row of 1e-5 (a BatchNorm
 * fold scale near zero: a zero-initialised last gamma) keeps 6e-6 of its own output scale, which is still far below 1e-6 of the
 * tensor's scale next to rows of order 0.1 (tests/test_dense_refs.py measures it on the restated split, the kernels give exactly
 * that: tests/test_gpu_dense_kernels.py).  Activations of magnitude ~1e-2 .. 6e4 at full accuracy (<= 1e-6 of the output scale); beyond 65504 they
 * saturate, below ~1e-3 the lo part becomes an fp16 subnormal and the error has an ABSOLUTE floor of ~3e-8 per activation
 * (1e-4 of the output scale at 1e-3) -- the outputs of BatchNorm / GroupNorm-normalised layers sit inside the envelope;
 * format 0 has no floor and 16 bits.  An image packed with format f must be applied with format f; only
 * forward images (transpose = 0) take format 1.  kgdet_conv_pack_multi: bit 62 of a descriptor's last word selects
 * format 1 for that row's forward image.  The plain entry points are format 0.
 * The library does not enforce the envelope: outside it format 1 clamps and still returns KGDET_OK.  The check is the caller's --
 * kgdet_range_scan_multi below scans the weights (limit |w s| <= 65504 / 2^8 = 255.875, s the folded BatchNorm scale), and
 * kgdet_amd/numerics.py runs it when a checkpoint is loaded and at the end of every epoch, policy KGDET_ENVELOPE = bf16 (default:
 * a violating layer's forward image is packed and applied in format 0, which has no range limit) | raise | warn | off.  Not
 * covered: activations of normal runs (numerics.audit scans them on request against 65504 / 131008), the deformable convolutions'
 * operands (packed on their own path) and gradients (format 0 already). */
int kgdet_conv_pack_fmt(const float *w, int32_t O, int32_t C, int32_t taps, int32_t transpose, void *packed,
                        int32_t operand_format, void *stream);
int kgdet_conv_pack_both_fmt(const float *w, int32_t O, int32_t C, int32_t taps, void *packed, void *packed_t,
                             int32_t forward_format, void *stream);
int kgdet_conv_apply_epilogue_fmt(const void *packed, const float *x, float *y, const float *bias, const float *residual,
                                  int32_t relu, int64_t B, int32_t M, int32_t K, int32_t H, int32_t W, int32_t taps,
                                  int32_t stride, int32_t operand_format, void *workspace, size_t workspace_bytes,
                                  void *stream);
/* ... with gate [B, M, Ho, Wo] (nullable): y = [gate > 0] * ([relu](conv + bias [+ residual])).  The backward of the ReLU in
 * front of a convolution (mmdet/models/backbones/resnet.py:240-262: relu(norm(conv(.))) feeding the next conv) applied in the
 * store of that convolution's grad_input kernel, gate = its forward input: the producer of the input then receives its
 * gradient already masked (kgdet_amd/backbone.py _GateLink). */
int kgdet_conv_apply_gated_fmt(const void *packed, const float *x, float *y, const float *bias, const float *residual,
                               int32_t relu, const float *gate, int64_t B, int32_t M, int32_t K, int32_t H, int32_t W,
                               int32_t taps, int32_t stride, int32_t operand_format, void *workspace, size_t workspace_bytes,
                               void *stream);
int kgdet_stem_conv7x7_s2_fmt(const void *packed, const float *x, float *y, int64_t B, int32_t H, int32_t W,
                              int32_t operand_format, void *stream);
/* forward and grad_input images of one weight in one launch (O and C multiples of 16) */
int kgdet_conv_pack_both(const float *w, int32_t O, int32_t C, int32_t taps, void *packed, void *packed_t, void *stream);
/* Both images of n weights in ONE launch (training re-packs every weight every step).  desc_dev: device table of n x 6
 * int64 {weight ptr, image ptr, transposed-image ptr, (O << 32) | C, (taps << 32) | first block, scale ptr or 0}, first
 * block = running sum of kgdet_conv_pack_blocks(O, C, taps) over the preceding entries; total_blocks = the sum over all
 * entries.  scale: float [O]; the images are those of w[o] * scale[o] (a frozen-statistics BatchNorm folded into the weight). */
int64_t kgdet_conv_pack_blocks(int32_t O, int32_t C, int32_t taps);
int kgdet_conv_pack_multi(const int64_t *desc_dev, int32_t n, int64_t total_blocks, void *stream);
size_t kgdet_conv_apply_workspace_bytes(int64_t B, int32_t M, int32_t K, int32_t H, int32_t W, int32_t taps,
                                        int32_t stride); /* mostly 0 */
int kgdet_conv_apply(const void *packed, const float *x, float *y, int64_t B, int32_t M, int32_t K, int32_t H, int32_t W,
                     int32_t taps, int32_t stride, void *workspace, size_t workspace_bytes, void *stream);
/* What kgdet_conv_apply* decides for a shape (host code, launches nothing; the launch reads the same plan).  out[]:
 *   0 patch     1: conv3x3_patch4 (3x3 stride 1), 0: conv_nn
 *   1 TX, 2 TY  conv3x3_patch4's pixel tile (0 for conv_nn)       3 NB  its 32-pixel blocks per tile: 4 | 5
 *   4 NW        conv_nn's waves along the pixels: 4 | 5 (128- or 160-pixel tiles)
 *   5 ks        K parts (> 1: partials in the workspace and a closing pass)
 *   6 halves    1: conv3x3_patch4<2, 4>, a workgroup per 64-row half
 *   7 tiles     output tiles (row tiles x pixel tiles x images)       8 n_nt  pixel tiles per image
 *   9 closer with bias, residual, relu or gate given, 10 closer with none of them:
 *     0 the kernel's own store, 1 conv1x1_sum_epilogue, 2 conv1x1_sum then kgdet_bias_act (odd pixel count: a gate is refused),
 *     3 conv1x1_sum */
#define KGDET_CONV_APPLY_PLAN_WORDS 11
int kgdet_conv_apply_plan(int64_t B, int32_t M, int32_t K, int32_t H, int32_t W, int32_t taps, int32_t stride,
                          int32_t out[KGDET_CONV_APPLY_PLAN_WORDS]);
/* the same with the inference epilogue fused into the store: y = [relu](conv + bias[m] [+ residual]); bias [M] and
 * residual [B, M, Ho, Wo] nullable (the folded-BatchNorm bottleneck at inference, kgdet_amd/backbone.py conv_bn). */
int kgdet_conv_apply_epilogue(const void *packed, const float *x, float *y, const float *bias, const float *residual,
                              int32_t relu, int64_t B, int32_t M, int32_t K, int32_t H, int32_t W, int32_t taps,
                              int32_t stride, void *workspace, size_t workspace_bytes, void *stream);
/* The stem convolution conv1 = Conv2d(3, 64, 7, stride 2, padding 3, bias none) (mmdet/models/backbones/resnet.py:487-488):
 * x [B, 3, H, W] -> y [B, 64, (H-1)/2+1, (W-1)/2+1] with the split-bf16 arithmetic of the other convolutions.  packed: the
 * image kgdet_conv_pack(w160, 64, 160, 1, 0, ...) of the weight flattened to [64, 147] and zero-padded to [64, 160].
 * Forward only (the stem is frozen: frozen_stages >= 0). */
int kgdet_stem_conv7x7_s2(const void *packed, const float *x, float *y, int64_t B, int32_t H, int32_t W, void *stream);
/* grad_x [B, C, Hin, Win] of the 3x3 stride-2 padding-1 convolution (the bottleneck's conv2 at the head of layers 2-4,
 * mmdet/models/backbones/resnet.py:142-186 with stride 2) from grad_y [B, O, ceil(Hin/2), ceil(Win/2)] and the TRANSPOSED image
 * of its weight (kgdet_conv_pack(w, O, C, 9, 1, ...)); O % 16 == 0.  Replaces ATen's convolution_backward (MIOpen). */
int kgdet_conv3x3_s2_grad_input(const void *packed_t, const float *grad_y, float *grad_x, int64_t B, int32_t C, int32_t O,
                                int32_t Hin, int32_t Win, void *stream);
/* grad_w [O, C, 3, 3] of the same stride-2 convolution: x [B, C, H, W], grad_y [B, O, ceil(H/2), ceil(W/2)].  The nine strided views of x are
 * gathered into the workspace once, the product over the pixels runs on the 1x1 weight-gradient kernels (deterministic).  O * C even.
 * Replaces ATen's convolution_backward (MIOpen igemm_wrw + layout transposes), mmdet/models/backbones/resnet.py:142-186. */
size_t kgdet_conv3x3_s2_grad_weight_workspace_bytes(int64_t B, int32_t O, int32_t C, int32_t H, int32_t W);
int kgdet_conv3x3_s2_grad_weight(const float *grad_y, const float *x, float *grad_w, int64_t B, int32_t O, int32_t C, int32_t H,
                                 int32_t W, void *workspace, size_t workspace_bytes, void *stream);
/* Grouped 3x3 convolution, padding 1, dilation 1, stride 1 or 2 (the bottleneck's conv2 of a ResNeXt,
 * mmdet/models/backbones/resnext.py:47-56), csrc/grouped_conv.hip: x [B, C, H, W], w [C, cpg, 3, 3] with cpg in {4, 8, 16, 32}
 * channels per group and C / cpg groups, y [B, C, Ho, Wo], Ho = (H - 1) / stride + 1, likewise Wo.  Plain fp32 operands, one
 * fp32 FMA chain per result, no atomics: every entry point returns the same bits for the same inputs.  The forward takes the
 * inference epilogue y = [relu](conv + bias[c]) (bias [C] nullable).  grad_weight sums over B * Ho * Wo in a fixed order: per
 * workgroup partials in the workspace, then one pass over them.  KGDET_E_SHAPE (nothing written) for another cpg, C % cpg != 0,
 * a stride outside {1, 2}, a null pointer or an output that overlaps another operand; KGDET_E_WORKSPACE for a short workspace. */
int kgdet_gconv3x3_forward(const float *x, const float *w, const float *bias, float *y, int64_t B, int32_t C, int32_t cpg,
                           int32_t H, int32_t W, int32_t stride, int32_t relu, void *stream);
int kgdet_gconv3x3_grad_input(const float *grad_y, const float *w, float *grad_x, int64_t B, int32_t C, int32_t cpg, int32_t H,
                              int32_t W, int32_t stride, void *stream);
size_t kgdet_gconv3x3_workspace_bytes(int64_t B, int32_t C, int32_t cpg, int32_t H, int32_t W, int32_t stride);
int kgdet_gconv3x3_grad_weight(const float *grad_y, const float *x, float *grad_w, int64_t B, int32_t C, int32_t cpg, int32_t H,
                               int32_t W, int32_t stride, void *workspace, size_t workspace_bytes, void *stream);
/* The same convolution at bf16 inference on channels-last storage, csrc/grouped_conv_nhwc.hip: x [B, H, W, C] bf16,
 * w [C][3][3][cpg] bf16 (the channels-last storage of a [C, cpg, 3, 3] tensor), bias fp32 [C] or NULL, y [B, Ho, Wo, C] bf16.
 * S = the sum of the exact bf16 products in fp32 (MFMA).  bias == NULL && relu == 0: y = bf16(S), the raw output that
 * kgdet_conv1x1_nhwc_residual_in takes with in_bias; otherwise y = bf16([relu](fp32(bf16(S)) + bias[c])), a NULL bias read as
 * 0 -- the roundings (to nearest even) of a bf16 convolution followed by kgdet_bias_act.  cpg in {4, 8, 16, 32}, C % cpg == 0,
 * C % 8 == 0, stride 1 or 2, B, H, W >= 1; grid limits: H, W <= 2^30, C <= 64 * 65535, B <= 2^31.  Every pointer 16-byte
 * aligned.  At cpg 4 and 8 the groups of one aligned 16-channel block share an MFMA with zero weights across groups: a
 * non-finite activation there reaches the block's other groups.  One launch on `stream`: no atomics, no workspace, no
 * read-back, equal bits from call to call.  KGDET_E_SHAPE, from the host before any launch with nothing written, for another
 * cpg or stride, C % cpg != 0, C % 8 != 0, a null x / w / y, a misaligned pointer, a size beyond the limits or a y that
 * overlaps an operand. */
int kgdet_gconv3x3_nhwc_bf16(const void *x, const void *w, const float *bias, void *y, int64_t B, int32_t C, int32_t cpg,
                             int32_t H, int32_t W, int32_t stride, int32_t relu, void *stream);
size_t kgdet_conv1x1_grad_weight_workspace_bytes(int64_t B, int32_t O, int32_t C, int64_t HW);
int kgdet_conv1x1_grad_weight(const float *grad_y, const float *x, float *grad_w, int64_t B, int32_t O, int32_t C,
                              int64_t HW, void *workspace, size_t workspace_bytes, void *stream);
/* 3x3 (stride 1, padding 1): grad_w [O, C, 3, 3]; needs C % 128 == 0 (else KGDET_E_UNSUPPORTED).  W % 4 != 0: both operands are
 * copied into the workspace with zero columns up to a multiple of 4 (one launch) first. */
size_t kgdet_conv3x3_grad_weight_workspace_bytes(int64_t B, int32_t O, int32_t C, int32_t H, int32_t W);
int kgdet_conv3x3_grad_weight(const float *grad_y, const float *x, float *grad_w, int64_t B, int32_t O, int32_t C,
                              int32_t H, int32_t W, void *workspace, size_t workspace_bytes, void *stream);
/* What the weight gradients decide for a shape (host code, launches nothing).  taps = 1: H = 1 and W = the pixel count (the
 * stride-2 route asks with C = 9 * its channels and W = its output pixels).  out[]:
 *   0 use_ntp   1: conv_ntp, 0: conv_nt8          1 padded   conv_nt8 on pad_rows2's copies
 *   2 aligned   W % 4 == 0 (conv_ntp<., aligned>) 3 splits   partials the closing pass adds
 *   4 spi       stages per image                  5 per      stages per split
 *   6, 7, 8     offsets of the workspace regions (partials, padded copies, per-row sums of grad_y) in units of 256 bytes
 *   9 tiles     128 x 128 tiles of grad_w */
#define KGDET_CONV_GRAD_WEIGHT_PLAN_WORDS 10
int kgdet_conv_grad_weight_plan(int64_t B, int32_t O, int32_t C, int32_t H, int64_t W, int32_t taps,
                                int32_t out[KGDET_CONV_GRAD_WEIGHT_PLAN_WORDS]);

/* Frozen-statistics BatchNorm (+ residual add) (+ ReLU) in one pass -- the norm_eval=True training path of
 * mmdet/models/backbones/resnet.py:240-262,518-525.  float32, NCHW: x, residual, y [N, C, HW]; gamma, beta (nullable:
 * 1 / 0), mean, var [C].     y = [relu](x * s + t [+ residual]),  s = gamma / sqrt(var + eps),  t = beta - mean * s.
 * y may alias x when x is not needed by a later backward. */
int kgdet_bn_act_forward(const float *x, const float *gamma, const float *beta, const float *mean, const float *var,
                         float eps, const float *residual, float *y, int64_t N, int32_t C, int64_t HW, int32_t relu,
                         void *stream);
/* Backward of the above.  g' = grad_y * [y > 0] (relu) else grad_y;  grad_x = g' * s (grad_x nullable);
 * grad_residual = g' is WRITTEN only when has_residual && relu (otherwise it equals grad_y and the caller reuses
 * that tensor); y is read only in that case.  partial: [2][C][P] with P = kgdet_bn_act_partials(N, C, HW):
 * partial[0][c][:] sums to grad_beta[c], partial[1][c][:] to grad_gamma[c] (per-workgroup partials in a fixed order:
 * deterministic, no atomics).  sums (nullable): [2][C] = the partials added in slot order by a second tiny launch --
 * sums[0] = grad_beta, sums[1] = grad_gamma; NULL: the caller adds them. */
int32_t kgdet_bn_act_partials(int64_t N, int32_t C, int64_t HW);
int kgdet_bn_act_backward(const float *grad_y, const float *x, const float *y, const float *gamma, const float *beta,
                          const float *mean, const float *var, float eps, int32_t has_residual, int32_t relu,
                          float *grad_x, float *grad_residual, float *partial, float *sums, int64_t N, int32_t C,
                          int64_t HW, void *stream);
/* Frozen-statistics BatchNorm folded into the convolution in front of it (mmdet resnet.py:518-525 norm_eval; replaces the
 * separate BatchNorm pass of resnet.py:240-262): the forward is kgdet_conv_apply_epilogue* with the image of w * s and bias t.
 * Backward: g = grad_z * [z > 0] (relu; without relu only the channel sums are formed and g is not written) + per-workgroup
 * partial channel sums [C][P], P = kgdet_bn_act_partials(N, C, HW); then per convolution kgdet_bn_fold_finish:
 * grad_beta = sum of partials, grad_gamma = (<w[o], G[o]> - mean * grad_beta) / sqrt(var + eps) with G the weight gradient
 * of conv(x, .) against g, and G scaled by s in place (= grad_w).  Deterministic. */
/* Inference, bf16 channels-last: conv3 + folded bn3 + identity add + ReLU of a bottleneck (mmdet/models/backbones/resnet.py:
 * 240-262) as ONE kernel: out[m][n] = [relu](bf16(sum_k x[m][k] weight[n][k]) + bias[n] + residual[m][n]); x [M, K], weight
 * [N, K], residual / out [M, N] bf16 (M = B*H*W), bias fp32 [N]; K % 16 == 0, K <= 512, N % 128 == 0 or N == 64.
 * residual == NULL: conv1 + folded bn1 + ReLU (no identity add) on the same kernel. */
int kgdet_conv1x1_nhwc_residual(const void *x, const void *weight, const float *bias, const void *residual, void *out,
                                int64_t M, int32_t K, int32_t N, int32_t relu, void *stream);
/* the same with x = the RAW output of the convolution in front (conv2 without its epilogue): relu(x + in_bias[k]) (rounded to
 * bf16, as the separate pass stores it) is applied to the activations as they are loaded; in_bias fp32 [K] */
int kgdet_conv1x1_nhwc_residual_in(const void *x, const float *in_bias, const void *weight, const float *bias,
                                   const void *residual, void *out, int64_t M, int32_t K, int32_t N, int32_t relu,
                                   void *stream);
int kgdet_bn_fold_backward(const float *grad_z, const float *z, int32_t relu, float *g, float *partial, int64_t N, int32_t C,
                           int64_t HW, void *stream);
int kgdet_bn_fold_finish(const float *partial, int32_t P, const float *w, float *G /*nullable*/, const float *s,
                         const float *mean, const float *var, float eps, float *grad_beta /*nullable*/,
                         float *grad_gamma /*nullable*/, int32_t O, int32_t CK, void *stream);
/* kgdet_conv1x1_grad_weight / kgdet_conv3x3_grad_weight with kgdet_bn_fold_finish as the epilogue of their split sum (one
 * launch less per convolution): grad_w = s * G, grad_beta, grad_gamma as above; bn_partial / P from kgdet_bn_fold_backward --
 * or bn_partial == NULL with P == 0: grad_y is final (no ReLU mask to apply, or applied already by kgdet_conv_apply_gated_fmt) and
 * its per-channel sums are formed inside the weight-gradient kernel, from the operand values it loads anyway (no pass of
 * kgdet_bn_fold_backward over grad_y at all). */
int kgdet_conv1x1_grad_weight_fold(const float *grad_y, const float *x, float *grad_w, int64_t B, int32_t O, int32_t C,
                                   int64_t HW, void *workspace, size_t workspace_bytes, const float *w, const float *s,
                                   const float *mean, const float *var, float eps, const float *bn_partial, int32_t P,
                                   float *grad_beta /*nullable*/, float *grad_gamma /*nullable*/, void *stream);
int kgdet_conv3x3_grad_weight_fold(const float *grad_y, const float *x, float *grad_w, int64_t B, int32_t O, int32_t C,
                                   int32_t H, int32_t W, void *workspace, size_t workspace_bytes, const float *w,
                                   const float *s, const float *mean, const float *var, float eps, const float *bn_partial,
                                   int32_t P, float *grad_beta /*nullable*/, float *grad_gamma /*nullable*/, void *stream);
/* The frozen stem: y = maxpool3x3/s2/p1(relu(batch_norm_eval(x))) in one pass (mmdet/models/backbones/resnet.py:487-491, 528);
 * x [N, C, H, W] -> y [N, C, (H-1)/2+1, (W-1)/2+1].  Forward only (conv1 / norm1 are frozen: frozen_stages >= 0). */
int kgdet_bn_relu_maxpool(const float *x, const float *gamma, const float *beta, const float *mean, const float *var,
                          float eps, float *y, int64_t N, int32_t C, int32_t H, int32_t W, void *stream);

/* Inference epilogue of a convolution with folded BatchNorm: x = [relu](x + bias[c] [+ residual]) in place.
 * x, residual: [N, C, HW] contiguous, or [N, HW, C] when channels_last != 0 (then C must be a multiple of 4
 * (float32) / 8 (bfloat16), else KGDET_E_UNSUPPORTED); dtype 0 = float32, 1 = bfloat16; bias [C] float32
 * (nullable); residual nullable.  No reference counterpart: it fuses the BatchNorm / residual add / ReLU passes of
 * mmdet/models/backbones/resnet.py:231-262 once the frozen statistics are folded into the weights. */
int kgdet_bias_act(void *x, const float *bias, const void *residual, int64_t N, int32_t C, int64_t HW, int32_t dtype,
                   int32_t relu, int32_t channels_last, void *stream);
/* The stem at inference with the frozen BatchNorm folded into conv1: y = maxpool3x3/s2/p1(relu(x + bias[c])) in one pass on
 * channels-last tensors (mmdet/models/backbones/resnet.py:487-491, 528); x [N, H, W, C] -> y [N, (H-1)/2+1, (W-1)/2+1, C];
 * dtype 0 = float32 (C % 4 == 0), 1 = bfloat16 (C % 8 == 0), else KGDET_E_UNSUPPORTED; bias [C] float32, nullable.  Same
 * values as kgdet_bias_act + max pooling (each element is rounded to the storage type before the maximum). */
int kgdet_bias_relu_maxpool_nhwc(const void *x, const float *bias, void *y, int64_t N, int32_t C, int32_t H, int32_t W,
                                 int32_t dtype, void *stream);

/* HIP runtime error (launch failure etc.) */
#define KGDET_E_UNSUPPORTED 4
#define KGDET_E_PARTIAL 5     /* a measurement switch (KGDET_OPT_BWD_PHASE) was set: only part of the call's outputs were written */

const char *kgdet_last_error(void); /* thread-local message for the last non-zero status */
int kgdet_version(void);            /* ABI version, currently 1 */
int kgdet_device_cu_count(void);    /* compute units of the current device (0 if none) */

/* Process-wide switches (diagnostics / accuracy studies; defaults 0).
 * KGDET_OPT_EXACT_BACKWARD != 0: kgdet_deform_conv_backward_input takes the exact-fp32 kernels (f32-input MFMA)
 * instead of the split-bf16 plane kernels it prefers for v1 problems -- the arithmetic of the reference's fp32
 * col2im path (deform_conv_cuda.cpp:260-371), used to measure what the hi/lo split costs over a training step. */
#define KGDET_OPT_EXACT_BACKWARD 0
/* (slot 1: KGDET_OPT_TAP_PAIRS in rounds 2-4, the column-wave forward in round 5 -- both kernels left the library, tools/experiments/;
 * setting it has no effect) */
#define KGDET_OPT_FWD_COLUMN_WAVE 1
/* KGDET_OPT_WGRAD_STREAMK != 0: kgdet_deform_conv_grad_weight_grouped keeps rounds 1-3's schedule -- 256 x 128 tiles, (tile,
 * stage) units dealt stream-K, partial tiles + fix-up -- where it would otherwise run the output-stationary kernel (round 4:
 * one 256 x 208 tile per workgroup for the whole reduction, csrc/dcn_backward_weight_os.hip).  Same results to round-off
 * (another summation order); for A/B measurements and so that both kernels stay under test. */
#define KGDET_OPT_WGRAD_STREAMK 2
/* KGDET_OPT_BWD_PHASE (measurement switch, bench.py `roofline.backward`): 1 = kgdet_deform_conv_backward_input_grouped launches
 * only its grad_input phase, 2 = only its grad_offset phase (the other product's outputs are left untouched), 0 = both. */
#define KGDET_OPT_BWD_PHASE 3
#define KGDET_OPT_COUNT 4
int kgdet_set_option(int32_t option, int32_t value);

/* ------------------------------------------------------------------------------------------
 * Deformable convolution v1 / v2
 * shape of one call; weight is [O, C/groups, kh, kw], offset [N, dg*2*kh*kw, Ho, Wo] with
 * (dy,dx) interleaved per tap, taps row-major; mask (v2) [N, dg*kh*kw, Ho, Wo].
 * ------------------------------------------------------------------------------------------ */
typedef struct kgdet_dcn_shape {
  int32_t N, C, H, W;
  int32_t O, kh, kw;
  int32_t stride_h, stride_w, pad_h, pad_w, dil_h, dil_w;
  int32_t groups, deformable_groups;
  /* Optional: the output (forward) / grad_output (backward) tensor is channels
   * [out_channel_offset, out_channel_offset + O) of a wider [N, out_channels_total, Ho, Wo] buffer, so
   * several convolutions can write straight into one concatenated feature map (KGDet concatenates
   * the 3x3 / 5x5 / 7x7 branches, R/../anchor_heads/reppoints_head_kp3rep_cas_1_assign_once.py:151-153).
   * Zero for both means a dense [N, O, Ho, Wo] tensor. */
  int32_t out_channel_offset, out_channels_total;
} kgdet_dcn_shape;

/* flags for the fused epilogue */
#define KGDET_DCN_RELU 1u /* out = max(out, 0) */
/* Forward arithmetic.  Default: bf16 MFMA on a hi/lo split of both fp32 operands (3 products, fp32
 * accumulate; <= 2^-16 relative error per product, i.e. fp32-accurate to ~1e-6 of the output scale).
 * KGDET_DCN_BF16: operands rounded to bf16 once (autocast inference).  KGDET_DCN_EXACT_FP32: the
 * v_mfma_f32_32x32x2_f32 kernel, bit-exact fp32 products (also used when a 16-channel slice of one input
 * image does not fit in LDS: H*W > 1344). */
#define KGDET_DCN_BF16 2u
#define KGDET_DCN_EXACT_FP32 4u

/* output spatial size, R/dcn/deform_conv.py:96-110; returns KGDET_E_SHAPE if it is < 1 */
int kgdet_dcn_output_size(const kgdet_dcn_shape *s, int32_t *Ho, int32_t *Wo);

/* bytes of the MFMA-friendly weight image [groups][kh*kw][C/groups (pad 16)][O/groups (pad 256)] */
size_t kgdet_dcn_packed_weight_bytes(const kgdet_dcn_shape *s);
/* bytes of scratch (split-K partial tiles) forward / backward need besides the packed weight */
size_t kgdet_dcn_workspace_bytes(const kgdet_dcn_shape *s);

/* weight [O, C/groups, kh, kw] (device) -> packed (device).  Cache it while the weight is unchanged. */
int kgdet_dcn_pack_weight(const kgdet_dcn_shape *s, const float *weight, float *packed, void *stream);
/* n weights at once (training re-packs every DeformConv weight every step: the six of a KGDet head stage in one launch);
 * same images as n kgdet_dcn_pack_weight calls. */
int kgdet_dcn_pack_weight_multi(int32_t n, const kgdet_dcn_shape *const *shapes, const float *const *weights,
                                float *const *packeds, void *stream);
/* The same with a choice of images (training re-packs every weight every step: 170 MB written per KGDet head stage for all four
 * images): bit 0 of `images` = the two fp32 images (exact-fp32 forward, fallback backward kernels), bit 1 = the two split (bf16
 * hi/lo) images of the default kernels.  kgdet_dcn_split_path_complete(shape) = 1 when every product of a convolution of that
 * shape has a split-operand kernel, i.e. nothing reads the fp32 images unless an exact-arithmetic switch is set.  The packed
 * buffer's layout and size do not change; images that are not packed are left as they are. */
int kgdet_dcn_pack_weight_images(int32_t n, const kgdet_dcn_shape *const *shapes, const float *const *weights,
                                 float *const *packeds, uint32_t images, void *stream);
int32_t kgdet_dcn_split_path_complete(const kgdet_dcn_shape *shape);
/* packed gradient image -> grad_weight [O, C/groups, kh, kw]; accumulate != 0 adds into grad_weight */
int kgdet_dcn_unpack_weight_grad(const kgdet_dcn_shape *s, const float *packed, float *grad_weight,
                                 int accumulate, void *stream);

/*
 * Forward.  Replaces deform_conv_forward_cuda (R/dcn/src/deform_conv_cuda.cpp:151-156) when
 * mask == NULL && bias == NULL, and modulated_deform_conv_cuda_forward (:486-492) otherwise.
 * `packed_weight` comes from kgdet_dcn_pack_weight.  output [N, O, Ho, Wo] is overwritten.
 * No column matrix is materialised: samples are gathered into LDS and contracted with MFMA.
 */
int kgdet_deform_conv_forward(const kgdet_dcn_shape *s, const float *input, const float *offset,
                              const float *mask /*nullable*/, const float *packed_weight,
                              const float *bias /*nullable*/, float *output, uint32_t flags,
                              void *workspace, size_t workspace_bytes, void *stream);

/* Scratch for kgdet_deform_conv_forward_grouped: split-K slabs plus one table of sampling records per problem
 * (also >= kgdet_dcn_workspace_bytes of every member, so the same buffer serves their backward calls). */
size_t kgdet_dcn_group_workspace_bytes(int32_t n, const kgdet_dcn_shape *const *shapes);

/* n independent forward problems in ONE launch: same results as n calls of kgdet_deform_conv_forward
 * with the same flags.  The KGDet head runs a 3x3, a 5x5 and a 7x7 deformable conv on each of two feature
 * maps per stage (reppoints_head_kp3rep_cas_1_assign_once.py:145-163); grouping them shares the split-K
 * partial tiles, the fix-up pass and the launch overhead.  All arrays have n entries; `masks` / `biases`
 * (or single entries) may be NULL.  workspace >= kgdet_dcn_group_workspace_bytes(n, shapes). */
int kgdet_deform_conv_forward_grouped(int32_t n, const kgdet_dcn_shape *const *shapes, const float *const *inputs,
                                      const float *const *offsets, const float *const *masks /*nullable*/,
                                      const float *const *packed_weights, const float *const *biases /*nullable*/,
                                      float *const *outputs, uint32_t flags, void *workspace,
                                      size_t workspace_bytes, void *stream);

/* grad_input only, on the plane kernel (transposed sampling; atomic-free, deterministic, overwrites grad_input).
 * Same quantity as the grad_input of kgdet_deform_conv_backward_input; weight groups and deformable groups run as
 * channel runs (channels that share both; at most 8 runs, each starting on a 256-channel boundary of its weight group or
 * ending before the next one); needs H*W, Ho*Wo <= 1344 (KGDET_E_UNSUPPORTED otherwise).  flags: KGDET_DCN_BF16 or 0
 * (hi/lo split).
 * workspace >= kgdet_dcn_workspace_bytes(s). */
int kgdet_deform_conv_grad_input(const kgdet_dcn_shape *s, const float *offset, const float *mask /*nullable*/,
                                 const float *packed_weight, const float *grad_output, float *grad_input,
                                 uint32_t flags, void *workspace, size_t workspace_bytes, void *stream);

/* grad_offset only (v1), with the column gradient W^T grad_out kept in registers and the feature plane in LDS.
 * Same quantity as the grad_offset of kgdet_deform_conv_backward_input; needs every deformable group inside ONE weight
 * group (groups == 1 with any number of deformable groups of whole 16-channel chunks, or deformable groups that subdivide
 * the weight groups), O / groups <= 256, H*W <= 1344 (KGDET_E_UNSUPPORTED otherwise).  Overwrites grad_offset.
 * workspace >= kgdet_dcn_workspace_bytes(s). */
int kgdet_deform_conv_grad_offset(const kgdet_dcn_shape *s, const float *input, const float *offset,
                                  const float *packed_weight, const float *grad_output, float *grad_offset,
                                  uint32_t flags, void *workspace, size_t workspace_bytes, void *stream);

/* grad_input and grad_offset of n v1 problems in two grouped launches (one per quantity); same results as
 * kgdet_deform_conv_grad_input + kgdet_deform_conv_grad_offset per problem.  n <= 8; every problem must be
 * eligible for both kernels and have groups == 1, deformable_groups == 1 (KGDET_E_UNSUPPORTED otherwise -- call the
 * single entry points).
 * ALIASED OUTPUTS ARE SUMMED (round 6): problems that pass the SAME grad_input pointer (the 3x3 / 5x5 / 7x7 convolutions of one
 * feature map) or the same grad_offset pointer (the two maps of a Kp3RepBlock, which share their offsets) get the SUM of their
 * results in that tensor -- added by the fix-up kernels in fixed order (problems ascending, reduction parts ascending), what
 * autograd's accumulation of the reference's per-call gradients (deform_conv.py:62-93) produces.  Up to four problems per pointer;
 * they must tile alike (same N, pixels, channel rows; grad_offset: same kernel size) and the launch must fit the static schedule,
 * else KGDET_E_UNSUPPORTED before anything is launched for that quantity (pass one tensor per problem and add them yourself).
 * workspace >= kgdet_dcn_group_workspace_bytes(n, shapes). */
int kgdet_deform_conv_backward_input_grouped(int32_t n, const kgdet_dcn_shape *const *shapes, const float *const *inputs,
                                             const float *const *offsets, const float *const *packed_weights,
                                             const float *const *grad_outputs, float *const *grad_inputs,
                                             float *const *grad_offsets, void *workspace, size_t workspace_bytes,
                                             void *stream);

/* grad_weight of n v1 problems (H*W <= 1344; weight groups and deformable groups as channel runs, at most 8 runs over
 * all problems) in one launch: a GEMM with the
 * reduction over pixels, sampled B stages from an LDS-resident plane, bf16 hi/lo split MFMA; grad_weights[i]
 * [O, C, kh, kw] is OVERWRITTEN.  KGDET_E_UNSUPPORTED for other shapes (use kgdet_deform_conv_backward_weight).
 * workspace >= kgdet_dcn_group_workspace_bytes(n, shapes). */
int kgdet_deform_conv_grad_weight_grouped(int32_t n, const kgdet_dcn_shape *const *shapes, const float *const *inputs,
                                          const float *const *offsets, const float *const *grad_outputs,
                                          float *const *grad_weights, void *workspace, size_t workspace_bytes,
                                          void *stream);

/*
 * Backward w.r.t. input and offset (and mask for v2).  Replaces
 * deform_conv_backward_input_cuda (deform_conv_cuda.cpp:260-266) and the input/offset/mask part
 * of modulated_deform_conv_cuda_backward (:566-573).  grad_offset / grad_mask are overwritten.
 * grad_input: pass it zero-filled, as R/dcn/deform_conv.py:73 does.  Maps whose 32-channel plane set
 * fits LDS (H*W <= 1088) take the atomic-free gather path, which overwrites it deterministically;
 * larger maps accumulate into it with float atomics like the reference.
 */
int kgdet_deform_conv_backward_input(const kgdet_dcn_shape *s, const float *input, const float *offset,
                                     const float *mask /*nullable*/, const float *packed_weight,
                                     const float *grad_output, float *grad_input, float *grad_offset,
                                     float *grad_mask /*nullable*/, void *workspace,
                                     size_t workspace_bytes, void *stream);

/*
 * Backward w.r.t. weight (and bias for v2).  Replaces deform_conv_backward_parameters_cuda
 * (deform_conv_cuda.cpp:373-378, scale = 1) and the weight/bias part of
 * modulated_deform_conv_cuda_backward.  grad_weight [O, C/groups, kh, kw] is overwritten
 * (accumulate == 0) or added to (accumulate != 0); grad_bias [O] likewise when not NULL.
 * accumulate == 0: bf16 hi/lo split MFMA kernels with natural-layout output -- an LDS-resident plane for maps up to 1344
 * pixels, corners gathered from a pixel-major copy of the input (in the workspace) beyond; any weight groups /
 * deformable groups of 16-channel multiples.  accumulate != 0 or KGDET_OPT_EXACT_BACKWARD: the fp32 MFMA kernel.
 */
int kgdet_deform_conv_backward_weight(const kgdet_dcn_shape *s, const float *input, const float *offset,
                                      const float *mask /*nullable*/, const float *grad_output,
                                      float *grad_weight, float *grad_bias /*nullable*/, int accumulate,
                                      void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * Deformable PS-RoI pooling.  Replaces deform_psroi_pooling_cuda_forward / _backward
 * (R/dcn/src/deform_pool_cuda.cpp:30-34, 54-59; kernels deform_pool_cuda_kernel.cu:53-140, 143-263).
 * rois [R,5] = (batch_idx,x1,y1,x2,y2); trans [R, 2*num_classes, part, part] (NULL when no_trans);
 * out/count [R, out_dim, P, P].
 * Backward OVERWRITES grad_input [B,C,H,W] and grad_trans (every element written exactly once: no pre-zeroing, no
 * atomics, bit-repeatable; the reference accumulates with atomicAdd into zero-filled tensors).  It needs
 * kgdet_deform_psroi_backward_workspace_bytes(s) bytes of caller-owned scratch (per-RoI bounding boxes + the
 * transposed grad_out / count quotient + the per-pixel contribution lists grad_data is summed from).
 * Envelope (LDS record table): pooled_size^2 * sample_per_part^2 <= 2048, pooled_size <= 16, group_size <= 16 --
 * KGDET_E_SHAPE beyond (the reference's configs use 7 / 4 / 1 or 7).
 * ------------------------------------------------------------------------------------------ */
typedef struct kgdet_psroi_shape {
  int32_t B, C, H, W;  /* data */
  int32_t R;           /* number of rois */
  int32_t out_dim, group_size, pooled_size, part_size, sample_per_part;
  int32_t no_trans, num_classes; /* num_classes = no_trans ? 1 : trans.size(1)/2 */
  float spatial_scale, trans_std;
} kgdet_psroi_shape;

size_t kgdet_deform_psroi_forward_workspace_bytes(const kgdet_psroi_shape *s);
int kgdet_deform_psroi_forward(const kgdet_psroi_shape *s, const float *data, const float *rois,
                               const float *trans, float *out, float *count, void *workspace, size_t workspace_bytes,
                               void *stream);
size_t kgdet_deform_psroi_backward_workspace_bytes(const kgdet_psroi_shape *s);
int kgdet_deform_psroi_backward(const kgdet_psroi_shape *s, const float *grad_out, const float *count,
                                const float *data, const float *rois, const float *trans,
                                float *grad_data, float *grad_trans, void *workspace, size_t workspace_bytes,
                                void *stream);

/* ------------------------------------------------------------------------------------------
 * Sigmoid focal loss.  Replaces sigmoid_focal_loss_cuda.forward / .backward
 * (R/sigmoid_focal_loss/src/sigmoid_focal_loss.cpp:40-45).  logits [num, C]; targets [num]
 * int64 (0 = background, 1..C = class); losses / d_logits [num, C].
 * ------------------------------------------------------------------------------------------ */
int kgdet_sigmoid_focal_loss_forward(const float *logits, const int64_t *targets, int64_t num,
                                     int32_t num_classes, float gamma, float alpha, float *losses,
                                     void *stream);
int kgdet_sigmoid_focal_loss_backward(const float *logits, const int64_t *targets, const float *d_losses,
                                      int64_t num, int32_t num_classes, float gamma, float alpha,
                                      float *d_logits, void *stream);

/* ------------------------------------------------------------------------------------------
 * Target assignment + the nine losses of the KGDet head (one pyramid level) without materialised targets.
 * Replaces, for RepPointsHeadKp3RepCas1AssignOnce.loss (reppoints_head_kp3rep_cas_1_assign_once.py:581-665):
 * PointAssigner.assign (core/bbox/assigners/point_assigner.py:23-121), point_target_kp (core/anchor/
 * point_target_kp.py:7-169), offset_to_pts (:537-579), FocalLoss / SmoothL1Loss with weight and avg_factor
 * (models/losses/focal_loss.py:28-82, smooth_l1_loss.py:8-45, utils.py:7-52; sigmoid_focal_loss_cuda.cu:24-97).
 * Prediction maps are the head's NCHW outputs: cls [B, num_classes, H, W], bbox [B, 4, H, W] (x1, y1, x2, y2
 * offsets), kpt [B, 2 * num_keypoints, H, W] ((y, x) offset pairs), three stages each.  Points are the level's grid
 * (x = column * stride, y = row * stride).  losses[9] = cls 1-3, bbox 1-3, kpt 1-3; num_total = sum over images of
 * max(positives, 1) (a device scalar; nothing is read by the host).  The backward call takes the forward call's
 * workspace (it holds the per-gt selections) and writes every element of the nine gradient maps.
 * Workspace layout: the first B * 64 * H * W floats are the selections dsel[b][g][i] -- row stride 64 whatever num_gt[b] is --
 * = the distance of point i to ground truth g where i is among its pos_num nearest (ties: the lowest point index), +inf
 * elsewhere; rows g >= num_gt[b] are not written.  A point goes to the selecting ground truth with the smallest value, the
 * earliest on equal values.  Per-workgroup partial sums follow.  A workspace shorter than kgdet_head_loss_workspace_bytes():
 * KGDET_E_WORKSPACE from either call.
 * Limits: B <= 16, 1..64 ground truths per image, H * W <= 4096.
 * ------------------------------------------------------------------------------------------ */
#define KGDET_HEAD_MAX_IMAGES 16
typedef struct kgdet_head_targets {
  int32_t B, H, W, num_classes, num_keypoints;
  float stride;
  int32_t num_gt[KGDET_HEAD_MAX_IMAGES];
  const float *gt_bboxes[KGDET_HEAD_MAX_IMAGES];     /* [num_gt, 4] */
  const int64_t *gt_labels[KGDET_HEAD_MAX_IMAGES];   /* [num_gt], NULL: every label 1 */
  const float *gt_keypoints[KGDET_HEAD_MAX_IMAGES];  /* [num_gt, num_keypoints, 3] (x, y, visibility) */
  /* valid extent of image b on the grid: rows < valid_h[b] and columns < valid_w[b] (ceil(pad_shape / stride), the flags of
   * reppoints_head_kp3rep_cas_1_assign_once.py:524-535); 0 = the whole grid.  Points beyond it are no candidates of the
   * assigner and carry label weight 0 (point_target_kp.py:107-161 with unmap): no loss, zero gradient. */
  int32_t valid_h[KGDET_HEAD_MAX_IMAGES], valid_w[KGDET_HEAD_MAX_IMAGES];
} kgdet_head_targets;
typedef struct kgdet_head_loss_cfg {
  int32_t pos_num;               /* PointAssigner.pos_num */
  float pos_weight;              /* label weight of positives (train_cfg.pos_weight <= 0 -> 1) */
  float normalize_term;          /* point_base_scale * stride */
  float gamma[3], alpha[3];      /* FocalLoss of stage 1-3 */
  float beta[6];                 /* SmoothL1Loss: bbox 1-3, kpt 1-3 */
  float loss_weight[9];          /* cls 1-3, bbox 1-3, kpt 1-3 */
} kgdet_head_loss_cfg;
typedef struct kgdet_head_maps {
  float *cls[3], *bbox[3], *kpt[3];
} kgdet_head_maps;
size_t kgdet_head_loss_workspace_bytes(const kgdet_head_targets *t);
int kgdet_head_loss_forward(const kgdet_head_targets *t, const kgdet_head_loss_cfg *cfg, const kgdet_head_maps *maps,
                            float *losses, float *num_total, void *workspace, size_t workspace_bytes, void *stream);
int kgdet_head_loss_backward(const kgdet_head_targets *t, const kgdet_head_loss_cfg *cfg, const kgdet_head_maps *maps,
                             const float *grad_losses, const float *num_total, const kgdet_head_maps *grads,
                             const void *workspace, size_t workspace_bytes, void *stream);
/* The same two calls with the per-image integers in DEVICE memory, so that a captured HIP graph of the training step can be
 * replayed on batches with other ground-truth counts and other valid extents.  table: device int32 [B][4] =
 * (num_gt, valid_h, valid_w, reserved 0) per image, 16-byte aligned, read when the kernels RUN (each workgroup reads its
 * image's row once, as one uniform load); gt_capacity in 1..64: every gt_bboxes[b] / gt_labels[b] / gt_keypoints[b] points
 * at a buffer of gt_capacity rows, of which the first num_gt are read -- later rows may hold anything.  The by-value num_gt /
 * valid_h / valid_w of the descriptor are ignored.  valid_h / valid_w keep their meaning (grid units; 0 or anything beyond the
 * grid = the whole grid).  The host cannot see the table at launch: the kernels clamp num_gt to [0, gt_capacity] and the
 * extents to the grid, so no table content makes them read outside a buffer; range checks (1 <= num_gt <= gt_capacity, an
 * extent of at least pos_num points) are the caller's, before it writes the table.  An image with count 0 has no positives:
 * every valid point is a negative, and the image contributes max(0, 1) = 1 to num_total.  The selection launch is
 * (gt_capacity, B) workgroups; workspace layout and size, arithmetic, summation orders and results are those of the by-value
 * calls -- equal counts and extents give equal bits.  A null or misaligned table, or gt_capacity outside 1..64:
 * KGDET_E_SHAPE, nothing written. */
int kgdet_head_loss_forward_table(const kgdet_head_targets *t, const kgdet_head_loss_cfg *cfg, const kgdet_head_maps *maps,
                                  const int32_t *table, int32_t gt_capacity, float *losses, float *num_total,
                                  void *workspace, size_t workspace_bytes, void *stream);
int kgdet_head_loss_backward_table(const kgdet_head_targets *t, const kgdet_head_loss_cfg *cfg, const kgdet_head_maps *maps,
                                   const int32_t *table, int32_t gt_capacity, const float *grad_losses,
                                   const float *num_total, const kgdet_head_maps *grads, const void *workspace,
                                   size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * Target assignment + the five loss families of the serial / parallel two-stage heads over the whole pyramid, without
 * materialised targets.  Replaces, for RepPointsHeadKpSerial / RepPointsHeadKpParallel (reppoints_head_kp_serial.py loss /
 * loss_single): PointAssigner.assign (core/bbox/assigners/point_assigner.py) for the init stage, bbox_overlaps
 * (core/bbox/geometry.py) + MaxIoUAssigner.assign_wrt_overlaps with gt_max_assign_all (core/bbox/assigners/
 * max_iou_assigner.py) for the refine stage, point_target_kp (core/anchor/point_target_kp.py), offset_to_pts and the
 * FocalLoss / SmoothL1Loss reductions.
 * Maps per level l (NCHW float32, grid H[l] x W[l], points x = column * stride[l], y = row * stride[l]): cls [B, C, H, W];
 * kpt_init / kpt_refine [B, 2 K, H, W], (y, x) offset pairs decoded as pred * stride + centre; box_init / box_refine
 * [B, 4, H, W] = the head's points2bbox of the raw reppoints maps, in stride units: the image-space box is
 * centre + box * stride, one rounding per operation (what the torch chain hands its assigner, bit for bit).
 * Init assignment: a ground truth lives on level int((log2(w / scale) + log2(h / scale)) / 2) - log2(stride[0]), clamped to
 * [0, L); its positives are the pos_num nearest valid points of that level under |(p - centre) / max(size, 1e-6)| (ties: the
 * lowest point index); a point several ground truths claim goes to the nearest, the earliest on a tie.
 * Refine assignment, over all levels' points of an image: IoU with the +1 convention of every point's init box; per point the
 * best IoU (lowest gt on equal values): 0 inside [neg_lo, neg_hi), gt + 1 from pos_iou_thr on, else -1; then every ground
 * truth whose maximum IoU over the valid points reaches min_pos_iou takes EVERY valid point at exactly that IoU, the last
 * such ground truth winning.  Invalid points: 0, label weight 0, best IoU -2.
 * losses[k * L + l], k = cls, bbox_init, bbox_refine, kpt_init, kpt_refine: loss_weight[k] * (sum over level l / num_total);
 * num_total[0] = init, [1] = refine: sum over the images of max(positives, 1) (cls, *_refine use [1]).  Device scalars;
 * nothing is read by the host; fixed summation orders.  grad_losses [5 * L] in the same order.  The backward call takes the
 * forward call's workspace and writes every element of the 5 * L gradient maps.
 * Workspace layout, N = sum of H[l] * W[l], points image-major then level-major, row-major inside a level; every table starts
 * on a 256-byte boundary, T = B * N * 4 rounded up to a multiple of 256 bytes:
 *   byte 0      int32 assigned_init[B][N]    (0 / gt + 1)
 *   byte T      int32 assigned_refine[B][N]  (-1 / 0 / gt + 1)
 *   byte 2 T    float best_iou[B][N]
 *   byte 3 T    internal tables and the per-workgroup partial sums.
 * Shorter than kgdet_serial_loss_workspace_bytes(): KGDET_E_WORKSPACE.
 * Cost beyond the configs' pos_num = 1: the init stage makes pos_num passes over a ground truth's level, and one workgroup per
 * image settles the points several ground truths claim by comparing all num_gt * pos_num selections pairwise (4096^2 at both
 * limits).
 * Limits: B <= 16, 1..64 ground truths per image, 1..8 levels whose strides are consecutive powers of two, up to 32768
 * points per level, pos_num 1..64 and not beyond any image's valid point count on any level.
 * ------------------------------------------------------------------------------------------ */
#define KGDET_SERIAL_MAX_LEVELS 8
typedef struct kgdet_serial_targets {
  int32_t B, L, num_classes, num_keypoints;
  int32_t H[KGDET_SERIAL_MAX_LEVELS], W[KGDET_SERIAL_MAX_LEVELS];
  float stride[KGDET_SERIAL_MAX_LEVELS];
  int32_t num_gt[KGDET_HEAD_MAX_IMAGES];
  const float *gt_bboxes[KGDET_HEAD_MAX_IMAGES];     /* [num_gt, 4] */
  const int64_t *gt_labels[KGDET_HEAD_MAX_IMAGES];   /* [num_gt], NULL: every label 1 */
  const float *gt_keypoints[KGDET_HEAD_MAX_IMAGES];  /* [num_gt, num_keypoints, 3] (x, y, visibility) */
  /* valid extent of image b on level l (ceil(pad_shape / stride), clamped to the grid); 0 = the whole grid */
  int32_t valid_h[KGDET_HEAD_MAX_IMAGES][KGDET_SERIAL_MAX_LEVELS], valid_w[KGDET_HEAD_MAX_IMAGES][KGDET_SERIAL_MAX_LEVELS];
} kgdet_serial_targets;
typedef struct kgdet_serial_loss_cfg {
  int32_t pos_num;                 /* init: PointAssigner.pos_num */
  float scale;                     /* init: PointAssigner.scale */
  float pos_iou_thr, neg_lo, neg_hi, min_pos_iou;   /* refine: MaxIoUAssigner (a float neg_iou_thr t is the range [0, t)) */
  float pos_weight;                /* label weight of refine positives (train_cfg.refine.pos_weight <= 0 -> 1) */
  float point_base_scale;          /* normalize_term of level l = point_base_scale * stride[l] */
  float gamma, alpha;              /* FocalLoss */
  float beta[4];                   /* SmoothL1Loss: bbox_init, bbox_refine, kpt_init, kpt_refine */
  float loss_weight[5];            /* cls, bbox_init, bbox_refine, kpt_init, kpt_refine */
} kgdet_serial_loss_cfg;
typedef struct kgdet_serial_maps {
  float *cls[KGDET_SERIAL_MAX_LEVELS], *box_init[KGDET_SERIAL_MAX_LEVELS], *box_refine[KGDET_SERIAL_MAX_LEVELS],
      *kpt_init[KGDET_SERIAL_MAX_LEVELS], *kpt_refine[KGDET_SERIAL_MAX_LEVELS];
} kgdet_serial_maps;
size_t kgdet_serial_loss_workspace_bytes(const kgdet_serial_targets *t, const kgdet_serial_loss_cfg *cfg);
int kgdet_serial_loss_forward(const kgdet_serial_targets *t, const kgdet_serial_loss_cfg *cfg, const kgdet_serial_maps *maps,
                              float *losses, float *num_total, void *workspace, size_t workspace_bytes, void *stream);
int kgdet_serial_loss_backward(const kgdet_serial_targets *t, const kgdet_serial_loss_cfg *cfg, const kgdet_serial_maps *maps,
                               const float *grad_losses, const float *num_total, const kgdet_serial_maps *grads,
                               const void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * Element-wise glue of the KGDet step as single passes (no native function in the reference).
 * kgdet_reppts_offsets_*: the deformable offsets of a Kp3RepBlock from the previous stage's reppoints,
 *   reppoints_head_kp3rep_cas_1_assign_once.py:131-143: for the 2 k^2-channel slices (k = kernel_sizes[0..2], consecutive)
 *   of reppts [B, C, HW]: out_k = (gm * part + (1 - gm) * part) - regular_grid_k; backward: grad_reppts = gm * grad_k on the
 *   slices (NULL grad_k: zeros), 0 on the channels beyond them.
 * kgdet_subsample2_*: y = x[:, :, ::2, ::2] of [planes, H, W] and grad_x = zero-stuffed grad_y (+ other, nullable) -- the
 *   stride-2 1x1 downsample branch of resnet.py:180-186 as a 1x1 convolution of the subsampled input; backward needs W % 4 == 0.
 * kgdet_pts_from_offsets_*: a level's predicted offsets pred [B, C = 2n, HW] as image coordinates pts [B, HW, 2n] =
 *   offset * stride + centre with (x, y) interleaved -- offset_to_pts of reppoints_head_kp_serial.py:400-421 (permute, flip when
 *   the channels are (y, x) pairs: y_first, multiply, add) in one pass; centres [B, HW, 2] = (x, y).  Values equal the torch
 *   chain's bit for bit (separate multiply and add).  Backward: grad_pred = transposed (pair-swapped) grad_pts * stride.
 * ------------------------------------------------------------------------------------------ */
int kgdet_reppts_offsets_forward(const float *reppts, int32_t B, int32_t C, int32_t HW, const int32_t *kernel_sizes, float gm,
                                 float *out0, float *out1, float *out2, void *stream);
int kgdet_reppts_offsets_backward(const float *g0, const float *g1, const float *g2, int32_t B, int32_t C, int32_t HW,
                                  const int32_t *kernel_sizes, float gm, float *grad_reppts, void *stream);
int kgdet_subsample2_forward(const float *x, float *y, int64_t planes, int32_t H, int32_t W, void *stream);
int kgdet_subsample2_backward(const float *grad_y, const float *other /*nullable*/, float *grad_x, int64_t planes, int32_t H,
                              int32_t W, void *stream);
int kgdet_pts_from_offsets_forward(const float *pred, const float *centres, float *pts, int64_t B, int32_t C, int64_t HW,
                                   float stride, int32_t y_first, void *stream);
int kgdet_pts_from_offsets_backward(const float *grad_pts, float *grad_pred, int64_t B, int32_t C, int64_t HW, float stride,
                                    int32_t y_first, void *stream);

/*
 * Gradient clipping + Adam over all parameters as multi-tensor passes: what OptimizerHook.after_train_iter does with
 * clip_grad_norm_(params, max_norm, 2) followed by torch.optim.Adam.step() (mmdet/core/utils/dist_utils.py:44-58; torch/optim/
 * adam.py).  table_dev: n rows of six int64 on the device -- {param, grad, exp_avg, exp_avg_sq (float32 pointers), numel,
 * first block}, a tensor taking ceil(numel / kgdet_optim_chunk()) blocks, rows in block order; total_blocks = their sum.
 * kgdet_multi_grad_norm: partial [total_blocks] scratch, norm_out[0] = ||all grads||_2.  kgdet_multi_clip_adam: gradients
 * are scaled by min(1, max_norm / (norm[0] + 1e-6)) in place (max_norm <= 0: no clipping), then the Adam update with
 * bias_correction1 = 1 - beta1^step and bias_correction2_sqrt = sqrt(1 - beta2^step) of the step being taken; weight decay
 * is added to the gradient (Adam, not AdamW); the betas come as doubles so that 1 - beta is rounded once, as torch does.  No amsgrad / maximize.  Deterministic; no host synchronisation.
 * Non-finite gradients behave as in torch: a NaN gradient makes norm[0] and the coefficient NaN, and every gradient, moment and
 * parameter of the table becomes NaN (clip_grad_norm_ multiplies by the clamped coefficient, and clamp keeps NaN) -- a poisoned
 * step is loud instead of updating the finite-gradient parameters unclipped; an infinite gradient makes the coefficient 0: that
 * element becomes NaN (inf * 0), every other gradient 0, and the step is taken from the moments alone.
 */
int32_t kgdet_optim_chunk(void);
int kgdet_multi_grad_norm(const int64_t *table_dev, int32_t n, int64_t total_blocks, float *partial, float *norm_out, void *stream);
int kgdet_multi_clip_adam(const int64_t *table_dev, int32_t n, int64_t total_blocks, const float *norm, float max_norm, float lr,
                          double beta1, double beta2, float eps, float weight_decay, float bias_correction1,
                          float bias_correction2_sqrt, void *stream);
/*
 * The same clip + Adam update with the step's schedule in DEVICE memory, for a training step captured as one HIP graph (kernel
 * arguments are frozen at capture; the reference's optimizer.step() -- dist_utils.py:57 -- takes them from host state every call):
 * sched[4] = {learning rate, 1 - beta1^t, sqrt(1 - beta2^t), t}.  The call first advances the schedule (t <- t + 1, corrections
 * recomputed in double precision; learning rate <- lr_ring[t % ring] when lr_ring != NULL: `ring` floats of page-locked host memory
 * the device reads in place, slot k written by the host before it launches step k), then applies the update with it.
 */
int kgdet_multi_clip_adam_dev(const int64_t *table_dev, int32_t n, int64_t total_blocks, const float *norm, float max_norm,
                              float *sched, const float *lr_ring /*nullable*/, int32_t ring, double beta1, double beta2, float eps,
                              float weight_decay, void *stream);
/*
 * Gradient clipping + momentum SGD over the same table: clip_grad_norm_(params, max_norm, 2) followed by torch.optim.SGD.step()
 * (torch/optim/sgd.py _single_tensor_sgd; the optimizer of the three DeepFashion2 configs: lr 5e-3, momentum 0.9, weight decay 1e-4).
 * Row: {param, grad, momentum_buffer, ignored, numel, first block} -- slot 2 may be 0 only when momentum == 0 (the buffer is then
 * neither read nor written; with momentum != 0 a row whose slot 2 is 0 is a table error: the caller that builds the table refuses
 * it, and the kernel leaves such a row untouched rather than read through the pointer); slot 3 is never dereferenced.  Rows and
 * blocks as above, so kgdet_multi_grad_norm serves both.  One pass, fp32, no atomics, deterministic:
 *   g' = g min(1, max_norm / (norm[0] + 1e-6)) (written back only when the coefficient is below 1 or NaN; max_norm <= 0: no clipping,
 *   norm may be NULL), d = g' + p weight_decay, buf = momentum buf + (1 - dampening) d, d = nesterov ? d + momentum buf : buf,
 *   p -= lr d.  momentum and dampening come as doubles so that momentum and 1 - dampening are rounded once.  Non-finite gradients
 * behave as described for Adam.  The first step of a torch optimizer (buf = d, no dampening) is not this kernel's: it needs the
 * buffers to exist.
 * kgdet_multi_clip_sgd_dev: the capturable form.  sched[4] as for Adam, of which SGD uses [0] = learning rate and [3] = steps
 * taken: the call advances sched[3] to t, loads sched[0] = lr_ring[t % ring] when lr_ring != NULL (page-locked host memory read in
 * place), then applies the update with sched[0].
 */
int kgdet_multi_clip_sgd(const int64_t *table_dev, int32_t n, int64_t total_blocks, const float *norm /*nullable*/, float max_norm,
                         float lr, double momentum, double dampening, float weight_decay, int32_t nesterov, void *stream);
int kgdet_multi_clip_sgd_dev(const int64_t *table_dev, int32_t n, int64_t total_blocks, const float *norm /*nullable*/,
                             float max_norm, float *sched, const float *lr_ring /*nullable*/, int32_t ring, double momentum,
                             double dampening, float weight_decay, int32_t nesterov, void *stream);

/*
 * Range scan of n_rows fp32 tensors in ONE kernel launch (csrc/range_scan.hip) -- the check of the format-1 (fp16 parts) envelope
 * of the dense convolutions above that kgdet_amd/numerics.py runs when a checkpoint is loaded and at the end of an epoch.  No
 * reference counterpart.  table_dev: device table of n_rows x 8 int64
 *   {tensor (float, 4-byte aligned), count, inner, gamma or 0, var or 0, bits of eps, bits of hi1 | bits of hi2 << 32, first block}
 * first block = running sum of kgdet_range_scan_blocks(count) over the preceding rows, total_blocks = the sum over all rows (a row
 * has at most 256 blocks, which stride over its chunks of kgdet_range_scan_chunk() elements).  inner > 0 and var != 0: element i is
 * multiplied by s[i / inner], s[o] = gamma[o] / sqrtf(var[o] + eps) (gamma 0: 1 / sqrtf(var[o] + eps)) -- the scale of a
 * frozen-statistics BatchNorm folded into an [O, C, k, k] weight with inner = C k k; gamma and var hold ceil(count / inner) floats.
 * Otherwise the values are scanned as they are.  records: device, n_rows x 4 uint32, OVERWRITTEN by every call:
 *   {bits of max |v s| over the finite products (0 when there is none), number of non-finite products,
 *    number of products with |v s| > hi1, number with |v s| > hi2 (an infinite product counts in both, a NaN in neither)}
 * Products are float32, rounded once.  Integer atomics only: the record does not depend on the schedule.  The envelope's limits
 * as the caller passes them: a (folded) forward weight hi1 = 65504 / 2^8 = 255.875 (the image stores w s 2^8 in fp16 parts: beyond,
 * the kernels clamp and still return KGDET_OK); an activation hi1 = 65504 (fp32-class up to here), hi2 = 131008 (11 bits up to
 * here, clamped beyond).  Not covered by the scan's callers: activations of normal runs (numerics.audit scans them on request),
 * the deformable convolutions' operands (their pack path is separate) and gradients (bf16 parts already: no range limit).
 */
int32_t kgdet_range_scan_chunk(void);
int64_t kgdet_range_scan_blocks(int64_t count);
int kgdet_range_scan_multi(const int64_t *table_dev, int32_t n_rows, int64_t total_blocks, uint32_t *records, void *stream);

/*
 * GroupNorm (+ ReLU) of the ConvModules of the head towers and the neck as one pass each way -- ATen runs it as ten kernels
 * per layer (mmdet/models/utils/conv_module.py:142-165: norm, then activate; mmdet/models/utils/norm.py GN = nn.GroupNorm).
 * x, y, grad_* [N, C, HW] float32 contiguous; gamma, beta [C] nullable; mean, rstd [N * groups] (saved for the backward);
 * C / groups <= 64.  Backward: grad_x nullable; dgamma_dbeta [2][N][C] = per-image rows of dgamma, then of dbeta (the caller
 * adds the N rows); relu != 0 masks grad_y where y <= 0.  Deterministic.
 */
int kgdet_gn_act_forward(const float *x, const float *gamma, const float *beta, int32_t groups, float eps, int32_t relu,
                         float *y, float *mean, float *rstd, int64_t N, int32_t C, int64_t HW, void *stream);
int kgdet_gn_act_backward(const float *grad_y, const float *x, const float *y, const float *gamma, const float *mean,
                          const float *rstd, int32_t groups, int32_t relu, float *grad_x, float *dgamma_dbeta, int64_t N,
                          int32_t C, int64_t HW, void *stream);
/*
 * The same for groups of any size: beyond 65536 elements per (image, group) -- the 100 x 168 level of the five-level heads:
 * 8 channels x 16800 pixels, 64 (image, group) pairs -- the pixels of a group are cut into kgdet_gn_act_slices(...) slices with
 * a workgroup each (slice moments combined with the parallel-variance formula; per-channel gradient sums added in slice
 * order: deterministic), through `scratch` of kgdet_gn_act_scratch_floats(...) floats (NULL when that is 0; the forward's and the
 * backward's scratch need not be the same buffer).  Small groups run the kernels above.
 */
int32_t kgdet_gn_act_slices(int64_t N, int32_t C, int32_t groups, int64_t HW);
size_t kgdet_gn_act_scratch_floats(int64_t N, int32_t C, int32_t groups, int64_t HW);
int kgdet_gn_act_forward_split(const float *x, const float *gamma, const float *beta, int32_t groups, float eps, int32_t relu,
                               float *y, float *mean, float *rstd, float *scratch, int64_t N, int32_t C, int64_t HW,
                               void *stream);
int kgdet_gn_act_backward_split(const float *grad_y, const float *x, const float *y, const float *gamma, const float *mean,
                                const float *rstd, int32_t groups, int32_t relu, float *grad_x, float *dgamma_dbeta,
                                float *scratch, int64_t N, int32_t C, int64_t HW, void *stream);
/* Inference under autocast: x, y bfloat16, fp32 arithmetic, no saved statistics; at most 65536 elements per group.
 * x and y [N, C, HW], or both channels-last [N, HW, C] when x_channels_last != 0. */
int kgdet_gn_act_forward_bf16(const void *x, int32_t x_channels_last, const float *gamma, const float *beta, int32_t groups,
                              float eps, int32_t relu, void *y, int64_t N, int32_t C, int64_t HW, void *stream);
/* the same for groups of any size (the 100 x 168 level of a five-level head: 8 channels x 16800 pixels per group): beyond 65536
 * elements the split kernels, `scratch` of kgdet_gn_act_scratch_floats(...) floats (NULL when that is 0) */
int kgdet_gn_act_forward_bf16_split(const void *x, int32_t x_channels_last, const float *gamma, const float *beta, int32_t groups,
                                    float eps, int32_t relu, void *y, float *scratch, int64_t N, int32_t C, int64_t HW,
                                    void *stream);

/*
 * Weighted smooth-L1 sum of the head's box / keypoint losses in one pass each way: what the reference computes as a chain of
 * element-wise torch ops (mmdet/models/losses/smooth_l1_loss.py:8-45, utils.py:7-52 called from KP3:621-665 with
 * pred / d and target / d):   sum_out[0] = sum_i weight[i] * l(|pred[i] / d - target[i] / d|),
 * l(x) = x < beta ? 0.5 x^2 / beta : x - 0.5 beta;   grad_pred[i] = grad_sum[0] * weight[i] * l'(.) / d.
 * n elements, weight nullable (all ones); partial: kgdet_smooth_l1_partials() floats of scratch; grad_sum: DEVICE scalar (no
 * host round trip).  The caller applies loss_weight and 1 / avg_factor to the sum.  Deterministic.
 */
int32_t kgdet_smooth_l1_partials(void);
int kgdet_smooth_l1_sum_forward(const float *pred, const float *target, const float *weight, int64_t n, float beta,
                                float divisor, float *partial, float *sum_out, void *stream);
int kgdet_smooth_l1_sum_backward(const float *pred, const float *target, const float *weight, const float *grad_sum, int64_t n,
                                 float beta, float divisor, float *grad_pred, void *stream);

/* ------------------------------------------------------------------------------------------
 * NMS.  kgdet_nms replaces nms_cpu.nms / nms_cuda.nms (R/nms/src/nms_cpu.cpp:62-68,
 * nms_kernel.cu:70-131) with the CPU semantics the project pins: +1 areas, suppress when
 * IoU >= thr, visiting order = score descending (ties: lower index first), result = kept
 * indices in ascending index order.  The greedy sweep runs on the device; nothing is copied
 * to the host.  dets [n,5] float32; keep [n] int64; *num_keep (device int64) receives the count.
 *
 * kgdet_nms_batched runs many independent problems (one per (image, class) group) in ONE
 * launch: segment i covers dets rows [seg_offsets[i], seg_offsets[i+1]); kept indices are
 * written segment-relative to keep + seg_offsets[i], counts to num_keep[i].
 * workspace: kgdet_nms_workspace_bytes(total_n, num_segments).
 *
 * kgdet_soft_nms replaces soft_nms_cpu (R/nms/src/soft_nms_cpu.pyx:22-127): method 1 linear,
 * 2 gaussian; out_dets [n,5], out_inds [n] int64, *num_out device int64.
 * ------------------------------------------------------------------------------------------ */
/* Segments of up to 4096 boxes are processed entirely in LDS; longer ones (nms_wrapper.py:8-49 takes any N) run the same
 * algorithm with their arrays in `workspace` (size from kgdet_nms_workspace_bytes; 16 bytes suffice when no segment
 * exceeds 4096 boxes).  Kept indices are bit-identical to nms_cpu.cpp either way. */
size_t kgdet_nms_workspace_bytes(int64_t total_n, int32_t num_segments);
/* multiclass_nms_kp for a whole batch (mmdet/core/post_processing/bbox_nms_kp.py:6-75 with type='nms'), two launches,
 * nothing read by the host: per (image, class) the candidates with score > score_thr are suppressed as kgdet_nms does;
 * per image the classes' survivors are concatenated (class order, ascending candidate row) and, beyond max_num, the
 * max_num highest scores are kept (ties: earlier first).  boxes [B, N, 4]; scores [B, N, score_stride] with class c in
 * column score_col0 + c; out_det [B, max_num, 5]; out_label (0-based class) and out_src (candidate row, for gathering the
 * landmarks) [B, max_num] int64; out_count [B] int64; rows past the count are zero.  Limits: N <= 4096 (one class's
 * boxes in LDS), C <= 64, C * min(N, max_num) <= 16384 (the select keys at most the first max_num survivors of a class by
 * score; a flip-TTA set of 2 x 1000 candidates x 13 classes with max_num 100 fits).
 * workspace: kgdet_multiclass_nms_workspace_bytes(B, N, C). */
size_t kgdet_multiclass_nms_workspace_bytes(int32_t B, int32_t N, int32_t C);
/* 1 when kgdet_multiclass_nms serves this problem (the limits above), 0 when it returns KGDET_E_UNSUPPORTED: the one
 * statement of the limits (callers deciding before a graph capture). */
int kgdet_multiclass_nms_supported(int32_t B, int32_t N, int32_t C, int32_t max_num);
int kgdet_multiclass_nms(const float *boxes, const float *scores, int32_t B, int32_t N, int32_t C,
                         int32_t score_stride, int32_t score_col0, float score_thr, float iou_thr, int32_t max_num,
                         float *out_det, int64_t *out_label, int64_t *out_src, int64_t *out_count, void *workspace,
                         size_t workspace_bytes, void *stream);
/* multiclass_nms_kp with test_cfg.nms.type = 'soft_nms' for a whole batch (bbox_nms_kp.py:25-50 ->
 * R/nms/nms_wrapper.py:52-78 -> R/nms/src/soft_nms_cpu.pyx:22-127), two launches, nothing read by the host (round 4: the
 * per-class host loop over kgdet_soft_nms kept config-5 inference eager): per (image, class) the candidates with
 * score > score_thr go through the reference's selection-sort loop in LDS, in ascending candidate row order as
 * `multi_bboxes[cls_inds]` hands them over (method 0 hard / 1 linear / 2 gaussian, `sigma`, `min_score` as soft_nms_cpu);
 * per image the survivors are concatenated class by class in the loop's own order and, beyond max_num, the max_num
 * highest DECAYED scores are kept (ties: earlier first).  Same array shapes as kgdet_multiclass_nms; out_det's fifth
 * column is the decayed score.  Limits: N * 36 bytes of LDS (N <= 4544), C <= 64, C * max_num <= 16384.
 * workspace: kgdet_multiclass_soft_nms_workspace_bytes(B, N, C). */
size_t kgdet_multiclass_soft_nms_workspace_bytes(int32_t B, int32_t N, int32_t C);
/* 1 when kgdet_multiclass_soft_nms serves this problem on chip (N * 36 bytes of LDS per segment, C <= 64, C * max_num keys <=
 * 16384), 0 when it returns KGDET_E_UNSUPPORTED: the one statement of the limits (callers deciding before a graph capture). */
int kgdet_multiclass_soft_nms_supported(int32_t B, int32_t N, int32_t C, int32_t max_num);
int kgdet_multiclass_soft_nms(const float *boxes, const float *scores, int32_t B, int32_t N, int32_t C,
                              int32_t score_stride, int32_t score_col0, float score_thr, float iou_thr,
                              int32_t method, float sigma, float min_score, int32_t max_num, float *out_det,
                              int64_t *out_label, int64_t *out_src, int64_t *out_count, void *workspace,
                              size_t workspace_bytes, void *stream);
/* Test-time augmentation merge (RepPointsDetectorKp.aug_test): A <= 16 augmentations of one image, each with its decoded
 * candidates in its own resized frame -- boxes [n, 4], scores [n, score_stride], landmarks [n, K, 3] (x, y, v), all
 * float32 and contiguous -- are mapped back to the original frame and concatenated in augmentation order into out_boxes
 * [T, 4], out_scores [T, score_stride], out_kpts [T, K, 3] (T = sum of n).  Per augmentation: when `flip`,
 * x1' = (img_w - x2) - 1, x2' = (img_w - x1) - 1, landmark x' = (img_w - x) - 1 and out slot k takes input slot
 * kpt_perm[k] (device int32 [K], an involution: flip_indices[0::2] // 2); then box coordinates and landmark x, y are
 * multiplied by (float)(1.0 / scale) (torch's division of a GPU tensor by a python float); visibility and scores are
 * copied.  One launch, the segments passed by value (capturable); n = 0 is allowed; kpt_perm may be NULL when no
 * segment is flipped.  K <= 1024; A > 16 returns KGDET_E_UNSUPPORTED. */
typedef struct kgdet_aug_segment {
  const float *boxes, *scores, *kpts;
  int64_t n;
  float img_w;
  double scale;    /* the python float itself: the reciprocal is rounded to fp32 from double, as torch does */
  int32_t flip;
} kgdet_aug_segment;
int kgdet_aug_merge(const kgdet_aug_segment *segs, int32_t A, int32_t score_stride, int32_t K, const int32_t *kpt_perm,
                    float *out_boxes, float *out_scores, float *out_kpts, void *stream);
/* Image preprocessing (datasets.ImageTransform on the device; kgdet_amd/preprocess.py): n_jobs <= KGDET_PREPROC_MAX_JOBS
 * jobs in ONE launch, the table passed by value (capturable, no host read).  A job resizes one raw uint8 H x W x 3 image
 * (interleaved, as decoded) to new_h x new_w -- bilinear, half-pixel centres, edge-clamped, no antialias, evaluated in fp32
 * WITHOUT contraction and rounded half-to-even to a grey level q -- writes norm_lut[c][q] (c the OUTPUT channel; the host
 * fills the table with (float32(q) - mean[c]) / std[c]) into its [3, out_h, out_w] float32 slot, mirrored left-right
 * inside the new_w columns when `flip`, and writes 0.0f to every slot element outside new_h x new_w (the slot may be a
 * reused buffer).  reverse_channels != 0: output channel c reads source channel 2 - c (to_rgb=False).  Per axis, with d the
 * index in the un-flipped resized image: src = max(scale * (d + 0.5f) - 0.5f, 0), i0 = min((int)src, n - 1),
 * i1 = i0 + (i0 < n - 1), l1 = src - i0, l0 = 1 - l1; v = ly0 * (lx0 * a + lx1 * b) + ly1 * (lx0 * c + lx1 * d).
 * Bit-exact against kgdet_amd/preprocess.py::image_transform_restatement.  Several jobs may read one source.  The last
 * destination dimension is contiguous; rows are stored 16 bytes at a time where dst, the strides and x allow.
 * n_jobs == 0 is a no-op; n_jobs > KGDET_PREPROC_MAX_JOBS returns KGDET_E_UNSUPPORTED (the caller splits); a null
 * pointer, a non-positive size, out < new, a row pitch / stride that does not hold its row return KGDET_E_SHAPE. */
#define KGDET_PREPROC_MAX_JOBS 32
typedef struct kgdet_preproc_job {
  const uint8_t *src;                      /* device, H x W x 3 interleaved, as decoded (RGB) */
  int32_t src_h, src_w, src_row_bytes;     /* row pitch >= 3 * src_w */
  float *dst;                              /* device, channel 0 of this job's [3, out_h, out_w] slot */
  int64_t dst_channel_stride;              /* elements */
  int32_t dst_row_stride;                  /* elements */
  int32_t new_h, new_w;                    /* resized size = img_shape */
  int32_t out_h, out_w;                    /* slot size = pad_shape or the batch's common size; zero-filled beyond new_h / new_w */
  float scale_y, scale_x;                  /* float32(src_h) / new_h, float32(src_w) / new_w, computed by the host in float32 */
  int32_t flip;                            /* horizontal, applied to the resized image (before padding) */
} kgdet_preproc_job;
int kgdet_image_preprocess(const kgdet_preproc_job *jobs, int32_t n_jobs, const float *norm_lut /* device [3][256] */,
                           int32_t reverse_channels, void *stream);
/* Image preprocessing under train-time extra_aug (kgdet_amd/augment.py draws the plan; kgdet_amd/preprocess.py): the launch
 * of kgdet_image_preprocess with photometric distortion on every source pixel and an expand / crop window in front of the
 * resize, n_jobs <= KGDET_PREPROC_AUG_MAX_JOBS jobs, the table passed by value (capturable, no host read; mean / std are
 * HOST pointers to 3 floats each, read during the call).  The image is float32 from the first step and is never quantised
 * to a grey level: out = (v - mean[c]) / std[c], one subtraction and one correctly rounded division (c the OUTPUT channel,
 * which reads source channel 2 - c when reverse_channels).  Everything is evaluated in fp32 WITHOUT contraction, every
 * operation rounded on its own; bit-exact against kgdet_amd/preprocess.py::image_transform_restatement_aug.
 * Colour, per source pixel (r, g, b) = the raw bytes as floats, only when KGDET_AUG_COLOUR is set (the HSV round trip then
 * runs whatever else is on; it is not the identity in fp32), max / min taken as (b > a ? b : a) / (b < a ? b : a):
 *   1. KGDET_AUG_BRIGHTNESS: x = x + delta        2. KGDET_AUG_CONTRAST and KGDET_AUG_CONTRAST_FIRST: x = x * alpha
 *   3. to HSV, EPS = 2^-23: v = max(r, g, b), vmin = min(r, g, b), diff = v - vmin, s = diff / (|v| + EPS),
 *      d = 60 / (diff + EPS); h = (g - b) * d if v == r, else (b - r) * d + 120 if v == g, else (r - g) * d + 240;
 *      if h < 0: h += 360
 *   4. KGDET_AUG_SATURATION: s = s * sat          5. KGDET_AUG_HUE: h = h + hue; if h > 360: h -= 360; if h < 0: h += 360
 *   6. to RGB: s == 0 gives r = g = b = v; else h = h * (float)(6.0 / 360.0); while h < 0: h += 6; while h >= 6: h -= 6;
 *      k = floor(h), f = h - k (k >= 6: k = 0, f = 0); t = [v, v * (1 - s), v * (1 - s * f), v * (1 - s * (1 - f))];
 *      (b, g, r) = t[i] for the index triple of sector k in [(1,3,0), (1,0,2), (3,0,1), (0,2,1), (0,1,3), (2,1,0)]
 *   7. KGDET_AUG_CONTRAST without KGDET_AUG_CONTRAST_FIRST: x = x * alpha
 *   8. KGDET_AUG_PERMUTE: new[j] = old[q[j]], q[j] = (perm >> 2j) & 3 over (r, g, b)
 * Window: the resize reads a virtual vh x vw image V; V[y][x] is the distorted raw pixel (y - oy, x - ox) where that lies
 * inside the raw image and fill[] (raw channel order, NOT distorted) elsewhere; oy / ox may be negative (a crop), and a window
 * that misses the raw image altogether is allowed.  The taps are those of kgdet_image_preprocess with n = vh / vw (scale_y =
 * float32(vh) / new_h, scale_x = float32(vw) / new_w), edge-clamped at V's borders; v = ly0 * (lx0 * a + lx1 * b) + ly1 * (lx0 *
 * c + lx1 * d); flip, zero padding beyond new_h x new_w and the 16-byte stores are the plain entry's.  Under
 * KGDET_AUG_COLOUR a workgroup distorts the reachable part of an output row's two source rows once into LDS; rows whose
 * reachable segment exceeds 1536 pixels are distorted per tap instead (the same bits either way).
 * Errors as the plain entry (KGDET_E_UNSUPPORTED for n_jobs > KGDET_PREPROC_AUG_MAX_JOBS: the caller splits), and
 * KGDET_E_SHAPE for vh / vw < 1, |oy| / |ox| beyond 2^20, a perm that is not a permutation of (0, 1, 2) under
 * KGDET_AUG_PERMUTE, unknown flag bits or a stage flag without KGDET_AUG_COLOUR, and -- under KGDET_AUG_COLOUR -- a delta / alpha / sat that is not finite or beyond
 * 65536 in magnitude or a |hue| above 720 (the bounds keep every intermediate finite and the two while loops to 3 trips). */
#define KGDET_PREPROC_AUG_MAX_JOBS 16
#define KGDET_AUG_COLOUR 1u
#define KGDET_AUG_BRIGHTNESS 2u
#define KGDET_AUG_CONTRAST 4u
#define KGDET_AUG_CONTRAST_FIRST 8u
#define KGDET_AUG_SATURATION 16u
#define KGDET_AUG_HUE 32u
#define KGDET_AUG_PERMUTE 64u
typedef struct kgdet_preproc_aug_job {
  const uint8_t *src;                      /* the fields of kgdet_preproc_job, with the same meaning ... */
  int32_t src_h, src_w, src_row_bytes;
  float *dst;
  int64_t dst_channel_stride;
  int32_t dst_row_stride;
  int32_t new_h, new_w;
  int32_t out_h, out_w;
  float scale_y, scale_x;                  /* ... except: float32(vh) / new_h, float32(vw) / new_w */
  int32_t flip;
  int32_t vh, vw;                          /* the virtual image the resize reads: the crop patch, else the canvas, else the raw image */
  int32_t oy, ox;                          /* where raw pixel (0, 0) sits in it: (top - y1, left - x1) */
  float fill[3];                           /* V outside the raw image, in the raw image's channel order */
  float delta, alpha, sat, hue;            /* brightness, contrast, saturation, hue (degrees); read only when their flag is set */
  int32_t perm;                            /* q[0] | q[1] << 2 | q[2] << 4 */
  uint32_t flags;                          /* KGDET_AUG_* */
} kgdet_preproc_aug_job;
int kgdet_image_preprocess_aug(const kgdet_preproc_aug_job *jobs, int32_t n_jobs, const float *mean /* host [3] */,
                               const float *std /* host [3] */, int32_t reverse_channels, void *stream);
/* COCO-style bbox / OKS evaluation on the device (evaluation.CocoEvaluator's similarity and matching steps;
 * kgdet_amd/evaluation_device.py packs the arrays and holds the numpy restatement).  All device pointers; one launch each
 * over the C (image, category) cells of `cells` int32 [C, 4] = (first detection, detections, first ground truth, ground
 * truths) into the packed arrays of ND detections (inside a cell in descending-score order) and NG ground truths;
 * sim_off int64 [C] = where the cell's row-major [D, G] block starts in sim (sim_size doubles).  A cell whose ranges leave
 * the arrays is skipped.  Coordinates, areas and similarities are float64, evaluated without contraction.
 * kgdet_coco_similarity: iou_type 0 = box IoU of d_box / g_box [n, 4] xywh, union = the detection's area against a crowd
 * ground truth (g_crowd int32), bit-identical to evaluation.box_iou_xywh; iou_type 1 = OKS over K landmarks of d_kxy
 * [ND, K, 2] against g_kpt [NG, K, 3] (x, y, v) with var [K] = (2 sigma)^2: the landmarks with v > 0 (g_nvis int32 [NG] =
 * their number) or, when there is none, all K by the distance to the doubled g_box; exponent argument
 * (dx^2 + dy^2) / var / (area + 2^-52) / 2 bit-identical to evaluation.oks, summed over a wave's lanes in a fixed order.
 * Pointers the chosen type does not read may be NULL.
 * kgdet_coco_match: the greedy sweep of CocoEvaluator._match for every (area range a < A, threshold t < T), A * T <= 64
 * (KGDET_E_SHAPE beyond): area_rng [A, 2], best0 [T] = min(threshold, 1 - 1e-10), g_ignore uint8 [NG] = the type's base
 * flag (crowd; keypoints: no labelled landmark either).  Writes d_match int32 [ND, A, T] = 1 + the packed index of the
 * matched ground truth or 0, d_ignore uint8 [ND, A, T], g_ignore_out uint8 [NG, A] (in packed order, not sorted);
 * g_taken uint8 [NG, A, T] is scratch, initialised by the kernel. */
int kgdet_coco_similarity(int32_t iou_type, const int32_t *cells, const int64_t *sim_off, int32_t C, int64_t ND, int64_t NG,
                          int64_t sim_size, const double *d_box, const double *d_kxy, const double *g_box,
                          const double *g_kpt, const double *g_area, const int32_t *g_crowd, const int32_t *g_nvis,
                          const double *var, int32_t K, double *sim, void *stream);
int kgdet_coco_match(const int32_t *cells, const int64_t *sim_off, int32_t C, int64_t ND, int64_t NG, int64_t sim_size,
                     const double *sim, const double *d_area, const double *g_area, const uint8_t *g_ignore,
                     const int32_t *g_crowd, const double *area_rng, int32_t A, const double *best0, int32_t T,
                     int32_t *d_match, uint8_t *d_ignore, uint8_t *g_ignore_out, uint8_t *g_taken, void *stream);
/* CocoEvaluator.accumulate on the device, from kgdet_coco_match's outputs as they lie in device memory (all pointers below
 * are device pointers).  Results are BIT-EQUAL to evaluation_device.DeviceCocoEvaluator.accumulate_restatement: counts are
 * int32, the two divisions are single float64 divisions without contraction, max and the comparisons are exact, and there
 * are no float atomics, so two runs give the same bits.
 * kgdet_coco_count_gt: n_gt int32 [K, A] = the number of ground truths g < NG with g_cat[g] == k (int32 [NG]) and
 * g_ignore[g, a] == 0 (uint8 [NG, A], kgdet_coco_match's g_ignore_out).  Every element is written (NG == 0: zeros).
 * kgdet_coco_accumulate: one workgroup per line (k, a, m, t) walks the category's sequence order[cat_cut[k] .. cat_cut[k+1])
 * in tiles of KGDET_COCO_ACC_TILE positions.  order int64 [ND]: the detections grouped by category, inside a category in
 * descending score, equal scores in (image, rank) order (ONE stable sort per evaluation); cat_cut int64 [K + 1]; rank int32
 * [ND] = the detection's position inside its cell; a position is selected when rank < max_dets[m] (int32 [M], ascending).
 * Over the selected positions tp counts d_match != 0 && !d_ignore and fp counts d_match == 0 && !d_ignore (int32 / uint8
 * [ND, A, T]); score float64 [ND]; rec_thrs float64 [R].  Written, every element of them:
 *   recall [T, K, A, M] = tp_total / n_gt; precision, scores [T, R, K, A, M]: with pos the first selected position where
 *   tp / n_gt >= rec_thrs[r] (searchsorted side='left'), max over the positions >= pos of tp / (fp + tp + 2^-52) and the
 *   score at pos; 0 where there is no such position (a line that selects nothing is all 0); all three -1 where
 *   n_gt[k, a] == 0.
 * An entry of order outside [0, ND) is skipped, cat_cut is clamped to [0, ND].
 * workspace: 16 * tp_cap bytes per line, K * A * M * T lines (float64 precision and score at the first position of every
 * true-positive count): workspace_bytes >= 16 * tp_cap * K * A * M * T, with tp_cap >= max over (k, a) of
 * min(cat_cut[k+1] - cat_cut[k], n_gt[k, a]) -- kgdet_coco_match never yields more true positives than that (a regular
 * ground truth is matched once); the host may take min(sequence length, ground truths of the category).  A line is
 * recorded up to min(sequence length, n_gt, tp_cap) true positives; flags no matching could have written (more) are counted
 * in recall and otherwise dropped, never stored out of bounds.
 * Refused before any launch: A, T < 1 or A * T > 64, K, M, R < 1 or K * A * M * T >= 2^31, ND outside [0, 2^31 - 1),
 * tp_cap < 0 (KGDET_E_SHAPE); a null pointer where data is required -- the detection arrays only when ND > 0, the workspace
 * only when tp_cap > 0 (KGDET_E_SHAPE); a workspace that is too small (KGDET_E_WORKSPACE).
 * kgdet_coco_pack_landmarks: kpt2json + load_results for landmark rows.  src float32 [n, 3K] (x, y, v per landmark);
 * kxy float64 [n, K, 2] = np.round(float64(x | y), num_digits) = rint(v * 10^d) / 10^d (ties to even, two float64
 * operations, no contraction); bbox float64 [n, 4] = (x0, y0, x1 - x0, y1 - y0) from the min / max over ALL K rounded
 * coordinates, area float64 [n] = (x1 - x0) * (y1 - y0).  Bit-equal to the host packing (the sign of a zero extent
 * corner follows the reduction order, as numpy's does).  One wave per row, KGDET_COCO_PACK_ROWS rows per workgroup, any n.
 * n == 0 is a no-op; K < 1, n < 0 or n > 2^31 - 1 rows, num_digits outside [0, 15] or a null pointer: KGDET_E_SHAPE. */
#define KGDET_COCO_ACC_TILE 1024
#define KGDET_COCO_PACK_ROWS 4
int kgdet_coco_count_gt(const uint8_t *g_ignore, const int32_t *g_cat, int64_t NG, int32_t K, int32_t A, int32_t *n_gt,
                        void *stream);
int kgdet_coco_accumulate(const int32_t *d_match, const uint8_t *d_ignore, const double *score, const int32_t *rank,
                          const int64_t *order, const int64_t *cat_cut, const int32_t *n_gt, const int32_t *max_dets,
                          const double *rec_thrs, int64_t ND, int32_t K, int32_t A, int32_t T, int32_t M, int32_t R,
                          int64_t tp_cap, double *precision, double *recall, double *scores, void *workspace,
                          size_t workspace_bytes, void *stream);
int kgdet_coco_pack_landmarks(const float *src, int64_t n, int32_t K, int32_t num_digits, double *kxy, double *bbox,
                              double *area, void *stream);
/* pack_test_results on the device: the detections of a test run as they lie in rows float32 [N, M, W], W = 7 + 3K (the
 * layout of get_bboxes_packed_tensor: box x1 y1 x2 y2, score, label, count, K landmarks x y v; runner.DeviceResults.rows),
 * ordered, rounded, cut and gathered into the packed arrays of evaluation_device.Packed for BOTH result kinds, bit-equal to
 * evaluation_device.pack_rows_restatement and so to pack_test_results(..., lazy_landmarks=True) on the host list.  All
 * pointers are device pointers except the two kgdet_coco_packed_dets structs themselves (host; their members are device
 * pointers).  rows needs 4-byte alignment only; kxy32 8-byte alignment.  Of image n only the first count rows are read,
 * count = trunc(rows[n, 0, 6]); a label is trunc(rows[n, i, 5]), rows whose label lies outside [0, L) are dropped as
 * bbox2result_kp drops them.
 * kgdet_coco_order_dets (one workgroup per image):  img_slot int32 [N] = the image's index into the packed ground truth's
 * sorted image ids (-1: unknown), cat_of_label int32 [L] = the label's index into its sorted category ids in [0, C) or -1
 * (such a row is never packed, but counts in the ids), n_cells = images of the ground truth x C.  Per row i < count with a
 * label in range it writes vals float64 [N, M, 6] = x, y, w, h, score, area: xywh = x1, y1, x2 - x1 + 1, y2 - y1 + 1 on the
 * widened values, xywh and the score rounded like Python's round(v, num_digits) -- with S = 10^d: p = |v| * S,
 * e = fma(|v|, S, -p), n = floor(p) or floor(p) + 1 by p - floor(p) against one half, at one half by the sign of e, at
 * e == 0 the even one; copysign(n / S, v) -- and area = w * h of the rounded values; and info int32 [N, M, 3] = the
 * category index or -1, k = the row's index in the image's enumeration (label ascending, then row order), and the rank inside
 * the (image, category) cell by descending rounded score, ties by k (-1, -1, -1 for a dropped row).  img_rows int32 [N] = the
 * rows of the image that count in the ids; cnt_bbox / cnt_kp int32 [n_cells]: min(rows of the cell, cut) at
 * [img_slot * C + c] for every c < C of every image with a known slot (cells of other images are not touched: zero them).
 * flags int32 [2], ADDED to (zero them): [0] values that are not finite or with |v| * 10^d >= 2^40, left unrounded;
 * [1] images whose count is not in [0, M] or that hold rows but no known slot (skipped), and, from the scatter, rows whose
 * place lies outside the output (skipped).  The caller reads the flags with the counts and treats non-zero as an error.
 * kgdet_coco_scatter_dets (one workgroup per image):  img_base int64 [N] = exclusive scan of img_rows in image order,
 * start_bbox / start_kp int64 [n_cells + 1] = exclusive scans of cnt_bbox / cnt_kp.  A row with rank < cut goes to
 * pos = start[cell] + rank of that kind: cell = img_slot * C + category, img_idx, cat_idx, id = img_base + k + 1 (int64
 * [n]), score [n], bbox [n, 4], area [n] (float64; bbox and area may be NULL: not written), and for out_kp kxy32 float32
 * [n, 3K] = the row's landmark columns (NULL: not gathered), one wave per row, 16-byte loads at the source's 4-byte
 * alignment and 8-byte stores (K even; 4-byte accesses for odd K).  Every element of the outputs is written when start and
 * n come from the order kernel's counts.
 * Refused before any launch (KGDET_E_SHAPE): num_digits outside [1, 9], M outside [1, KGDET_COCO_ORDER_MAX_ROWS], L outside
 * [1, KGDET_COCO_ORDER_MAX_LABELS], W != 7 + 3K with K >= 1, C outside [1, 32767], a negative size or cut, N >= 2^31, a
 * null pointer where data is required.  N == 0 is a no-op. */
#define KGDET_COCO_ORDER_MAX_ROWS 1024
#define KGDET_COCO_ORDER_MAX_LABELS 64
typedef struct {
  int64_t n;                               /* rows of the packed arrays */
  int64_t *cell, *img_idx, *cat_idx, *id;  /* [n] */
  double *score, *bbox, *area;             /* [n], [n, 4], [n]; bbox / area may be NULL */
  float *kxy32;                            /* [n, 3K] or NULL */
} kgdet_coco_packed_dets;
int kgdet_coco_order_dets(const float *rows, int64_t N, int32_t M, int32_t W, const int32_t *img_slot,
                          const int32_t *cat_of_label, int32_t L, int32_t C, int64_t n_cells, int32_t num_digits,
                          int32_t cut_bbox, int32_t cut_kp, double *vals, int32_t *info, int32_t *img_rows, int32_t *cnt_bbox,
                          int32_t *cnt_kp, int32_t *flags, void *stream);
int kgdet_coco_scatter_dets(const float *rows, int64_t N, int32_t M, int32_t W, const int32_t *img_slot, int32_t C,
                            int64_t n_cells, const double *vals, const int32_t *info, const int64_t *img_base,
                            const int64_t *start_bbox, const int64_t *start_kp, int32_t cut_bbox, int32_t cut_kp,
                            const kgdet_coco_packed_dets *out_bbox, const kgdet_coco_packed_dets *out_kp, int32_t *flags,
                            void *stream);
/* results2json on the device (csrc/coco_json.hip): the text of the two result files, byte for byte what json.dump (default
 * separators) writes for kpt2json's lists, from rows and from what kgdet_coco_order_dets left (vals, info; call it with
 * img_slot = 0 .. N - 1, cat_of_label = 0 .. L - 1 and C = L so that no row is dropped for lack of ground truth).
 * Record r = img_base[image] + k, every row with a label in [0, L):
 *   bbox       {"image_id": I, "bbox": [x, y, w, h], "score": s, "category_id": c}
 *   keypoints  {"image_id": I, "keypoints": [v0, ..., v(3K-1)], "score": s, "category_id": c}
 * I = img_ids[image], c = cat_ids[label] (int64, non-negative); x y w h s from vals; v = rint(float64(value) * 10^d) / 10^d;
 * each printed as repr of the double: [-] integer digits . fractional digits without trailing zeros, at least one; zero
 * keeps its sign.  num_digits d in 1 .. 4; domain finite and |v| * 10^d < 2^40 (a value outside stands as 0.0).
 * kgdet_coco_json_measure (one workgroup per image, one wave per row): len_bbox / len_kp int32 [n_records] = the byte length
 * of record r of either kind, rec_src int64 [n_records] = image * M + row; n_records >= the sum of img_rows (entries no
 * record owns are left as they are).  flags int32 [2], ADDED to: [0] landmark values of written rows outside the domain,
 * [1] rows whose record index lies outside [0, n_records).
 * kgdet_coco_json_write (one workgroup per record, the record assembled in LDS and stored 16 bytes at a time): offset int64
 * [>= r1 + 1] = where record r begins in the file's body WITH the ", " that separates it from record r - 1, i.e. the
 * exclusive scan of len[r] + (r > 0 ? 2 : 0).  Records r0 <= r < r1 of `kind` (0 bbox, 1 keypoints) are written to
 * out + offset[r] - offset[r0]; range_bytes = offset[r1] - offset[r0] as the caller read it back, out_bytes the size of out.
 * Nothing outside [out, out + range_bytes) is written; the enclosing [ and ] are the caller's.  A record whose text is not
 * offset[r + 1] - offset[r] bytes long or lies outside the range is skipped and counted in flags[1].
 * Refused before any launch (KGDET_E_SHAPE): num_digits outside [1, 4], W != 7 + 3K with K in [1, KGDET_COCO_JSON_MAX_K]
 * (a record's LDS image, 144 + 51 K bytes, stays under 64 KiB), M outside [1, KGDET_COCO_ORDER_MAX_ROWS], L outside [1,
 * KGDET_COCO_ORDER_MAX_LABELS], N outside [0, 2^31), a null pointer where data is required, r0 < 0, r1 < r0, r1 > N * M,
 * out_bytes < range_bytes, a kind other than 0 / 1.  N == 0 or r0 == r1 is a no-op. */
#define KGDET_COCO_JSON_MAX_K 1024
int kgdet_coco_json_measure(const float *rows, int64_t N, int32_t M, int32_t W, const double *vals, const int32_t *info,
                            const int64_t *img_base, const int64_t *img_ids, const int64_t *cat_ids, int32_t L,
                            int32_t num_digits, int32_t *len_bbox, int32_t *len_kp, int64_t *rec_src, int64_t n_records,
                            int32_t *flags, void *stream);
int kgdet_coco_json_write(int32_t kind, const float *rows, int64_t N, int32_t M, int32_t W, const double *vals,
                          const int64_t *rec_src, const int64_t *offset, const int64_t *img_ids, const int64_t *cat_ids,
                          int32_t L, int32_t num_digits, int64_t r0, int64_t r1, int64_t range_bytes, uint8_t *out,
                          int64_t out_bytes, int32_t *flags, void *stream);
/* Detections and landmarks drawn on images (csrc/draw.hip; kgdet_amd/visualize.py: DeviceDrawer), bit for bit the picture
 * visualize.draw_restatement defines: per drawn row (score > score_thr, an integer label in [0, L), a finite box) the box
 * outline of `thickness`, with `contour` the capsules of width `line_width` between consecutive visible landmarks, the
 * landmark discs of `radius` (in kpt_color 0xRRGGBB, or the class colour for -1) and the label "name|d.dd" in 5 x 7 glyphs
 * scaled by `font_scale`; a pixel shows the covering primitive of the greatest (row, layer), else its source value.
 * One launch draws n <= KGDET_DRAW_MAX_IMAGES images of different sizes, out of place, between two flat uint8 buffers in
 * device memory (RGB, H x W x 3, rows packed): table is a HOST array int64 [n][4] = (source offset, destination offset, H, W)
 * and row_block a HOST array int32 [n] = the image's block of rows [N, M, W7 = 7 + 3K] (device, the layout of
 * get_bboxes_packed_tensor; the count is column 6 of the block's row 0, cut to [0, M]).  Both are read before the launch and
 * travel as kernel arguments, as the jobs of kgdet_image_preprocess do, so every size and offset is checked here.  Device
 * tables: colors uint8 [L][3]; name_bytes uint8 [name_total] with name_off int32 [L + 1] (a name is at most 255 bytes);
 * ranges int32 [L][2] = the landmarks [a, b) of a label, or NULL for all K; glyphs uint8 [256][7] = the row masks of every
 * byte, bit 4 the left column.  One wave per tile of 64 x 16 pixels; no atomics, no workspace, nothing read back.
 * Refused before the launch with nothing written (KGDET_E_SHAPE): n outside [0, KGDET_DRAW_MAX_IMAGES], M outside [1,
 * KGDET_DRAW_MAX_ROWS], W7 != 7 + 3K with K in [1, KGDET_DRAW_MAX_K], L outside [1, KGDET_DRAW_MAX_LABELS], H or W outside
 * [1, 8192], thickness or radius outside [1, 64], line_width outside [1, 16], font_scale outside [1, 8], kpt_color outside
 * [-1, 0xffffff], an image outside its buffer, a row block outside [0, N), overlapping buffers, a null pointer where data is
 * required.  n == 0 is a no-op.  Destination ranges of different images must not overlap (not checked). */
#define KGDET_DRAW_MAX_IMAGES 32
#define KGDET_DRAW_MAX_ROWS 1024
#define KGDET_DRAW_MAX_K 1024
#define KGDET_DRAW_MAX_LABELS 64
int kgdet_draw_detections(const uint8_t *src, int64_t src_bytes, uint8_t *dst, int64_t dst_bytes, const int64_t *table,
                          const int32_t *row_block, int32_t n, const float *rows, int64_t N, int32_t M, int32_t W7,
                          const uint8_t *colors, int32_t L, const uint8_t *name_bytes, const int32_t *name_off,
                          int32_t name_total, const int32_t *ranges, const uint8_t *glyphs, float score_thr, int32_t thickness,
                          int32_t radius, int32_t contour, int32_t line_width, int32_t font_scale, int32_t kpt_color,
                          void *stream);
/* Baseline JPEG files of RGB pictures in device memory (csrc/jpeg.hip; kgdet_amd/jpeg.py: DeviceJpegEncoder), byte for byte
 * the file jpeg.jpeg_restatement defines: JFIF, SOF0, Y / Cb / Cr sampled 2x2 / 1x1 / 1x1, one interleaved scan, the Annex K.1
 * quantisation tables scaled by the IJG rule for `quality`, the Annex K.3 Huffman tables, integer colour conversion, DCT and
 * quantisation with the roundings stated there.  One call takes n <= KGDET_JPEG_MAX_IMAGES images of different sizes out of
 * one flat uint8 buffer (RGB, H x W x 3, rows packed): table is a HOST array int64 [n][4] = (source offset, file offset, H, W),
 * the layout of kgdet_draw_detections' table, read and checked before any launch -- the drawer's destination buffer and
 * table serve as they are.
 * kgdet_jpeg_encode: transform (one wave per MCU) -> int16 coefficients; measure (one wave per MCU, lane = zigzag place) ->
 * bits per MCU; a scan per image; pack (a workgroup per KGDET_JPEG_RANGE_BYTES bytes of the unstuffed stream, boundary MCUs
 * coded by both neighbours, bits ORed into LDS) -> the stream and the 0xFF count of each range; a scan of those counts.  All
 * of it stays in `workspace` (16-byte aligned, kgdet_jpeg_workspace_bytes(table, n) bytes: about 2 KiB per MCU, the stream at
 * its worst case; 0 for a table that would be refused); lengths int64 [n] (device) = the bytes of each file.  Column 1 of the
 * table is not read.  The caller reads `lengths` back -- the one read-back -- and sizes the output.
 * kgdet_jpeg_write: the same table, n, quality and workspace; file i goes to out + table[i][1] when lengths[i] <= capacity[i]
 * (HOST int64 [n]) and status[i] (device int32 [n]) becomes 0; else NOTHING of it is written and status[i] becomes 1.  Nothing
 * outside [out + table[i][1], + lengths[i]) is written.  The bytes do not depend on launch geometry or schedule (integers
 * only; LDS integer OR, no global atomics).
 * Refused before any launch with nothing written (KGDET_E_SHAPE): n outside [0, KGDET_JPEG_MAX_IMAGES], quality outside [1,
 * 100], H or W outside [1, 8192], an image outside the source buffer, a file offset / capacity outside the output buffer,
 * capacities of two images that overlap, overlapping source / workspace / lengths (encode) or output / workspace / status
 * (write), a workspace that is not 16-byte aligned, a negative size, a null pointer where data is required; a workspace that is
 * too small is KGDET_E_WORKSPACE.  n == 0 is a no-op. */
#define KGDET_JPEG_MAX_IMAGES 32
#define KGDET_JPEG_RANGE_BYTES 4096
size_t kgdet_jpeg_workspace_bytes(const int64_t *table, int32_t n);
int kgdet_jpeg_encode(const uint8_t *src, int64_t src_bytes, const int64_t *table, int32_t n, int32_t quality, void *workspace,
                      size_t workspace_bytes, int64_t *lengths, void *stream);
int kgdet_jpeg_write(const int64_t *table, int32_t n, int32_t quality, const void *workspace, size_t workspace_bytes,
                     const int64_t *capacity, uint8_t *out, int64_t out_bytes, int32_t *status, void *stream);
/* Baseline JPEG files -> RGB pictures in device memory (csrc/jpeg_decode.hip; kgdet_amd/jpeg.py: DeviceJpegDecoder), bit for
 * bit the picture jpeg.decode_restatement defines (libjpeg's islow inverse DCT, fancy chroma upsampling and colour conversion
 * in integers), which is held to PIL's decoder.  The host parses the header (jpeg.parse_header) and uploads the files' bytes;
 * `src` is one flat device buffer that holds, per image, the scan's bytes (from the first entropy byte up to at least the
 * marker that ends it) and a table block of KGDET_JPEG_DECODE_TABLE_BYTES bytes:
 *   [0, 192)    quantisation tables of components 0, 1, 2, uint8, natural (row-major) order
 *   [192, 224)  BITS of the DC Huffman tables 0 and 1      [224, 256)  their values, 16 each
 *   [256, 288)  BITS of the AC Huffman tables 0 and 1      [288, 800)  their values, 256 each
 *   [800, 803)  DC table of components 0, 1, 2             [803, 806)  AC table of components 0, 1, 2
 * The workspace begins with uint32 [32] stream lengths and uint32 [32] rounds the fixpoint took (the most of an image's chunks).
 * `jobs` is a HOST array [n], read and checked before any launch.  mode: one component (its scan is not padded to an MCU), or
 * three components Y / Cb / Cr sampled 1x1 / 1x1 / 1x1 or 2x2 / 1x1 / 1x1.  out + dst_offset receives H x W x 3 RGB bytes,
 * rows packed.  status (device int32 [n]) becomes 0, or non-zero for a scan the decoder refuses: KGDET_JPEG_DECODE_NO_MARKER
 * (no marker before the buffer ends), _NOT_EOI (another marker than EOI ends the scan), _BAD_SCAN (an unmatched code, a zigzag
 * index past 63, a DC category above 11 or an AC category above 10, a block count other than the frame's, an end that is not
 * within the last byte of the stream).  The output region of such an image may hold anything; nothing outside the image's own
 * regions is written.  The table block's CONTENT is not checked (it lies on the device): every index made from it is clamped.
 * Kernels, all on `stream`, no read-back, a workgroup per image in the first two:
 *   unstuff  the scan ends at the first 0xFF that a byte other than 0x00 follows; a counted scan and a compaction remove the
 *            0xFF 0x00 stuffing.
 *   huffman  self-synchronising parallel decoding.  The stream is cut into subsequences of KGDET_JPEG_DECODE_SUBSEQ_BITS bits; a
 *            lane decodes the symbols that START in its subsequence from an entry state (bit position, block slot of the MCU,
 *            zigzag index) and records its exit state and the blocks it completed.  The workgroup takes
 *            KGDET_JPEG_DECODE_CHUNK_LANES subsequences at a time: the first lane's entry is the true state, the others start
 *            cold, and exit[i] -> entry[i + 1] is iterated with barriers and a workgroup-wide vote until nothing changes (round
 *            k fixes lane k at the latest: at most as many rounds as lanes, whatever the picture; speculative lanes write
 *            states only; a lane whose predecessor's parse was invalid keeps its cold start).  Then an exclusive scan of the block counts, a second decode of every subsequence from its true
 *            state that stores the non-zero coefficients (int16, natural order, every index checked), and at the end the
 *            inclusive scan of the DC differences per component.
 *   idct     a thread per block: dequantise, inverse DCT -> sample planes.      colour  upsample, convert, 16-byte stores at
 *            destination alignment with byte heads and tails.
 * Integers only: the picture does not depend on launch geometry or schedule.  No global atomics.
 * Refused before any launch with nothing written (KGDET_E_SHAPE): n outside [0, KGDET_JPEG_DECODE_MAX_IMAGES], H or W outside
 * [1, 8192], an unknown mode, scan_bytes outside [2, 2^28], a scan or table block outside `src`, a picture outside `out`,
 * pictures that overlap, overlapping src / workspace / out / status, a workspace that is not 16-byte aligned or smaller than
 * kgdet_jpeg_decode_workspace_bytes(jobs, n) (0 for jobs that would be refused), a negative size, a null pointer where data is
 * required.  n == 0 is a no-op. */
#define KGDET_JPEG_DECODE_MAX_IMAGES 32
#define KGDET_JPEG_DECODE_SUBSEQ_BITS 512
#define KGDET_JPEG_DECODE_CHUNK_LANES 1024
#define KGDET_JPEG_DECODE_TABLE_BYTES 1024
#define KGDET_JPEG_DECODE_GREY 0
#define KGDET_JPEG_DECODE_444 1
#define KGDET_JPEG_DECODE_420 2
#define KGDET_JPEG_DECODE_NO_MARKER 1
#define KGDET_JPEG_DECODE_NOT_EOI 2
#define KGDET_JPEG_DECODE_BAD_SCAN 3
#define KGDET_JPEG_DECODE_STOPPED (-1) /* kgdet_jpeg_decode_stages with stages < 4: no picture */
typedef struct kgdet_jpeg_decode_job {
  int64_t scan_offset, scan_bytes; /* inside src */
  int64_t tables_offset;           /* inside src */
  int64_t dst_offset;              /* inside out */
  int32_t H, W, mode, reserved;
} kgdet_jpeg_decode_job;
size_t kgdet_jpeg_decode_workspace_bytes(const kgdet_jpeg_decode_job *jobs, int32_t n);
int kgdet_jpeg_decode(const uint8_t *src, int64_t src_bytes, const kgdet_jpeg_decode_job *jobs, int32_t n, void *workspace,
                      size_t workspace_bytes, uint8_t *out, int64_t out_bytes, int32_t *status, void *stream);
/* For timing only (tools/time_jpeg_decode.py): kgdet_jpeg_decode cut short after its first `stages` kernels (1 .. 4; 4 is the
 * whole call).  With stages < 4 no picture is left and every status becomes KGDET_JPEG_DECODE_STOPPED. */
int kgdet_jpeg_decode_stages(const uint8_t *src, int64_t src_bytes, const kgdet_jpeg_decode_job *jobs, int32_t n,
                             void *workspace, size_t workspace_bytes, uint8_t *out, int64_t out_bytes, int32_t *status,
                             void *stream, int32_t stages);
/* The files cameras and phones write (jpeg.parse_header(camera=True), jpeg.decode_restatement(camera=True)): the same
 * arguments, the same job table and the same layout of `src`, and additionally
 *   mode KGDET_JPEG_DECODE_422   Y / Cb / Cr sampled 2x1 / 1x1 / 1x1: an MCU is 16 wide and 8 high, its blocks Y left, Y right,
 *                                Cb, Cr; chroma by libjpeg's h2v1 fancy upsampling over ceil(W / 2) samples a row,
 *                                out[2x] = (3 c[x] + c[x-1] + 1) >> 2, out[2x+1] = (3 c[x] + c[x+1] + 2) >> 2, neighbours
 *                                replicated at the edges (a row of two samples is replicated, as libjpeg does);
 *   reserved                     the restart interval in MCUs, 0 .. 65535, 0: none.
 * For the files kgdet_jpeg_decode takes the pictures are the same bits.  With an interval of R MCUs the scan holds
 * nint = ceil(MCUs / R) intervals between the markers RSTm, m = 0, 1, .. 7, 0, ..; every interval is decoded on its own from the
 * state (its first bit, slot 0, a DC code next) with predictors 0, holds exactly its share of blocks (R MCUs, the last one the
 * remainder) and ends within the last byte of its data.  status may also become KGDET_JPEG_DECODE_BAD_RESTART: a marker out of
 * turn, a missing or a surplus marker, an interval with another block count than its share or another end -- an interval cut
 * short at its tail included: the true parse stops in front of the symbol that no longer fits.  _BAD_SCAN stays what an invalid
 * code on the true parse gives, and what a wrong count or end gives in a job with interval 0.  A restart marker in a job with
 * interval 0 ends the scan: _NOT_EOI.  0xFF 0xFF ends the scan too (no fill bytes in front of a marker).
 * Kernels (all on `stream`, no read-back, no global atomics):
 *   unstuff  a workgroup per image, as above; a restart marker does not end the scan and both its bytes are dropped.  The
 *            lane that meets one learns its ordinal from the same workgroup scan that places the kept bytes, checks its number
 *            and the count, and writes where the next interval's un-stuffed bytes begin.  The INTERVAL TABLE of an image in the
 *            workspace: uint32 [nint + 1] begin, uint32 [nint + 1] length (bytes), uint32 [nint + 1] first subsequence -- an
 *            interval is cut into subsequences of KGDET_JPEG_DECODE_SUBSEQ_BITS bits from ITS first bit, at least one.
 *   huffman  a workgroup per (tile, image).  A tile is a run of whole intervals: as many as hold
 *            KGDET_JPEG_DECODE_CHUNK_LANES subsequences' worth of the scan's bytes on average, 1 .. CHUNK_LANES of them (the host's
 *            plan, from scan_bytes and the frame alone), so an image with more than a chunk of stream is decoded by several
 *            workgroups.  A lane per subsequence, CHUNK_LANES at a time; a lane that holds an interval's first subsequence enters
 *            with the true state and never takes its predecessor's exit; where a chunk begins inside an interval it follows the
 *            chunk before it as above.  A uniform picture with interval 1 has one-byte intervals: a lane each.  Block indices
 *            are i * R * blocks-per-MCU plus a segmented scan; stores stay inside the interval's own blocks.  The DC scan
 *            restarts at every interval.  Each tile leaves uint32 (status, rounds) in the workspace.
 *   verdict  a workgroup per image: the status of the first tile that refused, and into the `rounds` words of the workspace
 *            header the most rounds of any chunk of any tile.
 *   idct, colour  as above, with mode 3's slots and the h2v1 rule.
 * Refused with KGDET_E_SHAPE before any launch: everything kgdet_jpeg_decode refuses (mode above 3 here), reserved outside
 * [0, 65535], a workspace smaller than kgdet_jpeg_decode_camera_workspace_bytes(jobs, n), which accounts for the interval tables
 * and the tiles' words.  kgdet_jpeg_decode itself keeps refusing mode 3 and never reads `reserved`. */
#define KGDET_JPEG_DECODE_422 3
#define KGDET_JPEG_DECODE_BAD_RESTART 4
size_t kgdet_jpeg_decode_camera_workspace_bytes(const kgdet_jpeg_decode_job *jobs, int32_t n);
int kgdet_jpeg_decode_camera(const uint8_t *src, int64_t src_bytes, const kgdet_jpeg_decode_job *jobs, int32_t n, void *workspace,
                             size_t workspace_bytes, uint8_t *out, int64_t out_bytes, int32_t *status, void *stream);
/* For timing only: kgdet_jpeg_decode_camera cut short after `stages` of unstuff, huffman + verdict, idct, colour. */
int kgdet_jpeg_decode_camera_stages(const uint8_t *src, int64_t src_bytes, const kgdet_jpeg_decode_job *jobs, int32_t n,
                                    void *workspace, size_t workspace_bytes, uint8_t *out, int64_t out_bytes, int32_t *status,
                                    void *stream, int32_t stages);
int kgdet_nms(const float *dets, int64_t n, float iou_thr, int64_t *keep, int64_t *num_keep,
              void *workspace, size_t workspace_bytes, void *stream);
int kgdet_nms_batched(const float *dets, const int64_t *seg_offsets, int32_t num_segments,
                      int64_t total_n, int64_t max_seg_len, float iou_thr, int64_t *keep,
                      int64_t *num_keep, void *workspace, size_t workspace_bytes, void *stream);
int kgdet_soft_nms(const float *dets, int64_t n, float iou_thr, int32_t method, float sigma,
                   float min_score, float *out_dets, int64_t *out_inds, int64_t *num_out,
                   void *stream);

/* ------------------------------------------------------------------------------------------
 * Moment bounding box ("points2bbox", transform_method='moment';
 * R/../models/anchor_heads/reppoints_head_kp3rep_cas_1_assign_once.py:342-391).
 * pts [B, 2*n_pts, H, W] with (y,x) interleaved per point (y_first != 0) or (x,y); moment_transfer [2] (already
 * blended with its detached copy by the caller); bbox [B, 4, H, W] = (x1,y1,x2,y2).
 * Mean and UNBIASED std (n-1) over the points; half extent = std * exp(transfer).
 * Backward returns grad_pts and grad_transfer[2] (accumulated into a zero-filled buffer).
 * ------------------------------------------------------------------------------------------ */
int kgdet_moment_bbox_forward(const float *pts, const float *moment_transfer, int32_t B, int32_t n_pts,
                              int32_t HW, int32_t y_first, float *bbox, void *stream);
/* backward: grad_pts and grad_transfer [2] are OVERWRITTEN; the two transfer sums leave the blocks as partials in the
 * caller's workspace and are added in block order (no float atomics: bit-repeatable).  Where all points of a location
 * coincide (std == 0) the box is the mean and grad_pts is the mean term (g_lo + g_hi) / n alone -- finite, what
 * torch.std's backward fills in for 0 / 0 (tests/test_gpu_pointwise_kernels.py). */
size_t kgdet_moment_bbox_backward_workspace_bytes(int32_t B, int32_t HW);
int kgdet_moment_bbox_backward(const float *pts, const float *moment_transfer, const float *grad_bbox,
                               int32_t B, int32_t n_pts, int32_t HW, int32_t y_first, float *grad_pts,
                               float *grad_transfer, void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* KGDET_HIP_H_ */
