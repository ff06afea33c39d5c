// Device expressions shared by the fused loss kernels (head_loss.hip, serial_loss.hip): the sigmoid focal loss with the
// float / double promotions of csrc/focal.hip.
#pragma once
#include <float.h>

#include "common.h"

namespace kgdet {

__device__ __forceinline__ double neg_softplus_d(float x) {  // as csrc/focal.hip
  const int ge = x >= 0;
  return -1. * x * ge - logf((float)(1. + expf((float)(x - 2. * x * ge))));
}

// sigmoid_focal_loss_cuda.cu:24-59 (same promotions as csrc/focal.hip)
__device__ __forceinline__ float focal_fwd(float x, int t, int d, float gamma, float alpha) {
  const float c1 = (t == (d + 1));
  const float c2 = ((t >= 0) & (t != (d + 1)));
  const float zn = (float)(1.0 - alpha), zp = alpha;
  const float p = (float)(1. / (1. + expf(-x)));
  const float term1 = powf((float)(1. - p), gamma) * logf(fmaxf(p, FLT_MIN));
  const float term2 = (float)(powf(p, gamma) * neg_softplus_d(x));
  float l = 0.0f;
  l += -c1 * term1 * zp;
  l += -c2 * term2 * zn;
  return l;
}

// :62-97
__device__ __forceinline__ float focal_bwd(float x, int t, int d, float gamma, float alpha) {
  const float c1 = (t == (d + 1));
  const float c2 = ((t >= 0) & (t != (d + 1)));
  const float zn = (float)(1.0 - alpha), zp = alpha;
  const float p = (float)(1. / (1. + expf(-x)));
  const float term1 = (float)(powf((float)(1. - p), gamma) * (1. - p - (p * gamma * logf(fmaxf(p, FLT_MIN)))));
  const float term2 = (float)(powf(p, gamma) * (neg_softplus_d(x) * (1. - p) * gamma - p));
  float g = 0.0f;
  g += -c1 * term1 * zp;
  g += -c2 * term2 * zn;
  return g;
}

}  // namespace kgdet
