// Adam's per-element update and its per-step scalars, shared by the dense bucket kernel (nr_data.hip) and the row-deferred
// table kernels (nr_adamrows.hip).  Both must produce the same bits from the same inputs, so there is ONE definition of each.
#pragma once
#include <math.h>

#include "nr_common.h"

struct AdamCfg {
  float beta1, beta2, eps, step_size, bc2_sqrt, grad_scale;
  int zero_grad;
};

// step_size = lr / (1 - beta1^step), bc2_sqrt = sqrt(1 - beta2^step): double arithmetic, then the cast (host)
static inline void nr_adam_bias(float lr, float beta1, float beta2, int step, float* step_size, float* bc2_sqrt) {
  const double bc1 = 1.0 - pow((double)beta1, (double)step), bc2 = 1.0 - pow((double)beta2, (double)step);
  *step_size = (float)((double)lr / bc1);
  *bc2_sqrt = (float)sqrt(bc2);
}

#ifdef __HIPCC__
__device__ __forceinline__ void adam1(float& p, float& g, float& m, float& v, const AdamCfg& c) {
  const float gr = g * c.grad_scale;
  m = fmaf(1.f - c.beta1, gr - m, m);                             // exp_avg.lerp_(grad, 1 - beta1)
  v = fmaf(c.beta2, v, (1.f - c.beta2) * gr * gr);                // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, 1 - beta2)
  const float denom = sqrtf(v) / c.bc2_sqrt + c.eps;              // sqrt(v) / sqrt(1 - beta2^t) + eps
  p -= c.step_size * (m / denom);                                 // step_size = lr / (1 - beta1^t)
  if (c.zero_grad) g = 0.f;
}
#endif
