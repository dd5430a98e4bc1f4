// The Adam update of this library, stated once: torch._single_tensor_adam's order of operations in f32, the per-step scalars
// it reads and their layout in device memory.  Every Adam-bearing kernel (dense_f32.hip, linear_bf16.hip) goes
// through here, which is what makes "fused == two-pass", "multi == single", "bf16 gradient == widened gradient" and
// "graph replay == eager" the same arithmetic by construction.
#pragma once
#include "pv_common.h"

namespace pv {

// The six f32 scalars of one optimiser step.  This field order IS the layout of the six-float device array that
// pv_adam_scalars_advance writes and the `_dev` entry points read (adam_scalars_load / adam_scalars_store below).
struct AdamScalars {
  float one_minus_b1, beta2, one_minus_b2, bc2_sqrt, eps, neg_step_size;
};
static_assert(sizeof(AdamScalars) == 6 * sizeof(float), "AdamScalars is the six-float device array");

// python-float (double) scalars exactly as torch computes them, each narrowed to f32 at the kernel boundary
__host__ __device__ inline AdamScalars adam_scalars(double lr, double beta1, double beta2, double eps, int step) {
  const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
  return AdamScalars{(float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)sqrt(bc2), (float)eps,
                     (float)(-(lr / bc1))};
}

__device__ __forceinline__ AdamScalars adam_scalars_load(const float* __restrict__ ad_dev) {
  return AdamScalars{ad_dev[0], ad_dev[1], ad_dev[2], ad_dev[3], ad_dev[4], ad_dev[5]};
}
__device__ __forceinline__ void adam_scalars_store(float* __restrict__ ad_dev, const AdamScalars& ad) {
  ad_dev[0] = ad.one_minus_b1, ad_dev[1] = ad.beta2, ad_dev[2] = ad.one_minus_b2;
  ad_dev[3] = ad.bc2_sqrt, ad_dev[4] = ad.eps, ad_dev[5] = ad.neg_step_size;
}

// One element; g arrives already scaled.  No step of it may be contracted into an FMA (the build's -ffp-contract=off).
// `ad` travels by value, and a kernel hands it either its array elements or locals copied in and out: chosen per kernel so
// that each compiles to the instruction stream its hand-written copy compiled to (profiles/adam_once/NOTES.md).
__device__ __forceinline__ void adam_update(float& p, float& m, float& v, float g, const AdamScalars ad) {
  m = m + ad.one_minus_b1 * (g - m);                  // exp_avg.lerp_(grad, 1 - beta1)
  v = v * ad.beta2 + (ad.one_minus_b2 * g) * g;       // mul_(beta2).addcmul_(g, g, 1 - beta2)
  const float denom = sqrtf(v) / ad.bc2_sqrt + ad.eps;
  p = p + ad.neg_step_size * (m / denom);             // addcdiv_(exp_avg, denom, -step_size)
}

}  // namespace pv
