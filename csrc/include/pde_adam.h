// Element-wise torch.optim.Adam / AdamW update (torch/optim/adam.py:347-460 single-tensor math),
// used by the fused flat optimizers (optim.hip).
#pragma once
#include <hip/hip_runtime.h>

// The second moment is a sum of two products, which contracts to an fma in two ways (either product
// may be the one that is rounded first).  Every call site names its form, so no compiler's choice can
// split the results of two kernels: VF = 1 (g * ((1-b2)*g) + rounded b2*v) in the float4 update of the
// main blocks, VF = 2 (b2 * v + rounded (1-b2)*g*g) in the fold blocks.
template <int VF>
__device__ __forceinline__ void adam_elem(float& p, float& m, float& v, float gr, float lr, float wd, int decoupled,
                                          float omb1, float omb2, float b2, float step_size, float bc2s, float eps) {
  if (wd != 0.f) {
    if (decoupled) p = p * (1.f - lr * wd);
    else gr = gr + wd * p;
  }
  m = m + omb1 * (gr - m);
  static_assert(VF == 1 || VF == 2, "name the contraction");
  if constexpr (VF == 1) v = __builtin_fmaf(gr, omb2 * gr, v * b2);
  else v = __builtin_fmaf(b2, v, omb2 * gr * gr);
  const float denom = sqrtf(v) / bc2s + eps;
  p = p - step_size * (m / denom);
}
