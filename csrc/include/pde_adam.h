// Element-wise torch.optim.Adam / AdamW update (torch/optim/adam.py:347-460 single-tensor math),
// used by the fused flat optimizers (optim.hip).
#pragma once
#include <hip/hip_runtime.h>

// The second moment is a sum of two products, which contracts to an fma in two ways (either product
// may be the one that is rounded first).  VF = 0 leaves the choice to the compiler: in the general
// Adam kernel it takes the first form in the grid-stride loop and the second in the fold blocks.
// The lean kernel pins each site to the same form (VF = 1 / 2), so both kernels give the same bits.
template <int VF = 0>
__device__ __forceinline__ void adam_elem(float& p, float& m, float& v, float gr, float lr, float wd, int decoupled,
                                          float omb1, float omb2, float b2, float step_size, float bc2s, float eps) {
  if (wd != 0.f) {
    if (decoupled) p = p * (1.f - lr * wd);
    else gr = gr + wd * p;
  }
  m = m + omb1 * (gr - m);
  if constexpr (VF == 1) v = __builtin_fmaf(gr, omb2 * gr, v * b2);
  else if constexpr (VF == 2) v = __builtin_fmaf(b2, v, omb2 * gr * gr);
  else v = v * b2 + omb2 * gr * gr;
  const float denom = sqrtf(v) / bc2s + eps;
  p = p - step_size * (m / denom);
}
