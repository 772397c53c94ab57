// Learning-rate schedules that survive hipGraph replay: a device table of one fp32 rate per
// optimizer step, indexed on the device by the step count the optimizer kernel already reads.
// Step t (1-based) uses lr_tab[min(t-1, lr_len-1)]: a run longer than the table keeps its last
// entry.  A null table returns the by-value lr untouched (no load, the captured-constant path).
// The address is block-uniform (kernel argument + the uniform step), so every block reads its one
// value once, before its element loop.
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ float sched_lr(float lr, const float* __restrict__ lr_tab, int lr_len, long long t) {
  if (lr_tab == nullptr) return lr;
  long long k = t - 1;
  if (k > (long long)lr_len - 1) k = (long long)lr_len - 1;
  if (k < 0) k = 0;
  return lr_tab[k];
}
