// The sampler with the logit processors (repetition / frequency / presence penalties, logit bias,
// min_new_tokens) and the kernel that seeds their history with the prompt.  PdeSampleProc and the layout of the
// token counts are documented in pde_decode.h, the sampler itself in decode_sample.h and decode.hip.
#include "pde_hip.h"
#include "pde_bf16.h"
#include "pde_decode.h"
#include "pde_rng.h"

#include <math.h>

namespace {

#include "decode_sample.h"

// grid (ceil(width / 256), B): thread (b, t) marks token idx[b, t] of the prompt of row b, t < len_b
__global__ __launch_bounds__(256) void k_count_prompt(const int64_t* __restrict__ idx, const int* __restrict__ state,
                                                      int* __restrict__ counts, int width, int stride, int T0, int Vp) {
  const int t = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  int len = T0 + state[PDE_DS_OFF + b];
  len = len < width ? len : width;
  if (t >= len) return;
  const int64_t tok = idx[(size_t)b * stride + t];
  if (tok < 0 || tok >= Vp) return;
  counts[(size_t)b * Vp + tok] = PDE_TC_PROMPT;      // the counts are zero: every writer stores this word
}


}  // namespace

extern "C" {

hipError_t pde_sample_proc(PdeSample a, PdeSampleProc p, hipStream_t st) {
  return sample_ok(a) && proc_ok(a, p) ? sample_launch(a, st, p) : hipErrorInvalidValue;
}

hipError_t pde_count_prompt(const int64_t* idx, const int* state, int* counts, int B, int width, int stride, int T0,
                            int Vp, hipStream_t st) {
  if (B < 1 || B > PDE_DS_MAX_ROWS || width < 1 || stride < width || T0 < 0 || Vp < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_count_prompt, dim3((width + 255) / 256, B), dim3(256), 0, st, idx, state, counts, width, stride,
                     T0, Vp);
  return hipGetLastError();
}

}  // extern "C"
