// extern "C" entry of the LM-head loss without logits (csrc/kernels/lm_head_stats.hip).
//
// For h [N, C] and w [Vp, C] (bf16, contiguous, 16-byte aligned; C % 64 == 0, Vp % 8 == 0, 1 <= V <= Vp, both
// operands below 2 GiB) and targets tg [N] (a target outside [0, V): the row does not count), with
// x_v = sum_k h[i, k] w[v, k] accumulated in fp32 and never stored:
//   lse[i]  = logsumexp_{v < V} x_v
//   xt[i]   = x_{tg[i]}
//   sx[i]   = sum_{v < V} x_v                       (computed when sx is given or sm.spread != 0)
//   rows[i] = sm.w[i] * (lse - sm.keep * xt - sm.spread * sx + sm.z * lse^2)
// Each output pointer is nullable; a row that does not count gets exact zeros in every output whatever h holds
// there, and sm.w is not read for it.  w[V:] is never read.  part is a workspace of S * N * 4 floats (16-byte
// aligned) with S = pde_lm_head_slices(N, V); it needs no initialisation.  Two launches on `st`, no atomics, no memset, no host read.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "pde_kernels.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct PdeLmHeadStats {
  const void* h;
  const void* w;
  const int64_t* tg;
  float* part;
  float* lse;
  float* xt;
  float* sx;
  float* rows;
  PdeXentSmooth sm;      // {null, 1, 0, 0}: rows = lse - xt
  int N, C, V, Vp, S;
} PdeLmHeadStats;

int pde_lm_head_slices(int N, int V);
hipError_t pde_lm_head_stats(PdeLmHeadStats p, hipStream_t st);

#ifdef __cplusplus
}
#endif
