// MXFP8 forward path: block-scaled e4m3 operands, their one-pass quantisers and the block-scaled MFMA GEMM
// (gemm_mxfp8.hip).  gfx950 only.
//
// Numeric definition (the CPU twin is ops/fp8.py, quantize_mx_reference):
//   a block is 32 consecutive elements of the last dimension (last dimension % 32 == 0);  amax = max |t| over
//   the block (fp32) = m * 2^e with m in [1, 2);  k = 0 when amax == 0, else k = 8 - e when m <= 1.75 and 7 - e
//   otherwise, clamped to k <= 127: the largest power of two with amax * 2^k <= 448 (pde_fp8.h's per-tensor rule,
//   per block; the OCP floor(log2 amax) - 8 rule differs only for m > 1.75, where it saturates and this does not);
//   q = e4m3fn_rne(clamp(fp32(t) * 2^k, -448, 448));  scale byte E = 127 - k (E8M0, in [0, 247], never 255);
//   the dequantised value is q * 2^(E - 127).
//   y[m][n] = bf16(sum_g 2^(Ex[m][g] + Ew[n][g] - 254) * (sum_{k in g} xq[m][k] wq[n][k]) + bias[n]),
//   fp32 accumulation, one rounding.
//
// An MX tensor is two arrays: the e4m3 bytes in the source's shape and the scale bytes [..., last / 32],
// both contiguous.  No kernel here needs a workspace, an atomic or a second pass: whoever holds 32 consecutive
// elements of a row quantises them on the spot, so every launch is capturable from the first call.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pde_kernels.h"

// most tensors one quantiser launch takes (a by-value table in the kernel arguments); the launcher chunks
// longer lists
#define PDE_MX_MAX_TENSORS 64

#ifdef __cplusplus
extern "C" {
#endif

// One tensor of a quantiser call: n contiguous bf16 values (n % 32 == 0, 16-byte aligned) -> n e4m3 bytes
// (8-byte aligned) and n / 32 scale bytes.
typedef struct {
  const void* src;
  void* dst;
  uint8_t* scale;
  int64_t n;
} PdeMxTensor;

// Quantise `count` tensors with one launch per PDE_MX_MAX_TENSORS of them.
hipError_t pde_mx_quantize(const PdeMxTensor* tensors, int count, hipStream_t st);

// y [M][N] bf16 = the block-scaled product of (xq [M][K], xe [M][K / 32]) and (wq [N][K], we [N][K / 32]) + bias;
// y2 != null: y = gelu(pre), y2 = gelu'(pre) with pre rounded to bf16 first.  aq != null (needs y2 and
// N % 32 == 0): the same launch also writes y as an MX tensor, aq [M][N] bytes and ae [M][N / 32] scale bytes,
// bit for bit the quantisation of the bf16 y it stores.  N % 8 == 0, K % 128 == 0.
hipError_t pde_gemm_mxfp8(const void* xq, const void* wq, const void* xe, const void* we, void* y, void* y2,
                          const void* bias, void* aq, void* ae, int M, int N, int K, hipStream_t st);

// pde_ln_fwd (pde_kernels.h) that also writes Y as an MX tensor: Q [N][C] bytes, E [N][C / 32] scale bytes, bit
// for bit the quantisation of the bf16 Y.  S, Y, mean and rstd are what pde_ln_fwd writes.  C % 32 == 0.
hipError_t pde_ln_fwd_mx(const void* X, const void* D, void* S, const void* G, const void* B, void* Y, float* mean,
                         float* rstd, void* Q, void* E, int N, int C, float eps, PdeDrop drop, hipStream_t st);

#ifdef __cplusplus
}
#endif
