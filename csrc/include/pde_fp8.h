// FP8 (OCP e4m3fn) forward path: per-tensor quantiser and the FP8 MFMA GEMM (gemm_fp8.hip).  gfx950 only.
//
// Numeric definition (the CPU twin is ops/fp8.py, quantize_reference):
//   amax = max |t| (fp32);  s = 2^k, the largest power of two with amax * s <= 448 (k <= 126 so that s and
//   1 / s are both normal fp32; s = 1 when amax == 0);  q = e4m3fn_rne(clamp(fp32(t) * s, -448, 448)).
//   y[m][n] = bf16((sum_k xq[m][k] * wq[n][k]) * (1 / sx) * (1 / sw) + bias[n]), fp32 accumulation.
//
// Scale block: two fp32 per tensor, {s, 1 / s}, written by the quantiser's cast pass on the device and read by
// the GEMM epilogue from the device -- never a launch argument, so a captured launch follows the data.
//
// Quantiser workspace: two uint32 words per table entry, {amax bits, finished-block count}, zero before the
// first use.  The amax pass folds max |t| into word 0 with an integer atomic max on the non-negative float's
// bits (order independent: two runs give the same bits); the cast pass reads it, and its last block writes the
// scale block and sets both words back to zero, so the same words serve the next call on the stream and a
// captured pair replays without a memset.  Calls that share a workspace must be ordered on one stream.
//
// Operand images: both GEMM operands are [rows][K] byte matrices, K contiguous.  An LDS stage holds a 128-byte
// K slice of BM x-rows and BN w-rows as [rows][128 B] images in the XOR-swizzled layout of pde_lds.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// most tensors one quantiser launch pair takes (a by-value table in the kernel arguments); the launcher chunks
// longer lists
#define PDE_FP8_MAX_TENSORS 64

#ifdef __cplusplus
extern "C" {
#endif

// One tensor of a quantiser call: n contiguous bf16 values (n % 16 == 0, 16-byte aligned) -> n e4m3 bytes
// (8-byte aligned) and the scale block {s, 1 / s}.
typedef struct {
  const void* src;
  void* dst;
  float* scale;
  int64_t n;
} PdeFp8Tensor;

// Quantise `count` tensors with two launches per PDE_FP8_MAX_TENSORS of them.  `work` holds 2 * count zeroed
// uint32 words (see above).
hipError_t pde_fp8_quantize(const PdeFp8Tensor* tensors, int count, uint32_t* work, hipStream_t st);

// y [M][N] bf16 = xq [M][K] . wq [N][K]^T * (xs[1] * ws[1]) + bias; y2 != null: y = gelu(pre), y2 = gelu'(pre)
// with pre rounded to bf16 first, as the bf16 GEMM's GELU epilogue does.  N % 8 == 0, K % 64 == 0.
hipError_t pde_gemm_fp8(const void* xq, const void* wq, const float* xs, const float* ws, void* y, void* y2,
                        const void* bias, int M, int N, int K, hipStream_t st);
void pde_gemm_fp8_tile(int* bm, int* bn);

#ifdef __cplusplus
}
#endif
