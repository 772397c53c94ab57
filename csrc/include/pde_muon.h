// Muon: momentum SGD whose update matrix is orthogonalised by a bf16 Newton-Schulz iteration (muon.hip).  gfx950.
//
// The numeric definition is written once in pytorch_distributed_example_amd/optim/muon.py (its CPU twin is
// ops.newton_schulz_reference); in short, per matrix W [R, C]:
//   M <- mu M + g;  U = g + mu M (nesterov) or M;  X <- bf16(U / (||U||_F + 1e-7)) in the wide orientation
//   [n = min(R, C), m = max(R, C)];  ns_steps times { A <- bf16(X X^T);  B <- bf16(b A + c A A);
//   X <- bf16(a X + B X) } with fp32 accumulation and one rounding each;  Wm <- Wm (1 - lr wd) - lr scale O,
//   W <- bf16(Wm), O = X in W's orientation, scale = sqrt(max(1, R / C)).
//
// Every launch takes a by-value table of up to PDE_MUON_MAX_MATS matrices (the launchers chunk longer lists), uses no
// atomics, no memset and no host read, and can be captured from its first call.
//
// Limits (hipErrorInvalidValue beyond them): R, C multiples of 64, every matrix below 2 GiB, pointers 16-byte
// aligned.  The matrices of a GEMM launch may differ in every dimension: each table entry carries its own.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define PDE_MUON_MAX_MATS 64

#ifdef __cplusplus
extern "C" {
#endif

// One problem of a grouped GEMM launch, all bf16 row-major.
//   symmetric:   D [rows, rows] = alpha C + beta P P^T,  P = A [rows, K], C symmetric [rows, rows] or null (alpha
//                ignored); B and cols are unused.  D comes out symmetric bit for bit.
//   rectangular: D [rows, cols] = alpha C + beta A^T B,  A [K, rows] (the caller passes a symmetric matrix, K = rows),
//                B [K, cols], C [rows, cols].  D must not alias B or C.
typedef struct {
  const void* A;
  const void* B;
  const void* C;
  void* D;
  int rows, cols, K;
  int tile0;   // filled by the launcher: first block of this problem
} PdeMuonGemm;

// One matrix of a streaming launch (R x C, row-major; wide = [min(R, C), max(R, C)] row-major).
//   prologue: src = g (bf16), f32 = momentum (fp32, null: U = g), dst = X0 (bf16, wide)
//   apply:    src = X (bf16, wide), f32 = master (fp32, null: dst = bf16 O), dst = W (bf16)
typedef struct {
  const void* src;
  float* f32;
  void* dst;
  int R, C;
  int blk0;    // filled by the launcher: first 64 x 64 tile (= first norm partial) of this matrix
  float scale; // apply: sqrt(max(1, R / C))
  float wd;    // apply: this matrix's weight decay
} PdeMuonMat;

hipError_t pde_muon_gemm_sym(PdeMuonGemm* probs, int count, float alpha, float beta, hipStream_t st);
hipError_t pde_muon_gemm_rect(PdeMuonGemm* probs, int count, float alpha, float beta, hipStream_t st);

// Two launches per table: momentum update + per-tile partial sums of U^2, then the fold of each matrix's partials in
// index order and the scaled bf16 X0 write.  `partials` holds one float per 64 x 64 tile of all matrices.
hipError_t pde_muon_prologue(PdeMuonMat* mats, int count, float* partials, float mu, int nesterov, float grad_scale,
                             hipStream_t st);
// Wm <- Wm (1 - lr wd) - lr scale O, W <- bf16(Wm); the rate of step t = *step_dev (when given, else `step`) comes
// from lr_tab when there is one (pde_lr.h).
hipError_t pde_muon_apply(PdeMuonMat* mats, int count, float lr, int step, const float* step_dev, const float* lr_tab,
                          int lr_len, hipStream_t st);
// tiles of a matrix in the streaming kernels (= its norm partials)
int64_t pde_muon_tiles(int R, int C);

#ifdef __cplusplus
}
#endif
