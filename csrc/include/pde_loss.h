// extern "C" launcher of the masked-loss target kernel (csrc/kernels/transformer.hip k_loss_targets) and
// the layout of the device-side info block it writes.
//
// Which targets count towards the loss, and what the loss is divided by, changes with every batch and is
// known only on the device.  Both live in device memory, never in a launch argument, so one captured
// training step replays correctly for every batch:
//
//   word 0   int32  count: targets that are selected, not ignore_index and inside [0, V)
//   word 1   fp32   inv: what the cross-entropy kernels and the loss sum multiply by --
//                   1 / denom[0] (0 when denom[0] <= 0) with a caller's denominator, else
//                   1 / max(count, 1) for the mean and 1 for the sum
//   word 2   int32  out_of_range: targets that are selected and not ignore_index but outside [0, V)
//                   (ignored, never an error: raising would need a host read)
//   word 3   reserved (0)
//
// The block is written whole, by one 16-byte vector store of the kernel's first thread.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#define PDE_LI_COUNT 0
#define PDE_LI_INV 1
#define PDE_LI_OOR 2
#define PDE_LI_WORDS 4

#define PDE_LOSS_MEAN 0
#define PDE_LOSS_SUM 1

#ifdef __cplusplus
extern "C" {
#endif

typedef struct PdeLossTargets {
  const int64_t* targets;     // [N]
  const uint8_t* loss_mask;   // [N] or null: 0 = not selected
  const int* doc_end;         // [N] or null (ops.doc_bounds): position t < T - 1 with doc_end == t is not selected
  const float* denom;         // [1] or null
  int64_t* eff;               // [N]: the target where it counts, else -1
  int* info;                  // PDE_LI_WORDS, 16-byte aligned
  int64_t ignore_index;
  int has_ignore;             // 0: no ignore_index
  int N, T, V;
  int mode;                   // PDE_LOSS_MEAN / PDE_LOSS_SUM (denom must be null with SUM)
} PdeLossTargets;
hipError_t pde_loss_targets(PdeLossTargets a, hipStream_t st);

#ifdef __cplusplus
}
#endif
