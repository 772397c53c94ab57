// Dropout masks: ONE stateless, counter-based definition shared by every kernel that drops
// (transformer.hip, attention.hip), the dropout_mask debug kernel (rng.hip) and, bit for bit, the
// vectorised CPU implementation in ops/rng.py.
//
// Generator: Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11).
//
//   key            64-bit seed                                     (state words 0, 1)
//   counter 0, 1   64-bit group index inside the site
//   counter 2      draw number: one per training forward           (state word 2)
//   counter 3      site (low 16 bits) | stream (high 16 bits)      (stream = state word 3)
//
// The RNG state / snapshot is four 32-bit words {seed lo, seed hi, draw, stream} in device memory
// (ops/rng.py DeviceRNG); kernels read the snapshot, never a host value, so a captured step draws
// new masks on every replay.
//
// Elementwise sites: group g covers elements 4g .. 4g+3, one 32-bit word each; element i is KEPT iff
//   word[i & 3] >= thr,  thr = floor(p * 2^32).
// Attention sites: group ((b*H + h) * T/4 + q/4) * T/4 + k/4 covers the 4 x 4 block of queries
// 4(q/4).. x keys 4(k/4)..; the byte (k & 3) of word (q & 3) decides (query q, key k): KEPT iff
//   byte >= thr,  thr = floor(p * 256).
// One call therefore serves a lane that holds 4 consecutive keys of one query (forward, dQ: one
// word) and a lane that holds 4 consecutive queries of one key (dK/dV: one byte of each word).  The
// price is the 8-bit threshold: the probability realised is thr / 256, and that value -- not p --
// sets the 1 / keep scale (ops/rng.py effective_p).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PDE_RNG_HD __host__ __device__ __forceinline__
#else
#define PDE_RNG_HD inline
#endif

namespace pde_rng {

PDE_RNG_HD void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                              uint32_t (&out)[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c0;
  out[1] = c1;
  out[2] = c2;
  out[3] = c3;
}

// the four words of group `group` of `site` under the snapshot st = {seed lo, seed hi, draw, stream}
PDE_RNG_HD void group_words(const uint32_t (&st)[4], uint32_t site, uint64_t group, uint32_t (&out)[4]) {
  philox4x32_10((uint32_t)group, (uint32_t)(group >> 32), st[2], (site & 0xffffu) | (st[3] << 16), st[0], st[1], out);
}

PDE_RNG_HD uint64_t attn_group(int bh, int T, int q, int k) {
  const uint64_t t4 = (uint64_t)(T >> 2);
  return ((uint64_t)bh * t4 + (uint64_t)(q >> 2)) * t4 + (uint64_t)(k >> 2);
}

}  // namespace pde_rng
