// Dropout RNG state kernel and the dropout_mask debug kernel (mask definition: pde_rng.h).
#include "pde_hip.h"
#include "pde_kernels.h"
#include "pde_rng.h"

namespace {

// snapshot = state; ++draw.  One thread: the state is 16 bytes, and the launch orders itself against
// the kernels that read the previous snapshot by being in the same stream (or captured graph).
__global__ void k_rng_next(uint32_t* __restrict__ state, uint32_t* __restrict__ snap) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    const uint32_t s0 = state[0], s1 = state[1], s2 = state[2], s3 = state[3];
    snap[0] = s0;
    snap[1] = s1;
    snap[2] = s2;
    snap[3] = s3;
    state[2] = s2 + 1u;
  }
}

// thread per group of an elementwise site: 4 consecutive elements
__global__ __launch_bounds__(256) void k_mask_elem(const uint32_t* __restrict__ rng, uint32_t site, uint32_t thr,
                                                   uint8_t* __restrict__ out, int64_t n) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (4 * g >= n) return;
  const uint32_t st[4] = {rng[0], rng[1], rng[2], rng[3]};
  uint32_t w[4];
  pde_rng::group_words(st, site, (uint64_t)g, w);
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (4 * g + e < n) out[4 * g + e] = w[e] >= thr;
}

// thread per group of an attention site: the 4 x 4 block of queries x keys; out is [BH, T, T]
__global__ __launch_bounds__(256) void k_mask_attn(const uint32_t* __restrict__ rng, uint32_t site, uint32_t thr,
                                                   uint8_t* __restrict__ out, int64_t ngroups, int T) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= ngroups) return;
  const uint32_t st[4] = {rng[0], rng[1], rng[2], rng[3]};
  uint32_t w[4];
  pde_rng::group_words(st, site, (uint64_t)g, w);
  const int64_t t4 = T >> 2;
  const int64_t kb = g % t4, qb = (g / t4) % t4, bh = g / (t4 * t4);
#pragma unroll
  for (int qi = 0; qi < 4; ++qi) {
    uchar4 m;
    m.x = ((w[qi] >> 0) & 0xffu) >= thr;
    m.y = ((w[qi] >> 8) & 0xffu) >= thr;
    m.z = ((w[qi] >> 16) & 0xffu) >= thr;
    m.w = ((w[qi] >> 24) & 0xffu) >= thr;
    *reinterpret_cast<uchar4*>(out + ((bh * T + 4 * qb + qi) * T + 4 * kb)) = m;
  }
}

}  // namespace

extern "C" {

hipError_t pde_rng_next(uint32_t* state, uint32_t* snapshot, hipStream_t st) {
  hipLaunchKernelGGL(k_rng_next, dim3(1), dim3(64), 0, st, state, snapshot);
  return hipGetLastError();
}

hipError_t pde_dropout_mask(const uint32_t* rng, uint32_t site, uint32_t thr, uint8_t* out, int64_t n, int attn_T,
                            hipStream_t st) {
  if (n <= 0) return hipSuccess;
  if (attn_T) {
    if (attn_T % 4 != 0 || n % ((int64_t)attn_T * attn_T) != 0) return hipErrorInvalidValue;
    const int64_t ng = n / 16;
    hipLaunchKernelGGL(k_mask_attn, dim3((unsigned)((ng + 255) / 256)), dim3(256), 0, st, rng, site, thr, out, ng,
                       attn_T);
  } else {
    const int64_t ng = (n + 3) / 4;
    hipLaunchKernelGGL(k_mask_elem, dim3((unsigned)((ng + 255) / 256)), dim3(256), 0, st, rng, site, thr, out, n);
  }
  return hipGetLastError();
}

}  // extern "C"
