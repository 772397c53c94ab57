// GPT-2 generation kernels: skinny linear (M <= 16), decode attention with KV-cache append, cache fill,
// decode embedding and the device-side sampler.  bf16 in / out, fp32 math, wave64.
//
// Whatever changes per generated token (position, output slot, RNG draw, finished flags) is read from the
// device state buffer of pde_decode.h, so a captured decode step replays correctly for every token.
//
// Design choices
//   skinny linear   v_mfma_f32_16x16x32_bf16 with x padded to 16 rows, not a VALU dot.  A VALU dot costs
//                   16 FMAs per weight element at M = 16 (4 cycles each in wave64), about 3x the cycles the
//                   CU's share of HBM bandwidth allows; one MFMA covers 16 weight rows x 32 k x 16 x-rows,
//                   so the cost no longer depends on M.  The A fragment of a lane is 8 consecutive k of one
//                   weight row: exactly one 16-byte global load straight to VGPRs, no LDS staging.  The x
//                   fragment comes from L2 the same way and is reused for TPB row tiles.  The 4 waves of a
//                   block split the block's K range and combine through LDS in wave order; when N / 16 row
//                   tiles cannot fill 256 CUs, K is also split over `S` blocks that write fp32 slabs, summed
//                   in slab order by k_skinny_combine.  Nothing depends on arrival order.
//   attention       (b, h) x fixed 128-key chunks; every chunk writes an fp32 partial {max, sum, 64 outputs}
//                   and a second kernel combines the partials in chunk order.  Probabilities stay fp32.
//   combines        both split reductions (skinny K slabs, attention chunks) are a second launch, not a
//                   last-arriving block: stream order makes the partials visible with no fence, counter or
//                   per-call reset, and the sum order is the slab / chunk index by construction.
//   sampler         one block per row; radix select (2 x 8 bits) for the top-k threshold, Gumbel-max with
//                   Philox words addressed as pde_rng::group_words; a one-thread tail kernel advances the
//                   state after every row has read it.  Top-p is a second radix select over the same key,
//                   weighted by exp(z - z_max) in 64-bit fixed point: integer LDS atomics sum in any order
//                   to the same bits, which float atomics would not.  It is a template instantiation of
//                   its own, so the sampler without top-p is the code it was.
//   processors      penalties, logit bias and min_new_tokens live in the sampler, the only place where a decode
//                   step's logits and the rows' histories meet: two more instantiations (PROC) write the
//                   processed row to a bf16 workspace first and then run the same passes on it; the history is a
//                   [B, Vp] counts buffer that the kernel reads and advances, so a captured step follows it.
//   ragged batches  row b sits at position p_b = state position + state offset of row b; every block of
//                   the attention, the embedding and the sampler derives what it does from its own p_b.
#include "pde_hip.h"
#include "pde_bf16.h"
#include "pde_act.h"
#include "pde_decode.h"
#include "pde_rng.h"

#include <math.h>

namespace {

// ------------------------------------------------------------------------------------- skinny linear
// grid (row-tile groups, S); block 256 = 4 waves.  Block (t, s) covers TPB tiles of 16 weight rows and
// the s-th of S slices of K; its wave w takes the w-th quarter of that slice in k32-steps.
// MFMA D = A B with A = W tile (i = weight row), B = x^T (j = x row): lane l loads A[i = l & 15][8 k of
// group l >> 4] and B[the same 8 k][j = l & 15], and holds D[n = 4 (l >> 4) + r][m = l & 15], r = 0..3.
template <int TPB>
__global__ __launch_bounds__(256) void k_skinny(const bf16_t* __restrict__ x, const bf16_t* __restrict__ W,
                                                const bf16_t* __restrict__ bias, bf16_t* __restrict__ y,
                                                float* __restrict__ part, int M, int N, int K, int S, int gelu) {
  __shared__ f32x4 red[4][TPB][64];
  const int l = threadIdx.x & 63, w = threadIdx.x >> 6, r = l & 15, g = l >> 4;
  const int tile0 = blockIdx.x * TPB, s = blockIdx.y;
  const int nsteps = K >> 5, slices = S * 4, sl = s * 4 + w;
  const int k_beg = (int)((int64_t)nsteps * sl / slices), k_end = (int)((int64_t)nsteps * (sl + 1) / slices);
  const bool xrow = r < M;
  const uint4* xp = reinterpret_cast<const uint4*>(x + (size_t)(xrow ? r : 0) * K) + g;
  const uint4* wp[TPB];
#pragma unroll
  for (int t = 0; t < TPB; ++t) {
    int n = (tile0 + t) * 16 + r;
    n = n < N ? n : N - 1;          // rows past N (last tile): any valid row, the result is dropped
    wp[t] = reinterpret_cast<const uint4*>(W + (size_t)n * K) + g;
  }
  f32x4 acc[TPB];
#pragma unroll
  for (int t = 0; t < TPB; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
  for (int ks = k_beg; ks < k_end; ++ks) {
    uint4 wv[TPB];
#pragma unroll
    for (int t = 0; t < TPB; ++t) wv[t] = wp[t][ks * 4];
    const uint4 xv = xrow ? xp[ks * 4] : make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
    for (int t = 0; t < TPB; ++t)
      acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, wv[t]),
                                                       __builtin_bit_cast(bf16x8, xv), acc[t], 0, 0, 0);
  }
#pragma unroll
  for (int t = 0; t < TPB; ++t) red[w][t][l] = acc[t];
  __syncthreads();
  if (w < TPB) {   // wave w finishes tile w: the four K quarters in wave order
    const f32x4 v = ((red[0][w][l] + red[1][w][l]) + red[2][w][l]) + red[3][w][l];
    const int n = (tile0 + w) * 16 + g * 4, m = r;
    if (m < M && n < N) {
      if (part) {
        *reinterpret_cast<f32x4*>(part + ((size_t)s * M + m) * N + n) = v;
      } else {
        float f[4] = {v[0], v[1], v[2], v[3]};
        if (bias) {
          float bf[4];
          unpack4(*reinterpret_cast<const uint2*>(bias + n), bf);
#pragma unroll
          for (int e = 0; e < 4; ++e) f[e] += bf[e];
        }
        if (gelu) {
#pragma unroll
          for (int e = 0; e < 4; ++e) f[e] = gelu_t(f[e], nullptr);
        }
        *reinterpret_cast<uint2*>(y + (size_t)m * N + n) = pack4(f);
      }
    }
  }
}

// y = bf16(sum over the S slabs in slab order (+ bias) (-> GELU)); thread per 4 outputs
__global__ __launch_bounds__(256) void k_skinny_combine(const float* __restrict__ part, const bf16_t* __restrict__ bias,
                                                        bf16_t* __restrict__ y, int MN, int N, int S, int gelu) {
  const int i = (blockIdx.x * 256 + threadIdx.x) * 4;
  if (i >= MN) return;
  f32x4 v = *reinterpret_cast<const f32x4*>(part + i);
  for (int s = 1; s < S; ++s) v += *reinterpret_cast<const f32x4*>(part + (size_t)s * MN + i);
  float f[4] = {v[0], v[1], v[2], v[3]};
  if (bias) {
    float bf[4];
    unpack4(*reinterpret_cast<const uint2*>(bias + (i % N)), bf);
#pragma unroll
    for (int e = 0; e < 4; ++e) f[e] += bf[e];
  }
  if (gelu) {
#pragma unroll
    for (int e = 0; e < 4; ++e) f[e] = gelu_t(f[e], nullptr);
  }
  *reinterpret_cast<uint2*>(y + i) = pack4(f);
}

// ------------------------------------------------------------------------------------- decode attention
// device code shared with decode_beam.hip, which instantiates the kernel with a beam search's ancestor table
#include "decode_attn.h"

// ------------------------------------------------------------------------------------- cache fill / embedding
// thread per 16 bytes: (kv, b, h, t < T0, 8-element chunk)
__global__ __launch_bounds__(256) void k_cache_fill(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ cache, int B,
                                                    int H, int Tpad, int T0, int Tmax) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t total = (int64_t)2 * B * H * T0 * 8;
  if (i >= total) return;
  const int ch = (int)(i & 7);
  int64_t r = i >> 3;
  const int t = (int)(r % T0);
  r /= T0;
  const int h = (int)(r % H);
  r /= H;
  const int b = (int)(r % B), kv = (int)(r / B);
  const int C = H * 64;
  const uint4 v = *reinterpret_cast<const uint4*>(qkv + ((size_t)b * Tpad + t) * 3 * C + (1 + kv) * C + h * 64 + ch * 8);
  *reinterpret_cast<uint4*>(cache + ((((size_t)kv * B + b) * H + h) * Tmax + t) * 64 + ch * 8) = v;
}

// grid (blocks of a row, B): thread per 8 elements of out[b, :]
__global__ __launch_bounds__(256) void k_dec_embed(const int64_t* __restrict__ tok, const bf16_t* __restrict__ wte,
                                                   const bf16_t* __restrict__ wpe, const int* __restrict__ state,
                                                   bf16_t* __restrict__ out, int B, int C, int Vp, int n_pos) {
  const int i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y, c = i * 8;
  const int p = state[PDE_DS_POS] + state[PDE_DS_OFF + b];
  if (b >= B || c >= C || p < 0 || p >= n_pos) return;
  int64_t id = tok[b];
  id = id < 0 ? 0 : (id >= Vp ? Vp - 1 : id);
  float a[8], e[8];
  unpack8(*reinterpret_cast<const uint4*>(wte + (size_t)id * C + c), a);
  unpack8(*reinterpret_cast<const uint4*>(wpe + (size_t)p * C + c), e);
#pragma unroll
  for (int k = 0; k < 8; ++k) a[k] += e[k];
  *reinterpret_cast<uint4*>(out + (size_t)b * C + c) = pack8(a);
}

// ------------------------------------------------------------------------------------- sampler
// device code shared with decode_proc.hip, which instantiates the sampler with the logit processors
#include "decode_sample.h"

}  // namespace

extern "C" {

int pde_skinny_splits(int N, int K) {
  if (N <= 0 || K <= 0) return 1;
  const int ntiles = (N + 15) / 16, tpb = ntiles >= 1024 ? 4 : 1, nblk = (ntiles + tpb - 1) / tpb;
  int S = (256 + nblk - 1) / nblk;
  const int cap = (K >> 5) / 4;        // every wave of every slice keeps at least one k32-step
  if (S > cap) S = cap;
  if (S > 8) S = 8;
  return S < 1 ? 1 : S;
}

hipError_t pde_skinny_linear(const void* x, const void* W, const void* bias, void* y, float* part, int M, int N, int K,
                             int gelu, hipStream_t st) {
  if (M < 1 || M > 16 || N < 8 || N % 8 != 0 || K < 64 || K % 64 != 0) return hipErrorInvalidValue;
  const int S = pde_skinny_splits(N, K);
  if (S > 1 && part == nullptr) return hipErrorInvalidValue;
  const int ntiles = (N + 15) / 16;
  float* pp = S > 1 ? part : nullptr;
  const bf16_t* bp = S > 1 ? nullptr : (const bf16_t*)bias;
  if (ntiles >= 1024)
    hipLaunchKernelGGL(k_skinny<4>, dim3((ntiles + 3) / 4, S), dim3(256), 0, st, (const bf16_t*)x, (const bf16_t*)W, bp,
                       (bf16_t*)y, pp, M, N, K, S, gelu);
  else
    hipLaunchKernelGGL(k_skinny<1>, dim3(ntiles, S), dim3(256), 0, st, (const bf16_t*)x, (const bf16_t*)W, bp,
                       (bf16_t*)y, pp, M, N, K, S, gelu);
  PDE_HIP_CHECK(hipGetLastError());
  if (S > 1) {
    const int MN = M * N;
    hipLaunchKernelGGL(k_skinny_combine, dim3((MN / 4 + 255) / 256), dim3(256), 0, st, (const float*)part,
                       (const bf16_t*)bias, (bf16_t*)y, MN, N, S, gelu);
  }
  return hipGetLastError();
}

int pde_decode_attn_chunk(void) { return DC_CH; }

hipError_t pde_decode_attention(const void* qkv, void* cache, const int* state, float* part, void* out, int B, int H,
                                int Tmax, float scale, hipStream_t st) {
  if (B < 1 || B > PDE_DS_MAX_ROWS || H < 1 || Tmax < 1) return hipErrorInvalidValue;
  return dec_attn_launch(qkv, cache, state, part, out, B, H, Tmax, scale, st);
}

hipError_t pde_cache_fill(const void* qkv, void* cache, int B, int H, int Tpad, int T0, int Tmax, hipStream_t st) {
  if (B < 1 || H < 1 || T0 < 1 || T0 > Tpad || T0 > Tmax) return hipErrorInvalidValue;
  const int64_t total = (int64_t)2 * B * H * T0 * 8;
  hipLaunchKernelGGL(k_cache_fill, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, (const bf16_t*)qkv,
                     (bf16_t*)cache, B, H, Tpad, T0, Tmax);
  return hipGetLastError();
}

hipError_t pde_decode_embed(const int64_t* tok, const void* wte, const void* wpe, const int* state, void* out, int B,
                            int C, int Vp, int n_pos, hipStream_t st) {
  if (B < 1 || B > PDE_DS_MAX_ROWS || C < 8 || C % 8 != 0 || Vp < 1 || n_pos < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_dec_embed, dim3((C / 8 + 255) / 256, B), dim3(256), 0, st, tok, (const bf16_t*)wte,
                     (const bf16_t*)wpe, state, (bf16_t*)out, B, C, Vp, n_pos);
  return hipGetLastError();
}

hipError_t pde_sample(PdeSample a, hipStream_t st) {
  return sample_ok(a) ? sample_launch(a, st) : hipErrorInvalidValue;
}

}  // extern "C"
