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
constexpr int DC_CH = 128;      // keys per block
constexpr int DC_PART = 66;     // floats per partial: max, sum, 64 outputs

// grid (chunks of Tmax, H, B), block 256 (b is a grid index of its own, so the row's state words can be
// loaded before any other arithmetic).  Scores: thread pair (2j, 2j + 1) holds the two 32-dim halves of
// key c * 128 + j.  Outputs: thread (kg = tid >> 3, dg = tid & 7) holds dims 8 dg.. of keys kg + 32 i.  Every
// K / V row comes straight from global memory to VGPRs, all loads issued before the first use.  Row p (the
// new token; p = p_b, the position of batch row b) is taken from the c_attn row and written to the cache by
// the block whose chunk holds p.  Blocks of chunks past p return: the grid is sized by Tmax.
__global__ __launch_bounds__(256) void k_dec_attn(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ cache,
                                                  const int* __restrict__ state, float* __restrict__ part, int B, int H,
                                                  int Tmax, int nch, float scale) {
  __shared__ float ps[DC_CH];
  __shared__ float ored[32][64];
  __shared__ float wred[2][4];
  const int c = blockIdx.x, h = blockIdx.y, b = blockIdx.z, bh = b * H + h;
  const int p = state[PDE_DS_POS] + state[PDE_DS_OFF + b];
  if (p < 0 || p >= Tmax || c * DC_CH > p) return;      // uniform per block
  const int C = H * 64, tid = threadIdx.x, w = tid >> 6;
  const bf16_t* row = qkv + (size_t)b * 3 * C + h * 64;  // q; + C: k; + 2C: v
  bf16_t* Kc = cache + (size_t)bh * Tmax * 64;
  bf16_t* Vc = Kc + (size_t)B * H * Tmax * 64;

  const int j1 = c * DC_CH + (tid >> 1), half = tid & 1;
  uint4 kv[4], vv[4], qv[4];
  {
    const uint4* src = reinterpret_cast<const uint4*>(j1 == p ? row + C + half * 32 : Kc + (size_t)j1 * 64 + half * 32);
#pragma unroll
    for (int i = 0; i < 4; ++i) kv[i] = j1 <= p ? src[i] : make_uint4(0u, 0u, 0u, 0u);
    if (j1 == p) {
      uint4* dst = reinterpret_cast<uint4*>(Kc + (size_t)p * 64 + half * 32);
#pragma unroll
      for (int i = 0; i < 4; ++i) dst[i] = kv[i];
    }
  }
  const int dg = tid & 7, kg = tid >> 3;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int j = c * DC_CH + kg + 32 * i;
    if (j < p) vv[i] = *reinterpret_cast<const uint4*>(Vc + (size_t)j * 64 + dg * 8);
    else if (j == p) {
      vv[i] = *reinterpret_cast<const uint4*>(row + 2 * C + dg * 8);
      *reinterpret_cast<uint4*>(Vc + (size_t)p * 64 + dg * 8) = vv[i];
    } else vv[i] = make_uint4(0u, 0u, 0u, 0u);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) qv[i] = reinterpret_cast<const uint4*>(row + half * 32)[i];

  float dot = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float a[8], q[8];
    unpack8(kv[i], a);
    unpack8(qv[i], q);
#pragma unroll
    for (int e = 0; e < 8; ++e) dot += a[e] * q[e];
  }
  dot += __shfl_xor(dot, 1, 64);
  const float sc = j1 <= p ? dot * scale : -INFINITY;
  const float wm = wave_max(sc);
  if ((tid & 63) == 0) wred[0][w] = wm;
  __syncthreads();
  const float m = fmaxf(fmaxf(wred[0][0], wred[0][1]), fmaxf(wred[0][2], wred[0][3]));   // finite: key c*128 <= p
  const float pj = j1 <= p ? expf(sc - m) : 0.f;
  const float wsum = wave_sum(half == 0 ? pj : 0.f);
  if ((tid & 63) == 0) wred[1][w] = wsum;
  if (half == 0) ps[tid >> 1] = pj;
  __syncthreads();
  const float lsum = ((wred[1][0] + wred[1][1]) + wred[1][2]) + wred[1][3];

  float acc[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float pr = ps[kg + 32 * i];
    float f[8];
    unpack8(vv[i], f);
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] += pr * f[e];
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) ored[kg][dg * 8 + e] = acc[e];
  __syncthreads();
  if (tid < 64) {
    float o = 0.f;
    for (int k = 0; k < 32; ++k) o += ored[k][tid];
    float* dst = part + ((size_t)bh * nch + c) * DC_PART;
    dst[2 + tid] = o;
    if (tid == 0) {
      dst[0] = m;
      dst[1] = lsum;
    }
  }
}

// grid (H, B), block 64: the partials of chunks 0 .. p_b / 128 in chunk order
__global__ __launch_bounds__(64) void k_dec_attn_combine(const float* __restrict__ part, const int* __restrict__ state,
                                                         bf16_t* __restrict__ out, int H, int Tmax, int nch) {
  const int h = blockIdx.x, b = blockIdx.y, bh = b * H + h, d = threadIdx.x;
  const int p = state[PDE_DS_POS] + state[PDE_DS_OFF + b];
  if (p < 0 || p >= Tmax) return;
  const int nact = p / DC_CH + 1;
  const float* src = part + (size_t)bh * nch * DC_PART;
  float m = -INFINITY;
  for (int c = 0; c < nact; ++c) m = fmaxf(m, src[c * DC_PART]);
  float L = 0.f, O = 0.f;
  for (int c = 0; c < nact; ++c) {
    const float wgt = expf(src[c * DC_PART] - m);
    L += wgt * src[c * DC_PART + 1];
    O += wgt * src[c * DC_PART + 2 + d];
  }
  out[(size_t)b * H * 64 + h * 64 + d] = f2bf(O / L);
}

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
  const int nch = (Tmax + DC_CH - 1) / DC_CH;
  hipLaunchKernelGGL(k_dec_attn, dim3(nch, H, B), dim3(256), 0, st, (const bf16_t*)qkv, (bf16_t*)cache, state, part, B,
                     H, Tmax, nch, scale);
  PDE_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(k_dec_attn_combine, dim3(H, B), dim3(64), 0, st, (const float*)part, state, (bf16_t*)out, H, Tmax,
                     nch);
  return hipGetLastError();
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
