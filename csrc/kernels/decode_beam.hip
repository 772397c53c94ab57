// Beam search over the shared KV cache of the GPT-2 decode step: the decode attention that reads its keys through
// an ancestor table, the two-stage beam selection that takes the sampler's place, the finalisation and the prefill's
// cache fill.  PdeBeamTable / PdeBeam / PdeBeamFinal are documented in pde_decode.h, the definition of a beam step in
// ops/decode.py.  A unit of its own, as the sampler's variants are: the plain attention and the plain sampler keep the
// instruction streams they had.
//
// Design choices
//   cache        never moved.  A group's rows are permuted every step, so the table is double-buffered and the half
//                to read follows the state's step parity: a captured launch has fixed pointers.  The copy of a step
//                is at most 16 rows x Tmax bytes; a physical reorder would be the whole cache.
//   selection    inside a row, score order is logit order, so a row contributes its K best logits and no more: the
//                sampler's exact radix select over the bf16 key finds the K-th value, one more pass collects what
//                lies above it, and the ties at it are taken lowest index first, one atomic minimum per tie.  The
//                group's <= K * K candidates are then ranked by counting in one small block.
//   arithmetic   fp32 row maximum and sum of exponentials in a fixed order (thread, wave, waves in order), so two
//                identical rows give identical bits and a cross-beam tie resolves by index on the device too.
#include "pde_hip.h"
#include "pde_bf16.h"
#include "pde_decode.h"
#include "pde_rng.h"

#include <math.h>

namespace {

#include "decode_attn.h"
#include "decode_sample.h"     // key16, radix_pick, SM_NT

// the 8 bf16 of group g8 of a row as raw bits
__device__ __forceinline__ void row_bits8(const bf16_t* row, int g8, uint32_t* u) {
  const uint4 v = reinterpret_cast<const uint4*>(row)[g8];
  u[0] = v.x & 0xffffu; u[1] = v.x >> 16; u[2] = v.y & 0xffffu; u[3] = v.y >> 16;
  u[4] = v.z & 0xffffu; u[5] = v.z >> 16; u[6] = v.w & 0xffffu; u[7] = v.w >> 16;
}

// ------------------------------------------------------------------------------------- stage 1
// grid R, block SM_NT.  A row that does not exist yet (step 0, k > 0) or is finished writes no candidates: stage 2
// knows.  16-byte loads throughout (Vp % 8 == 0).
__global__ __launch_bounds__(SM_NT) void k_beam_rows(PdeBeam a) {
  __shared__ uint32_t hist[4][256];
  __shared__ uint32_t sel[2];
  __shared__ float fred[SM_NT / 64];
  __shared__ uint64_t list[PDE_DS_MAX_ROWS];
  __shared__ uint32_t ngt, tmin[2];
  const int r = blockIdx.x, tid = threadIdx.x, w = tid >> 6;
  const int K = a.K, V = a.V, ng8 = a.Vp >> 3;
  const int step = a.state[PDE_DS_STEP];
  const bool fin = a.eos >= 0 && a.state[PDE_DS_FIN + r] != 0;
  const bool exists = step > 0 || r % K == 0;
  const bf16_t* row = reinterpret_cast<const bf16_t*>(a.logits) + (size_t)r * a.Vp;
  if (exists && a.logits_out && step >= 0 && step < a.max_new) {
    bf16_t* dst = reinterpret_cast<bf16_t*>(a.logits_out) + ((size_t)r * a.max_new + step) * V;
    for (int v = tid; v < V; v += SM_NT) dst[v] = row[v];
  }
  if (!exists || fin) return;                  // uniform per block

  // lse = max + log(sum exp(x - max)) over the first V columns
  float mx = -INFINITY;
  for (int g8 = tid; g8 < ng8; g8 += SM_NT) {
    uint32_t u[8];
    row_bits8(row, g8, u);
#pragma unroll
    for (int e = 0; e < 8; ++e)
      if (8 * g8 + e < V) mx = fmaxf(mx, bf2f(u[e]));
  }
  mx = wave_max(mx);
  if ((tid & 63) == 0) fred[w] = mx;
  __syncthreads();
  for (int i = 0; i < SM_NT / 64; ++i) mx = fmaxf(mx, fred[i]);
  __syncthreads();
  float se = 0.f;
  for (int g8 = tid; g8 < ng8; g8 += SM_NT) {
    uint32_t u[8];
    row_bits8(row, g8, u);
#pragma unroll
    for (int e = 0; e < 8; ++e)
      if (8 * g8 + e < V) se += expf(bf2f(u[e]) - mx);
  }
  se = wave_sum(se);
  if ((tid & 63) == 0) fred[w] = se;
  __syncthreads();
  float tot = 0.f;
  for (int i = 0; i < SM_NT / 64; ++i) tot += fred[i];
  const float lse = mx + logf(tot);

  // the key of the K-th largest logit and m, how many of the elements equal to it belong to the K (the sampler's
  // two-pass radix select; K <= V, so it always finds one)
  uint32_t hi = 0, k = (uint32_t)K, thr = 0, m = 0;
  for (int pass = 0; pass < 2; ++pass) {
    for (int i = tid; i < 1024; i += SM_NT) (&hist[0][0])[i] = 0u;
    __syncthreads();
    for (int g8 = tid; g8 < ng8; g8 += SM_NT) {
      uint32_t u[8];
      row_bits8(row, g8, u);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        if (8 * g8 + e >= V) continue;
        const uint32_t key = key16(u[e]);
        if (pass == 0) atomicAdd(&hist[w & 3][key >> 8], 1u);
        else if ((key >> 8) == hi) atomicAdd(&hist[w & 3][key & 0xffu], 1u);
      }
    }
    __syncthreads();
    if (w == 0) radix_pick(hist, k, sel);
    __syncthreads();
    if (pass == 0) {
      hi = sel[0];
      k = sel[1];
    } else {
      thr = (hi << 8) | sel[0];
      m = sel[1];
    }
    __syncthreads();
  }
  m = m < 1u ? 1u : (m > (uint32_t)K ? (uint32_t)K : m);

  // list[0 .. K-m): the elements above the threshold, in any order; list[K-m .. K): the m lowest indices at it,
  // one pass each (the first pass does both).  Entry = key << 32 | ~index: descending = value down, index up
  if (tid == 0) ngt = 0u;
  int prev = -1;
  for (uint32_t round = 0; round < m; ++round) {
    if (tid == 0) tmin[round & 1] = 0xffffffffu;
    __syncthreads();
    uint32_t lmin = 0xffffffffu;
    for (int g8 = tid; g8 < ng8; g8 += SM_NT) {
      uint32_t u[8];
      row_bits8(row, g8, u);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int v = 8 * g8 + e;
        if (v >= V) continue;
        const uint32_t key = key16(u[e]);
        if (round == 0 && key > thr) {
          const uint32_t slot = atomicAdd(&ngt, 1u);
          if (slot < (uint32_t)K - m) list[slot] = ((uint64_t)key << 32) | (uint32_t)~(uint32_t)v;
        }
        if (key == thr && v > prev && (uint32_t)v < lmin) lmin = (uint32_t)v;
      }
    }
    if (lmin != 0xffffffffu) atomicMin(&tmin[round & 1], lmin);
    __syncthreads();
    uint32_t t = tmin[round & 1];
    t = t < (uint32_t)V ? t : 0u;              // the row holds m elements at the threshold: never taken
    if (tid == 0) list[(uint32_t)K - m + round] = ((uint64_t)thr << 32) | (uint32_t)~t;
    prev = (int)t;
  }
  __syncthreads();
  if (tid < K) {                               // rank by counting: the entries differ in their index
    const uint64_t e = list[tid];
    int rank = 0;
    for (int j = 0; j < K; ++j) rank += list[j] > e ? 1 : 0;
    const uint32_t key = (uint32_t)(e >> 32);
    const uint32_t bits = (key & 0x8000u) ? (key & 0x7fffu) : (~key & 0xffffu);     // key16 inverted
    a.cand_score[(size_t)r * K + rank] = a.score[r] + (bf2f(bits) - lse);
    a.cand_tok[(size_t)r * K + rank] = (int)~(uint32_t)e;
  }
}

// ------------------------------------------------------------------------------------- stage 2
// grid B, block 256: thread c < K * K is candidate i = c % K of parent k = c / K.  Everything the group reads of its
// rows' S, len and flags is in registers before the barrier that precedes the first store to them.
constexpr int BM_NT = 256;
__global__ __launch_bounds__(BM_NT) void k_beam_merge(PdeBeam a) {
  __shared__ float cs[BM_NT];
  __shared__ int cf[BM_NT];
  __shared__ int par[PDE_DS_MAX_ROWS];
  const int b = blockIdx.x, tid = threadIdx.x, K = a.K, R = a.B * K, g0 = b * K;
  const int step = a.state[PDE_DS_STEP];
  const int p = a.state[PDE_DS_POS] + a.state[PDE_DS_OFF + g0];
  const int k = tid / K, i = tid - k * K, r = g0 + (k < K ? k : 0);
  const bool fin = a.eos >= 0 && a.state[PDE_DS_FIN + r] != 0;
  const bool valid = k < K && (step > 0 || k == 0) && (!fin || i == 0);
  float sc = -INFINITY;
  int tok = 0, ln = 0;
  if (valid) {
    sc = fin ? a.score[r] : a.cand_score[(size_t)r * K + i];
    tok = fin ? a.eos : a.cand_tok[(size_t)r * K + i];
    ln = a.len[r];
  }
  const int flat = valid ? k * a.V + tok : 0x7fffffff;
  cs[tid] = sc;
  cf[tid] = flat;
  if (tid < PDE_DS_MAX_ROWS) par[tid] = 0;     // a group always has K candidates; a bad state must not index past it
  __syncthreads();
  int rank = 0;
  const int n = K * K;
  for (int j = 0; j < n; ++j) {
    const int fj = cf[j];
    const float sj = cs[j];
    rank += (fj != 0x7fffffff && (sj > sc || (sj == sc && fj < flat))) ? 1 : 0;
  }
  if (valid && rank < K) {                     // new beam j = rank of the group
    const int d = g0 + rank;
    const bool nf = fin || tok == a.eos;
    par[rank] = k;
    a.next[d] = tok;
    a.score[d] = sc;
    a.len[d] = ln + (fin ? 0 : 1);
    if (a.eos >= 0) a.state[PDE_DS_FIN + d] = nf ? 1 : 0;
    if (step >= 0 && step < a.max_new) {
      a.tok_trace[(size_t)step * R + d] = tok;
      a.parent_trace[(size_t)step * R + d] = k;
      a.score_trace[(size_t)step * R + d] = sc;
    }
  }
  __syncthreads();
  // the other half of the table: the parent's entries below p, and at p the parent's own row.  4 entries per
  // thread and round; the last word's entries past p are the parent's and are never read
  if (p < 0 || p >= a.Tmax) return;
  const unsigned char* rd = a.anc + (size_t)(step & 1) * PDE_DS_MAX_ROWS * a.stride;
  unsigned char* wr = a.anc + (size_t)((step & 1) ^ 1) * PDE_DS_MAX_ROWS * a.stride;
  const int nw = (p >> 2) + 1;
  for (int j = 0; j < K; ++j) {
    const int src = g0 + par[j];
    const uint32_t* s32 = reinterpret_cast<const uint32_t*>(rd + (size_t)src * a.stride);
    uint32_t* d32 = reinterpret_cast<uint32_t*>(wr + (size_t)(g0 + j) * a.stride);
    for (int wd = tid; wd < nw; wd += BM_NT) {
      uint32_t v = s32[wd];
      if (wd == nw - 1) {
        const int sh = 8 * (p & 3);
        v = (v & ~(0xffu << sh)) | ((uint32_t)src << sh);
      }
      d32[wd] = v;
    }
  }
}

// tail of the beam step: every block has read the state.  The draw number stays: beam search draws nothing
__global__ void k_beam_advance(int* __restrict__ state) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    state[PDE_DS_POS] += 1;
    state[PDE_DS_STEP] += 1;
  }
}

// ------------------------------------------------------------------------------------- finalisation
// grid B, block 64: thread j < K ranks row b * K + j and walks its hypothesis back through the parents
__global__ __launch_bounds__(64) void k_beam_finalize(PdeBeamFinal a) {
  __shared__ double fs[PDE_DS_MAX_ROWS];
  const int b = blockIdx.x, j = threadIdx.x, K = a.K, R = a.B * K, g0 = b * K;
  double s = 0.0;
  if (j < K) {
    s = (double)a.score[g0 + j] / pow((double)a.len[g0 + j], a.length_penalty);
    fs[j] = s;
  }
  __syncthreads();
  if (j >= K) return;
  int rank = 0;
  for (int i = 0; i < K; ++i) rank += (fs[i] > s || (fs[i] == s && i < j)) ? 1 : 0;
  a.scores[g0 + rank] = (float)s;
  const int base = a.T0 + a.state[PDE_DS_OFF + g0];
  if (base < 0 || base + a.n_steps > a.out_stride) return;
  int64_t* dst = a.out + (size_t)(g0 + rank) * a.out_stride + base;
  int row = j;
  for (int t = a.n_steps - 1; t >= 0; --t) {
    dst[t] = a.tok_trace[(size_t)t * R + g0 + row];
    const int pr = a.parent_trace[(size_t)t * R + g0 + row];
    row = pr >= 0 && pr < K ? pr : 0;
  }
}

// thread per 16 bytes: (kv, b, h, t < T0, 8-element chunk) -> cache row b * K
__global__ __launch_bounds__(256) void k_cache_fill_beam(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ cache,
                                                         int B, int K, int H, int Tpad, int T0, int Tmax) {
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
  *reinterpret_cast<uint4*>(cache + ((((size_t)kv * B * K + (size_t)b * K) * H + h) * Tmax + t) * 64 + ch * 8) = v;
}

bool beam_shape_ok(int B, int K) { return B >= 1 && K >= 1 && B * K <= PDE_DS_MAX_ROWS; }

}  // namespace

extern "C" {

hipError_t pde_decode_attention_beam(const void* qkv, void* cache, const int* state, float* part, void* out, int B,
                                     int H, int Tmax, float scale, PdeBeamTable t, hipStream_t st) {
  if (B < 1 || B > PDE_DS_MAX_ROWS || H < 1 || Tmax < 1 || !t.anc || t.stride < Tmax) return hipErrorInvalidValue;
  return dec_attn_launch(qkv, cache, state, part, out, B, H, Tmax, scale, st, t);
}

hipError_t pde_beam_step(PdeBeam a, hipStream_t st) {
  if (!beam_shape_ok(a.B, a.K) || a.V < a.K || a.V > a.Vp || a.Vp % 8 != 0 || a.eos >= a.V || a.Tmax < 1 ||
      a.stride < a.Tmax || a.stride % 4 != 0 || a.max_new < 0 || (int64_t)a.K * a.Vp > 0x7ffffff0)
    return hipErrorInvalidValue;
  if (!a.logits || !a.state || !a.next || !a.score || !a.len || !a.cand_score || !a.cand_tok || !a.anc ||
      (a.max_new > 0 && (!a.tok_trace || !a.parent_trace || !a.score_trace)))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_beam_rows, dim3(a.B * a.K), dim3(SM_NT), 0, st, a);
  PDE_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(k_beam_merge, dim3(a.B), dim3(BM_NT), 0, st, a);
  PDE_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(k_beam_advance, dim3(1), dim3(64), 0, st, a.state);
  return hipGetLastError();
}

hipError_t pde_beam_finalize(PdeBeamFinal a, hipStream_t st) {
  if (!beam_shape_ok(a.B, a.K) || a.T0 < 0 || a.n_steps < 1 || a.out_stride < a.T0 + a.n_steps ||
      !(a.length_penalty == a.length_penalty))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_beam_finalize, dim3(a.B), dim3(64), 0, st, a);
  return hipGetLastError();
}

hipError_t pde_cache_fill_beam(const void* qkv, void* cache, int B, int K, int H, int Tpad, int T0, int Tmax,
                               hipStream_t st) {
  if (!beam_shape_ok(B, K) || H < 1 || T0 < 1 || T0 > Tpad || T0 > Tmax) return hipErrorInvalidValue;
  const int64_t total = (int64_t)2 * B * H * T0 * 8;
  hipLaunchKernelGGL(k_cache_fill_beam, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, (const bf16_t*)qkv,
                     (bf16_t*)cache, B, K, H, Tpad, T0, Tmax);
  return hipGetLastError();
}

}  // extern "C"
