// Prompt-lookup speculative decoding on the GPT-2 decode step: the decode attention over sibling rows that share one
// cache row per prompt, and the verify launch -- row argmax, acceptance, emission, next drafts -- that takes the
// sampler's place.  PdeSpecRows / PdeSpec are documented in pde_decode.h, the definition of a step in ops/decode.py.
// A unit of its own, as the beam search is: the plain attention and the plain sampler keep the instruction streams
// they had.
//
// Design choices
//   cache        one row per prompt, not per physical row.  A draft row needs the keys of the rows before it in its
//                group, and those are in the c_attn output of the very launch it runs in: it loads them from there
//                (L2-resident, written by the launch before) and the cache only ever holds one copy of a position.
//                Every row appends its own position; what a rejected draft appended is overwritten by the next step's
//                rows before anything reads it, because that step's positions start right after the accepted ones.
//   exactness    the loads aside, the attention is the plain kernel's code on the plain kernel's chunk grid, the
//                skinny GEMMs give every row its own MFMA column, and the argmax is the sampler's rule (lowest index
//                of the maximum over the first V columns), so an accepted token has the bits of a plain step.
//   verify       stage 1, a block per logits row: 16-byte loads, the per-thread best in ascending index order, then
//                lanes, then waves in wave order -- (value, index) pairs under one total order, so the result does
//                not depend on the reduction tree.  Stage 2, a block per prompt: every thread derives the accepted
//                count from the <= 16 argmax words (no broadcast, no barrier), the emitted tokens go to `out`, and
//                the lookup runs over `out` itself, one history position per thread, suffix length by suffix length,
//                with a block maximum for the latest match.  A one-thread tail folds the finished flags into `done`.
//   replay       nothing is armed or cleared between launches: a finished group's block returns before it reads or
//                writes anything else, so a replay after the end is a no-op.
#include "pde_hip.h"
#include "pde_bf16.h"
#include "pde_decode.h"

#include <math.h>

namespace {

#include "decode_attn.h"

constexpr int SP_NT = 1024;
constexpr int SP_NW = SP_NT / 64;

// (v, i) beats (bv, bi): the larger value, the lower index among equal ones
__device__ __forceinline__ bool arg_beats(float v, int i, float bv, int bi) { return v > bv || (v == bv && i < bi); }

// ------------------------------------------------------------------------------------- stage 1
// grid B * q_in, block SP_NT: arg[r] = the lowest index attaining the maximum of logits[r, :V]
__global__ __launch_bounds__(SP_NT) void k_spec_argmax(PdeSpec a) {
  __shared__ float wv[SP_NW];
  __shared__ int wi[SP_NW];
  const int r = blockIdx.x, tid = threadIdx.x;
  if (a.state[PDE_DS_FIN + r / a.q_in] != 0) return;     // uniform per block
  const uint4* row = reinterpret_cast<const uint4*>(reinterpret_cast<const bf16_t*>(a.logits) + (size_t)r * a.Vp);
  const int ng8 = a.Vp >> 3, V = a.V;
  float bv = -INFINITY;
  int bi = 0x7fffffff;                         // no element yet: any real one at -inf still beats it
  for (int g8 = tid; g8 < ng8; g8 += SP_NT) {
    float f[8];
    unpack8(row[g8], f);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int v = 8 * g8 + e;
      if (v < V && arg_beats(f[e], v, bv, bi)) {
        bv = f[e];
        bi = v;
      }
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const float ov = __shfl_xor(bv, off, 64);
    const int oi = __shfl_xor(bi, off, 64);
    if (arg_beats(ov, oi, bv, bi)) {
      bv = ov;
      bi = oi;
    }
  }
  if ((tid & 63) == 0) {
    wv[tid >> 6] = bv;
    wi[tid >> 6] = bi;
  }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < SP_NW; ++w)
      if (arg_beats(wv[w], wi[w], bv, bi)) {
        bv = wv[w];
        bi = wi[w];
      }
    a.arg[r] = bi < V ? bi : 0;
  }
}

// the block's maximum of v; `red` is reused by the next call
__device__ __forceinline__ int block_max(int v, int* red) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const int o = __shfl_xor(v, off, 64);
    v = o > v ? o : v;
  }
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  int m = red[0];
  for (int w = 1; w < SP_NW; ++w) m = red[w] > m ? red[w] : m;
  __syncthreads();
  return m;
}

// ------------------------------------------------------------------------------------- stage 2
// grid B, block SP_NT.  Everything the block reads of n, next and the flags is in registers before the barrier
// that precedes the first store to them.
__global__ __launch_bounds__(SP_NT) void k_spec_group(PdeSpec a) {
  __shared__ int red[SP_NW];
  const int b = blockIdx.x, tid = threadIdx.x, q = a.K + 1, g0 = b * q, in0 = b * a.q_in;
  const bool was_fin = a.state[PDE_DS_FIN + b] != 0;
  const int n = a.n[b], len = a.len[b], L = len + n, rem = a.max_new - n, base = a.state[PDE_DS_POS];
  // rows that take part: row i can emit the (i + 1)-th token from here
  int na = 0;
  while (na < a.q_in && na < rem && L - 1 + na < a.n_pos) ++na;
  const bool bad = n < 0 || len < 1 || na < 1 || len + a.max_new > a.out_stride;      // a state that fits no generation
  int e = 1;
  bool hit = false;
  if (!was_fin && !bad) {
    while (e < na && a.next[g0 + e] == (int64_t)a.arg[in0 + e - 1]) ++e;
    if (a.eos >= 0)
      for (int i = 0; i < e; ++i)
        if (a.arg[in0 + i] == a.eos) {
          e = i + 1;
          hit = true;
          break;
        }
  }
  __syncthreads();
  if (was_fin || bad) return;                  // uniform per block

  int64_t* h = a.out + (size_t)b * a.out_stride;
  if (tid < e) h[L + tid] = a.arg[in0 + tid];
  if (hit)                                     // what a plain generation shows after an eos
    for (int t = L + e + tid; t < len + a.max_new; t += SP_NT) h[t] = a.eos;
  if (a.logits_out)
    for (int i = 0; i < e; ++i) {
      const bf16_t* src = reinterpret_cast<const bf16_t*>(a.logits) + (size_t)(in0 + i) * a.Vp;
      bf16_t* dst = reinterpret_cast<bf16_t*>(a.logits_out) + ((size_t)b * a.max_new + n + i) * a.V;
      for (int v = tid; v < a.V; v += SP_NT) dst[v] = src[v];
    }
  const int n2 = n + e, L2 = L + e, rem2 = a.max_new - n2;
  const bool fin = hit || rem2 <= 0;
  if (tid == 0) {
    a.n[b] = n2;
    a.steps[b] += a.q_in > 1 ? 1 : 0;
    a.accepted[b] += e - 1;
    a.state[PDE_DS_FIN + b] = fin ? 1 : 0;
  }
  __syncthreads();                             // the emitted tokens are part of the history now

  // prompt lookup: the latest earlier occurrence of the last m tokens, longest m first
  int j = -1;
  if (!fin) {
    int m = a.ngram < L2 - 1 ? a.ngram : L2 - 1;
    for (; m >= 1 && j < 0; --m) {
      int64_t suf[PDE_HIST_MAX_NGRAM];
#pragma unroll
      for (int t = 0; t < PDE_HIST_MAX_NGRAM; ++t) suf[t] = t < m ? h[L2 - m + t] : 0;
      int best = -1;
      for (int jj = m - 1 + tid; jj <= L2 - 2; jj += SP_NT) {
        bool same = true;
#pragma unroll
        for (int t = 0; t < PDE_HIST_MAX_NGRAM; ++t)
          if (t < m) same = same && h[jj - m + 1 + t] == suf[t];
        if (same) best = jj;
      }
      j = block_max(best, red);
    }
  }
  if (tid < q) {
    const int i = tid;
    const bool active = !fin && (i == 0 || (i < rem2 && L2 - 1 + i < a.n_pos));
    int64_t tok = h[L2 - 1];
    if (active && i > 0 && j >= 0) tok = h[j + 1 + (i - 1) % (L2 - 1 - j)];
    a.next[g0 + i] = tok;
    a.state[PDE_DS_OFF + g0 + i] = L2 - 1 + (active ? i : 0) - base;
  }
}

// tail: every group's flag is written
__global__ void k_spec_tail(PdeSpec a) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    int all = 1;
    for (int b = 0; b < a.B; ++b) all &= a.state[PDE_DS_FIN + b] != 0 ? 1 : 0;
    *a.done = all;
  }
}

}  // namespace

extern "C" {

hipError_t pde_decode_attention_spec(const void* qkv, void* cache, const int* state, float* part, void* out, int R,
                                     int H, int Tmax, float scale, PdeSpecRows s, hipStream_t st) {
  if (R < 1 || R > PDE_DS_MAX_ROWS || H < 1 || Tmax < 1 || s.q < 1 || R % s.q != 0) return hipErrorInvalidValue;
  return dec_attn_launch(qkv, cache, state, part, out, R, H, Tmax, scale, st, s);
}

hipError_t pde_spec_step(PdeSpec a, hipStream_t st) {
  if (a.B < 1 || a.K < 1 || a.B * (a.K + 1) > PDE_DS_MAX_ROWS || (a.q_in != 1 && a.q_in != a.K + 1) || a.V < 1 ||
      a.V > a.Vp || a.Vp % 8 != 0 || a.eos >= a.V || a.max_new < 1 || a.out_stride < 1 || a.n_pos < 1 || a.ngram < 1 ||
      a.ngram > PDE_HIST_MAX_NGRAM)
    return hipErrorInvalidValue;
  if (!a.logits || !a.state || !a.next || !a.out || !a.len || !a.n || !a.steps || !a.accepted || !a.arg || !a.done)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_spec_argmax, dim3(a.B * a.q_in), dim3(SP_NT), 0, st, a);
  PDE_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(k_spec_group, dim3(a.B), dim3(SP_NT), 0, st, a);
  PDE_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(k_spec_tail, dim3(1), dim3(64), 0, st, a);
  return hipGetLastError();
}

}  // extern "C"
