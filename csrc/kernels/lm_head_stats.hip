// LM-head loss without logits for gfx950: per-row softmax statistics of x = h . w[:V]^T, bf16 in, fp32
// accumulate on v_mfma_f32_32x32x16_bf16, with the logits living only in accumulator registers.
//
//   lse_i = logsumexp_{v < V} x_iv      xt_i = x_{i, tg_i}      sx_i = sum_{v < V} x_iv   (SX instantiation only)
//
// for h [N, C], w [Vp, C] (both K-contiguous rows), targets tg [N] (outside [0, V): the row does not count).
// It is a GEMM whose epilogue is an online log-sum-exp over the vocabulary, the way attention.hip treats its keys.
//
// Work split.  Grid = row tiles (256 rows of h) x S vocabulary slices; block id -> (slice, row tile) through
// xcd_remap, so the blocks of one XCD walk the SAME slice of w over neighbouring row tiles and share it in L2.  A
// block loops over the 256-wide vocabulary tiles of its slice and keeps its rows' running (m, l, sx) in registers:
// it streams its slice of w once (per tile: 256 x C of w and 256 x C of h, the operand traffic per flop of
// gemm.fprop's 256 x 256 LM-head tile).  The host picks S = floor(CUs / row tiles), clamped to the tile count and
// evened out (pde_lm_head_slices): 4 slices at N = 16384, 50 at N = 1024.
//
// Block = 512 threads = 8 waves as 2 (vocabulary) x 4 (rows); a wave owns 128 vocabulary rows x 64 rows of h = 4 x 2
// accumulators of 32 x 32 (128 accumulator registers).  The score tile is TRANSPOSED, S^T = W_tile . H^T: w is the
// A operand (vocabulary on accumulator registers: reg e of lane (r, hh) is vocabulary row (e&3) + 8(e>>2) + 4hh of
// the sub-tile), h the B operand (rows on lanes: column r).  Both operands are K-contiguous, so both fragments are
// plain row reads (ds_read_b128) of the swizzled [rows][64 bf16] image of pde_lds.h: nothing here needs the
// transposed read (trpair).  A row's running max and sum live in lane r and its mirror lane r + 32: the per-tile
// update is in-lane over 64 accumulator values plus ONE lane exchange, never a 32-lane reduction per row.
//
// Data movement.  K is staged 64 deep.  A stage = the w image (256 rows, 32 KB) + the h image (32 KB), filled by
// LDS-DMA (glds16; the swizzle goes into the per-lane source address, glds_row / glds_chunk): 8 wave-instructions
// per wave and stage.  Two stage buffers (128 KB) form the ring over the flat (vocabulary tile, k tile) stream, which
// runs on across vocabulary tiles: per stage a counted vmcnt wait (this wave's pieces of the stage; nothing younger
// has been issued yet, so the count is 0), one raw s_barrier, then the next stage's 8 pieces spread two per k-step
// between the fragment reads and the MFMAs, so the DMA of stage f + 1 -- the first of the next vocabulary tile
// included -- lands under the MFMAs of stage f and under the softmax update.  Fragment reads are inline asm with
// immediate offsets (no VALU on LDS addresses, no vmcnt(0) drain in front of them), double-buffered by k-step.
// Ragged row tiles and w rows >= V are given the out-of-range offset kOOB, for which the bounds-checked buffer load
// writes zeros: w[V:Vp] is never read, whatever it holds (NaN included), and its columns are exact zeros in sx.
// For max / exp the columns v >= V are SELECTED out by index (-inf), never multiplied away; only the tile that
// crosses V pays for the select (block-uniform branch).
//
// Softmax arithmetic.  l = sum exp2((x - m) * log2(e)) on the bare v_exp_f32, with the running max m kept UNSCALED:
// x - m is exact near the maximum and exactly 0 at it, so lse = m + ln l returns the maximum logit itself when one
// column dominates (a pre-scaled max, one fma per logit, would send it through * log2(e) * ln 2 and miss by an
// ulp).  The rescale of l is skipped when no row's max grew.  A row that has seen only selected-out columns keeps
// m = -inf and takes exp2((x - 0) * log2(e)), never exp2(-inf - -inf).
//
// Fixed-order combine.  The two vocabulary waves of a block meet through LDS (wave 0 first), the block writes one
// float4 (m, l, sx, xt) per row into part[slice][row], and k_lmhead_finish -- one thread per row, coalesced float4
// reads -- folds the S slices in slice order.  No atomics, no memset, no host read: two runs give the same bits, and
// a captured launch replays.
//
// xt is captured in the loop, by a column compare on the very accumulator that feeds lse, so lse >= xt holds as it
// does in exact arithmetic and a confidently right row gives a loss of +0, never a negative one (a separate fp32 dot
// h_i . w[tg_i] sums in another order and misses lse by an ulp of the logit).  The compare runs only where it can
// hit: a wave-uniform test of "some row's target lies in this wave's 128 columns" guards it, which fails for about
// 9 tiles in 10 at GPT-2's vocabulary.  Every other wave, lane half and slice contributes an exact 0 to the sum.
//
// Rows that do not count.  A block whose 256 targets are all outside [0, V) leaves at once (block-uniform).  The
// finishing kernel branches on the target: an ignored row writes exact zeros by select and reads neither its
// partials nor its weight.  Rows are columns of the MFMA's B operand, so NaN in one row never
// reaches another.  The finishing kernel also applies the loss definition of ops.lm_head_loss (PdeXentSmooth):
//   rows_i = w_i * (lse - keep * xt - spread * sx + z * lse^2)
#include <algorithm>
#include <type_traits>

#include "pde_bf16.h"
#include "pde_hip.h"
#include "pde_kernels.h"
#include "pde_lds.h"
#include "pde_lmhead.h"

namespace {

using namespace pde_lds;

constexpr int BR = 256, BV = 256;                  // block tile: rows of h x vocabulary rows of w
constexpr int WIMG = BV * 128, HIMG = BR * 128;    // [rows][64 bf16] images
constexpr int STAGE = WIMG + HIMG, NST = 2;
constexpr int TV = 4, TR = 2;                      // 32 x 32 accumulators of a wave: vocabulary x rows
constexpr float kLog2e = 1.4426950408889634f, kLn2 = 0.6931471805599453f;

struct LmArgs {
  const bf16_t* h;
  const bf16_t* w;
  const int64_t* tg;
  float4* part;          // [S][N] (m, l, sx, xt)
  int N, C, V, Vp;
  int rtiles, per;       // row tiles; vocabulary tiles per slice
};

template <int I, int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    static_for<I + 1, N>(f);
  }
}

template <int OFF>
__device__ __forceinline__ bf16x8 rd128(uint32_t addr) {
  bf16x8 v;
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF));
  return v;
}

__device__ __forceinline__ float fexp2(float x) { return __builtin_amdgcn_exp2f(x); }

// (m, l) <- (m, l) + (m2, l2); an empty side (m = -inf) adds an exact 0
__device__ __forceinline__ void ml_combine(float& m, float& l, float m2, float l2) {
  const float mn = fmaxf(m, m2);
  l = (m == -INFINITY ? 0.f : l * exp2f((m - mn) * kLog2e)) +
      (m2 == -INFINITY ? 0.f : l2 * exp2f((m2 - mn) * kLog2e));
  m = mn;
}

// One vocabulary tile's accumulators of row sub-tile J folded into the running (rmax, ls, sx, xt) of this lane's row.
// vb: vocabulary index of accumulator (0, J) register 0 of this lane; tgt: the row's target (-1: none).
// RAG: the tile crosses V.
template <bool SX, bool RAG, int J>
__device__ __forceinline__ void row_update(f32x16 (&acc)[TV][TR], int vb, int V, int tgt, float& rmax, float& ls,
                                           float& sx, float& xt) {
  float mx = -INFINITY;
  const int rel = tgt - vb;                        // this lane's half holds offsets 32i + 8(e>>2) + (e&3) (+ 4hh in vb)
  if (__any((uint32_t)(rel + (vb & 4)) < 128u)) {  // some row's target is a column of this wave
#pragma unroll
    for (int i = 0; i < TV; ++i)
#pragma unroll
      for (int e = 0; e < 16; ++e) xt = rel == 32 * i + (e & 3) + 8 * (e >> 2) ? acc[i][J][e] : xt;
  }
  if constexpr (SX) {                              // a column >= V is an exact 0 here: its w row was never loaded
    float sxl = 0.f;
#pragma unroll
    for (int i = 0; i < TV; ++i)
#pragma unroll
      for (int e = 0; e < 16; ++e) sxl += acc[i][J][e];
    sx += sxl;
    if constexpr (RAG) __builtin_amdgcn_sched_barrier(0);   // the sum is done before the select rewrites acc
  }
#pragma unroll
  for (int i = 0; i < TV; ++i)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      float x = acc[i][J][e];
      if constexpr (RAG) {
        x = vb + 32 * i + (e & 3) + 8 * (e >> 2) < V ? x : -INFINITY;
        acc[i][J][e] = x;
      }
      mx = fmaxf(mx, x);
    }
  mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
  const float mn = fmaxf(rmax, mx);
  if (__any(mn > rmax)) {                       // some row's running max grew: rescale l
    const float alpha = mn == -INFINITY ? 1.f : fexp2((rmax - mn) * kLog2e);
    ls *= alpha;
    rmax = mn;
  }
  const float sub = rmax == -INFINITY ? 0.f : rmax;   // a row that has seen no column yet: exp2(-inf - 0) = 0
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < TV; ++i)
#pragma unroll
    for (int e = 0; e < 16; ++e) s += fexp2((acc[i][J][e] - sub) * kLog2e);
  ls += s;
}

// grid rtiles * S, 512 threads
template <bool SX>
__global__ __launch_bounds__(512, 1) void k_lmhead_stats(LmArgs a) {
  __shared__ __attribute__((aligned(16))) char smem[NST * STAGE];
  const int t = threadIdx.x, l = t & 63, r = l & 31, hh = l >> 5;
  const int w = __builtin_amdgcn_readfirstlane(t >> 6), wv = w & 1, wr = w >> 1;
  const int id = xcd_remap(blockIdx.x, gridDim.x);
  const int slice = id / a.rtiles, r0 = (id - slice * a.rtiles) * BR;
  {   // a tile whose rows are all ignored has nothing to compute: its partials are never read
    const int row = r0 + (t & (BR - 1));
    bool live = false;
    if (row < a.N) {
      const int64_t g = a.tg[row];
      live = g >= 0 && g < a.V;
    }
    if (!__syncthreads_or(live)) return;
  }
  const int nvt = (a.V + BV - 1) / BV;
  const int vt0 = slice * a.per, vt1 = min(vt0 + a.per, nvt);
  const int KT = a.C >> 6, NF = (vt1 - vt0) * KT;
  const rsrc_t wres = make_rsrc(a.w, (uint32_t)a.Vp * (uint32_t)a.C * 2u);
  const rsrc_t hres = make_rsrc(a.h, (uint32_t)a.N * (uint32_t)a.C * 2u);

  // ---- LDS-DMA: wave w fills the 8-row groups 8u + w (u < 4) of both images ----
  const int lrow = glds_row(l), lch = glds_chunk(l, w & 1);
  uint32_t hoff[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int row = r0 + 8 * (8 * u + w) + lrow;
    hoff[u] = row < a.N ? ((uint32_t)row * (uint32_t)a.C + 8u * lch) * 2u : kOOB;
  }
  const int wrow = 8 * w + lrow;                    // + 64u: this lane's row of the w image
  auto issue_piece = [&](auto P_, int vt, int kt, int buf) {
    constexpr int P = decltype(P_)::value;
    const char* st = smem + buf * STAGE;
    if constexpr (P < 4) {
      const int v = vt * BV + 64 * P + wrow;
      glds16(wres, st + (8 * P + w) * 1024,
             v < a.V ? ((uint32_t)v * (uint32_t)a.C + 64u * kt + 8u * lch) * 2u : kOOB);
    } else {
      constexpr int U = P - 4;
      glds16(hres, st + WIMG + (8 * U + w) * 1024, hoff[U] + 128u * kt);
    }
  };

  // ---- fragment lane bases: rows base + (lane & 31), chunk 2S + (lane >> 5) of k-step S ----
  const int wrow0 = wv * 128 + r, hrow0 = wr * 64 + r;
  const uint32_t lds0 = (uint32_t)(uintptr_t)(lds_char*)smem;
  const uint2 wb = make_uint2(lds0 + toff(wrow0, hh), lds0 + toff(wrow0, 2 + hh));
  const uint2 hb = make_uint2(lds0 + WIMG + toff(hrow0, hh), lds0 + WIMG + toff(hrow0, 2 + hh));

  f32x16 acc[TV][TR];
#pragma unroll
  for (int i = 0; i < TV; ++i)
#pragma unroll
    for (int j = 0; j < TR; ++j) acc[i][j] = f32x16{0.f};
  float rmax[TR], ls[TR], sx[TR], xt[TR];
  int tgt[TR];
#pragma unroll
  for (int j = 0; j < TR; ++j) {
    rmax[j] = -INFINITY;
    ls[j] = sx[j] = xt[j] = 0.f;
    const int row = r0 + hrow0 + 32 * j;
    tgt[j] = -1;
    if (row < a.N) {
      const int64_t g = a.tg[row];
      tgt[j] = g >= 0 && g < a.V ? (int)g : -1;
    }
  }

  int ivt = vt0, ikt = 0;                            // the stage the next issue fills
  auto advance = [&]() {
    if (++ikt == KT) {
      ikt = 0;
      ++ivt;
    }
  };
  if (NF > 0) {
    static_for<0, 8>([&](auto P_) { issue_piece(P_, ivt, ikt, 0); });
    advance();
  }
  int vt = vt0, kt = 0;
  bf16x8 fw[2][TV], fh[2][TR];
  for (int f = 0; f < NF; ++f) {
    wait_vm<0>();
    __builtin_amdgcn_s_barrier();
    const bool do_issue = f + 1 < NF;
    const int buf = f & 1;
    const uint32_t so = buf * STAGE;
    const uint2 wa = add2(wb, so), ha = add2(hb, so);
    auto load = [&](auto S_, bf16x8* fw_, bf16x8* fh_) {
      constexpr int S = decltype(S_)::value;
      static_for<0, TV>([&](auto I_) {
        constexpr int i = decltype(I_)::value;
        fw_[i] = rd128<4096 * i + 512 * (S >> 1)>((S & 1) ? wa.y : wa.x);
      });
      static_for<0, TR>([&](auto J_) {
        constexpr int j = decltype(J_)::value;
        fh_[j] = rd128<4096 * j + 512 * (S >> 1)>((S & 1) ? ha.y : ha.x);
      });
    };
    load(std::integral_constant<int, 0>{}, fw[0], fh[0]);
    lgkm_fence();
    static_for<0, 4>([&](auto S_) {
      constexpr int S = decltype(S_)::value;
      if constexpr (S < 3) load(std::integral_constant<int, S + 1>{}, fw[(S + 1) & 1], fh[(S + 1) & 1]);
      if (do_issue) static_for<2 * S, 2 * S + 2>([&](auto P_) { issue_piece(P_, ivt, ikt, buf ^ 1); });
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int i = 0; i < TV; ++i)
#pragma unroll
        for (int j = 0; j < TR; ++j) acc[i][j] = mfma_bf16(fw[S & 1][i], fh[S & 1][j], acc[i][j]);
      if constexpr (S < 3) {
        __builtin_amdgcn_sched_barrier(0);           // the wait stays behind this k-step's MFMAs
        lgkm_fence();
      }
    });
    if (do_issue) advance();
    if (++kt == KT) {                                // the vocabulary tile is complete: fold it, start the next
      const int vb = vt * BV + wv * 128 + 4 * hh;
      if (vt * BV + BV > a.V) {
        row_update<SX, true, 0>(acc, vb, a.V, tgt[0], rmax[0], ls[0], sx[0], xt[0]);
        row_update<SX, true, 1>(acc, vb, a.V, tgt[1], rmax[1], ls[1], sx[1], xt[1]);
      } else {
        row_update<SX, false, 0>(acc, vb, a.V, tgt[0], rmax[0], ls[0], sx[0], xt[0]);
        row_update<SX, false, 1>(acc, vb, a.V, tgt[1], rmax[1], ls[1], sx[1], xt[1]);
      }
#pragma unroll
      for (int i = 0; i < TV; ++i)
#pragma unroll
        for (int j = 0; j < TR; ++j) acc[i][j] = f32x16{0.f};
      kt = 0;
      ++vt;
    }
  }
  // ---- the two lane halves of a row, then the two vocabulary waves (wave 0 first), then one float4 per row ----
#pragma unroll
  for (int j = 0; j < TR; ++j) {
    ls[j] += __shfl_xor(ls[j], 32, 64);
    sx[j] += __shfl_xor(sx[j], 32, 64);
    xt[j] += __shfl_xor(xt[j], 32, 64);              // one half holds the target's logit, the other an exact 0
  }
  __syncthreads();                                   // every wave is done reading the stage buffers
  float4* ex = reinterpret_cast<float4*>(smem);      // [BR]
  if (wv == 1 && hh == 0) {
#pragma unroll
    for (int j = 0; j < TR; ++j) ex[wr * 64 + 32 * j + r] = make_float4(rmax[j], ls[j], sx[j], xt[j]);
  }
  __syncthreads();
  if (wv == 0 && hh == 0) {
#pragma unroll
    for (int j = 0; j < TR; ++j) {
      const int lr = wr * 64 + 32 * j + r, row = r0 + lr;
      const float4 o = ex[lr];
      float m = rmax[j], s = ls[j];
      ml_combine(m, s, o.x, o.y);
      if (row < a.N) a.part[(size_t)slice * a.N + row] = make_float4(m, s, sx[j] + o.z, xt[j] + o.w);
    }
  }
}

struct LmFinish {
  const int64_t* tg;
  const float4* part;
  float* lse;            // each nullable
  float* xt;
  float* sx;
  float* rows;
  PdeXentSmooth sm;
  int N, V, S;
};

// One thread per row: the S partials in slice order, then the loss row.
__global__ __launch_bounds__(256) void k_lmhead_finish(LmFinish a) {
  const int row = blockIdx.x * 256 + threadIdx.x;
  if (row >= a.N) return;
  const int64_t g = a.tg[row];
  float lse = 0.f, xt = 0.f, sx = 0.f, loss = 0.f;
  if (g >= 0 && g < a.V) {                           // an ignored row reads nothing more
    float m = -INFINITY, s = 0.f;
    for (int q = 0; q < a.S; ++q) {
      const float4 p = a.part[(size_t)q * a.N + row];
      ml_combine(m, s, p.x, p.y);
      sx += p.z;
      xt += p.w;
    }
    lse = m + log2f(s) * kLn2;
    const float wr = a.sm.w ? a.sm.w[row] : 1.f;
    loss = wr * (((lse - a.sm.keep * xt) - a.sm.spread * sx) + a.sm.z * lse * lse);
  }
  if (a.lse) a.lse[row] = lse;
  if (a.xt) a.xt[row] = xt;
  if (a.sx) a.sx[row] = sx;
  if (a.rows) a.rows[row] = loss;
}

int g_lm_num_cu = 0;
int lm_num_cu() {
  if (g_lm_num_cu == 0) {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
      n = 256;
    g_lm_num_cu = n;
  }
  return g_lm_num_cu;
}

// vocabulary tiles per slice for the S of pde_lm_head_slices
int lm_tiles_per_slice(int N, int V) {
  const int rtiles = (N + BR - 1) / BR, nvt = (V + BV - 1) / BV;
  const int want = std::min(std::max(lm_num_cu() / rtiles, 1), nvt);
  return (nvt + want - 1) / want;
}

}  // namespace

extern "C" int pde_lm_head_slices(int N, int V) {
  const int nvt = (V + BV - 1) / BV, per = lm_tiles_per_slice(N, V);
  return (nvt + per - 1) / per;
}

extern "C" hipError_t pde_lm_head_stats(PdeLmHeadStats p, hipStream_t st) {
  if (p.N < 1 || p.V < 1 || p.V > p.Vp || p.C < 64 || p.C % 64 != 0 || p.Vp % 8 != 0) return hipErrorInvalidValue;
  if ((uint64_t)p.Vp * p.C * 2 >= kOOB || (uint64_t)p.N * p.C * 2 >= kOOB) return hipErrorInvalidValue;
  if (p.S != pde_lm_head_slices(p.N, p.V)) return hipErrorInvalidValue;
  const bool with_sx = p.sx != nullptr || p.sm.spread != 0.f;
  LmArgs a{reinterpret_cast<const bf16_t*>(p.h), reinterpret_cast<const bf16_t*>(p.w), p.tg,
           reinterpret_cast<float4*>(p.part), p.N, p.C, p.V, p.Vp, (p.N + BR - 1) / BR,
           lm_tiles_per_slice(p.N, p.V)};
  const dim3 grid((unsigned)(a.rtiles * p.S));
  if (with_sx) hipLaunchKernelGGL(k_lmhead_stats<true>, grid, dim3(512), 0, st, a);
  else hipLaunchKernelGGL(k_lmhead_stats<false>, grid, dim3(512), 0, st, a);
  PDE_HIP_CHECK(hipGetLastError());
  LmFinish f{p.tg, reinterpret_cast<const float4*>(p.part), p.lse, p.xt, p.sx, p.rows, p.sm, p.N, p.V, p.S};
  hipLaunchKernelGGL(k_lmhead_finish, dim3((unsigned)((p.N + 255) / 256)), dim3(256), 0, st, f);
  return hipGetLastError();
}
