// Muon's hot path (definition: optim/muon.py, interface: pde_muon.h): a grouped bf16 MFMA GEMM for the small
// square-ish products of the Newton-Schulz iteration, and the two streaming kernels around it.  gfx950 only.
//
// k_muon_gemm<SYM>: one launch serves every matrix of a stage.  A block owns one 128 x 128 output tile of one
// problem (by-value table, block -> problem by a prefix walk); 4 waves of 64 x 64 (2 x 2 v_mfma_f32_32x32x16_bf16),
// K in 64-wide stages, double-buffered, filled by LDS-DMA into the swizzled images of pde_lds.h.
//
//  * Tile 128 x 128: a 768 x 768 symmetric output has 21 upper tiles, 252 for one kind of matrix over 12 layers --
//    one round of the 256 CUs -- and 1008 for all 48 matrices of a stage; at two blocks per CU (64 KB of LDS and
//    under 128 VGPRs each) that is two rounds.  256-wide tiles leave 6 per matrix (most of the chip idle per kind),
//    64-wide tiles halve the flops per staged byte.  Ragged edges (n = 192, 320: multiples of 64, not of 128) cost
//    nothing: rows and columns past the matrix are zero-filled by the loads and skipped by the stores.
//  * SYM (A = X X^T, A A = A A^T): both operands are K-contiguous, fragments are row reads (ds_read_b128).  Only
//    tiles i <= j are computed; the mirror tile is written from the same accumulators by a transposed store, and
//    diagonal tiles once.  The operand order of an MFMA does not change its sum, so the output equals its
//    transpose bit for bit.
//  * rectangular (X <- a X + B X): everything is kept physically in the wide orientation (the prologue writes X0
//    transposed for a tall matrix and the apply kernel reads it back transposed), so there is one rectangular form.
//    Its reduction runs over the ROW index of X, and -- B being symmetric -- over the row index of B too:
//    D = B^T X.  Both operands are therefore staged as [k][64-column] images and read with ds_read_b64_tr_b16 in
//    the same k order (pde_lds.h trpair), the arrangement of conv.hip's k_wgrad; no row-read operand has to meet a
//    transposed one.  Keeping tall matrices tall instead would need the transposed form in stage 1 as well and a
//    second rectangular kernel; the two 64 x 64 LDS transposes in the streaming kernels are cheaper than that.
//  * Epilogue: the fp32 accumulators go through LDS (64 rows at a time, the stage buffers reused), the alpha C term
//    is read with 16-byte loads and added in fp32 before the one rounding, stores are 16 bytes.
//
// k_muon_momentum / k_muon_x0 / k_muon_apply: streaming kernels over 64 x 64 tiles with 16-byte accesses.  The
// Frobenius norm is reduced per matrix in a fixed order (per-tile partials, folded in index order by every block
// that needs it): no atomics, the same bits on every run and replica.
#include "pde_hip.h"
#include "pde_bf16.h"
#include "pde_lds.h"
#include "pde_lr.h"
#include "pde_muon.h"

#include <cmath>
#include <type_traits>

namespace {

using namespace pde_lds;

constexpr int kThreads = 256;
constexpr int BT = 128;                       // output tile
constexpr int IMG = 16384;                    // one operand's stage: 128 rows x 64 k (SYM) or 64 k x 128 columns
constexpr int STAGE = 2 * IMG, NST = 2;
constexpr int RSF = 132;                      // fp32 row stride of the epilogue's 64-row half tile (floats)
static_assert(64 * RSF * 4 <= NST * STAGE, "epilogue tile fits the stage buffers");

struct GemmTab {
  PdeMuonGemm p[PDE_MUON_MAX_MATS];
  int count;
  float alpha, beta;
};

// the one expression of the alpha C + beta acc epilogue (direct and mirror stores must round alike)
__device__ __forceinline__ float axpy1(float alpha, float c, float beta, float v) { return fmaf(alpha, c, beta * v); }

// 8 consecutive outputs: v[e] (fp32 accumulators) -> bf16 at d, with the C term when there is one
__device__ __forceinline__ void store8(const PdeMuonGemm& P, size_t o, float* v, float alpha, float beta) {
  if (P.C != nullptr) {
    float c[8];
    unpack8(*reinterpret_cast<const uint4*>(static_cast<const bf16_t*>(P.C) + o), c);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = axpy1(alpha, c[e], beta, v[e]);
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] *= beta;
  }
  *reinterpret_cast<uint4*>(static_cast<bf16_t*>(P.D) + o) = pack8(v);
}

template <bool SYM>
__global__ __launch_bounds__(kThreads, 2) void k_muon_gemm(GemmTab a) {
  __shared__ __attribute__((aligned(16))) char smem[NST * STAGE];
  const int t = threadIdx.x, l = t & 63, w = __builtin_amdgcn_readfirstlane(t >> 6);
  const int id = xcd_remap(blockIdx.x, gridDim.x);
  int pi = 0;
  while (pi + 1 < a.count && id >= a.p[pi + 1].tile0) ++pi;
  const PdeMuonGemm& P = a.p[pi];
  int local = id - P.tile0, ti, tj;
  const int ncols = SYM ? P.rows : P.cols;
  if constexpr (SYM) {                               // upper tiles, row by row
    const int T = (P.rows + BT - 1) / BT;
    ti = 0;
    while (local >= T - ti) { local -= T - ti; ++ti; }
    tj = ti + local;
  } else {
    const int TN = (P.cols + BT - 1) / BT;
    ti = local / TN;
    tj = local - ti * TN;
  }
  const int i0 = ti * BT, j0 = tj * BT;
  const int KT = P.K >> 6;

  // LDS-DMA sources.  SYM: instruction u fills 8-row group 4u + w of a [128 rows][64 k] image.  Otherwise: group
  // (4u + w) & 7 of the 64-column image (4u + w) >> 3 of a [64 k][128 columns] stage (k_wgrad's arrangement).
  const int lrow = glds_row(l), ch = glds_chunk(l, w & 1);
  const uint32_t abytes = (uint32_t)((size_t)P.rows * P.K * 2);
  const uint32_t bbytes = SYM ? abytes : (uint32_t)((size_t)P.K * P.cols * 2);
  const rsrc_t ar = make_rsrc(P.A, abytes), br = make_rsrc(SYM ? P.A : P.B, bbytes);
  uint32_t aoff[4], boff[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int q = 4 * u + w;
    if constexpr (SYM) {
      const int ra = i0 + 8 * q + lrow, rb = j0 + 8 * q + lrow;
      aoff[u] = ra < P.rows ? (uint32_t)(ra * P.K + ch * 8) * 2u : kOOB;
      boff[u] = rb < P.rows ? (uint32_t)(rb * P.K + ch * 8) * 2u : kOOB;
    } else {
      const int k = 8 * (q & 7) + lrow, ca = i0 + (q >> 3) * 64 + ch * 8, cb = j0 + (q >> 3) * 64 + ch * 8;
      aoff[u] = ca < P.rows ? (uint32_t)(k * P.rows + ca) * 2u : kOOB;
      boff[u] = cb < P.cols ? (uint32_t)(k * P.cols + cb) * 2u : kOOB;
    }
  }
  const uint32_t astep = SYM ? 128u : (uint32_t)P.rows * 128u, bstep = SYM ? 128u : (uint32_t)P.cols * 128u;
  auto issue = [&](int kt, int buf) {
    const char* Ai = smem + buf * STAGE;
    const char* Bi = Ai + IMG;
#pragma unroll
    for (int u = 0; u < 4; ++u)
      glds16(ar, Ai + (4 * u + w) * 1024, aoff[u] == kOOB ? kOOB : aoff[u] + (uint32_t)kt * astep);
#pragma unroll
    for (int u = 0; u < 4; ++u)
      glds16(br, Bi + (4 * u + w) * 1024, boff[u] == kOOB ? kOOB : boff[u] + (uint32_t)kt * bstep);
  };

  const int wm = w >> 1, wn = w & 1, lr = l & 31, lh = l >> 5;
  const uint32_t lds_base = (uint32_t)(uintptr_t)(lds_char*)smem;
  const uint2 a_lane = add2(tr_lane_off(), colblk_off(wm * 2));
  const uint2 b_lane = add2(tr_lane_off(), colblk_off(wn * 2));
  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x16{0.f};

  issue(0, 0);
  int buf = 0;
  for (int kt = 0; kt < KT; ++kt) {
    wait_vm<0>();
    __builtin_amdgcn_s_barrier();                    // stage kt landed; every wave is done with stage kt - 1
    if (kt + 1 < KT) issue(kt + 1, buf ^ 1);
    auto mm = [&](const bf16x8* fa, const bf16x8* fb) {
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = mfma_bf16(fa[i], fb[j], acc[i][j]);
    };
    if constexpr (SYM) {
      const char* Ai = smem + buf * STAGE;
      const char* Bi = Ai + IMG;
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        bf16x8 fa[2], fb[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) fa[i] = row_frag(Ai, wm * 64 + i * 32 + lr, 2 * s + lh);
#pragma unroll
        for (int j = 0; j < 2; ++j) fb[j] = row_frag(Bi, wn * 64 + j * 32 + lr, 2 * s + lh);
        mm(fa, fb);
      }
    } else {
      const uint32_t sb = lds_base + buf * STAGE;
      const uint2 ab = add2(a_lane, sb), bb = add2(b_lane, sb + IMG);
      bf16x8 fa0[2], fb0[2], fa1[2], fb1[2];
      auto frags = [&](auto S, bf16x8* fa, bf16x8* fb) {
        constexpr int O = 2048 * decltype(S)::value;
        fa[0] = trpair<O>(ab);
        fa[1] = trpair<O + colblk_off(1)>(ab);
        fb[0] = trpair<O>(bb);
        fb[1] = trpair<O + colblk_off(1)>(bb);
      };
      frags(std::integral_constant<int, 0>{}, fa0, fb0);
      lgkm_fence();
      frags(std::integral_constant<int, 1>{}, fa1, fb1);
      mm(fa0, fb0);
      lgkm_fence();
      frags(std::integral_constant<int, 2>{}, fa0, fb0);
      mm(fa1, fb1);
      lgkm_fence();
      frags(std::integral_constant<int, 3>{}, fa1, fb1);
      mm(fa0, fb0);
      lgkm_fence();
      mm(fa1, fb1);
    }
    buf ^= 1;
  }
  __syncthreads();                                   // every wave is done with the stage buffers

  // ---- epilogue: 64 rows at a time through LDS in fp32 ----
  float* ft = reinterpret_cast<float*>(smem);
  const bool mirror = SYM && ti != tj;
  for (int h = 0; h < 2; ++h) {
    if (wm == h) {
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int q = 0; q < 16; ++q)
            ft[(i * 32 + (q & 3) + 8 * (q >> 2) + 4 * lh) * RSF + wn * 64 + j * 32 + lr] = acc[i][j][q];
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 4; ++u) {                    // D[i0 + 64h + r][j0 + 8cc ..]
      const int c = t + kThreads * u, r = c >> 4, cc = c & 15;
      const int grow = i0 + 64 * h + r, gcol = j0 + cc * 8;
      if (grow < P.rows && gcol < ncols) {
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = ft[r * RSF + cc * 8 + e];
        store8(P, (size_t)grow * ncols + gcol, v, a.alpha, a.beta);
      }
    }
    if (mirror) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {                  // D[j0 + c2][i0 + 64h + 8rc ..] = the tile's transpose
        const int c = t + kThreads * u, rc = c & 7, c2 = c >> 3;
        const int grow = j0 + c2, gcol = i0 + 64 * h + rc * 8;
        if (grow < P.rows && gcol < P.rows) {
          float v[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] = ft[(rc * 8 + e) * RSF + c2];
          store8(P, (size_t)grow * P.rows + gcol, v, a.alpha, a.beta);
        }
      }
    }
    __syncthreads();
  }
}

// ============================================================================ streaming kernels
struct MatTab {
  PdeMuonMat m[PDE_MUON_MAX_MATS];
  int count;
};

constexpr int TS = 64;                          // streaming tile edge
constexpr int TRS = 72;                         // bf16 row stride of the transposing LDS tile (144 B)

struct TilePos {
  int mi, r0, c0;
};
__device__ __forceinline__ TilePos tile_of(const MatTab& a, int blk) {
  int mi = 0;
  while (mi + 1 < a.count && blk >= a.m[mi + 1].blk0) ++mi;
  const int local = blk - a.m[mi].blk0, tcs = a.m[mi].C / TS;
  const int tr = local / tcs;
  return TilePos{mi, tr * TS, (local - tr * tcs) * TS};
}

// u (fp32) of 8 consecutive elements at o: the momentum rule of the definition; UPDATE also writes M
template <bool UPDATE>
__device__ __forceinline__ void load_u(const PdeMuonMat& M, size_t o, float mu, int nesterov, float gs, float* u) {
  float g[8];
  unpack8(*reinterpret_cast<const uint4*>(static_cast<const bf16_t*>(M.src) + o), g);
#pragma unroll
  for (int e = 0; e < 8; ++e) g[e] *= gs;
  if (M.f32 == nullptr) {
#pragma unroll
    for (int e = 0; e < 8; ++e) u[e] = g[e];
    return;
  }
  float4* mp = reinterpret_cast<float4*>(M.f32 + o);
  float4 m0 = mp[0], m1 = mp[1];
  float m[8] = {m0.x, m0.y, m0.z, m0.w, m1.x, m1.y, m1.z, m1.w};
  if (UPDATE) {
#pragma unroll
    for (int e = 0; e < 8; ++e) m[e] = fmaf(mu, m[e], g[e]);
    mp[0] = make_float4(m[0], m[1], m[2], m[3]);
    mp[1] = make_float4(m[4], m[5], m[6], m[7]);
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) u[e] = nesterov ? fmaf(mu, m[e], g[e]) : m[e];
}

// block sum in a fixed order: xor-shuffle tree per wave, the four waves in index order
__device__ __forceinline__ float block_sum(float v, float* red) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  const float s = ((red[0] + red[1]) + red[2]) + red[3];
  __syncthreads();
  return s;
}

__global__ __launch_bounds__(kThreads) void k_muon_momentum(MatTab a, float* __restrict__ partials, float mu,
                                                            int nesterov, float gs) {
  __shared__ float red[4];
  const TilePos tp = tile_of(a, blockIdx.x);
  const PdeMuonMat& M = a.m[tp.mi];
  const int t = threadIdx.x;
  float ss = 0.f;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int c = t + kThreads * k, r = c >> 3, cc = c & 7;
    float u[8];
    load_u<true>(M, (size_t)(tp.r0 + r) * M.C + tp.c0 + cc * 8, mu, nesterov, gs, u);
#pragma unroll
    for (int e = 0; e < 8; ++e) ss = fmaf(u[e], u[e], ss);
  }
  ss = block_sum(ss, red);
  if (t == 0) partials[blockIdx.x] = ss;
}

__global__ __launch_bounds__(kThreads) void k_muon_x0(MatTab a, const float* __restrict__ partials, float mu,
                                                      int nesterov, float gs) {
  __shared__ float red[4];
  __shared__ __attribute__((aligned(16))) bf16_t tl[TS * TRS];
  const TilePos tp = tile_of(a, blockIdx.x);
  const PdeMuonMat& M = a.m[tp.mi];
  const int t = threadIdx.x;
  // ||U||^2: thread t takes partials t, t + 256, ... in order, then the fixed block tree
  const int np = (M.R / TS) * (M.C / TS);
  float ss = 0.f;
  for (int i = t; i < np; i += kThreads) ss += partials[M.blk0 + i];
  ss = block_sum(ss, red);
  const float den = sqrtf(ss) + 1e-7f;
  const bool tall = M.R > M.C;
  bf16_t* X = static_cast<bf16_t*>(M.dst);
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int c = t + kThreads * k, r = c >> 3, cc = c & 7;
    float u[8];
    load_u<false>(M, (size_t)(tp.r0 + r) * M.C + tp.c0 + cc * 8, mu, nesterov, gs, u);
#pragma unroll
    for (int e = 0; e < 8; ++e) u[e] = u[e] / den;
    const uint4 pk = pack8(u);
    if (tall) *reinterpret_cast<uint4*>(tl + r * TRS + cc * 8) = pk;
    else *reinterpret_cast<uint4*>(X + (size_t)(tp.r0 + r) * M.C + tp.c0 + cc * 8) = pk;
  }
  if (tall) {                                        // block-uniform: X0 [C][R] = U^T through the LDS tile
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int c = t + kThreads * k, oc = c >> 3, rc = c & 7;
      __attribute__((aligned(16))) bf16_t v[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = tl[(rc * 8 + e) * TRS + oc];
      *reinterpret_cast<uint4*>(X + (size_t)(tp.c0 + oc) * M.R + tp.r0 + rc * 8) = *reinterpret_cast<const uint4*>(v);
    }
  }
}

__global__ __launch_bounds__(kThreads) void k_muon_apply(MatTab a, float lr, int step, const float* __restrict__ step_dev,
                                                         const float* __restrict__ lr_tab, int lr_len) {
  __shared__ __attribute__((aligned(16))) bf16_t tl[TS * TRS];
  const TilePos tp = tile_of(a, blockIdx.x);
  const PdeMuonMat& M = a.m[tp.mi];
  const int t = threadIdx.x;
  if (step_dev) step = (int)*step_dev;               // capturable: the count lives on the device
  lr = sched_lr(lr, lr_tab, lr_len, step);
  const float keep = 1.f - lr * M.wd, sc = lr * M.scale;
  const bool tall = M.R > M.C;
  const bf16_t* X = static_cast<const bf16_t*>(M.src);
  if (tall) {                                        // O[r][c] = X[c][r]: the wide tile through LDS
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int c = t + kThreads * k, oc = c >> 3, rc = c & 7;
      *reinterpret_cast<uint4*>(tl + oc * TRS + rc * 8) =
          *reinterpret_cast<const uint4*>(X + (size_t)(tp.c0 + oc) * M.R + tp.r0 + rc * 8);
    }
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int c = t + kThreads * k, r = c >> 3, cc = c & 7;
    const size_t o = (size_t)(tp.r0 + r) * M.C + tp.c0 + cc * 8;
    uint4 ov;
    if (tall) {
      __attribute__((aligned(16))) bf16_t v[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = tl[(cc * 8 + e) * TRS + r];
      ov = *reinterpret_cast<const uint4*>(v);
    } else {
      ov = *reinterpret_cast<const uint4*>(X + o);
    }
    if (M.f32 == nullptr) {                          // the orthogonalisation alone: dst = O
      *reinterpret_cast<uint4*>(static_cast<bf16_t*>(M.dst) + o) = ov;
      continue;
    }
    float of[8];
    unpack8(ov, of);
    float4* mp = reinterpret_cast<float4*>(M.f32 + o);
    const float4 m0 = mp[0], m1 = mp[1];
    float m[8] = {m0.x, m0.y, m0.z, m0.w, m1.x, m1.y, m1.z, m1.w};
#pragma unroll
    for (int e = 0; e < 8; ++e) m[e] = fmaf(-sc, of[e], m[e] * keep);
    mp[0] = make_float4(m[0], m[1], m[2], m[3]);
    mp[1] = make_float4(m[4], m[5], m[6], m[7]);
    *reinterpret_cast<uint4*>(static_cast<bf16_t*>(M.dst) + o) = pack8(m);
  }
}

bool dims_ok(int64_t r, int64_t c) { return r >= 64 && c >= 64 && r % 64 == 0 && c % 64 == 0 && r * c * 2 < (1LL << 31); }
bool al16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

template <bool SYM>
hipError_t launch_gemm(PdeMuonGemm* probs, int count, float alpha, float beta, hipStream_t st) {
  if (probs == nullptr || count < 1) return hipErrorInvalidValue;
  for (int i = 0; i < count; ++i) {
    const PdeMuonGemm& p = probs[i];
    const int cols = SYM ? p.rows : p.cols;
    if (!dims_ok(p.rows, p.K) || !dims_ok(p.rows, cols) || !dims_ok(p.K, cols)) return hipErrorInvalidValue;
    if (p.A == nullptr || p.D == nullptr || !al16(p.A) || !al16(p.D) || !al16(p.C)) return hipErrorInvalidValue;
    if (!SYM && (p.B == nullptr || p.C == nullptr || !al16(p.B) || p.D == p.B || p.D == p.C)) return hipErrorInvalidValue;
  }
  for (int base = 0; base < count; base += PDE_MUON_MAX_MATS) {
    GemmTab tab;
    tab.count = count - base < PDE_MUON_MAX_MATS ? count - base : PDE_MUON_MAX_MATS;
    tab.alpha = alpha;
    tab.beta = beta;
    int64_t tiles = 0;
    for (int i = 0; i < tab.count; ++i) {
      PdeMuonGemm& p = probs[base + i];
      p.tile0 = (int)tiles;
      const int64_t T = (p.rows + BT - 1) / BT;
      tiles += SYM ? T * (T + 1) / 2 : T * ((p.cols + BT - 1) / BT);
      tab.p[i] = p;
    }
    if (tiles >= (1LL << 31)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_muon_gemm<SYM>, dim3((unsigned)tiles), dim3(kThreads), 0, st, tab);
    PDE_HIP_CHECK(hipGetLastError());
  }
  return hipSuccess;
}

// the chunks of a streaming launch: fills blk0 (relative to the chunk) and returns the chunk's tile count
int64_t fill_tab(MatTab& tab, PdeMuonMat* mats, int base, int count) {
  tab.count = count - base < PDE_MUON_MAX_MATS ? count - base : PDE_MUON_MAX_MATS;
  int64_t tiles = 0;
  for (int i = 0; i < tab.count; ++i) {
    mats[base + i].blk0 = (int)tiles;
    tiles += pde_muon_tiles(mats[base + i].R, mats[base + i].C);
    tab.m[i] = mats[base + i];
  }
  return tiles;
}

hipError_t check_mats(const PdeMuonMat* mats, int count) {
  if (mats == nullptr || count < 1) return hipErrorInvalidValue;
  for (int i = 0; i < count; ++i) {
    const PdeMuonMat& m = mats[i];
    if (!dims_ok(m.R, m.C) || m.src == nullptr || m.dst == nullptr || !al16(m.src) || !al16(m.dst) || !al16(m.f32))
      return hipErrorInvalidValue;
  }
  return hipSuccess;
}

}  // namespace

extern "C" {

int64_t pde_muon_tiles(int R, int C) { return (int64_t)(R / TS) * (C / TS); }

hipError_t pde_muon_gemm_sym(PdeMuonGemm* probs, int count, float alpha, float beta, hipStream_t st) {
  return launch_gemm<true>(probs, count, alpha, beta, st);
}

hipError_t pde_muon_gemm_rect(PdeMuonGemm* probs, int count, float alpha, float beta, hipStream_t st) {
  return launch_gemm<false>(probs, count, alpha, beta, st);
}

hipError_t pde_muon_prologue(PdeMuonMat* mats, int count, float* partials, float mu, int nesterov, float grad_scale,
                             hipStream_t st) {
  PDE_HIP_CHECK(check_mats(mats, count));
  if (partials == nullptr) return hipErrorInvalidValue;
  for (int base = 0; base < count; base += PDE_MUON_MAX_MATS) {
    MatTab tab;
    const int64_t tiles = fill_tab(tab, mats, base, count);
    if (tiles >= (1LL << 31)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_muon_momentum, dim3((unsigned)tiles), dim3(kThreads), 0, st, tab, partials, mu, nesterov,
                       grad_scale);
    hipLaunchKernelGGL(k_muon_x0, dim3((unsigned)tiles), dim3(kThreads), 0, st, tab, partials, mu, nesterov, grad_scale);
    PDE_HIP_CHECK(hipGetLastError());
    partials += tiles;
  }
  return hipSuccess;
}

hipError_t pde_muon_apply(PdeMuonMat* mats, int count, float lr, int step, const float* step_dev, const float* lr_tab,
                          int lr_len, hipStream_t st) {
  PDE_HIP_CHECK(check_mats(mats, count));
  if (lr_tab != nullptr && lr_len < 1) return hipErrorInvalidValue;
  for (int base = 0; base < count; base += PDE_MUON_MAX_MATS) {
    MatTab tab;
    const int64_t tiles = fill_tab(tab, mats, base, count);
    if (tiles >= (1LL << 31)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_muon_apply, dim3((unsigned)tiles), dim3(kThreads), 0, st, tab, lr, step, step_dev, lr_tab, lr_len);
    PDE_HIP_CHECK(hipGetLastError());
  }
  return hipSuccess;
}

}  // extern "C"
