// FP8 (OCP e4m3fn) forward GEMM for the GPT-2 block projections and its per-tensor quantiser (pde_fp8.h holds
// the numeric definition and the workspace protocol).
//
//   y[m][n] = bf16((sum_k xq[m][k] * wq[n][k]) * (1/sx) * (1/sw) + bias[n])        (+ the GELU pair)
//
// k_gemm_fp8: block tile 256 x 128, 8 waves as 4 x 2, each wave 64 x 64 = 2 x 2 accumulators of
// v_mfma_scale_f32_32x32x64_f8f6f4 (formats 0 = e4m3, E8M0 scales 0x7f = 1).  One tile per block, XCD-aware id
// remap and groups of 8 row tiles as in gemm.hip.
//
// K is staged in 128-byte slices (two 64-deep MFMA steps) through a ring of three 48 KB LDS stages filled by
// LDS-DMA (buffer_load ... lds, 16 B per lane, six 1 KB wave-instructions per wave and slice).  Per slice:
//   s_waitcnt vmcnt(6)  -- this wave's part of slice s landed, slice s + 1 stays in flight
//   s_barrier           -- everyone's part landed, and everyone left the buffer of slice s - 1
//   issue slice s + 2 into that buffer (always six loads: past K they carry the out-of-range offset, which
//                       fills zeros into a buffer nobody reads, so the allowance is one constant)
//   16 ds_read_b128 of both steps' fragments, lgkmcnt(8), 4 MFMAs, lgkmcnt(0), 4 MFMAs
// The loop holds no store, so no store is ever part of a vmcnt allowance; the output stores come after a
// vmcnt(0) and leave with the block.  Chunks past K (the K % 128 == 64 tail) and rows past M / N are filled
// with zeros by the buffer resource's range check.  LDS reads are inline asm (as in gemm.hip: the compiler would
// drain the in-flight DMA in front of an LDS read it can see).
//
// Operand layout of the 32x32x64 form, confirmed by tests/test_fp8_gpu.py at (8, 8, 64) .. (512, 768, 3072):
//   lane l supplies row l & 31 of its operand and 32 K bytes in 8 VGPRs; this kernel gives it the 32
//   consecutive bytes starting at 32 * (l >> 5) of the 64-deep step, read as two 16-byte chunks.  Both operands
//   use the same map, so the product does not depend on which K bytes the hardware pairs inside a lane half.
//   Accumulator register r of lane l is D[(r & 3) + 8 * (r >> 2) + 4 * (l >> 5)][l & 31], D's rows being the
//   first operand's.  The MFMA runs with w first and x second, so a lane holds four consecutive columns of y
//   per register quad: y[32 i + (l & 31)][32 j + 8 g + 4 (l >> 5) + e] in register 4 g + e of accumulator (i, j).
//
// Epilogue: scale by the device scalars xs[1] * ws[1] (both powers of two: exact), add the bias in fp32, round
// once to bf16 into an LDS tile, then coalesced 16-byte row stores; with GELU the store loop applies
// gelu2_d (pde_act.h) to the bf16-rounded pre-activation exactly as gemm.hip's kGelu epilogue does.
//
// Quantiser: k_fp8_amax (16-byte loads, integer max over the bf16 magnitudes, one atomic max per block) and
// k_fp8_cast (16-byte loads, v_cvt_pk_fp8_f32 after the clamp, 8-byte stores; its last block writes {s, 1/s}
// and re-arms the workspace).  Both walk a by-value table of tensors, 8192 values per block.
#include "pde_act.h"
#include "pde_bf16.h"
#include "pde_fp8.h"
#include "pde_hip.h"
#include "pde_lds.h"

namespace {

using namespace pde_lds;

// ------------------------------------------------------------------------------------------ quantiser
constexpr int QT = 256, QIT = 4, QVEC = QT * QIT;      // 16-byte vectors (8 values each) per block

struct QEnt {
  const uint4* src;
  uint2* dst;
  float* scale;
  uint32_t n8;      // 16-byte vectors
  uint32_t blk0;    // first block of this tensor
};
struct QTab {
  QEnt e[PDE_FP8_MAX_TENSORS];
  uint32_t* work;   // {amax bits, finished blocks} per entry
  int n;
};

__device__ __forceinline__ int q_find(const QTab& t, uint32_t b) {
  int i = 0;
  while (i + 1 < t.n && t.e[i + 1].blk0 <= b) ++i;
  return i;
}

__device__ __forceinline__ uint32_t amax2(uint32_t m, uint32_t w) {
  return max(m, max(w & 0x7fffu, (w >> 16) & 0x7fffu));
}

__global__ __launch_bounds__(QT) void k_fp8_amax(QTab t) {
  __shared__ uint32_t sh[QT / 64];
  const int i = q_find(t, blockIdx.x);
  const uint4* src = t.e[i].src;
  const uint32_t n8 = t.e[i].n8, base = (blockIdx.x - t.e[i].blk0) * QVEC + threadIdx.x;
  uint4 v[QIT];
#pragma unroll
  for (int it = 0; it < QIT; ++it) {
    const uint32_t idx = base + it * QT;
    v[it] = idx < n8 ? src[idx] : make_uint4(0, 0, 0, 0);
  }
  uint32_t m = 0;                                      // max of the bf16 magnitudes' bit patterns
#pragma unroll
  for (int it = 0; it < QIT; ++it) m = amax2(amax2(amax2(amax2(m, v[it].x), v[it].y), v[it].z), v[it].w);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, o, 64));
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int q = 1; q < QT / 64; ++q) m = max(m, sh[q]);
    if (m) atomicMax(t.work + 2 * i, m << 16);         // the fp32 bits of a non-negative bf16
  }
}

__device__ __forceinline__ float q_clamp(float v) { return __builtin_amdgcn_fmed3f(v, -448.f, 448.f); }

__global__ __launch_bounds__(QT) void k_fp8_cast(QTab t) {
  const int i = q_find(t, blockIdx.x);
  const uint4* src = t.e[i].src;
  uint2* dst = t.e[i].dst;
  const uint32_t n8 = t.e[i].n8, base = (blockIdx.x - t.e[i].blk0) * QVEC + threadIdx.x;
  uint4 v[QIT];
#pragma unroll
  for (int it = 0; it < QIT; ++it) {
    const uint32_t idx = base + it * QT;
    v[it] = idx < n8 ? src[idx] : make_uint4(0, 0, 0, 0);
  }
  // s = 2^k: amax = m * 2^e with m in [1, 2); 448 = 1.75 * 2^8, so k = 8 - e when m <= 1.75, else 7 - e
  const uint32_t ab = t.work[2 * i];
  int k = ((ab & 0x7fffffu) <= 0x600000u ? 8 : 7) - ((int)(ab >> 23) - 127);
  k = ab == 0 ? 0 : min(k, 126);
  const float s = __uint_as_float((uint32_t)(k + 127) << 23), inv = __uint_as_float((uint32_t)(127 - k) << 23);
#pragma unroll
  for (int it = 0; it < QIT; ++it) {
    const uint32_t idx = base + it * QT;
    if (idx < n8) {
      float f[8];
      unpack8(v[it], f);
#pragma unroll
      for (int e = 0; e < 8; ++e) f[e] = q_clamp(f[e] * s);
      int w0 = 0, w1 = 0;
      w0 = __builtin_amdgcn_cvt_pk_fp8_f32(f[0], f[1], w0, false);
      w0 = __builtin_amdgcn_cvt_pk_fp8_f32(f[2], f[3], w0, true);
      w1 = __builtin_amdgcn_cvt_pk_fp8_f32(f[4], f[5], w1, false);
      w1 = __builtin_amdgcn_cvt_pk_fp8_f32(f[6], f[7], w1, true);
      dst[idx] = make_uint2((uint32_t)w0, (uint32_t)w1);
    }
  }
  // every thread of this block has consumed the amax word; the block that arrives last knows every block has
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t nb = (n8 + QVEC - 1) / QVEC;
    __threadfence();
    if (atomicAdd(t.work + 2 * i + 1, 1u) == nb - 1) {
      t.e[i].scale[0] = s;
      t.e[i].scale[1] = inv;
      t.work[2 * i] = 0;
      t.work[2 * i + 1] = 0;
    }
  }
}

// ------------------------------------------------------------------------------------------ GEMM
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x8 __attribute__((ext_vector_type(8)));

constexpr int BM = 256, BN = 128, WM = 4, WN = 2, TM = 2, TN = 2, NW = WM * WN, NT = 64 * NW, NST = 3;
constexpr int XBYTES = BM * 128, WBYTES = BN * 128, STAGE = XBYTES + WBYTES;
constexpr int XG = BM / 8 / NW, WG = BN / 8 / NW, LPS = XG + WG;     // LDS-DMA wave-instructions per wave and slice
constexpr int RS = BN * 2 + 16;                                      // epilogue tile row stride (bytes)
static_assert(BM == WM * TM * 32 && BN == WN * TN * 32, "wave tiles cover the block tile");
static_assert(NW % 2 == 0, "a wave's 8-row groups share one parity (one chunk map per lane)");
static_assert(BM * RS <= NST * STAGE && NST * STAGE <= 160 * 1024, "LDS");

struct Fp8GemmArgs {
  const void* X;
  const void* W;
  const float* xs;       // {s, 1/s} of x
  const float* ws;       // {s, 1/s} of w
  bf16_t* Y;
  bf16_t* Y2;            // GELU: gelu'(pre) (Y gets gelu(pre))
  const bf16_t* bias;    // [N] or null
  uint32_t x_bytes, w_bytes;
  int M, N, K, mtiles, ntiles;
};

template <int OFF>
__device__ __forceinline__ i32x4 rd128(uint32_t addr) {
  i32x4 v;
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF));
  return v;
}
template <int N>
__device__ __forceinline__ void wait_lgkm() {
  __builtin_amdgcn_sched_barrier(0);       // the earlier step's MFMAs stay above the wait ...
  asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(N) : "memory");
  __builtin_amdgcn_sched_barrier(0);       // ... and the MFMAs that consume asm-loaded fragments below it
}
__device__ __forceinline__ i32x8 cat(i32x4 a, i32x4 b) { return __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7); }

template <bool GELU>
__global__ __launch_bounds__(NT, 1) void k_gemm_fp8(Fp8GemmArgs a) {
  __shared__ __attribute__((aligned(1024))) char smem[NST * STAGE];   // the ^ 16 of the lane bases needs bit 4 clear

  const int t = threadIdx.x, l = t & 63, lr = l & 31, lh = l >> 5;
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);   // wave-uniform: scalar addresses
  const int wm = w / WN, wn = w % WN;
  const int id = xcd_remap(blockIdx.x, gridDim.x);
  constexpr int G = 8;                                    // row tiles per group: an XCD's blocks share operand rows
  const int grp = id / (G * a.ntiles), r2 = id - grp * (G * a.ntiles);
  const int gsz = min(G, a.mtiles - grp * G);
  const int m0 = (grp * G + r2 % gsz) * BM, n0 = (r2 / gsz) * BN;

  // ---- LDS-DMA source offsets (bytes) of this wave's 8-row groups at slice 0; rows past M / N stay out of range
  const int lrow = glds_row(l), kc = 16 * glds_chunk(l, w & 1);
  uint32_t xoff[XG], woff[WG];
#pragma unroll
  for (int u = 0; u < XG; ++u) {
    const int m = m0 + 8 * (NW * u + w) + lrow;
    xoff[u] = m < a.M ? (uint32_t)m * (uint32_t)a.K + kc : kOOB;
  }
#pragma unroll
  for (int v = 0; v < WG; ++v) {
    const int n = n0 + 8 * (NW * v + w) + lrow;
    woff[v] = n < a.N ? (uint32_t)n * (uint32_t)a.K + kc : kOOB;
  }
  const rsrc_t xr = make_rsrc(a.X, a.x_bytes), wr = make_rsrc(a.W, a.w_bytes);
  auto issue = [&](int slice, int buf) {
    const char* Xs = smem + buf * STAGE;
    const uint32_t k0 = 128u * slice;
    const bool in = (int)(k0 + kc) < a.K;                 // past K (the half slice of K % 128 == 64): zeros
#pragma unroll
    for (int u = 0; u < XG; ++u) glds16(xr, Xs + (NW * u + w) * 1024, in ? xoff[u] + k0 : kOOB);
#pragma unroll
    for (int v = 0; v < WG; ++v) glds16(wr, Xs + XBYTES + (NW * v + w) * 1024, in ? woff[v] + k0 : kOOB);
  };

  // ---- fragment lane bases: row (wave's first row + l & 31), chunks 2 lh and 2 lh + 1 of step 0 (the second is
  // the first with bit 4 flipped); step 1 is +512 and the next 32 rows +4096, both immediates
  const uint32_t lds0 = (uint32_t)(uintptr_t)(lds_char*)smem;
  const uint32_t xb = lds0 + toff(wm * 64 + lr, 2 * lh), wb = lds0 + XBYTES + toff(wn * 64 + lr, 2 * lh);

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = f32x16{0.f};

  const int nk = (a.K + 127) >> 7;
  issue(0, 0);
  issue(1, 1);
  int buf = 0;
  for (int s = 0; s < nk; ++s) {
    wait_vm<LPS>();
    __builtin_amdgcn_s_barrier();
    issue(s + 2, buf >= 1 ? buf - 1 : NST - 1);           // (s + 2) % 3: the buffer of slice s - 1
    const uint32_t x0 = xb + buf * STAGE, x1 = x0 ^ 16u, w0 = wb + buf * STAGE, w1 = w0 ^ 16u;
    i32x4 fx[2][TM][2], fw[2][TN][2];
    fx[0][0][0] = rd128<0>(x0);       fx[0][0][1] = rd128<0>(x1);
    fx[0][1][0] = rd128<4096>(x0);    fx[0][1][1] = rd128<4096>(x1);
    fw[0][0][0] = rd128<0>(w0);       fw[0][0][1] = rd128<0>(w1);
    fw[0][1][0] = rd128<4096>(w0);    fw[0][1][1] = rd128<4096>(w1);
    fx[1][0][0] = rd128<512>(x0);     fx[1][0][1] = rd128<512>(x1);
    fx[1][1][0] = rd128<4608>(x0);    fx[1][1][1] = rd128<4608>(x1);
    fw[1][0][0] = rd128<512>(w0);     fw[1][0][1] = rd128<512>(w1);
    fw[1][1][0] = rd128<4608>(w0);    fw[1][1][1] = rd128<4608>(w1);
    wait_lgkm<8>();                                       // step 0's fragments (LDS reads return in order)
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      if (ks == 1) wait_lgkm<0>();
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(
              cat(fw[ks][j][0], fw[ks][j][1]), cat(fx[ks][i][0], fx[ks][i][1]), acc[i][j], 0, 0, 0, 0x7f7f7f7f, 0,
              0x7f7f7f7f);
    }
    buf = buf == NST - 1 ? 0 : buf + 1;
  }
  wait_vm<0>();            // the zero-fill loads of the slices past K
  __syncthreads();         // every wave is done with the stage buffers: the LDS tile may be written

  // ---- epilogue: acc * (1/sx)(1/sw) + bias -> bf16 LDS tile -> 16-byte row stores
  const float sc = a.xs[1] * a.ws[1];
#pragma unroll
  for (int j = 0; j < TN; ++j)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int nl = wn * 64 + 32 * j + 8 * g + 4 * lh;
      float bv[4] = {0.f, 0.f, 0.f, 0.f};
      if (a.bias != nullptr && n0 + nl < a.N) unpack4(*reinterpret_cast<const uint2*>(a.bias + n0 + nl), bv);
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        const int ml = wm * 64 + 32 * i + lr;
        const float v[4] = {acc[i][j][4 * g] * sc + bv[0], acc[i][j][4 * g + 1] * sc + bv[1],
                            acc[i][j][4 * g + 2] * sc + bv[2], acc[i][j][4 * g + 3] * sc + bv[3]};
        *reinterpret_cast<uint2*>(smem + ml * RS + nl * 2) = pack4(v);
      }
    }
  __syncthreads();
  constexpr int CPR = BN / 8;                              // 16-byte chunks per tile row
#pragma unroll 4
  for (int c = t; c < BM * CPR; c += NT) {
    const int row = c / CPR, cc = c - row * CPR;
    const int m = m0 + row, n = n0 + 8 * cc;
    if (m < a.M && n < a.N) {
      const uint4 v = *reinterpret_cast<const uint4*>(smem + row * RS + cc * 16);
      const size_t o = (size_t)m * a.N + n;
      if constexpr (!GELU) {
        *reinterpret_cast<uint4*>(a.Y + o) = v;
      } else {                                             // Y = gelu(pre), Y2 = gelu'(pre) (the backward's factor)
        const uint32_t pw[4] = {v.x, v.y, v.z, v.w};
        uint32_t ya[4], da[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          pde_f2 d;
          const pde_f2 y = gelu2_d(pde_f2{bf_lo(pw[e]), bf_hi(pw[e])}, d);
          ya[e] = pack_bf2(y.x, y.y);
          da[e] = pack_bf2(d.x, d.y);
        }
        *reinterpret_cast<uint4*>(a.Y + o) = make_uint4(ya[0], ya[1], ya[2], ya[3]);
        *reinterpret_cast<uint4*>(a.Y2 + o) = make_uint4(da[0], da[1], da[2], da[3]);
      }
    }
  }
}

}  // namespace

extern "C" hipError_t pde_fp8_quantize(const PdeFp8Tensor* tensors, int count, uint32_t* work, hipStream_t st) {
  for (int c0 = 0; c0 < count; c0 += PDE_FP8_MAX_TENSORS) {
    QTab t;
    t.n = count - c0 < PDE_FP8_MAX_TENSORS ? count - c0 : PDE_FP8_MAX_TENSORS;
    t.work = work + 2 * c0;
    uint64_t blocks = 0;
    for (int i = 0; i < t.n; ++i) {
      const PdeFp8Tensor& s = tensors[c0 + i];
      if (s.n <= 0 || s.n % 16 != 0 || s.n / 8 > 0x7fffffffLL) return hipErrorInvalidValue;
      t.e[i].src = static_cast<const uint4*>(s.src);
      t.e[i].dst = static_cast<uint2*>(s.dst);
      t.e[i].scale = s.scale;
      t.e[i].n8 = (uint32_t)(s.n / 8);
      t.e[i].blk0 = (uint32_t)blocks;
      blocks += (t.e[i].n8 + QVEC - 1) / QVEC;
    }
    if (blocks > 0x7fffffffULL) return hipErrorInvalidValue;
    k_fp8_amax<<<dim3((unsigned)blocks), dim3(QT), 0, st>>>(t);
    PDE_HIP_CHECK(hipGetLastError());
    k_fp8_cast<<<dim3((unsigned)blocks), dim3(QT), 0, st>>>(t);
    PDE_HIP_CHECK(hipGetLastError());
  }
  return hipSuccess;
}

extern "C" void pde_gemm_fp8_tile(int* bm, int* bn) {
  *bm = BM;
  *bn = BN;
}

extern "C" hipError_t pde_gemm_fp8(const void* xq, const void* wq, const float* xs, const float* ws, void* y, void* y2,
                                   const void* bias, int M, int N, int K, hipStream_t st) {
  if (M <= 0 || N <= 0 || K <= 0 || N % 8 != 0 || K % 64 != 0) return hipErrorInvalidValue;
  // 32-bit buffer offsets: every row the tiles may name, in or out of range, stays below the out-of-range mark
  if (((int64_t)M + BM) * K >= (int64_t)kOOB || ((int64_t)N + BN) * K >= (int64_t)kOOB) return hipErrorInvalidValue;
  Fp8GemmArgs a;
  a.X = xq;
  a.W = wq;
  a.xs = xs;
  a.ws = ws;
  a.Y = static_cast<bf16_t*>(y);
  a.Y2 = static_cast<bf16_t*>(y2);
  a.bias = static_cast<const bf16_t*>(bias);
  a.x_bytes = (uint32_t)((int64_t)M * K);
  a.w_bytes = (uint32_t)((int64_t)N * K);
  a.M = M;
  a.N = N;
  a.K = K;
  a.mtiles = (M + BM - 1) / BM;
  a.ntiles = (N + BN - 1) / BN;
  const dim3 grid((unsigned)(a.mtiles * a.ntiles)), block(NT);
  if (y2 != nullptr) k_gemm_fp8<true><<<grid, block, 0, st>>>(a);
  else k_gemm_fp8<false><<<grid, block, 0, st>>>(a);
  return hipGetLastError();
}
