// MXFP8 forward path (pde_mxfp8.h holds the numeric definition): the block-scaled GEMM k_gemm_mxfp8 and the
// quantisers that need no amax pass, k_mx_quant and k_ln_fwd_mx.
//
// k_gemm_mxfp8 keeps k_gemm_fp8's measured skeleton (gemm_fp8.hip): block tile 256 x 128, 8 waves as 4 x 2, each
// wave 2 x 2 accumulators of v_mfma_scale_f32_32x32x64_f8f6f4, K in 128-byte slices through a ring of three LDS
// stages filled by LDS-DMA, two 64-deep MFMA steps per slice, XCD-aware tile order.  The operand layout differs
// in one point, see "Lane-to-scale map" below.
//
// The path of the scales (what is new).  A 128-byte slice is four MX blocks per row, and K % 128 == 0, so the
// scale bytes of one row and one slice are one aligned dword of the [rows][K / 32] scale matrix.  They travel
// through LDS: every stage is widened by a [512 rows][4 B] image (2 KB; rows 0..255 x, 256..383 w, the rest
// padding), filled by the 4-byte LDS-DMA form -- one wave-instruction per wave and slice covers 64 rows (waves
// 0..3: x rows, 4..5: w rows, 6..7: an out-of-range offset into the padding, so every wave issues the same
// seven loads per slice and the vmcnt allowance stays one constant).  Three stages of 50 KB fit in 160 KB.  A lane
// reads the dwords of its two x rows and two w rows with ds_read_b32 (issued ahead of the fragment reads, so the
// lgkmcnt(8) that releases step 0 covers them) and needs byte 2 * step + (l >> 5) of each.  The byte select of the
// instruction's scale operands is an immediate, the same for all lanes; it stays 0, the form gemm_fp8.hip's unit
// scales run with, and the lane shifts its dword right by 8 * (l >> 5) for step 0 and by 16 more for step 1:
// eight v_lshrrev per slice and wave beside eight 16-pass MFMAs.  The loop holds no store and no vmcnt(0);
// slices past K and rows past M / N carry the out-of-range offset, which fills zeros (zero data under a 2^-127
// scale: a zero term).
//
// Lane-to-scale map, as found on the hardware (a one-hot operand under coded scales; tests/test_mxfp8_gpu.py holds
// it, its operands giving every block a scale that differs from its row neighbours' and from the same block one row
// down).  The scale of lane l does NOT apply to the 32 K values lane l supplies.  Of a 64-deep step the instruction
// takes K 16 h .. 16 h + 15 from registers 0..3 and K 32 + 16 h .. 32 + 16 h + 15 from registers 4..7 of the lanes
// with l >> 5 == h, and it applies the scale byte of lane r (l < 32) to K 0..31 of row r and that of lane 32 + r to
// K 32..63.  gemm_fp8.hip's layout (32 consecutive bytes per lane) is a K permutation that both operands share,
// which unit scales cannot see; with block scales it pairs the halves of two blocks under each scale.  So here lane l
// reads the 16-byte chunks h and 2 + h of the step (the second is the first with address bit 5 flipped), which puts
// the operands in the instruction's own K order, and it supplies the scale of block 2 * step + h of row l & 31.
//
// Epilogue: bias in fp32, one rounding to bf16 into an LDS tile, 16-byte row stores; with GELU the store loop
// applies gelu2_d to the bf16-rounded pre-activation as gemm.hip does, and with AMX it also emits gelu(pre) as an
// MX tensor: a thread holds 8 consecutive values, four adjacent lanes one 32-block of a row, so the block amax is
// a two-step DPP quad exchange over the bf16 magnitude bits; each thread stores 8 e4m3 bytes and the first of
// the four the scale byte.  N % 32 == 0 makes a quad all in or all out of range.
//
// k_mx_quant: one pass, a 16-byte load per lane, the same quad exchange, v_cvt_pk_fp8_f32 after the clamp, an
// 8-byte store per lane and one scale byte per block, over a by-value table of tensors.
// k_ln_fwd_mx: transformer.hip's k_ln_fwd, statement for statement, plus the MX output: a lane holds 4 consecutive
// columns per chunk, a block is 8 consecutive lanes, the amax of the bf16-rounded outputs is a three-step DPP
// exchange (two quad permutes and a half-row mirror).  It lives here, not in transformer.hip, so the existing
// instantiations are not recompiled and this file's no-packed-fp32 flag covers it.  Its S, Y, mean and rstd must
// be k_ln_fwd's bit for bit, so the roundings that k_ln_fwd's sixteen instantiations all compile to are written
// out here instead of being left to fp contraction (which fused the first chunk's d * d into the variance sum
// in this file and not in that one): contraction is off in the kernel and its helper, so d * d and
// d * (1 / keep) are rounded products, and the output is one explicit fma of the rounded (v - mean) * rstd with
// gamma and beta.
#include "pde_act.h"
#include "pde_bf16.h"
#include "pde_hip.h"
#include "pde_lds.h"
#include "pde_mxfp8.h"
#include "pde_rng.h"

namespace {

using namespace pde_lds;

// ------------------------------------------------------------------------------------------ block scale
__device__ __forceinline__ uint32_t amax2(uint32_t m, uint32_t w) {      // max with both bf16 magnitudes of w
  return max(m, max(w & 0x7fffu, (w >> 16) & 0x7fffu));
}
template <int CTRL>
__device__ __forceinline__ uint32_t dpp_max(uint32_t m) {
  return max(m, (uint32_t)__builtin_amdgcn_mov_dpp((int)m, CTRL, 0xf, 0xf, true));
}
__device__ __forceinline__ uint32_t quad_max(uint32_t m) {               // lanes ^ 1, lanes ^ 2
  return dpp_max<0x4E>(dpp_max<0xB1>(m));
}
// k of a block from the bf16 magnitude bits of its amax = m * 2^e: 448 = 1.75 * 2^8, so 8 - e when m <= 1.75,
// else 7 - e (a bf16 subnormal has e <= -127: past the clamp either way)
__device__ __forceinline__ int mx_k(uint32_t ab) {
  const int k = ((ab & 0x7fu) <= 0x60u ? 8 : 7) - ((int)(ab >> 7) - 127);
  return ab == 0 ? 0 : min(k, 127);
}
__device__ __forceinline__ float pow2f(int k) { return __uint_as_float((uint32_t)(k + 127) << 23); }   // -126..127
__device__ __forceinline__ float q_clamp(float v) { return __builtin_amdgcn_fmed3f(v, -448.f, 448.f); }
__device__ __forceinline__ uint32_t cast4(const float* f, float s) {
  int w = 0;
  w = __builtin_amdgcn_cvt_pk_fp8_f32(q_clamp(f[0] * s), q_clamp(f[1] * s), w, false);
  w = __builtin_amdgcn_cvt_pk_fp8_f32(q_clamp(f[2] * s), q_clamp(f[3] * s), w, true);
  return (uint32_t)w;
}
// 8 bf16 values of one quarter block -> 8 e4m3 bytes and the block's k (the four lanes of a quad hold a block)
__device__ __forceinline__ uint2 mx_quad8(uint4 v, int& k) {
  k = mx_k(quad_max(amax2(amax2(amax2(amax2(0u, v.x), v.y), v.z), v.w)));
  const float s = pow2f(k);
  float f[8];
  unpack8(v, f);
  return make_uint2(cast4(f, s), cast4(f + 4, s));
}

// ------------------------------------------------------------------------------------------ quantiser
constexpr int QT = 256, QIT = 4, QVEC = QT * QIT;      // 16-byte vectors (8 values each) per block

struct MxEnt {
  const uint4* src;
  uint2* dst;
  uint8_t* scale;
  uint32_t n8;      // 16-byte vectors (a multiple of 4: whole blocks)
  uint32_t blk0;    // first thread block of this tensor
};
struct MxTab {
  MxEnt e[PDE_MX_MAX_TENSORS];
  int n;
};

__global__ __launch_bounds__(QT) void k_mx_quant(MxTab t) {
  int i = 0;
  while (i + 1 < t.n && t.e[i + 1].blk0 <= blockIdx.x) ++i;
  const uint4* src = t.e[i].src;
  uint2* dst = t.e[i].dst;
  uint8_t* sc = t.e[i].scale;
  const uint32_t n8 = t.e[i].n8, base = (blockIdx.x - t.e[i].blk0) * QVEC + threadIdx.x;
  uint4 v[QIT];
#pragma unroll
  for (int it = 0; it < QIT; ++it) {
    const uint32_t idx = base + it * QT;
    v[it] = idx < n8 ? src[idx] : make_uint4(0, 0, 0, 0);
  }
#pragma unroll
  for (int it = 0; it < QIT; ++it) {
    const uint32_t idx = base + it * QT;               // idx & ~3 .. | 3 are one quad and one block: in or out together
    int k;
    const uint2 q = mx_quad8(v[it], k);
    if (idx < n8) {
      dst[idx] = q;
      if ((idx & 3u) == 0) sc[idx >> 2] = (uint8_t)(127 - k);
    }
  }
}

// ------------------------------------------------------------------------------------------ LayerNorm
struct DropSite {                                      // transformer.hip's: keep flags of 4 consecutive elements
  uint32_t st[4];
  uint32_t site, thr;
  float inv_keep;
  __device__ __forceinline__ explicit DropSite(const PdeDrop& d) : site(d.site), thr(d.thr), inv_keep(d.inv_keep) {
#pragma unroll
    for (int i = 0; i < 4; ++i) st[i] = d.rng[i];
  }
  __device__ __forceinline__ void apply(uint64_t group, float (&v)[4]) const {
#pragma clang fp contract(off)
    uint32_t w[4];
    pde_rng::group_words(st, site, group, w);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = w[e] >= thr ? v[e] * inv_keep : 0.f;
  }
};

template <int NCH, bool DROP>
__global__ __launch_bounds__(256) void k_ln_fwd_mx(const bf16_t* __restrict__ X, const bf16_t* __restrict__ D,
                                                   bf16_t* __restrict__ S, const bf16_t* __restrict__ G,
                                                   const bf16_t* __restrict__ Bt, bf16_t* __restrict__ Y,
                                                   float* __restrict__ mean_out, float* __restrict__ rstd_out,
                                                   uint32_t* __restrict__ Q, uint8_t* __restrict__ E, int N, int C,
                                                   float eps, PdeDrop drop) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= N) return;  // wave-uniform
  const int nc = C >> 2;
  const uint2* xr = reinterpret_cast<const uint2*>(X + (size_t)row * C);
  const uint2* g4 = reinterpret_cast<const uint2*>(G);
  const uint2* b4 = reinterpret_cast<const uint2*>(Bt);
  float v[NCH][4], gg[NCH][4], bb[NCH][4];
  uint2 wx[NCH], wd[NCH], wg[NCH], wb[NCH];
  const uint2* dr = D ? reinterpret_cast<const uint2*>(D + (size_t)row * C) : nullptr;
#pragma unroll
  for (int j = 0; j < NCH; ++j) {  // issue every load first (clamped index, no branch)
    const int c = min(lane + 64 * j, nc - 1);
    wx[j] = xr[c];
    wd[j] = dr ? dr[c] : make_uint2(0u, 0u);
    wg[j] = g4[c];
    wb[j] = b4[c];
  }
  if (D) {  // residual add, rounded to bf16 (the stored residual stream is bf16)
    uint2* sr = reinterpret_cast<uint2*>(S + (size_t)row * C);
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
      float a[4], b[4];
      unpack4(wx[j], a);
      unpack4(wd[j], b);
      if constexpr (DROP) DropSite(drop).apply((uint64_t)row * nc + min(lane + 64 * j, nc - 1), b);
#pragma unroll
      for (int e = 0; e < 4; ++e) a[e] += b[e];
      wx[j] = pack4(a);
      if (lane + 64 * j < nc) sr[lane + 64 * j] = wx[j];
    }
  }
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < NCH; ++j) {
    const bool ok = lane + 64 * j < nc;
    unpack4(wx[j], v[j]);
#pragma unroll
    for (int e = 0; e < 4; ++e) s += ok ? v[j][e] : 0.f;
  }
  const float mean = wave_sum(s) / (float)C;
  float q = 0.f;
#pragma unroll
  for (int j = 0; j < NCH; ++j) {
    const bool ok = lane + 64 * j < nc;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float d = v[j][e] - mean;
      q += ok ? d * d : 0.f;
    }
  }
  const float rstd = rsqrtf(wave_sum(q) / (float)C + eps);
  uint2* yr = reinterpret_cast<uint2*>(Y + (size_t)row * C);
  uint32_t* qr = Q + (size_t)row * nc;
  uint8_t* er = E + (size_t)row * (C >> 5);
#pragma unroll
  for (int j = 0; j < NCH; ++j) {
    const int c = lane + 64 * j;
    unpack4(wg[j], gg[j]);
    unpack4(wb[j], bb[j]);
    float o[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = __builtin_fmaf((v[j][e] - mean) * rstd, gg[j][e], bb[j][e]);
    const uint2 yw = pack4(o);
    // the block of columns 32 b .. 32 b + 31 is the 8 lanes c = 8 b .. 8 b + 7; nc % 8 == 0, so they are in or
    // out of range together and the exchange runs with every lane active
    const int k = mx_k(dpp_max<0x141>(quad_max(amax2(amax2(0u, yw.x), yw.y))));
    unpack4(yw, o);
    const uint32_t qw = cast4(o, pow2f(k));
    if (c < nc) {
      yr[c] = yw;
      qr[c] = qw;
      if ((lane & 7) == 0) er[c >> 3] = (uint8_t)(127 - k);
    }
  }
  if (lane == 0) {
    mean_out[row] = mean;
    rstd_out[row] = rstd;
  }
}

// ------------------------------------------------------------------------------------------ GEMM
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x8 __attribute__((ext_vector_type(8)));

constexpr int BM = 256, BN = 128, WM = 4, WN = 2, TM = 2, TN = 2, NW = WM * WN, NT = 64 * NW, NST = 3;
constexpr int XBYTES = BM * 128, WBYTES = BN * 128, SOFF = XBYTES + WBYTES, SBYTES = NW * 256, STAGE = SOFF + SBYTES;
constexpr int XG = BM / 8 / NW, WG = BN / 8 / NW, LPS = XG + WG + 1;  // LDS-DMA wave-instructions per wave and slice
constexpr int RS = BN * 2 + 16;                                      // epilogue tile row stride (bytes)
static_assert(BM == WM * TM * 32 && BN == WN * TN * 32, "wave tiles cover the block tile");
static_assert(NW % 2 == 0, "a wave's 8-row groups share one parity (one chunk map per lane)");
static_assert(BM + BN <= 64 * NW && BM % 64 == 0 && BN % 64 == 0, "one scale wave-instruction per 64 rows");
static_assert(STAGE % 1024 == 0, "the ^ 32 of the lane bases needs bit 5 of every stage base clear");
static_assert(BM * RS <= NST * STAGE && NST * STAGE <= 160 * 1024, "LDS");

struct MxGemmArgs {
  const void* X;
  const void* W;
  const void* XE;        // [M][K / 32] scale bytes
  const void* WE;        // [N][K / 32]
  bf16_t* Y;
  bf16_t* Y2;            // GELU: gelu'(pre) (Y gets gelu(pre))
  const bf16_t* bias;    // [N] or null
  uint2* AQ;             // AMX: Y as e4m3 bytes [M][N]
  uint8_t* AE;           //      and its scale bytes [M][N / 32]
  uint32_t x_bytes, w_bytes, xe_bytes, we_bytes;
  int M, N, K, mtiles, ntiles;
};

template <int OFF>
__device__ __forceinline__ i32x4 rd128(uint32_t addr) {
  i32x4 v;
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF));
  return v;
}
template <int OFF>
__device__ __forceinline__ uint32_t rd32(uint32_t addr) {
  uint32_t v;
  asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF));
  return v;
}
template <int N>
__device__ __forceinline__ void wait_lgkm() {
  __builtin_amdgcn_sched_barrier(0);       // the earlier step's MFMAs stay above the wait ...
  asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(N) : "memory");
  __builtin_amdgcn_sched_barrier(0);       // ... and the MFMAs that consume asm-loaded fragments below it
}
__device__ __forceinline__ i32x8 cat(i32x4 a, i32x4 b) { return __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7); }
// 4-byte LDS-DMA: lane l of the wave writes lds + 4 * l
__device__ __forceinline__ void glds4(rsrc_t r, const char* lds, uint32_t off) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (__attribute__((address_space(3))) void*)lds, 4, off, 0, 0, 0);
}

template <bool GELU, bool AMX>
__global__ __launch_bounds__(NT, 1) void k_gemm_mxfp8(MxGemmArgs a) {
  __shared__ __attribute__((aligned(1024))) char smem[NST * STAGE];

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
  // ---- this wave's scale rows: x rows 64 w + l (waves 0..3), w rows 64 (w - 4) + l (4..5), nothing (6..7)
  constexpr int SXW = BM / 64, SWW = BN / 64;
  const bool sx = w < SXW, sw = !sx && w < SXW + SWW;
  const int srow = sx ? m0 + 64 * w + l : n0 + 64 * (w - SXW) + l;
  const uint32_t soff = (sx && srow < a.M) || (sw && srow < a.N) ? (uint32_t)srow * (uint32_t)(a.K >> 5) : kOOB;
  const rsrc_t xr = make_rsrc(a.X, a.x_bytes), wr = make_rsrc(a.W, a.w_bytes);
  const rsrc_t sr = make_rsrc(sx ? a.XE : a.WE, sx ? a.xe_bytes : a.we_bytes);
  auto issue = [&](int slice, int buf) {
    const char* Xs = smem + buf * STAGE;
    const uint32_t k0 = 128u * slice;
    const bool in = (int)k0 < a.K;                        // past K: zeros into a buffer nobody reads
#pragma unroll
    for (int u = 0; u < XG; ++u) glds16(xr, Xs + (NW * u + w) * 1024, in ? xoff[u] + k0 : kOOB);
#pragma unroll
    for (int v = 0; v < WG; ++v) glds16(wr, Xs + XBYTES + (NW * v + w) * 1024, in ? woff[v] + k0 : kOOB);
    glds4(sr, Xs + SOFF + w * 256, in ? soff + 4u * slice : kOOB);
  };

  // ---- fragment lane bases: row (wave's first row + l & 31), chunks lh and 2 + lh of step 0 (the second is the
  // first with bit 5 flipped); step 1 is +512 and the next 32 rows +4096 (scale dwords: +128), all immediates
  const uint32_t lds0 = (uint32_t)(uintptr_t)(lds_char*)smem;
  const uint32_t xb = lds0 + toff(wm * 64 + lr, lh), wb = lds0 + XBYTES + toff(wn * 64 + lr, lh);
  const uint32_t xsb = lds0 + SOFF + 4 * (wm * 64 + lr), wsb = lds0 + SOFF + 4 * (BM + wn * 64 + lr);
  const uint32_t sh0 = 8u * lh, sh1 = sh0 + 16u;          // this lane's byte of a scale dword, per step

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = f32x16{0.f};

  const int nk = a.K >> 7;
  issue(0, 0);
  issue(1, 1);
  int buf = 0;
  for (int s = 0; s < nk; ++s) {
    wait_vm<LPS>();
    __builtin_amdgcn_s_barrier();
    issue(s + 2, buf >= 1 ? buf - 1 : NST - 1);           // (s + 2) % 3: the buffer of slice s - 1
    const uint32_t x0 = xb + buf * STAGE, x1 = x0 ^ 32u, w0 = wb + buf * STAGE, w1 = w0 ^ 32u;
    const uint32_t xs0 = xsb + buf * STAGE, ws0 = wsb + buf * STAGE;
    uint32_t ex[TM], ew[TN];
    i32x4 fx[2][TM][2], fw[2][TN][2];
    ex[0] = rd32<0>(xs0);             ex[1] = rd32<128>(xs0);
    ew[0] = rd32<0>(ws0);             ew[1] = rd32<128>(ws0);
    fx[0][0][0] = rd128<0>(x0);       fx[0][0][1] = rd128<0>(x1);
    fx[0][1][0] = rd128<4096>(x0);    fx[0][1][1] = rd128<4096>(x1);
    fw[0][0][0] = rd128<0>(w0);       fw[0][0][1] = rd128<0>(w1);
    fw[0][1][0] = rd128<4096>(w0);    fw[0][1][1] = rd128<4096>(w1);
    fx[1][0][0] = rd128<512>(x0);     fx[1][0][1] = rd128<512>(x1);
    fx[1][1][0] = rd128<4608>(x0);    fx[1][1][1] = rd128<4608>(x1);
    fw[1][0][0] = rd128<512>(w0);     fw[1][0][1] = rd128<512>(w1);
    fw[1][1][0] = rd128<4608>(w0);    fw[1][1][1] = rd128<4608>(w1);
    wait_lgkm<8>();                                       // the scales and step 0's fragments (LDS reads return in order)
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      if (ks == 1) wait_lgkm<0>();
      const uint32_t sh = ks ? sh1 : sh0;
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(
              cat(fw[ks][j][0], fw[ks][j][1]), cat(fx[ks][i][0], fx[ks][i][1]), acc[i][j], 0, 0, 0,
              (int)(ew[j] >> sh), 0, (int)(ex[i] >> sh));
    }
    buf = buf == NST - 1 ? 0 : buf + 1;
  }
  wait_vm<0>();            // the zero-fill loads of the slices past K
  __syncthreads();         // every wave is done with the stage buffers: the LDS tile may be written

  // ---- epilogue: acc + bias -> bf16 LDS tile -> 16-byte row stores
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
        const float v[4] = {acc[i][j][4 * g] + bv[0], acc[i][j][4 * g + 1] + bv[1], acc[i][j][4 * g + 2] + bv[2],
                            acc[i][j][4 * g + 3] + bv[3]};
        *reinterpret_cast<uint2*>(smem + ml * RS + nl * 2) = pack4(v);
      }
    }
  __syncthreads();
  constexpr int CPR = BN / 8;                              // 16-byte chunks per tile row
  static_assert(CPR % 4 == 0 && NT % CPR == 0, "a 32-column block is one aligned lane quad");
#pragma unroll 4
  for (int c = t; c < BM * CPR; c += NT) {
    const int row = c / CPR, cc = c - row * CPR;
    const int m = m0 + row, n = n0 + 8 * cc;
    if (m < a.M && n < a.N) {                              // AMX: N % 32 == 0, so the same for a whole quad
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
        if constexpr (AMX) {                               // the stored bf16 activation, quantised where it is held
          int k;
          a.AQ[o >> 3] = mx_quad8(make_uint4(ya[0], ya[1], ya[2], ya[3]), k);
          if ((cc & 3) == 0) a.AE[o >> 5] = (uint8_t)(127 - k);
        }
      }
    }
  }
}

}  // namespace

extern "C" hipError_t pde_mx_quantize(const PdeMxTensor* tensors, int count, hipStream_t st) {
  for (int c0 = 0; c0 < count; c0 += PDE_MX_MAX_TENSORS) {
    MxTab t;
    t.n = count - c0 < PDE_MX_MAX_TENSORS ? count - c0 : PDE_MX_MAX_TENSORS;
    uint64_t blocks = 0;
    for (int i = 0; i < t.n; ++i) {
      const PdeMxTensor& s = tensors[c0 + i];
      if (s.n <= 0 || s.n % 32 != 0 || s.n / 8 > 0x7fffffffLL) return hipErrorInvalidValue;
      t.e[i].src = static_cast<const uint4*>(s.src);
      t.e[i].dst = static_cast<uint2*>(s.dst);
      t.e[i].scale = s.scale;
      t.e[i].n8 = (uint32_t)(s.n / 8);
      t.e[i].blk0 = (uint32_t)blocks;
      blocks += (t.e[i].n8 + QVEC - 1) / QVEC;
    }
    if (blocks > 0x7fffffffULL) return hipErrorInvalidValue;
    k_mx_quant<<<dim3((unsigned)blocks), dim3(QT), 0, st>>>(t);
    PDE_HIP_CHECK(hipGetLastError());
  }
  return hipSuccess;
}

extern "C" hipError_t pde_gemm_mxfp8(const void* xq, const void* wq, const void* xe, const void* we, void* y, void* y2,
                                     const void* bias, void* aq, void* ae, int M, int N, int K, hipStream_t st) {
  if (M <= 0 || N <= 0 || K <= 0 || N % 8 != 0 || K % 128 != 0) return hipErrorInvalidValue;
  if ((aq != nullptr) != (ae != nullptr) || (aq != nullptr && (y2 == nullptr || N % 32 != 0))) return hipErrorInvalidValue;
  // 32-bit buffer offsets: every row the tiles may name, in or out of range, stays below the out-of-range mark
  if (((int64_t)M + BM) * K >= (int64_t)kOOB || ((int64_t)N + BN) * K >= (int64_t)kOOB) return hipErrorInvalidValue;
  MxGemmArgs a;
  a.X = xq;
  a.W = wq;
  a.XE = xe;
  a.WE = we;
  a.Y = static_cast<bf16_t*>(y);
  a.Y2 = static_cast<bf16_t*>(y2);
  a.bias = static_cast<const bf16_t*>(bias);
  a.AQ = static_cast<uint2*>(aq);
  a.AE = static_cast<uint8_t*>(ae);
  a.x_bytes = (uint32_t)((int64_t)M * K);
  a.w_bytes = (uint32_t)((int64_t)N * K);
  a.xe_bytes = a.x_bytes >> 5;
  a.we_bytes = a.w_bytes >> 5;
  a.M = M;
  a.N = N;
  a.K = K;
  a.mtiles = (M + BM - 1) / BM;
  a.ntiles = (N + BN - 1) / BN;
  const dim3 grid((unsigned)(a.mtiles * a.ntiles)), block(NT);
  if (aq != nullptr) k_gemm_mxfp8<true, true><<<grid, block, 0, st>>>(a);
  else if (y2 != nullptr) k_gemm_mxfp8<true, false><<<grid, block, 0, st>>>(a);
  else k_gemm_mxfp8<false, false><<<grid, block, 0, st>>>(a);
  return hipGetLastError();
}

extern "C" hipError_t pde_ln_fwd_mx(const void* X, const void* D, void* S, const void* G, const void* B, void* Y,
                                    float* mean, float* rstd, void* Q, void* E, int N, int C, float eps, PdeDrop drop,
                                    hipStream_t st) {
  if (N <= 0 || C <= 0 || C % 32 != 0) return hipErrorInvalidValue;
  const int nch = (C / 4 + 63) / 64;
  dim3 grid((N + 3) / 4);
  if (drop.rng && !D) return hipErrorInvalidValue;   // dropout acts on the residual summand
#define LNF(K)                                                                                                   \
  case K:                                                                                                        \
    if (drop.rng)                                                                                                \
      k_ln_fwd_mx<K, true><<<grid, dim3(256), 0, st>>>((const bf16_t*)X, (const bf16_t*)D, (bf16_t*)S,            \
                                                        (const bf16_t*)G, (const bf16_t*)B, (bf16_t*)Y, mean, rstd, \
                                                        (uint32_t*)Q, (uint8_t*)E, N, C, eps, drop);              \
    else                                                                                                         \
      k_ln_fwd_mx<K, false><<<grid, dim3(256), 0, st>>>((const bf16_t*)X, (const bf16_t*)D, (bf16_t*)S,           \
                                                         (const bf16_t*)G, (const bf16_t*)B, (bf16_t*)Y, mean, rstd, \
                                                         (uint32_t*)Q, (uint8_t*)E, N, C, eps, drop);             \
    break;
  switch (nch) {
    LNF(1) LNF(2) LNF(3) LNF(4) LNF(5) LNF(6) LNF(7) LNF(8)
    default: return hipErrorInvalidValue;
  }
#undef LNF
  return hipGetLastError();
}
