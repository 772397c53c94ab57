// The decode attention of the GPT-2 decode step: device code shared by two translation units.
// decode.hip instantiates the plain kernel (k_dec_attn<>), decode_beam.hip the one that reads the keys through a
// beam search's ancestor table (k_dec_attn<PdeBeamTable>).  As with the sampler (decode_sample.h) the extra
// arguments travel in a by-value struct that only the second instantiation takes, and the two are compiled apart,
// so the plain kernel keeps its argument layout and its instruction stream.  Include inside the unit's anonymous
// namespace, after pde_hip.h, pde_bf16.h and pde_decode.h.
#pragma once

constexpr int DC_CH = 128;      // keys per block
constexpr int DC_PART = 66;     // floats per partial: max, sum, 64 outputs

// the table half that the step at hand reads, row b (PdeBeamTable in pde_decode.h)
__device__ __forceinline__ const unsigned char* beam_anc(const int* state, int b, const PdeBeamTable& t) {
  return t.anc + ((size_t)(state[PDE_DS_STEP] & 1) * PDE_DS_MAX_ROWS + b) * t.stride;
}

// grid (chunks of Tmax, H, B), block 256 (b is a grid index of its own, so the row's state words can be
// loaded before any other arithmetic).  Scores: thread pair (2j, 2j + 1) holds the two 32-dim halves of
// key c * 128 + j.  Outputs: thread (kg = tid >> 3, dg = tid & 7) holds dims 8 dg.. of keys kg + 32 i.  Every
// K / V row comes straight from global memory to VGPRs, all loads issued before the first use.  Row p (the
// new token; p = p_b, the position of batch row b) is taken from the c_attn row and written to the cache by
// the block whose chunk holds p.  Blocks of chunks past p return: the grid is sized by Tmax.
// With a table (`Beam` = PdeBeamTable) key j < p of row b is read from the cache row anc[b][j] instead of b; an
// entry that names no row of the cache reads row b.  Row p is still written to row b, and everything after the
// loads is the same code, so the output equals the plain kernel's on a cache gathered through the table bit for bit.
template <typename... Beam>
__global__ __launch_bounds__(256) void k_dec_attn(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ cache,
                                                  const int* __restrict__ state, float* __restrict__ part, int B, int H,
                                                  int Tmax, int nch, float scale, Beam... beam) {
  constexpr bool BEAM = sizeof...(Beam) == 1;
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
  [[maybe_unused]] const unsigned char* anc = nullptr;
  if constexpr (BEAM) anc = beam_anc(state, b, beam...);

  const int j1 = c * DC_CH + (tid >> 1), half = tid & 1;
  uint4 kv[4], vv[4], qv[4];
  {
    const bf16_t* Ks = Kc;
    if constexpr (BEAM) {
      if (j1 < p) {
        const int a = anc[j1];
        Ks = cache + (size_t)((a < B ? a : b) * H + h) * Tmax * 64;
      }
    }
    const uint4* src = reinterpret_cast<const uint4*>(j1 == p ? row + C + half * 32 : Ks + (size_t)j1 * 64 + half * 32);
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
    if (j < p) {
      const bf16_t* Vs = Vc;
      if constexpr (BEAM) {
        const int a = anc[j];
        Vs = cache + ((size_t)B * H + (size_t)((a < B ? a : b) * H + h)) * Tmax * 64;
      }
      vv[i] = *reinterpret_cast<const uint4*>(Vs + (size_t)j * 64 + dg * 8);
    } else if (j == p) {
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

// the two launches over checked arguments
template <typename... Beam>
hipError_t dec_attn_launch(const void* qkv, void* cache, const int* state, float* part, void* out, int B, int H,
                           int Tmax, float scale, hipStream_t st, Beam... beam) {
  const int nch = (Tmax + DC_CH - 1) / DC_CH;
  hipLaunchKernelGGL((k_dec_attn<Beam...>), dim3(nch, H, B), dim3(256), 0, st, (const bf16_t*)qkv, (bf16_t*)cache,
                     state, part, B, H, Tmax, nch, scale, beam...);
  PDE_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(k_dec_attn_combine, dim3(H, B), dim3(64), 0, st, (const float*)part, state, (bf16_t*)out, H, Tmax,
                     nch);
  return hipGetLastError();
}
