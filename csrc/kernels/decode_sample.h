// The device-side sampler of the GPT-2 decode step: device code, and the host-side checks and launch tail, shared by
// three translation units.
// decode.hip instantiates the plain sampler (k_sample<TOPP>), decode_proc.hip the one with the logit processors
// (k_sample<TOPP, PdeSampleProc>), decode_hist.hip the one with the history constraints on top of them
// (k_sample<TOPP, PdeSampleProc, PdeSampleHist>).  They are compiled apart on purpose: in one unit the extra instantiations
// changed how the compiler inlined and unswitched the nucleus stage of the plain top-p sampler, and a generation
// without processors is to run the instruction streams it ran before.  Include inside the unit's anonymous
// namespace, after pde_hip.h, pde_bf16.h, pde_decode.h and pde_rng.h.
#pragma once

// order-preserving 16-bit key of a bf16 value (-0 counts as +0, as in a float compare)
__device__ __forceinline__ uint32_t key16(uint32_t u) {
  u &= 0xffffu;
  if (u == 0x8000u) u = 0u;
  return (u & 0x8000u) ? (~u & 0xffffu) : (u | 0x8000u);
}
__device__ __forceinline__ uint32_t fkey32(float f) {
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t lo = __shfl_xor((uint32_t)v, o, 64), hi = __shfl_xor((uint32_t)(v >> 32), o, 64);
    const uint64_t t = ((uint64_t)hi << 32) | lo;
    v = t > v ? t : v;
  }
  return v;
}

// wave 0: the bin (counting from bin 255 down) that holds the k-th largest element, and k's rank inside it.
// hist: [4 waves][256 bins]; sel[0] = bin, sel[1] = rank left
__device__ __forceinline__ void radix_pick(const uint32_t (*hist)[256], uint32_t k, uint32_t* sel) {
  const int l = threadIdx.x;    // 0..63
  uint32_t cnt[4], c = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    cnt[q] = hist[0][4 * l + q] + hist[1][4 * l + q] + hist[2][4 * l + q] + hist[3][4 * l + q];
    c += cnt[q];
  }
  uint32_t s = c;               // suffix sum over lanes >= l
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t t = __shfl_down(s, o, 64);
    if (l + o < 64) s += t;
  }
  const uint32_t excl = s - c;
  if (excl < k && k <= s) {
    uint32_t rem = k - excl;
    int bin = 4 * l;
#pragma unroll
    for (int q = 3; q >= 0; --q) {
      if (rem <= cnt[q]) {
        bin = 4 * l + q;
        break;
      }
      rem -= cnt[q];
    }
    sel[0] = (uint32_t)bin;
    sel[1] = rem;
  }
}

// wave 0, weighted form: the bin (counting from bin 255 down) at which the running mass first reaches
// `target`, and the part of the target that bin has to cover.  whist: [4 waves][256 bins] of fixed-point mass;
// 1 <= target <= total mass, so exactly one lane writes.  wsel[0] = bin, wsel[1] = target left
__device__ __forceinline__ void radix_pick_mass(const uint64_t (*whist)[256], uint64_t target, uint64_t* wsel) {
  const int l = threadIdx.x;    // 0..63
  uint64_t cnt[4], c = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    cnt[q] = whist[0][4 * l + q] + whist[1][4 * l + q] + whist[2][4 * l + q] + whist[3][4 * l + q];
    c += cnt[q];
  }
  uint64_t s = c;               // suffix sum over lanes >= l
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t lo = __shfl_down((uint32_t)s, o, 64), hi = __shfl_down((uint32_t)(s >> 32), o, 64);
    if (l + o < 64) s += ((uint64_t)hi << 32) | lo;
  }
  const uint64_t excl = s - c;
  if (excl < target && target <= s) {
    uint64_t rem = target - excl;
    int bin = 4 * l;
#pragma unroll
    for (int q = 3; q >= 0; --q) {
      if (rem <= cnt[q]) {
        bin = 4 * l + q;
        break;
      }
      rem -= cnt[q];
    }
    wsel[0] = (uint64_t)bin;
    wsel[1] = rem;
  }
}

// 2^40 * exp(z - zmax), rounded: the mass of one candidate in fixed point (z <= zmax, so at most 2^40)
__device__ __forceinline__ uint64_t mass_fx(float z, float zmax) {
  return (uint64_t)rintf(expf(z - zmax) * 1099511627776.0f);
}

// The nucleus stage: among the candidates (key16 >= thr) the key of the largest logit value t with
// mass{logit >= t} >= top_p * total mass.  Same two 8-bit passes as the top-k select, with every candidate
// counted by its mass; the sums are integers, so the result does not depend on the order of the atomics.
// All threads of the block call it; whist / wsel / wmax are its LDS.
__device__ __forceinline__ uint32_t nucleus_threshold(const bf16_t* __restrict__ row, int V, int ngrp, uint32_t thr,
                                                      float inv_temp, double top_p, uint64_t (*whist)[256],
                                                      uint64_t* wsel, uint32_t* wmax, int nthreads) {
  const int tid = threadIdx.x, w = tid >> 6;
  if (tid == 0) wsel[0] = wsel[1] = 0ull;     // a row of NaNs has no mass and picks nothing: key 0 then
  // the largest key of the row: always a candidate, and z is monotone in the key (inv_temp > 0)
  uint32_t mk = 0;
  for (int gi = tid; gi < ngrp; gi += nthreads) {
    const uint2 w2 = reinterpret_cast<const uint2*>(row)[gi];
    const uint32_t u[4] = {w2.x & 0xffffu, w2.x >> 16, w2.y & 0xffffu, w2.y >> 16};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const uint32_t key = 4 * gi + e < V ? key16(u[e]) : 0u;
      mk = key > mk ? key : mk;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t t = __shfl_xor(mk, o, 64);
    mk = t > mk ? t : mk;
  }
  if ((tid & 63) == 0) wmax[w] = mk;
  __syncthreads();
  for (int i = 0; i < nthreads / 64; ++i) mk = wmax[i] > mk ? wmax[i] : mk;
  const uint32_t mbits = (mk & 0x8000u) ? (mk & 0x7fffu) : (~mk & 0xffffu);     // key16 inverted
  const float zmax = bf2f(mbits) * inv_temp;

  uint32_t hi = 0;
  uint64_t target = 0;
  for (int pass = 0; pass < 2; ++pass) {
    for (int i = tid; i < 1024; i += nthreads) (&whist[0][0])[i] = 0ull;
    __syncthreads();
    for (int gi = tid; gi < ngrp; gi += nthreads) {
      const uint2 w2 = reinterpret_cast<const uint2*>(row)[gi];
      const uint32_t u[4] = {w2.x & 0xffffu, w2.x >> 16, w2.y & 0xffffu, w2.y >> 16};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (4 * gi + e >= V) continue;
        const uint32_t key = key16(u[e]);
        if (key < thr) continue;
        if (pass == 0) atomicAdd((unsigned long long*)&whist[w & 3][key >> 8],
                                 (unsigned long long)mass_fx(bf2f(u[e]) * inv_temp, zmax));
        else if ((key >> 8) == hi) atomicAdd((unsigned long long*)&whist[w & 3][key & 0xffu],
                                             (unsigned long long)mass_fx(bf2f(u[e]) * inv_temp, zmax));
      }
    }
    __syncthreads();
    if (pass == 0) {
      if (tid < 64) {          // total mass -> target, by every lane of wave 0 alike
        uint64_t c = 0;
        for (int q = 0; q < 4; ++q)
          c += whist[0][4 * tid + q] + whist[1][4 * tid + q] + whist[2][4 * tid + q] + whist[3][4 * tid + q];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
          const uint32_t lo = __shfl_xor((uint32_t)c, o, 64), h2 = __shfl_xor((uint32_t)(c >> 32), o, 64);
          c += ((uint64_t)h2 << 32) | lo;
        }
        uint64_t t = (uint64_t)ceil(top_p * (double)c);
        t = t < 1 ? 1 : (t > c ? c : t);
        radix_pick_mass(whist, t, wsel);
      }
    } else if (w == 0) {
      radix_pick_mass(whist, target, wsel);
    }
    __syncthreads();
    if (pass == 0) {
      hi = (uint32_t)wsel[0];
      target = wsel[1];
    }
    __syncthreads();
  }
  return (hi << 8) | (uint32_t)wsel[0];
}

// grid B, block SM_NT (16 waves: a row of 50304 logits is ~50 per thread and pass; the 4 histograms are
// shared by waves w, w + 4, ...).  TOPP adds the nucleus stage between the top-k select and the Gumbel pass.
constexpr int SM_NT = 1024;

// The logit processors of one element (PdeSampleProc in pde_decode.h): x the fp32 logit, c its counts word.
// Every operation is rounded on its own -- the CPU definition is numpy float32, one operation per line -- so
// contraction is off here: hipcc would turn x - freq * n into one fused multiply-add otherwise.
__device__ __forceinline__ float proc_logit(float x, int c, float bias, bool has_bias, bool ban,
                                            const PdeSampleProc& p) {
#pragma clang fp contract(off)
  const int n = c & PDE_TC_COUNT;
  if (c != 0) x = x > 0.f ? x * p.inv_rep : x * p.rep;
  const float fn = p.freq * (float)n;
  x = x - fn;
  x = x - (n > 0 ? p.pres : 0.f);
  if (has_bias) x = x + bias;
  return ban ? -INFINITY : x;
}

// `Proc` is empty, or PdeSampleProc for the PROC instantiations (the logit processors): their arguments travel in
// a second by-value struct that only they take, as PdeXentSmooth does for the loss kernels, so the other two
// keep their kernel-argument layout and their instruction streams.
// PROC adds a prologue: the block computes its row's processed logits y once, 8 columns per thread and round --
// 16 bytes of logits, 2 x 16 of counts, 2 x 16 of bias -- into the bf16 workspace row, and after a block barrier
// `row` is that workspace row: every pass below runs on y as it runs on the raw logits.  The prologue is the
// block's only reader of its counts row, so thread 0 can add the emitted token with a plain load and store at
// the end.  logits_out keeps copying the raw row.
// HIST (a third struct, PdeSampleHist, on top of PROC) adds the history constraints of pde_decode.h.  The row's
// history is out[b, 0 : L], L = len_b + step, both from the state.  After the prologue's barrier the block walks
// the history: thread j compares the n - 1 tokens before position j with the last n - 1 and stores bf16 -inf to
// y[h[j]] on a match (every writer stores the same value: no atomic), one thread per banned sequence compares its
// head with the history's tail and bans its last token, and a second barrier makes y final for the passes.  In
// the tail wave 0 matches the stop sequences against the generated tokens with the emitted one in place, one
// sequence per lane and round, and a wave minimum picks the lowest index.  Nothing reads `out` at or past L.
__device__ __forceinline__ const PdeSampleProc& proc_args(const PdeSampleProc& p) { return p; }
__device__ __forceinline__ const PdeSampleProc& proc_args(const PdeSampleProc& p, const PdeSampleHist&) { return p; }
__device__ __forceinline__ const PdeSampleHist& hist_args(const PdeSampleProc&, const PdeSampleHist& h) { return h; }
template <bool TOPP, typename... Proc>
__global__ __launch_bounds__(SM_NT) void k_sample(PdeSample a, Proc... proc) {
  constexpr bool PROC = sizeof...(Proc) >= 1;
  constexpr bool HIST = sizeof...(Proc) == 2;
  [[maybe_unused]] PdeSampleProc p{};
  if constexpr (PROC) p = proc_args(proc...);
  [[maybe_unused]] PdeSampleHist hc{};
  if constexpr (HIST) hc = hist_args(proc...);
  __shared__ uint32_t hist[4][256];
  __shared__ uint32_t sel[2];
  __shared__ uint64_t bred[SM_NT / 64];
  const int b = blockIdx.x, tid = threadIdx.x, w = tid >> 6;
  const bf16_t* row = reinterpret_cast<const bf16_t*>(a.logits) + (size_t)b * a.Vp;
  const uint32_t st[4] = {(uint32_t)a.state[PDE_DS_RNG], (uint32_t)a.state[PDE_DS_RNG + 1],
                          (uint32_t)a.state[PDE_DS_RNG + 2], (uint32_t)a.state[PDE_DS_RNG + 3]};
  const int step = a.state[PDE_DS_STEP];
  const int fin = a.state[PDE_DS_FIN + b];
  const int slot = a.T0 + a.state[PDE_DS_OFF + b] + step;      // read here, with the other state words
  const int V = a.V, ngrp = a.Vp >> 2;
  [[maybe_unused]] const bf16_t* raw = row;

  if constexpr (PROC) {
    int* cnt = p.counts + (size_t)b * a.Vp;
    const float* bias = p.bias ? p.bias + (size_t)b * p.bias_stride : nullptr;
    bf16_t* y = reinterpret_cast<bf16_t*>(p.work) + (size_t)b * a.Vp;
    const int ban_v = step < p.min_new ? a.eos : -1;           // eos < 0 (none): nothing to ban
    for (int g8 = tid; g8 < (a.Vp >> 3); g8 += SM_NT) {        // Vp % 8 == 0
      const uint4 lv = reinterpret_cast<const uint4*>(raw)[g8];
      const int4 c0 = reinterpret_cast<const int4*>(cnt)[2 * g8], c1 = reinterpret_cast<const int4*>(cnt)[2 * g8 + 1];
      float4 b0 = make_float4(0.f, 0.f, 0.f, 0.f), b1 = b0;
      if (bias) {
        b0 = reinterpret_cast<const float4*>(bias)[2 * g8];
        b1 = reinterpret_cast<const float4*>(bias)[2 * g8 + 1];
      }
      float x[8];
      unpack8(lv, x);
      const int c[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
      const float bb[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
      for (int e = 0; e < 8; ++e) x[e] = proc_logit(x[e], c[e], bb[e], bias != nullptr, 8 * g8 + e == ban_v, p);
      reinterpret_cast<uint4*>(y)[g8] = pack8(x);
    }
    __syncthreads();            // the row of y, written by the whole block, is read by the whole block
    row = y;
  }

  // history constraints: slot = len_b + step is the history's length L.  A state that points outside `out`
  // switches them off; a finished row emits eos whatever is banned, so its y stays as the processors left it.
  [[maybe_unused]] bool hist_on = false;
  [[maybe_unused]] const int64_t* h = nullptr;
  if constexpr (HIST) {
    hist_on = step >= 0 && slot >= step && slot <= a.out_stride && !(a.eos >= 0 && fin);
    h = a.out + (size_t)b * a.out_stride;
    if (hist_on) {
      const int L = slot, n = hc.n;
      bf16_t* y = reinterpret_cast<bf16_t*>(p.work) + (size_t)b * a.Vp;
      const bf16_t ninf = f2bf(-INFINITY);
      if (n >= 1 && L >= n - 1) {
        for (int j = n - 1 + tid; j < L; j += SM_NT) {
          bool eq = true;
          for (int i = 1; i < n; ++i) eq &= h[j - i] == h[L - i];
          const int64_t v = h[j];
          if (eq && v >= 0 && v < V) y[v] = ninf;
        }
      }
      for (int q = tid; q < hc.n_ban; q += SM_NT) {
        const int o0 = hc.ban[q], m = hc.ban[q + 1] - o0;
        const int* seq = hc.ban + hc.n_ban + 1 + o0;
        if (m < 1 || L < m - 1) continue;
        bool eq = true;
        for (int i = 0; i < m - 1; ++i) eq &= h[L - m + 1 + i] == (int64_t)seq[i];
        const int v = seq[m - 1];
        if (eq && v >= 0 && v < V) y[v] = ninf;
      }
    }
    __syncthreads();            // the bans, stored by any thread, are read by the whole block
  }

  uint32_t thr = 0;             // candidates: key16 >= thr
  if (!a.greedy && a.top_k > 0 && a.top_k < V) {
    uint32_t hi = 0, k = (uint32_t)a.top_k;
    for (int pass = 0; pass < 2; ++pass) {
      for (int i = tid; i < 1024; i += SM_NT) (&hist[0][0])[i] = 0u;
      __syncthreads();
      for (int gi = tid; gi < ngrp; gi += SM_NT) {
        const uint2 w2 = reinterpret_cast<const uint2*>(row)[gi];
        const uint32_t u[4] = {w2.x & 0xffffu, w2.x >> 16, w2.y & 0xffffu, w2.y >> 16};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if (4 * gi + e >= V) continue;
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
      }
      __syncthreads();
    }
  }
  if constexpr (TOPP) {
    if (!a.greedy) {
      __shared__ uint64_t whist[4][256];
      __shared__ uint64_t wsel[2];
      __shared__ uint32_t wmax[SM_NT / 64];
      thr = nucleus_threshold(row, V, ngrp, thr, a.inv_temp, a.top_p, whist, wsel, wmax, SM_NT);
    }
  }

  // best = max over candidates of (score key << 32 | ~index): highest score, lowest index on ties
  uint64_t best = 0;
  for (int gi = tid; gi < ngrp; gi += SM_NT) {
    const uint2 w2 = reinterpret_cast<const uint2*>(row)[gi];
    const uint32_t u[4] = {w2.x & 0xffffu, w2.x >> 16, w2.y & 0xffffu, w2.y >> 16};
    if (a.greedy) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const uint32_t v = 4u * gi + e;
        if ((int)v >= V) continue;
        const uint64_t cand = ((uint64_t)key16(u[e]) << 32) | (uint32_t)~v;
        best = cand > best ? cand : best;
      }
    } else {
      bool c[4], any = false;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        c[e] = 4 * gi + e < V && key16(u[e]) >= thr;
        any |= c[e];
      }
      if (!any) continue;
      uint32_t ww[4];
      pde_rng::group_words(st, 0u, (uint64_t)b * (uint64_t)ngrp + (uint64_t)gi, ww);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (!c[e]) continue;
        const uint32_t v = 4u * gi + e;
        const float uu = ((float)(ww[e] >> 9) + 0.5f) * 1.1920928955078125e-07f;   // 2^-23, exact
        const float gum = -logf(-logf(uu));
        const float sc = bf2f(u[e]) * a.inv_temp + gum;
        const uint64_t cand = ((uint64_t)fkey32(sc) << 32) | (uint32_t)~v;
        best = cand > best ? cand : best;
      }
    }
  }
  best = wave_max_u64(best);
  if ((tid & 63) == 0) bred[w] = best;
  __syncthreads();
  [[maybe_unused]] int hit = -1;  // lowest index of a stop sequence that ends at the token emitted now
  if constexpr (HIST) {
    // hist_on: the row was not finished, so the token is the block's best.  Every lane of wave 0 holds wave 0's
    // maximum after the xor reduction and reads the other waves' from LDS.
    if (w == 0 && hist_on && a.eos >= 0 && hc.n_stop > 0) {
      uint64_t bb = best;
      for (int i = 1; i < SM_NT / 64; ++i) bb = bred[i] > bb ? bred[i] : bb;
      const int64_t tok = (int64_t)(uint32_t)~(uint32_t)bb;
      const int L = slot;
      int mine = 0x7fffffff;
      for (int q = tid; q < hc.n_stop; q += 64) {
        const int o0 = hc.stop[q], m = hc.stop[q + 1] - o0;
        const int* seq = hc.stop + hc.n_stop + 1 + o0;
        if (m < 1 || step + 1 < m) continue;                 // the match lies in the generated tokens
        bool eq = tok == (int64_t)seq[m - 1];
        for (int i = 0; i < m - 1; ++i) eq &= h[L - m + 1 + i] == (int64_t)seq[i];
        if (eq) {
          mine = q;
          break;
        }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const int t = __shfl_xor(mine, o, 64);
        mine = t < mine ? t : mine;
      }
      if (mine != 0x7fffffff) hit = mine;
    }
  }
  if (tid == 0) {
    for (int i = 1; i < SM_NT / 64; ++i) best = bred[i] > best ? bred[i] : best;
    int64_t tok = (int64_t)(uint32_t)~(uint32_t)best;
    if (a.eos >= 0) {
      if (fin) tok = a.eos;
      if (tok == a.eos) a.state[PDE_DS_FIN + b] = 1;
    }
    if constexpr (HIST) {
      if (hit >= 0) {
        a.state[PDE_DS_FIN + b] = 1;
        hc.stop_hit[b] = hit;
      }
    }
    a.next[b] = tok;
    if (a.thr_out) a.thr_out[b] = (int)thr;
    if (step >= 0 && slot >= 0 && slot < a.out_stride) a.out[(size_t)b * a.out_stride + slot] = tok;
    if constexpr (PROC) {       // the forced eos of a finished row counts too: it is what `out` holds
      if (tok >= 0 && tok < V) p.counts[(size_t)b * a.Vp + tok] += 1;
    }
  }
  if (a.logits_out && step >= 0 && step < a.max_new) {
    bf16_t* dst = reinterpret_cast<bf16_t*>(a.logits_out) + ((size_t)b * a.max_new + step) * V;
    if constexpr (PROC) {
      for (int v = tid; v < V; v += SM_NT) dst[v] = raw[v];
    } else {
      for (int v = tid; v < V; v += SM_NT) dst[v] = row[v];
    }
  }
}

// tail of the sampler launch: every row has read the state
__global__ void k_dec_advance(int* __restrict__ state) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    state[PDE_DS_POS] += 1;
    state[PDE_DS_STEP] += 1;
    state[PDE_DS_RNG + 2] = (int)((uint32_t)state[PDE_DS_RNG + 2] + 1u);
  }
}

// ---------------------------------------------------------------------------------------- host side
// The argument checks of pde_sample, pde_sample_proc and pde_sample_hist, and the tail of their launch.
static inline bool sample_ok(const PdeSample& a) {
  return a.B >= 1 && a.B <= PDE_DS_MAX_ROWS && a.V >= 1 && a.V <= a.Vp && a.Vp % 8 == 0 && a.top_k >= 0 &&
         a.top_p >= 0.0;      // false for a NaN
}
static inline bool proc_ok(const PdeSample& a, const PdeSampleProc& p) {
  if (!p.counts || !p.work || (p.bias && p.bias_stride != 0 && p.bias_stride != a.Vp)) return false;
  return p.min_new >= 0 && (p.min_new == 0 || a.eos >= 0) && a.eos < a.V;
}
static inline bool hist_ok(const PdeSample& a, const PdeSampleHist& h) {
  if (!a.out || a.out_stride < 1 || h.n < 0 || h.n > PDE_HIST_MAX_NGRAM) return false;
  if (h.n_ban < 0 || h.n_ban > PDE_HIST_MAX_SEQS || (h.n_ban > 0 && !h.ban)) return false;
  if (h.n_stop < 0 || h.n_stop > PDE_HIST_MAX_SEQS) return false;
  return h.n_stop == 0 || (h.stop && h.stop_hit && a.eos >= 0);
}

// k_sample<TOPP, Proc...> over the checked arguments -- TOPP only when the nucleus stage has something to do --
// then the state's advance
template <typename... Proc>
hipError_t sample_launch(const PdeSample& a, hipStream_t st, Proc... proc) {
  if (!a.greedy && a.top_p > 0.0 && a.top_p < 1.0)
    hipLaunchKernelGGL((k_sample<true, Proc...>), dim3(a.B), dim3(SM_NT), 0, st, a, proc...);
  else
    hipLaunchKernelGGL((k_sample<false, Proc...>), dim3(a.B), dim3(SM_NT), 0, st, a, proc...);
  PDE_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(k_dec_advance, dim3(1), dim3(64), 0, st, a.state);
  return hipGetLastError();
}
