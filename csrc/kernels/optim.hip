// Fused optimizers over flat fp32 buffers (one launch per step for ALL parameters).
//
// Adam / AdamW reproduce torch.optim.Adam's single-tensor math (torch/optim/adam.py:347-460):
//   m = lerp(m, g, 1-b1); v = v*b2 + (1-b2)*g*g
//   p -= (lr / (1-b1^t)) * m / (sqrt(v)/sqrt(1-b2^t) + eps)
// The step counter lives on the device: every block reads t = *step + 1 and the last block to
// arrive publishes *step = t (arrival counter reset in the same block), so the whole optimizer
// step is capturable in a hipGraph and replayable without host involvement.  `bump` = number of
// consecutive int64 counters advanced by the last block (0: none; [0] is the optimizer step);
// bump < 0: the caller's earlier kernel already advanced the counter, t = *step, no fan-in at all.
// lr_tab (nullable): a device table of per-step learning rates, step t uses lr_tab[min(t-1, lr_len-1)]
// (pde_lr.h), so a captured launch follows a schedule; null = the by-value lr.
// grad_scale folds the DDP 1/world_size average (or any loss scale) into the update.
// Two Adam kernels are compiled, k_adam<PROF, NTP, AR>:
//   AR = false, the lean kernel: every call without a peer (the single-GPU LeNet step, GPT-2, ResNet-18).
//     Its one argument is the Lean struct, which carries what the host worked out to size the grid
//     (holes, compressed length, block counts per role, 1-b1, 1-b2): no peer code, no pass loop, no
//     64-bit division.  Fold blocks have the lowest block ids (the longest chain starts first); a
//     block fetches its arguments in one batch, issues the scalar load of *step and its first
//     iteration's vector loads, and only then waits for the step and does the lr-table lookup and
//     the bias-correction powf / sqrt / divide, under the loads.  k_sgd has the same shape.
//   AR = true, the general kernel: the fused all-reduce below (side blocks first, two passes); also
//     what pde_optim_force_general selects for a peer-less call, so tests can compare the two.
// Optional fused all-reduce (Adam only, the W > 1 "fused" LeNet schedule): the first ar_nvb blocks
// all-reduce the flat range [ar_lo4, n4) (the conv-gradient bucket) across ranks with the xGMI peer
// protocol while the other blocks update [0, ar_lo4); those blocks then wait for the reduction (the
// completing side block publishes the optimizer step t in *ar_epoch) before updating the rest.
// Side blocks have the lowest block ids, so they are dispatched first: no wait can starve them.
// Optional epilogue: repack the LeNet conv2 weight [50][20][5][5] into the [k'][64] layout the
// conv2 forward kernel streams (k' = (kh*5+kw)*20+ci), so no separate repack launch exists.
#include "pde_hip.h"
#include "pde_kernels.h"
#include "pde_lenet.h"
#include "pde_peer_dev.h"
#include "pde_adam.h"
#include "pde_lr.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <type_traits>

namespace {

struct Pack {
  long long off;   // flat offset of conv2.weight, -1 = no repack
  float* dst;      // mode 1: [500][64] (lenet.hip F1); mode 2: the LDS-DMA image of lenet_v2.hip
  int mode;
};

struct Fold1 {
  long long off;   // first element of the canonical gradient (replica 0); -1 = none
  int len;         // elements per replica unit (multiple of 4)
  int nrep;        // replicas (1 = nothing to fold)
  int stride;      // floats between replicas (multiple of 4)
};
struct Fold {      // up to two replicated gradient ranges (LeNet: conv1 atomic replicas, conv2 wgrad slabs)
  Fold1 f[2];
};

// Folded ranges (whole replica sets [off, off + nrep*stride)) are holes of the main index space;
// appended fold blocks own them.  Each canonical float4 gets kLS lanes: lane l sums replicas
// l, l+kLS, ..., a 2-step xor shuffle combines the lanes, and lane l then updates element l of the
// float4 (the old one-thread-per-float4 fold issued 19 loads per thread on the last ~27 blocks and
// ended the kernel 2 us after every other block).  The guarded loads compile to one basic block
// each, with a vmcnt(0) between most of them (tools/isa_load_order.py); making them unconditional
// on clamped addresses puts them in one batch but did not shorten the fold blocks
// (profiles/lenet_load_order/rejected_adam_fold_batch/).
// The general Adam kernel appends the fold blocks (highest block ids) and derives holes, block counts
// and lane addresses on the device (make_holes, fold_blocks, fold_elem, fold_lane).  The lean Adam
// kernel and k_sgd put the fold blocks first and take all of that from the host in the Lean struct
// (lean_fold_addr / lean_fold_load / lean_fold_sum: the same loads and the same order of additions,
// all issued before the wait for the step counter).
constexpr int kMaxFold = 16;
constexpr int kLS = 4;

struct Holes {
  long long lo[2], len[2];   // in float4 units, sorted, lo = huge when unused
};

__host__ __device__ __forceinline__ bool fold_on(const Fold1& f) { return f.off >= 0 && f.nrep > 1; }

__host__ __device__ __forceinline__ Holes make_holes(const Fold& fd) {
  Holes h{{(long long)1 << 60, (long long)1 << 60}, {0, 0}};
  for (int k = 0; k < 2; ++k) {
    const Fold1& f = fd.f[k];
    if (fold_on(f)) {
      h.lo[k] = f.off / 4;
      h.len[k] = (long long)f.nrep * f.stride / 4;
    }
  }
  if (h.lo[1] < h.lo[0]) {
    const long long a = h.lo[0], b = h.len[0];
    h.lo[0] = h.lo[1]; h.len[0] = h.len[1];
    h.lo[1] = a; h.len[1] = b;
  }
  return h;
}

__device__ __forceinline__ long long hole_map(const Holes& h, long long c) {   // compressed -> real index
  if (c >= h.lo[0]) c += h.len[0];
  if (c >= h.lo[1]) c += h.len[1];
  return c;
}

// fold blocks per range: kLS lanes for each float4 of the canonical slot (stride / 4 float4s)
__host__ __device__ __forceinline__ int fold_blocks(const Fold1& f) {
  return fold_on(f) ? (int)(((long long)f.stride / 4 * kLS + 255) / 256) : 0;
}

struct FoldLane {
  long long e;   // flat element this lane updates (-1: none)
  float g;       // its folded gradient (before grad_scale)
};

// The flat element fold lane (fb, threadIdx.x) updates (-1: none) -- known before any load, so the
// optimizer state of that element is fetched in the same round trip as the replicas.
__device__ __forceinline__ long long fold_elem(const Fold& fd, int fb) {
  const int nb0 = fold_blocks(fd.f[0]);
  const int k = fb < nb0 ? 0 : 1;
  const Fold1& f = fd.f[k];
  const long long j = ((long long)(k ? fb - nb0 : fb) * 256 + threadIdx.x) / kLS;
  return j < f.stride / 4 ? f.off + 4 * j + threadIdx.x % kLS : -1;
}

// fb = fold-block index (0-based over both ranges).  All lanes of the wave take part in the shuffles.
__device__ __forceinline__ FoldLane fold_lane(const Fold& fd, float* __restrict__ g, int fb) {
  const int nb0 = fold_blocks(fd.f[0]);
  const int k = fb < nb0 ? 0 : 1;
  const Fold1& f = fd.f[k];
  const long long j = ((long long)(k ? fb - nb0 : fb) * 256 + threadIdx.x) / kLS;   // float4 in the slot
  const int lane = threadIdx.x % kLS;
  const bool valid = j < f.stride / 4;
  const int nrep = (valid && 4 * j < f.len) ? f.nrep : 1;            // past len: no replicas to add
  const float4* g4 = reinterpret_cast<const float4*>(g) + f.off / 4 + (valid ? j : 0);
  const int s4 = f.stride / 4;
  float4 x[kMaxFold / kLS];
#pragma unroll
  for (int q = 0; q < kMaxFold / kLS; ++q) {
    const int r = lane + q * kLS;
    x[q] = (valid && r < nrep) ? g4[(long long)r * s4] : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  float4 a = x[0];
#pragma unroll
  for (int q = 1; q < kMaxFold / kLS; ++q) { a.x += x[q].x; a.y += x[q].y; a.z += x[q].z; a.w += x[q].w; }
#pragma unroll
  for (int o = 1; o < kLS; o <<= 1) {
    a.x += __shfl_xor(a.x, o); a.y += __shfl_xor(a.y, o); a.z += __shfl_xor(a.z, o); a.w += __shfl_xor(a.w, o);
  }
  const float mine = lane == 0 ? a.x : lane == 1 ? a.y : lane == 2 ? a.z : a.w;
  return FoldLane{valid ? f.off + 4 * j + lane : -1, mine};
}

__device__ __forceinline__ void pack_store(const Pack& pk, long long i, float v) {
  const long long e64 = i - pk.off;
  if (pk.off >= 0 && e64 >= 0 && e64 < 25000) {
    const int e = (int)e64;                 // 32-bit index math (64-bit division is ~100 instructions)
    if (pk.mode == 2) {
      pk.dst[pde_lenet_wp_index(e)] = v;
    } else {
      const int co = e / 500, k = e - co * 500, ci = k / 25, r = k - ci * 25;
      pk.dst[(r * 20 + ci) * 64 + co] = v;
    }
  }
}

// The arrival add carries a data dependency on the step value this block read, so it cannot be
// issued before that read returned: no block can observe the bumped counter.
__device__ __forceinline__ bool last_block(unsigned* arrive, long long t) {
  __shared__ int is_last;
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned prev = atomicAdd(arrive, t > 0 ? 1u : 2u);
    is_last = (prev == gridDim.x - 1);
  }
  __syncthreads();
  return is_last != 0;
}

struct FusedAR {
  pde::PeerDev pd;
  long long lo4;            // first float4 of the all-reduced range (range = [lo4, n4))
  long long* epoch;         // completion word: the optimizer step t of the reduced call
  int nvb;                  // side blocks (0 = no fused all-reduce)
  int two;
};

__device__ __forceinline__ void wait_epoch(const long long* epoch, long long t, const pde::PeerDev& pd) {
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
    // relaxed polling (an acquire per poll would invalidate the L2 under the side blocks' feet),
    // one acquire once the completion word is seen
    while (__hip_atomic_load(epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != t) {
      __builtin_amdgcn_s_sleep(2);
      if ((int64_t)(__builtin_amdgcn_s_memrealtime() - t0) > 2 * pd.timeout) break;   // failure latched by the side blocks
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  }
  __syncthreads();
}

template <bool PROF, bool NTP, bool AR>
__global__ __launch_bounds__(256) std::enable_if_t<AR> k_adam(float* __restrict__ p, float* __restrict__ g,
                                              float* __restrict__ m, float* __restrict__ v, long long n4,
                                              float lr, float b1, float b2, float eps, float wd, int decoupled,
                                              float grad_scale, long long* __restrict__ step,
                                              unsigned* __restrict__ arrive, int bump, Pack pk, Fold fd, FusedAR ar,
                                              unsigned long long* __restrict__ prof,
                                              const float* __restrict__ lr_tab, int lr_len) {
  // AR = true: the general kernel (fused all-reduce side blocks, two passes), the W > 1 adam1 / adam2 routes
  if constexpr (PROF) {
    if (threadIdx.x == 0) prof[(size_t)blockIdx.x * 8] = __builtin_amdgcn_s_memrealtime();
  }
  const long long t = bump < 0 ? *step : *step + 1;   // bump < 0: counter pre-advanced by an earlier kernel
  lr = sched_lr(lr, lr_tab, lr_len, t);
  __shared__ uint32_t lds2[2];
  const Holes holes = make_holes(fd);
  const long long n4c = n4 - holes.len[0] - holes.len[1];   // compressed index space (replicas skipped)
  const int nmain = (int)gridDim.x - fold_blocks(fd.f[0]) - fold_blocks(fd.f[1]);
  long long i0 = (long long)blockIdx.x * blockDim.x + threadIdx.x, istride = (long long)nmain * blockDim.x;
  long long lo = 0, hi = n4c;                         // pass 1 range; pass 2 = [ar.lo4, n4c) after the wait
  if (ar.nvb > 0) {
    if ((int)blockIdx.x < ar.nvb) {
      if (pde::peer_ar_f32_vblock(ar.pd, g + 4 * ar.lo4, g + 4 * ar.lo4, 4 * (n4 - ar.lo4), 1.f, blockIdx.x,
                                  ar.nvb, ar.two != 0, lds2))
        __hip_atomic_store(ar.epoch, t, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
      i0 = n4;                                        // no parameter work in side blocks
    } else {
      i0 = (long long)(blockIdx.x - ar.nvb) * blockDim.x + threadIdx.x;
      istride = (long long)(nmain - ar.nvb) * blockDim.x;
      hi = ar.lo4;
    }
  }
  const float bc1 = 1.f - powf(b1, (float)t);
  const float bc2 = 1.f - powf(b2, (float)t);
  const float step_size = lr / bc1;
  const float bc2s = sqrtf(bc2);
  const float omb1 = 1.f - b1, omb2 = 1.f - b2;
  float4* p4 = reinterpret_cast<float4*>(p);
  float4* g4 = reinterpret_cast<float4*>(g);
  float4* m4 = reinterpret_cast<float4*>(m);
  float4* v4 = reinterpret_cast<float4*>(v);
  const int nfb = fold_blocks(fd.f[0]) + fold_blocks(fd.f[1]);
  const int fb = (int)blockIdx.x - ((int)gridDim.x - nfb);   // >= 0: fold block
  for (int pass = 0; pass < 2; ++pass) {
  if (pass == 1 && fb < 0) {
    if (ar.nvb == 0 || (int)blockIdx.x < ar.nvb) break;   // block-uniform: wait_epoch has barriers
    wait_epoch(ar.epoch, t, ar.pd);                   // the all-reduced range is ready
    lo = ar.lo4;
    hi = n4c;
  }
  if (fb >= 0) {                                     // fold block: its own range, one pass
    if (pass == 1) break;
    if (ar.nvb > 0) wait_epoch(ar.epoch, t, ar.pd);   // the reduced replicas must be complete
    const long long e0 = fold_elem(fd, fb);
    float pa = 0.f, ma = 0.f, va = 0.f;
    if (e0 >= 0) {                                   // issued before the replica loads
      pa = p[e0];
      ma = m[e0];
      va = v[e0];
    }
    const FoldLane fl = fold_lane(fd, g, fb);
    if (fl.e >= 0) {
      adam_elem(pa, ma, va, fl.g * grad_scale, lr, wd, decoupled, omb1, omb2, b2, step_size, bc2s, eps);
      if constexpr (NTP) {     // NTP: nothing of this launch is left dirty in the XCD L2s (see below)
        __builtin_nontemporal_store(pa, p + fl.e);
        __builtin_nontemporal_store(ma, m + fl.e);
        __builtin_nontemporal_store(va, v + fl.e);
        __builtin_nontemporal_store(fl.g, g + fl.e);   // p.grad holds the true (folded) gradient
      } else {
        p[fl.e] = pa; m[fl.e] = ma; v[fl.e] = va;
        g[fl.e] = fl.g;                                // p.grad holds the true (folded) gradient
      }
      pack_store(pk, fl.e, pa);
    }
    continue;
  }
  for (long long ic = lo + i0; ic < hi; ic += istride) {
    const long long i = hole_map(holes, ic);
    float4 pp = p4[i], gg = g4[i], mm = m4[i], vv = v4[i];
    float* pa = &pp.x; float* ga = &gg.x; float* ma = &mm.x; float* va = &vv.x;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      adam_elem(pa[j], ma[j], va[j], ga[j] * grad_scale, lr, wd, decoupled, omb1, omb2, b2, step_size, bc2s, eps);
      pack_store(pk, 4 * i + j, pa[j]);
    }
    // the moments are read again only by the next step's Adam: streamed out (non-temporal) rather than
    // left dirty in the XCD L2s for the end-of-kernel write-back that the next kernel waits behind.
    // NTP: the parameters too -- their next readers (the next step's forward kernels) run on other
    // XCDs' L2s anyway, so a dirty line here only lengthens this kernel's end-of-kernel write-back
    typedef float nt_f4 __attribute__((ext_vector_type(4)));
    if constexpr (NTP) __builtin_nontemporal_store(*reinterpret_cast<nt_f4*>(&pp), reinterpret_cast<nt_f4*>(p4 + i));
    else p4[i] = pp;
    __builtin_nontemporal_store(*reinterpret_cast<nt_f4*>(&mm), reinterpret_cast<nt_f4*>(m4 + i));
    __builtin_nontemporal_store(*reinterpret_cast<nt_f4*>(&vv), reinterpret_cast<nt_f4*>(v4 + i));
  }
  }
  if (bump > 0 && last_block(arrive, t) && threadIdx.x == 0) {
    step[0] = t;
    for (int c = 1; c < bump; ++c) step[c] += 1;   // extra device counters (e.g. batch position)
    *arrive = 0u;
  }
  if constexpr (PROF) {
    if (threadIdx.x == 0) prof[(size_t)blockIdx.x * 8 + 1] = __builtin_amdgcn_s_memrealtime();
  }
}

// ---- the lean kernels: every call without a fused all-reduce (k_adam<.,.,false>) and every k_sgd ----
// One by-value struct: everything the host already worked out to size the grid (holes, compressed
// length, block counts per role, 1-b1, 1-b2) travels as an argument, so a block fetches its
// arguments in one batch and does no 64-bit division.
struct Lean {
  float* p; float* g; float* m; float* v;   // SGD: m = momentum buffer, v unused
  long long* step;
  unsigned* arrive;
  const float* lr_tab;
  unsigned long long* prof;
  float* pack_dst;
  long long pack_off;        // -1 = no repack
  Holes holes;
  long long n4c;             // compressed float4 count (replica sets skipped)
  long long f_off[2];        // fold ranges in block order (range 0's blocks first); see Fold1
  int f_len[2], f_nrep[2], f_s4[2];   // f_s4 = stride / 4
  int nfb0, nfb;             // fold blocks of range 0, of both ranges; 0 = no fold
  int nmain;                 // main (grid-stride) blocks
  int pack_mode, bump, lr_len, flag;   // flag: Adam decoupled / SGD nesterov
  float lr, grad_scale, wd;
  float a, b, oma, omb, eps;   // Adam: b1, b2, 1-b1, 1-b2, eps; SGD: momentum, dampening
};

// Block ids: fold blocks first (their chain is the longest: seven loads, two shuffle rounds, scattered
// 4-byte stores and the Wp index arithmetic), then the main blocks.
struct LeanFold {
  long long e;      // flat element this lane updates (-1: none)
  int nrep;         // replicas this lane's float4 has (1 past len)
  int lane;
  const float4* g4; // replica 0 of this lane's float4
  long long s4;
};

__device__ __forceinline__ LeanFold lean_fold_addr(const Lean& a, const long long (&f_off)[2], int fb) {
  const int k = fb < a.nfb0 ? 0 : 1;
  const int j = (int)(((unsigned)(k ? fb - a.nfb0 : fb) * 256u + threadIdx.x) / kLS);   // float4 in the slot
  const int lane = threadIdx.x % kLS;
  const int s4 = a.f_s4[k];
  const bool valid = j < s4;
  LeanFold f;
  f.e = valid ? f_off[k] + 4 * j + lane : -1;
  f.nrep = (valid && 4 * j < a.f_len[k]) ? a.f_nrep[k] : (valid ? 1 : 0);
  f.lane = lane;
  f.g4 = reinterpret_cast<const float4*>(a.g + f_off[k]) + (valid ? j : 0);   // f_off % 4 == 0
  f.s4 = s4;
  return f;
}

// the replica loads of fold_lane, and its sum (same order of additions)
__device__ __forceinline__ void lean_fold_load(const LeanFold& f, float4 (&x)[kMaxFold / kLS]) {
#pragma unroll
  for (int q = 0; q < kMaxFold / kLS; ++q) {
    const int r = f.lane + q * kLS;
    x[q] = r < f.nrep ? f.g4[(long long)r * f.s4] : make_float4(0.f, 0.f, 0.f, 0.f);
  }
}

__device__ __forceinline__ float lean_fold_sum(const LeanFold& f, const float4 (&x)[kMaxFold / kLS]) {
  float4 a = x[0];
#pragma unroll
  for (int q = 1; q < kMaxFold / kLS; ++q) { a.x += x[q].x; a.y += x[q].y; a.z += x[q].z; a.w += x[q].w; }
#pragma unroll
  for (int o = 1; o < kLS; o <<= 1) {
    a.x += __shfl_xor(a.x, o); a.y += __shfl_xor(a.y, o); a.z += __shfl_xor(a.z, o); a.w += __shfl_xor(a.w, o);
  }
  return f.lane == 0 ? a.x : f.lane == 1 ? a.y : f.lane == 2 ? a.z : a.w;
}

struct AdamStep {   // per-launch constants that need the step counter
  float lr, step_size, bc2s;
};

__device__ __forceinline__ AdamStep adam_step(const Lean& a, long long t) {
  AdamStep c;
  c.lr = sched_lr(a.lr, a.lr_tab, a.lr_len, t);
  const float bc1 = 1.f - powf(a.a, (float)t);
  const float bc2 = 1.f - powf(a.b, (float)t);
  c.step_size = c.lr / bc1;
  c.bc2s = sqrtf(bc2);
  return c;
}

template <bool NTP>
__device__ __forceinline__ void adam_f4(const Lean& a, const AdamStep& c, long long i, float4 pp, float4 gg,
                                        float4 mm, float4 vv) {
  const Pack pk{a.pack_off, a.pack_dst, a.pack_mode};
  float4* p4 = reinterpret_cast<float4*>(a.p);
  float4* m4 = reinterpret_cast<float4*>(a.m);
  float4* v4 = reinterpret_cast<float4*>(a.v);
  float* pa = &pp.x; float* ga = &gg.x; float* ma = &mm.x; float* va = &vv.x;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    adam_elem<1>(pa[j], ma[j], va[j], ga[j] * a.grad_scale, c.lr, a.wd, a.flag, a.oma, a.omb, a.b, c.step_size,
                 c.bc2s, a.eps);
    pack_store(pk, 4 * i + j, pa[j]);
  }
  // moments non-temporal, NTP: the parameters too (see the general kernel)
  typedef float nt_f4 __attribute__((ext_vector_type(4)));
  if constexpr (NTP) __builtin_nontemporal_store(*reinterpret_cast<nt_f4*>(&pp), reinterpret_cast<nt_f4*>(p4 + i));
  else p4[i] = pp;
  __builtin_nontemporal_store(*reinterpret_cast<nt_f4*>(&mm), reinterpret_cast<nt_f4*>(m4 + i));
  __builtin_nontemporal_store(*reinterpret_cast<nt_f4*>(&vv), reinterpret_cast<nt_f4*>(v4 + i));
}

// AR = false: no fused all-reduce, one pass.  Order of a block: arguments (one wait); the scalar
// load of *step issued; the first iteration's vector loads issued (a fold block: p / m / v and its
// replicas); only then the wait for the step, the lr table and the bias-correction powf / sqrt /
// divide, all under the vector loads; update and stores.  The sched_barriers pin that order.
template <bool PROF, bool NTP, bool AR>
__global__ __launch_bounds__(256) std::enable_if_t<!AR> k_adam(const Lean a) {
  if constexpr (PROF) {
    if (threadIdx.x == 0) a.prof[(size_t)blockIdx.x * 8] = __builtin_amdgcn_s_memrealtime();
  }
  const long long s0 = *a.step;
  long long f_off[2] = {a.f_off[0], a.f_off[1]};
  asm("" : "+s"(f_off[0]), "+s"(f_off[1]));            // fetched with the other arguments, not on the fold path
  __builtin_amdgcn_sched_barrier(0);
  long long t;
  if ((int)blockIdx.x < a.nfb) {                       // fold block
    const LeanFold f = lean_fold_addr(a, f_off, blockIdx.x);
    float pa = 0.f, ma = 0.f, va = 0.f;
    if (f.e >= 0) {
      pa = a.p[f.e];
      ma = a.m[f.e];
      va = a.v[f.e];
    }
    float4 x[kMaxFold / kLS];
    lean_fold_load(f, x);
    __builtin_amdgcn_sched_barrier(0);
    t = a.bump < 0 ? s0 : s0 + 1;                      // bump < 0: counter pre-advanced by an earlier kernel
    const AdamStep c = adam_step(a, t);
    const float gf = lean_fold_sum(f, x);
    if (f.e >= 0) {
      adam_elem<2>(pa, ma, va, gf * a.grad_scale, c.lr, a.wd, a.flag, a.oma, a.omb, a.b, c.step_size, c.bc2s, a.eps);
      if constexpr (NTP) {
        __builtin_nontemporal_store(pa, a.p + f.e);
        __builtin_nontemporal_store(ma, a.m + f.e);
        __builtin_nontemporal_store(va, a.v + f.e);
        __builtin_nontemporal_store(gf, a.g + f.e);    // p.grad holds the true (folded) gradient
      } else {
        a.p[f.e] = pa; a.m[f.e] = ma; a.v[f.e] = va;
        a.g[f.e] = gf;                                 // p.grad holds the true (folded) gradient
      }
      pack_store(Pack{a.pack_off, a.pack_dst, a.pack_mode}, f.e, pa);
    }
  } else {
    const float4* p4 = reinterpret_cast<const float4*>(a.p);
    const float4* g4 = reinterpret_cast<const float4*>(a.g);
    const float4* m4 = reinterpret_cast<const float4*>(a.m);
    const float4* v4 = reinterpret_cast<const float4*>(a.v);
    const long long mb = (int)blockIdx.x - a.nfb;
    long long ic = mb * 256 + threadIdx.x;
    const long long istride = (long long)a.nmain * 256;
    if (mb * 256 < a.n4c) {                            // block-uniform; false only for an empty buffer
      // iteration 0 leads: unconditional loads (a ragged last block reads its last float4 again)
      const bool on = ic < a.n4c;
      const long long i = hole_map(a.holes, on ? ic : a.n4c - 1);
      const float4 pp = p4[i], gg = g4[i], mm = m4[i], vv = v4[i];
      __builtin_amdgcn_sched_barrier(0);
      t = a.bump < 0 ? s0 : s0 + 1;
      const AdamStep c = adam_step(a, t);
      if (on) adam_f4<NTP>(a, c, i, pp, gg, mm, vv);
      for (ic += istride; ic < a.n4c; ic += istride) {
        const long long i2 = hole_map(a.holes, ic);
        adam_f4<NTP>(a, c, i2, p4[i2], g4[i2], m4[i2], v4[i2]);
      }
    } else {
      t = a.bump < 0 ? s0 : s0 + 1;
    }
  }
  if (a.bump > 0 && last_block(a.arrive, t) && threadIdx.x == 0) {
    a.step[0] = t;
    for (int c = 1; c < a.bump; ++c) a.step[c] += 1;   // extra device counters (e.g. batch position)
    *a.arrive = 0u;
  }
  if constexpr (PROF) {
    if (threadIdx.x == 0) a.prof[(size_t)blockIdx.x * 8 + 1] = __builtin_amdgcn_s_memrealtime();
  }
}

__device__ __forceinline__ void sgd_elem(float& p, float& b, float d, float lr, float momentum, float dampening,
                                         float wd, int nesterov, long long t) {
  if (wd != 0.f) d = d + wd * p;
  if (momentum != 0.f) {
    // a sum of two products: pinned to the contraction hipcc has always chosen here (momentum * b rounded first)
    b = (t == 1) ? d : __builtin_fmaf(1.f - dampening, d, momentum * b);
    d = nesterov ? d + momentum * b : b;
  }
  p = p - lr * d;
}

// torch.optim.SGD semantics (torch/optim/sgd.py): d_p = g + wd*p; buf = momentum*buf + (1-dampening)*d_p
// (buf = d_p on the first step); d_p = nesterov ? d_p + momentum*buf : buf; p -= lr*d_p.
// Same argument struct and block order as the lean Adam kernel (fold blocks first, iteration 0's
// loads ahead of the wait for the step counter).  MOM: momentum != 0, the buffer exists.
template <bool MOM>
__device__ __forceinline__ void sgd_f4(const Lean& a, float lr, long long t, long long i, float4 pp, float4 gg,
                                       float4 bb) {
  const Pack pk{a.pack_off, a.pack_dst, a.pack_mode};
  float* pa = &pp.x; float* ga = &gg.x; float* ba = &bb.x;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    sgd_elem(pa[j], ba[j], ga[j] * a.grad_scale, lr, MOM ? a.a : 0.f, a.b, a.wd, a.flag, t);
    pack_store(pk, 4 * i + j, pa[j]);
  }
  reinterpret_cast<float4*>(a.p)[i] = pp;
  if constexpr (MOM) reinterpret_cast<float4*>(a.m)[i] = bb;
}

// a main block of k_sgd; returns the step t
template <bool MOM>
__device__ __forceinline__ long long sgd_main(const Lean& a, long long s0) {
  const float4* p4 = reinterpret_cast<const float4*>(a.p);
  const float4* g4 = reinterpret_cast<const float4*>(a.g);
  const float4* b4 = reinterpret_cast<const float4*>(a.m);
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  const long long mb = (int)blockIdx.x - a.nfb;
  long long ic = mb * 256 + threadIdx.x;
  const long long istride = (long long)a.nmain * 256;
  if (mb * 256 >= a.n4c) return a.bump < 0 ? s0 : s0 + 1;   // block-uniform; only for an empty buffer
  const bool on = ic < a.n4c;                          // a ragged last block reads its last float4 again
  const long long i = hole_map(a.holes, on ? ic : a.n4c - 1);
  const float4 pp = p4[i], gg = g4[i];
  const float4 bb = MOM ? b4[i] : zero;
  __builtin_amdgcn_sched_barrier(0);
  const long long t = a.bump < 0 ? s0 : s0 + 1;
  const float lr = sched_lr(a.lr, a.lr_tab, a.lr_len, t);
  if (on) sgd_f4<MOM>(a, lr, t, i, pp, gg, bb);
  for (ic += istride; ic < a.n4c; ic += istride) {
    const long long i2 = hole_map(a.holes, ic);
    sgd_f4<MOM>(a, lr, t, i2, p4[i2], g4[i2], MOM ? b4[i2] : zero);
  }
  return t;
}

__global__ __launch_bounds__(256) void k_sgd(const Lean a) {
  const long long s0 = *a.step;
  long long f_off[2] = {a.f_off[0], a.f_off[1]};
  asm("" : "+s"(f_off[0]), "+s"(f_off[1]));            // fetched with the other arguments, not on the fold path
  __builtin_amdgcn_sched_barrier(0);
  const float momentum = a.a;
  long long t;
  if ((int)blockIdx.x < a.nfb) {                       // fold block
    const LeanFold f = lean_fold_addr(a, f_off, blockIdx.x);
    float pa = 0.f, ba = 0.f;
    if (f.e >= 0) {
      pa = a.p[f.e];
      if (momentum != 0.f) ba = a.m[f.e];
    }
    float4 x[kMaxFold / kLS];
    lean_fold_load(f, x);
    __builtin_amdgcn_sched_barrier(0);
    t = a.bump < 0 ? s0 : s0 + 1;
    const float lr = sched_lr(a.lr, a.lr_tab, a.lr_len, t);
    const float gf = lean_fold_sum(f, x);
    if (f.e >= 0) {
      sgd_elem(pa, ba, gf * a.grad_scale, lr, momentum, a.b, a.wd, a.flag, t);
      a.p[f.e] = pa;
      if (momentum != 0.f) a.m[f.e] = ba;
      a.g[f.e] = gf;
      pack_store(Pack{a.pack_off, a.pack_dst, a.pack_mode}, f.e, pa);
    }
  } else {
    t = momentum != 0.f ? sgd_main<true>(a, s0) : sgd_main<false>(a, s0);
  }
  if (a.bump > 0 && last_block(a.arrive, t) && threadIdx.x == 0) {
    a.step[0] = t;
    for (int c = 1; c < a.bump; ++c) a.step[c] += 1;   // extra device counters (e.g. batch position)
    *a.arrive = 0u;
  }
}

__global__ void k_lenet_pack_w2(const float* __restrict__ w2, float* __restrict__ dst) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < 500 * 64) {
    const int kp = i >> 6, co = i & 63, r = kp / 20, ci = kp % 20;
    dst[i] = co < 50 ? w2[co * 500 + ci * 25 + r] : 0.f;
  }
}

__global__ void k_scale(float* __restrict__ x, long long n, float s) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
    x[i] *= s;
}

inline int grid_for(long long n4) {
  long long blocks = (n4 + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  if (blocks < 1) blocks = 1;
  return (int)blocks;
}

// geometry of a lean launch; the hyper-parameters are filled in by the caller
Lean lean_args(float* p, float* g, float* m, float* v, long long n4, long long* step, unsigned* arrive, int bump,
               const Pack& pk, const Fold& fd, const float* lr_tab, int lr_len) {
  Lean a{};
  a.p = p; a.g = g; a.m = m; a.v = v;
  a.step = step; a.arrive = arrive; a.bump = bump;
  a.lr_tab = lr_tab; a.lr_len = lr_len;
  a.pack_dst = pk.dst; a.pack_off = pk.off; a.pack_mode = pk.mode;
  a.holes = make_holes(fd);
  a.n4c = n4 - a.holes.len[0] - a.holes.len[1];
  for (int k = 0; k < 2; ++k) {
    a.f_off[k] = fd.f[k].off; a.f_len[k] = fd.f[k].len; a.f_nrep[k] = fd.f[k].nrep; a.f_s4[k] = fd.f[k].stride / 4;
  }
  a.nfb0 = fold_blocks(fd.f[0]);
  a.nfb = a.nfb0 + fold_blocks(fd.f[1]);
  a.nmain = grid_for(a.n4c);
  return a;
}

bool g_force_general = false;   // pde_optim_force_general

}  // namespace

extern "C" {

void pde_optim_force_general(int on) { g_force_general = on != 0; }

hipError_t pde_adam_flat(float* p, float* g, float* m, float* v, long long n, float lr, float b1, float b2,
                         float eps, float wd, int decoupled, float grad_scale, long long* step, unsigned* arrive,
                         int bump, long long pack_off, float* pack_dst, long long fold_off, int fold_len,
                         int fold_nrep, int fold_stride, const void* peer_dev, long long ar_off, long long* ar_epoch,
                         int ar_two, int pack_mode, long long fold2_off, int fold2_len, int fold2_nrep,
                         int fold2_stride, const float* lr_tab, int lr_len, hipStream_t st) {
  if (n % 4) return hipErrorInvalidValue;
  if (lr_tab != nullptr && lr_len < 1) return hipErrorInvalidValue;
  const long long n4 = n / 4;
  FusedAR ar{};
  if (peer_dev != nullptr && ar_epoch != nullptr) {
    if (ar_off % 4 || ar_off < 0 || ar_off >= n) return hipErrorInvalidValue;
    std::memcpy(&ar.pd, peer_dev, sizeof(ar.pd));
    ar.lo4 = ar_off / 4;
    ar.epoch = ar_epoch;
    ar.two = ar_two;
    const long long m4 = n4 - ar.lo4, work = ar_two ? (m4 + ar.pd.world - 1) / ar.pd.world : m4;
    ar.nvb = (int)std::min<long long>(32, std::max<long long>(1, (work + 255) / 256));
  }
  const Fold fdh{{Fold1{fold_off, fold_len, fold_nrep, fold_stride}, Fold1{fold2_off, fold2_len, fold2_nrep, fold2_stride}}};
  const Holes hh = make_holes(fdh);
  const long long n4c = n4 - hh.len[0] - hh.len[1];
  if (ar.nvb > 0 && (hh.len[0] || hh.len[1]) && hh.lo[0] < ar.lo4) return hipErrorInvalidValue;   // holes above ar range start
  for (int k = 0; k < 2; ++k)
    if (fold_on(fdh.f[k]) && (fdh.f[k].off % 4 || fdh.f[k].stride % 4 || fdh.f[k].nrep > kMaxFold ||
                              fdh.f[k].off + (long long)fdh.f[k].nrep * fdh.f[k].stride > n))
      return hipErrorInvalidValue;
  const int nfb = fold_blocks(fdh.f[0]) + fold_blocks(fdh.f[1]);
  unsigned long long* prof = pde_lenet_prof_slot(5);
  static const bool ntp = [] {
    const char* e = getenv("PDE_ADAM_NT_P");
    return e != nullptr && e[0] == '1';   // default off: neutral in a same-box A/B (profiles/r5_lenet/)
  }();
#define PDE_ADAM_LAUNCH(P, N)                                                                                   \
  hipLaunchKernelGGL((k_adam<P, N, true>), dim3(grid_for(n4c) + ar.nvb + nfb), dim3(256), 0, st, p, g, m, v, n4, lr, b1, \
                     b2, eps, wd, decoupled, grad_scale, step, arrive, bump, Pack{pack_off, pack_dst, pack_mode},    \
                     Fold{{Fold1{fold_off, fold_len, fold_nrep, fold_stride},                                      \
                           Fold1{fold2_off, fold2_len, fold2_nrep, fold2_stride}}},                                \
                     ar, P ? prof : nullptr, lr_tab, lr_len)
#define PDE_ADAM_LEAN(P, N) hipLaunchKernelGGL((k_adam<P, N, false>), dim3(la.nfb + la.nmain), dim3(256), 0, st, la)
  if (ar.nvb == 0 && !g_force_general) {   // no peer: the lean kernel
    Lean la = lean_args(p, g, m, v, n4, step, arrive, bump, Pack{pack_off, pack_dst, pack_mode}, fdh, lr_tab, lr_len);
    la.prof = prof;
    la.lr = lr; la.grad_scale = grad_scale; la.wd = wd; la.flag = decoupled;
    la.a = b1; la.b = b2; la.oma = 1.f - b1; la.omb = 1.f - b2; la.eps = eps;
    if (prof) {
      if (ntp) PDE_ADAM_LEAN(true, true); else PDE_ADAM_LEAN(true, false);
    } else {
      if (ntp) PDE_ADAM_LEAN(false, true); else PDE_ADAM_LEAN(false, false);
    }
  } else if (prof) {
    if (ntp) PDE_ADAM_LAUNCH(true, true); else PDE_ADAM_LAUNCH(true, false);
  } else {
    if (ntp) PDE_ADAM_LAUNCH(false, true); else PDE_ADAM_LAUNCH(false, false);
  }
#undef PDE_ADAM_LEAN
#undef PDE_ADAM_LAUNCH
  return hipGetLastError();
}

hipError_t pde_sgd_flat(float* p, float* g, float* buf, long long n, float lr, float momentum, float dampening,
                        float wd, int nesterov, float grad_scale, long long* step, unsigned* arrive, int bump,
                        long long pack_off, float* pack_dst, long long fold_off, int fold_len, int fold_nrep,
                        int fold_stride, int pack_mode, long long fold2_off, int fold2_len, int fold2_nrep,
                        int fold2_stride, const float* lr_tab, int lr_len, hipStream_t st) {
  if (n % 4) return hipErrorInvalidValue;
  if (lr_tab != nullptr && lr_len < 1) return hipErrorInvalidValue;
  const long long n4 = n / 4;
  const Fold fdh{{Fold1{fold_off, fold_len, fold_nrep, fold_stride}, Fold1{fold2_off, fold2_len, fold2_nrep, fold2_stride}}};
  for (int k = 0; k < 2; ++k)
    if (fold_on(fdh.f[k]) && (fdh.f[k].off % 4 || fdh.f[k].stride % 4 || fdh.f[k].nrep > kMaxFold ||
                              fdh.f[k].off + (long long)fdh.f[k].nrep * fdh.f[k].stride > n))
      return hipErrorInvalidValue;
  Lean la = lean_args(p, g, buf, nullptr, n4, step, arrive, bump, Pack{pack_off, pack_dst, pack_mode}, fdh, lr_tab, lr_len);
  la.lr = lr; la.grad_scale = grad_scale; la.wd = wd; la.flag = nesterov;
  la.a = momentum; la.b = dampening;
  hipLaunchKernelGGL(k_sgd, dim3(la.nfb + la.nmain), dim3(256), 0, st, la);
  return hipGetLastError();
}

hipError_t pde_lenet_pack_w2(const float* w2, float* dst, hipStream_t st) {
  hipLaunchKernelGGL(k_lenet_pack_w2, dim3((500 * 64 + 255) / 256), dim3(256), 0, st, w2, dst);
  return hipGetLastError();
}

hipError_t pde_scale(float* x, long long n, float s, hipStream_t st) {
  hipLaunchKernelGGL(k_scale, dim3(grid_for((n + 3) / 4)), dim3(256), 0, st, x, n, s);
  return hipGetLastError();
}

}  // extern "C"
