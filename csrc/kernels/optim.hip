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
// Every kernel takes the Lean struct: what the host worked out to size the grid (holes, compressed
// length, block counts per role, 1-b1, 1-b2) travels by value, so no block divides or derives
// geometry.  One gradient fold (fold_addr / fold_load / fold_sum), one float4 update (adam_f4), one
// fold-lane update (adam_fold_update), one set of step constants (adam_step) and one step-publish
// tail (publish_step) serve them all.
// k_adam<PROF, NTP, AR>:
//   AR = false, the lean kernel, the base: every call without a peer (the single-GPU LeNet step,
//     GPT-2, ResNet-18).  Fold blocks have the lowest block ids (the longest chain starts first); a
//     block fetches its arguments in one batch, issues the scalar load of *step and its first
//     iteration's vector loads, and only then waits for the step and does the lr-table lookup and
//     the bias-correction powf / sqrt / divide, under the loads.  k_sgd has the same shape.
//   AR = true, the general kernel: the same helpers plus the fused all-reduce roles, whose arguments
//     are the FusedAR struct (Adam only, the W > 1 "fused" LeNet schedule).  The first ar.nvb blocks
//     all-reduce the flat range [ar.lo4, ar.n4) (the conv-gradient bucket) across ranks with the xGMI
//     peer protocol while the main blocks update [0, ar.lo4); those then wait for the reduction (the
//     completing side block publishes the optimizer step t in *ar.epoch) before updating the rest.
//     Side blocks have the lowest block ids, so they are dispatched first: no wait can starve them;
//     the fold blocks, which wait too, have the highest.  None of the lean kernel's load-ordering
//     devices: a plain grid-stride loop.  Also what pde_optim_force_general selects for a peer-less
//     call (no side blocks, one pass), so tests can compare the two kernels.
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

// Gradient replicas: a fold range (PdeFold) is nrep copies of a gradient, stride floats apart.  The
// whole replica set [off, off + nrep*stride) is a hole of the main index space; fold blocks own it.
// Each canonical float4 gets kLS lanes: lane l sums replicas l, l+kLS, ..., a 2-step xor shuffle
// combines the lanes, and lane l then updates element l of the float4 (the old one-thread-per-float4
// fold issued 19 loads per thread on the last ~27 blocks and ended the kernel 2 us after every other
// block).  The guarded loads compile to one basic block each, with a vmcnt(0) between most of them
// (tools/isa_load_order.py); making them unconditional on clamped addresses puts them in one batch
// but did not shorten the fold blocks (profiles/lenet_load_order/rejected_adam_fold_batch/).
constexpr int kMaxFold = 16;
constexpr int kLS = 4;

struct Holes {
  long long lo[2], len[2];   // in float4 units, sorted, lo = huge when unused
};

__device__ __forceinline__ long long hole_map(const Holes& h, long long c) {   // compressed -> real index
  if (c >= h.lo[0]) c += h.len[0];
  if (c >= h.lo[1]) c += h.len[1];
  return c;
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

// the tail of a kernel: the last block to arrive publishes the step and resets the fan-in
__device__ __forceinline__ void publish_step(long long* step, unsigned* arrive, int bump, long long t) {
  if (bump > 0 && last_block(arrive, t) && threadIdx.x == 0) {
    step[0] = t;
    for (int c = 1; c < bump; ++c) step[c] += 1;   // extra device counters (e.g. batch position)
    *arrive = 0u;
  }
}

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
  long long f_off[2];        // fold ranges in block order (range 0's blocks first); see PdeFold
  int f_len[2], f_nrep[2], f_s4[2];   // f_s4 = stride / 4
  int nfb0, nfb;             // fold blocks of range 0, of both ranges; 0 = no fold
  int nmain;                 // main (grid-stride) blocks
  int pack_mode, bump, lr_len, flag;   // flag: Adam decoupled / SGD nesterov
  float lr, grad_scale, wd;
  float a, b, oma, omb, eps;   // Adam: b1, b2, 1-b1, 1-b2, eps; SGD: momentum, dampening
};

// What fold lane (fb, threadIdx.x) works on; fb = fold-block index, 0-based over both ranges.  Known
// before any load, so the optimizer state of the element is fetched in the same round trip as the replicas.
struct FoldAddr {
  long long e;      // flat element this lane updates (-1: none)
  int nrep;         // replicas this lane's float4 has (1 past len)
  int lane;
  const float4* g4; // replica 0 of this lane's float4
  long long s4;
};

__device__ __forceinline__ FoldAddr fold_addr(const Lean& a, const long long (&f_off)[2], int fb) {
  const int k = fb < a.nfb0 ? 0 : 1;
  const int j = (int)(((unsigned)(k ? fb - a.nfb0 : fb) * 256u + threadIdx.x) / kLS);   // float4 in the slot
  const int lane = threadIdx.x % kLS;
  const int s4 = a.f_s4[k];
  const bool valid = j < s4;
  FoldAddr f;
  f.e = valid ? f_off[k] + 4 * j + lane : -1;
  f.nrep = (valid && 4 * j < a.f_len[k]) ? a.f_nrep[k] : (valid ? 1 : 0);
  f.lane = lane;
  f.g4 = reinterpret_cast<const float4*>(a.g + f_off[k]) + (valid ? j : 0);   // f_off % 4 == 0
  f.s4 = s4;
  return f;
}

// the replica loads of a lane, and their sum.  All lanes of the wave take part in the shuffles.
__device__ __forceinline__ void fold_load(const FoldAddr& f, float4 (&x)[kMaxFold / kLS]) {
#pragma unroll
  for (int q = 0; q < kMaxFold / kLS; ++q) {
    const int r = f.lane + q * kLS;
    x[q] = r < f.nrep ? f.g4[(long long)r * f.s4] : make_float4(0.f, 0.f, 0.f, 0.f);
  }
}

__device__ __forceinline__ float fold_sum(const FoldAddr& f, const float4 (&x)[kMaxFold / kLS]) {
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

// the update of a fold lane's element (f.e >= 0) from its loaded state and folded gradient gf
template <bool NTP>
__device__ __forceinline__ void adam_fold_update(const Lean& a, const AdamStep& c, const FoldAddr& f, float pa, float ma,
                                               float va, float gf) {
  adam_elem<2>(pa, ma, va, gf * a.grad_scale, c.lr, a.wd, a.flag, a.oma, a.omb, a.b, c.step_size, c.bc2s, a.eps);
  if constexpr (NTP) {     // NTP: nothing of this launch is left dirty in the XCD L2s (see adam_f4)
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

// AR = false, the lean kernel: no fused all-reduce, one pass.  Block ids: fold blocks first (their
// chain is the longest: seven loads, two shuffle rounds, scattered 4-byte stores and the Wp index
// arithmetic), then the main blocks.  Order of a block: arguments (one wait); the scalar
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
    const FoldAddr f = fold_addr(a, f_off, blockIdx.x);
    float pa = 0.f, ma = 0.f, va = 0.f;
    if (f.e >= 0) {
      pa = a.p[f.e];
      ma = a.m[f.e];
      va = a.v[f.e];
    }
    float4 x[kMaxFold / kLS];
    fold_load(f, x);
    __builtin_amdgcn_sched_barrier(0);
    t = a.bump < 0 ? s0 : s0 + 1;                      // bump < 0: counter pre-advanced by an earlier kernel
    const AdamStep c = adam_step(a, t);
    const float gf = fold_sum(f, x);
    if (f.e >= 0) adam_fold_update<NTP>(a, c, f, pa, ma, va, gf);
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
  // publish_step, spelled out: called here it changes the register allocation of the PROF instantiations
  if (a.bump > 0 && last_block(a.arrive, t) && threadIdx.x == 0) {
    a.step[0] = t;
    for (int c = 1; c < a.bump; ++c) a.step[c] += 1;   // extra device counters (e.g. batch position)
    *a.arrive = 0u;
  }
  if constexpr (PROF) {
    if (threadIdx.x == 0) a.prof[(size_t)blockIdx.x * 8 + 1] = __builtin_amdgcn_s_memrealtime();
  }
}

// What the fused all-reduce roles of the general kernel need beyond Lean.
struct FusedAR {
  pde::PeerDev pd;
  long long n4;             // uncompressed float4 count of the buffer
  long long lo4;            // first float4 of the all-reduced range (range = [lo4, n4)); no hole lies below it
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

// AR = true, the general kernel: the W > 1 adam1 / adam2 routes.  Block ids: ar.nvb side blocks
// (dispatched first, so no waiting block can starve them), a.nmain main blocks, a.nfb fold blocks.
// Main blocks run two passes, [0, ar.lo4) and, once the reduction is complete, [ar.lo4, a.n4c); fold
// blocks wait for it before their loads (the reduced replicas must be complete).  Without side
// blocks (ar.nvb == 0) nothing waits and the one pass is [0, a.n4c).
template <bool PROF, bool NTP, bool AR>
__global__ __launch_bounds__(256) std::enable_if_t<AR> k_adam(const Lean a, const FusedAR ar) {
  if constexpr (PROF) {
    if (threadIdx.x == 0) a.prof[(size_t)blockIdx.x * 8] = __builtin_amdgcn_s_memrealtime();
  }
  const long long t = a.bump < 0 ? *a.step : *a.step + 1;   // bump < 0: counter pre-advanced by an earlier kernel
  __shared__ uint32_t lds2[2];
  const int mb = (int)blockIdx.x - ar.nvb;                  // main-block index; the roles are block-uniform
  AdamStep c{};
  if (mb >= 0) c = adam_step(a, t);                         // side blocks have no use for the step constants
  if (mb < 0) {                                             // side block: no parameter work
    if (pde::peer_ar_f32_vblock(ar.pd, a.g + 4 * ar.lo4, a.g + 4 * ar.lo4, 4 * (ar.n4 - ar.lo4), 1.f, blockIdx.x,
                                ar.nvb, ar.two != 0, lds2))
      __hip_atomic_store(ar.epoch, t, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
  } else if (mb >= a.nmain) {                               // fold block
    if (ar.nvb > 0) wait_epoch(ar.epoch, t, ar.pd);
    const FoldAddr f = fold_addr(a, a.f_off, mb - a.nmain);
    float pa = 0.f, ma = 0.f, va = 0.f;
    if (f.e >= 0) {                                         // issued before the replica loads
      pa = a.p[f.e];
      ma = a.m[f.e];
      va = a.v[f.e];
    }
    float4 x[kMaxFold / kLS];
    fold_load(f, x);
    const float gf = fold_sum(f, x);
    if (f.e >= 0) adam_fold_update<NTP>(a, c, f, pa, ma, va, gf);
  } else {
    const float4* p4 = reinterpret_cast<const float4*>(a.p);
    const float4* g4 = reinterpret_cast<const float4*>(a.g);
    const float4* m4 = reinterpret_cast<const float4*>(a.m);
    const float4* v4 = reinterpret_cast<const float4*>(a.v);
    const long long istride = (long long)a.nmain * 256;
    long long ic = (long long)mb * 256 + threadIdx.x, hi = ar.nvb > 0 ? ar.lo4 : a.n4c;
    for (int pass = 0;; ++pass) {
      for (; ic < hi; ic += istride) {
        const long long i = hole_map(a.holes, ic);
        adam_f4<NTP>(a, c, i, p4[i], g4[i], m4[i], v4[i]);
      }
      if (pass == 1 || ar.nvb == 0) break;
      wait_epoch(ar.epoch, t, ar.pd);                       // the all-reduced range is ready
      ic = ar.lo4 + (long long)mb * 256 + threadIdx.x;
      hi = a.n4c;
    }
  }
  publish_step(a.step, a.arrive, a.bump, t);
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
    const FoldAddr f = fold_addr(a, f_off, blockIdx.x);
    float pa = 0.f, ba = 0.f;
    if (f.e >= 0) {
      pa = a.p[f.e];
      if (momentum != 0.f) ba = a.m[f.e];
    }
    float4 x[kMaxFold / kLS];
    fold_load(f, x);
    __builtin_amdgcn_sched_barrier(0);
    t = a.bump < 0 ? s0 : s0 + 1;
    const float lr = sched_lr(a.lr, a.lr_tab, a.lr_len, t);
    const float gf = fold_sum(f, x);
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
  publish_step(a.step, a.arrive, a.bump, t);
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

inline bool fold_on(const PdeFold& f) { return f.off >= 0 && f.nrep > 1; }

// the layout checks of both entry points
bool flat_layout_ok(const PdeFlatOpt& o) {
  if (o.n % 4) return false;
  if (o.lr_tab != nullptr && o.lr_len < 1) return false;
  for (const PdeFold& f : o.fold)
    if (fold_on(f) && (f.off % 4 || f.stride % 4 || f.nrep > kMaxFold || f.off + (long long)f.nrep * f.stride > o.n))
      return false;
  return true;
}

// The kernel arguments of a checked call: everything but the optimizer's own hyper-parameters (flag, a, b, ...).
// A fold range gets kLS lanes for each float4 of its canonical slot (stride / 4 float4s).
Lean lean_args(const PdeFlatOpt& o) {
  Lean a{};
  a.p = o.p; a.g = o.g; a.m = o.m; a.v = o.v;
  a.step = o.step; a.arrive = o.arrive; a.bump = o.bump;
  a.lr_tab = o.lr_tab; a.lr_len = o.lr_len;
  a.pack_dst = o.pack_dst; a.pack_off = o.pack_off; a.pack_mode = o.pack_mode;
  a.lr = o.lr; a.grad_scale = o.grad_scale; a.wd = o.wd;
  a.holes = Holes{{(long long)1 << 60, (long long)1 << 60}, {0, 0}};
  int nfb[2] = {0, 0};
  for (int k = 0; k < 2; ++k) {
    const PdeFold& f = o.fold[k];
    a.f_off[k] = f.off; a.f_len[k] = f.len; a.f_nrep[k] = f.nrep; a.f_s4[k] = f.stride / 4;
    if (!fold_on(f)) continue;
    a.holes.lo[k] = f.off / 4;
    a.holes.len[k] = (long long)f.nrep * f.stride / 4;
    nfb[k] = (int)(((long long)f.stride / 4 * kLS + 255) / 256);
  }
  if (a.holes.lo[1] < a.holes.lo[0]) {
    std::swap(a.holes.lo[0], a.holes.lo[1]);
    std::swap(a.holes.len[0], a.holes.len[1]);
  }
  a.n4c = o.n / 4 - a.holes.len[0] - a.holes.len[1];
  a.nfb0 = nfb[0];
  a.nfb = nfb[0] + nfb[1];
  a.nmain = grid_for(a.n4c);
  return a;
}

bool g_force_general = false;   // pde_optim_force_general

}  // namespace

extern "C" {

void pde_optim_force_general(int on) { g_force_general = on != 0; }

hipError_t pde_adam_flat(const PdeFlatOpt* o, float b1, float b2, float eps, int decoupled, const void* peer_dev,
                         long long ar_off, long long* ar_epoch, int ar_two, hipStream_t st) {
  if (!flat_layout_ok(*o)) return hipErrorInvalidValue;
  Lean la = lean_args(*o);
  la.prof = pde_lenet_prof_slot(5);
  la.flag = decoupled;
  la.a = b1; la.b = b2; la.oma = 1.f - b1; la.omb = 1.f - b2; la.eps = eps;
  FusedAR ar{};
  ar.n4 = o->n / 4;
  if (peer_dev != nullptr && ar_epoch != nullptr) {
    if (ar_off % 4 || ar_off < 0 || ar_off >= o->n) return hipErrorInvalidValue;
    std::memcpy(&ar.pd, peer_dev, sizeof(ar.pd));
    ar.lo4 = ar_off / 4;
    ar.epoch = ar_epoch;
    ar.two = ar_two;
    const long long m4 = ar.n4 - ar.lo4, work = ar_two ? (m4 + ar.pd.world - 1) / ar.pd.world : m4;
    ar.nvb = (int)std::min<long long>(32, std::max<long long>(1, (work + 255) / 256));
  }
  if (ar.nvb > 0 && (la.holes.len[0] || la.holes.len[1]) && la.holes.lo[0] < ar.lo4)
    return hipErrorInvalidValue;   // holes above ar range start
  static const bool ntp = [] {
    const char* e = getenv("PDE_ADAM_NT_P");
    return e != nullptr && e[0] == '1';   // default off: neutral in a same-box A/B (profiles/r5_lenet/)
  }();
  const bool lean = ar.nvb == 0 && !g_force_general;   // no peer: the lean kernel
  const dim3 grid(ar.nvb + la.nmain + la.nfb);
#define PDE_ADAM_LAUNCH(P, N)                                                                 \
  do {                                                                                        \
    if (lean) hipLaunchKernelGGL((k_adam<P, N, false>), grid, dim3(256), 0, st, la);          \
    else hipLaunchKernelGGL((k_adam<P, N, true>), grid, dim3(256), 0, st, la, ar);            \
  } while (0)
  if (la.prof) {
    if (ntp) PDE_ADAM_LAUNCH(true, true); else PDE_ADAM_LAUNCH(true, false);
  } else {
    if (ntp) PDE_ADAM_LAUNCH(false, true); else PDE_ADAM_LAUNCH(false, false);
  }
#undef PDE_ADAM_LAUNCH
  return hipGetLastError();
}

hipError_t pde_sgd_flat(const PdeFlatOpt* o, float momentum, float dampening, int nesterov, hipStream_t st) {
  if (!flat_layout_ok(*o)) return hipErrorInvalidValue;
  Lean la = lean_args(*o);
  la.flag = nesterov;
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
