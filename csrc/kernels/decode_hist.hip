// The sampler with the history constraints (no-repeat n-gram, banned sequences, stop sequences) on top of the
// logit processors.  PdeSampleHist is documented in pde_decode.h, the kernel in decode_sample.h.  A unit of its
// own for the reason decode_proc.hip is one: the instantiations that existed keep their instruction streams.
#include "pde_hip.h"
#include "pde_bf16.h"
#include "pde_decode.h"
#include "pde_rng.h"

#include <math.h>

namespace {

#include "decode_sample.h"

}  // namespace

extern "C" {

hipError_t pde_sample_hist(PdeSample a, PdeSampleProc p, PdeSampleHist h, hipStream_t st) {
  if (a.B < 1 || a.B > PDE_DS_MAX_ROWS || a.V < 1 || a.V > a.Vp || a.Vp % 8 != 0 || a.top_k < 0)
    return hipErrorInvalidValue;
  if (!(a.top_p >= 0.0)) return hipErrorInvalidValue;
  if (!p.counts || !p.work || (p.bias && p.bias_stride != 0 && p.bias_stride != a.Vp)) return hipErrorInvalidValue;
  if (p.min_new < 0 || (p.min_new > 0 && a.eos < 0) || a.eos >= a.V) return hipErrorInvalidValue;
  if (!a.out || a.out_stride < 1 || h.n < 0 || h.n > PDE_HIST_MAX_NGRAM) return hipErrorInvalidValue;
  if (h.n_ban < 0 || h.n_ban > PDE_HIST_MAX_SEQS || (h.n_ban > 0 && !h.ban)) return hipErrorInvalidValue;
  if (h.n_stop < 0 || h.n_stop > PDE_HIST_MAX_SEQS) return hipErrorInvalidValue;
  if (h.n_stop > 0 && (!h.stop || !h.stop_hit || a.eos < 0)) return hipErrorInvalidValue;
  if (!a.greedy && a.top_p > 0.0 && a.top_p < 1.0)
    hipLaunchKernelGGL((k_sample<true, PdeSampleProc, PdeSampleHist>), dim3(a.B), dim3(SM_NT), 0, st, a, p, h);
  else
    hipLaunchKernelGGL((k_sample<false, PdeSampleProc, PdeSampleHist>), dim3(a.B), dim3(SM_NT), 0, st, a, p, h);
  PDE_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(k_dec_advance, dim3(1), dim3(64), 0, st, a.state);
  return hipGetLastError();
}

}  // extern "C"
