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
  return sample_ok(a) && proc_ok(a, p) && hist_ok(a, h) ? sample_launch(a, st, p, h) : hipErrorInvalidValue;
}

}  // extern "C"
