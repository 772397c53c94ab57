// extern "C" launchers of the GPT-2 decode kernels (csrc/kernels/decode.hip) and the layout of the
// device-side decode state they share.
//
// Everything that changes from one generated token to the next lives in the state buffer, never in a
// launch argument, so one captured decode step replays correctly for every token:
//
//   words 0..3   sampling RNG state {seed lo, seed hi, draw, stream}  (ops/rng.py DeviceRNG layout)
//   word  4      position p of the token the next decode step embeds / attends from
//   word  5      step: index of the next token to generate (output slot T0 + step)
//   words 6, 7   reserved
//   words 8..23  per-row "finished" flags (a row that has emitted eos keeps emitting it)
//   words 24..39 per-row position offsets off_b = len_b - max(len) <= 0 of a ragged prompt batch, constant
//                for the whole generation: row b is at position p + off_b and its output slot is
//                T0 + off_b + step, with T0 = max(len) the launch argument.  All zero: one prompt length.
//
// The sampler launch reads the state; its one-thread tail kernel advances p, step and the draw number.
//
// The logit processors (repetition / frequency / presence penalties, logit bias, min_new_tokens) keep their
// history in a buffer of their own, the token counts: int32 [B, Vp], word (b, v) =
//
//   bit  30      token v occurs in the prompt of row b (set once by pde_count_prompt, never cleared)
//   bits 0..29   n_v: how often row b has generated v so far (the sampler adds 1 at the token it emits)
//
// so "seen" is word != 0.  The state and its 40 words do not change.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#define PDE_DS_RNG 0
#define PDE_DS_POS 4
#define PDE_DS_STEP 5
#define PDE_DS_FIN 8
#define PDE_DS_MAX_ROWS 16
#define PDE_DS_OFF 24
#define PDE_DS_WORDS 40
#define PDE_TC_PROMPT 0x40000000       // token counts: the prompt flag
#define PDE_TC_COUNT 0x3fffffff        // token counts: mask of n_v

#ifdef __cplusplus
extern "C" {
#endif

// y[M, N] = x[M, K] W[N, K]^T (+ bias) (-> tanh-GELU), bf16, 1 <= M <= 16, K % 64 == 0, N % 8 == 0.
// pde_skinny_splits(N, K) > 1 means the launch splits K over that many blocks per row tile and needs
// `part`: splits * M * N floats (slabs summed in slab order by a second kernel).
int pde_skinny_splits(int N, int K);
hipError_t pde_skinny_linear(const void* x, const void* W, const void* bias, void* y, float* part, int M, int N, int K,
                             int gelu, hipStream_t st);

// keys per block of the decode attention (a constant of the kernel)
int pde_decode_attn_chunk(void);
// cache: one layer, [2][B][H][Tmax][64] bf16; qkv: [B, 3 * H * 64] c_attn output of the new token, row b at
// position p_b = state[PDE_DS_POS] + state[PDE_DS_OFF + b] (B <= PDE_DS_MAX_ROWS);
// part: B * H * ceil(Tmax / chunk) * 66 floats; out: [B, H * 64]
hipError_t pde_decode_attention(const void* qkv, void* cache, const int* state, float* part, void* out, int B, int H,
                                int Tmax, float scale, hipStream_t st);
// K and V of positions 0 .. T0-1 of a prefill c_attn output [B, Tpad, 3 * H * 64] -> one layer's cache
hipError_t pde_cache_fill(const void* qkv, void* cache, int B, int H, int Tpad, int T0, int Tmax, hipStream_t st);
// out[b] = wte[tok[b]] + wpe[p_b]
hipError_t pde_decode_embed(const int64_t* tok, const void* wte, const void* wpe, const int* state, void* out, int B,
                            int C, int Vp, int n_pos, hipStream_t st);

typedef struct PdeSample {
  const void* logits;   // [B, Vp] bf16
  int* state;           // PDE_DS_WORDS
  int64_t* next;        // [B]
  int64_t* out;         // [B, out_stride]; token -> out[b, T0 + off_b + step]
  void* logits_out;     // [B, max_new, V] bf16 or null
  int* thr_out;         // [B] or null (tests): the effective threshold (top-k, raised by top-p) as its 16-bit
                        // key, 0 with neither
  int B, V, Vp, T0, out_stride, max_new;
  float inv_temp;       // fp32(1 / temperature); unused when greedy
  int greedy;           // temperature == 0
  int top_k;            // 0: all V
  int eos;              // -1: none
  double top_p;         // nucleus mass in (0, 1); 0 or >= 1: off.  Unused when greedy
} PdeSample;
hipError_t pde_sample(PdeSample a, hipStream_t st);

// The logit processors of a sampler launch.  With x the fp32 value of a logit, c the counts word of (b, v),
// n = c & PDE_TC_COUNT and s the state's step, every operation rounded on its own (no fused multiply-add):
//   if (c != 0) x = x > 0 ? x * inv_rep : x * rep;
//   x = (x - freq * float(n)) - (n > 0 ? pres : 0);
//   if (bias) x = x + bias[b * bias_stride + v];
//   if (s < min_new && v == eos) x = -inf;
//   y = bf16(x), round-to-nearest-even
// The sampler of pde_sample then runs on y, and counts[b, token] += 1.  logits_out keeps receiving the raw row.
typedef struct PdeSampleProc {
  int* counts;          // [B, Vp] token counts
  const float* bias;    // [1 or B, Vp] fp32 (pad columns 0), 16-byte aligned, or null
  void* work;           // [B, Vp] bf16, 16-byte aligned: receives y (all Vp columns of every row)
  int bias_stride;      // Vp, or 0 for one row shared by the batch
  int min_new;          // 0: off; needs eos >= 0 otherwise
  float rep, inv_rep;   // fp32(r), fp32(1 / r); 1, 1: off
  float freq, pres;
} PdeSampleProc;
hipError_t pde_sample_proc(PdeSample a, PdeSampleProc p, hipStream_t st);

// The history constraints of a sampler launch, on top of the logit processors.  Row b's history is
// h[0 .. L-1] = out[b, 0 : L] with L = len_b + step, len_b = T0 + state[PDE_DS_OFF + b], both from the state.
// A sequence table is packed int32: [count + 1 offsets][tokens], sequence q = tokens[offsets[q] .. offsets[q + 1]).
//   n-gram (n >= 1, L >= n - 1):  v is banned iff h[j-n+1 .. j-1] == h[L-n+1 .. L-1] and h[j] == v for some
//                                 n - 1 <= j <= L - 1
//   banned sequence of m tokens:  seq[m-1] is banned iff L >= m - 1 and h[L-m+1 .. L-1] == seq[0 .. m-2]
//   a ban:                        y = -inf, after the bias and before the sampling; a finished row has none
//   stop sequence of m tokens:    a row that was not finished and emits `tok` at step s becomes finished, and
//                                 stop_hit[b] = the lowest such q, iff s + 1 >= m and
//                                 out[b, len_b+s-m+1 .. len_b+s] == seq with tok in place (needs eos >= 0)
// Tokens outside [0, V) ban nothing.  Nothing is read from `out` at or past L.
#define PDE_HIST_MAX_NGRAM 8
#define PDE_HIST_MAX_SEQS 256          // per table
typedef struct PdeSampleHist {
  const int* ban;       // table of banned sequences, or null with n_ban == 0
  const int* stop;      // table of stop sequences, or null with n_stop == 0
  int* stop_hit;        // [B]; needed with n_stop > 0
  int n;                // no_repeat_ngram_size, 0: off
  int n_ban, n_stop;
} PdeSampleHist;
hipError_t pde_sample_hist(PdeSample a, PdeSampleProc p, PdeSampleHist h, hipStream_t st);

// counts[b, idx[b, t]] = PDE_TC_PROMPT for t < len_b = T0 + state[PDE_DS_OFF + b] (clamped to [0, width]); idx is
// [B, width] with row stride `stride`.  To be called on zeroed counts: duplicates store the same word, so the
// stores need no atomic.  Tokens outside [0, Vp) are skipped.
hipError_t pde_count_prompt(const int64_t* idx, const int* state, int* counts, int B, int width, int stride, int T0,
                            int Vp, hipStream_t st);

// ------------------------------------------------------------------------------------------ beam search
// num_beams = K hypotheses per prompt live in the physical rows r = b * K + k of the R = B * K <= PDE_DS_MAX_ROWS
// rows the decode step has; the rows of one prompt share its position offset.  The KV cache is never reordered:
// an ancestor table says which physical row holds each position's K and V of the hypothesis that lives in row r.
//
//   anc        bytes [2][PDE_DS_MAX_ROWS][stride], stride >= Tmax and a multiple of 4.  A decode step at the state's
//              step s reads half s & 1; the beam step at s reads that half and writes the other one:
//              anc'[b*K + j][t] = anc[b*K + parent_j][t] for t < p_b, and anc'[b*K + j][p_b] = b*K + parent_j (the
//              parent's own row, where it appended position p_b).  Entries past p_b are never read.
//   state      words 8..23 are the rows' finished flags, as for the sampler; the draw number does not move.
typedef struct PdeBeamTable {
  const unsigned char* anc;
  int stride;
} PdeBeamTable;
// pde_decode_attention with key j < p_b of row b read from cache row anc[b][j]; row p_b is appended to row b
hipError_t pde_decode_attention_beam(const void* qkv, void* cache, const int* state, float* part, void* out, int B,
                                     int H, int Tmax, float scale, PdeBeamTable t, hipStream_t st);

// One beam step (definition: ops/decode.py).  Stage 1, a block per row: lse_r and the row's K best logits, lowest
// index first among equal ones, as (score = S[r] + (x - lse_r), token) pairs in cand_*.  Stage 2, a block per
// prompt: the K best of the group's candidates by (score descending, parent * V + token ascending) become the new
// rows; it writes next, S, the finished flags, len, the trace slots of step s and the other half of the table.  A
// one-thread tail then advances position and step.
typedef struct PdeBeam {
  const void* logits;     // [R, Vp] bf16; at step 0 only rows b * K are read
  int* state;             // PDE_DS_WORDS
  int64_t* next;          // [R]
  float* score;           // [R] S
  int* len;               // [R] generated tokens, the finishing eos included
  float* cand_score;      // [R, K] workspace
  int* cand_tok;          // [R, K] workspace
  unsigned char* anc;     // the table, both halves
  int* tok_trace;         // [max_new, R]
  int* parent_trace;      // [max_new, R]
  float* score_trace;     // [max_new, R]
  void* logits_out;       // [R, max_new, V] bf16 or null
  int B, K, V, Vp, Tmax, stride, max_new;
  int eos;                // -1: none
} PdeBeam;
hipError_t pde_beam_step(PdeBeam a, hipStream_t st);

// After the last step: rank the K rows of every prompt by S / len^length_penalty (descending, lower row first on
// ties; computed in fp64) and write hypothesis of rank i to out[b, i, len_b .. len_b + n_steps) by walking the
// parents back from its last row, one thread per hypothesis; scores[b, i] = fp32 of its ranking score.
typedef struct PdeBeamFinal {
  const int* state;
  const float* score;
  const int* len;
  const int* tok_trace;
  const int* parent_trace;
  int64_t* out;           // [B, K, out_stride]
  float* scores;          // [B, K]
  int B, K, T0, out_stride, n_steps;
  double length_penalty;
} PdeBeamFinal;
hipError_t pde_beam_finalize(PdeBeamFinal a, hipStream_t st);

// pde_cache_fill for a beam search: prompt b of the prefill c_attn output [B, Tpad, 3 * H * 64] goes to row
// b * K of a cache of B * K rows
hipError_t pde_cache_fill_beam(const void* qkv, void* cache, int B, int K, int H, int Tpad, int T0, int Tmax,
                               hipStream_t st);

#ifdef __cplusplus
}
#endif
