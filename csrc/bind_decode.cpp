// torch bindings of the GPT-2 decode kernels (csrc/kernels/decode.hip).
// Every entry validates device / dtype / contiguity / shape / alignment before launching on the current stream.
#include "pde_bind.h"
#include "pde_decode.h"

namespace pde {
namespace {

void check_al16(const at::Tensor& t, const char* name) {
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, name, " must be 16-byte aligned");
}

void check_state(const at::Tensor& state) {
  check_cuda(state, "decode state", I32, PDE_DS_WORDS);
  TORCH_CHECK(state.numel() == PDE_DS_WORDS, "decode state holds ", PDE_DS_WORDS, " words");
}

int64_t skinny_splits(int64_t N, int64_t K) { return pde_skinny_splits((int)N, (int)K); }

void skinny_linear(const at::Tensor& x, const at::Tensor& w, const OptT& bias, const at::Tensor& y, const OptT& part,
                   bool gelu) {
  TORCH_CHECK(x.dim() == 2 && w.dim() == 2 && y.dim() == 2, "skinny_linear: x [M, K], w [N, K], y [M, N]");
  const int64_t M = x.size(0), K = x.size(1), N = w.size(0);
  TORCH_CHECK(M >= 1 && M <= 16, "skinny_linear: 1 <= M <= 16, got ", M);
  TORCH_CHECK(K % 64 == 0 && K >= 64 && N % 8 == 0 && N >= 8, "skinny_linear: K % 64 == 0 and N % 8 == 0, got K ", K,
              ", N ", N);
  TORCH_CHECK(w.size(1) == K && y.size(0) == M && y.size(1) == N, "skinny_linear: shapes do not match");
  check_cuda(x, "x", BF16);
  check_cuda(w, "w", BF16);
  check_cuda(y, "y", BF16);
  check_al16(x, "x");
  check_al16(w, "w");
  check_al16(y, "y");
  const void* bp = optr<void>(bias, "bias", BF16, N);
  TORCH_CHECK(bp == nullptr || reinterpret_cast<uintptr_t>(bp) % 8 == 0, "bias must be 8-byte aligned");
  const int64_t S = pde_skinny_splits((int)N, (int)K);
  float* pp = optr<float>(part, "part", F32, S > 1 ? S * M * N : 0);
  TORCH_CHECK(S == 1 || pp != nullptr, "skinny_linear: this shape splits K ", S, " ways and needs `part`");
  TORCH_CHECK(pp == nullptr || reinterpret_cast<uintptr_t>(pp) % 16 == 0, "part must be 16-byte aligned");
  hip_check(pde_skinny_linear(x.data_ptr(), w.data_ptr(), bp, y.data_ptr(), pp, (int)M, (int)N, (int)K, gelu ? 1 : 0,
                              cur_stream()),
            "skinny_linear");
}

int64_t decode_attn_chunk() { return pde_decode_attn_chunk(); }

// cache: one layer [2, B, H, Tmax, 64]
void check_cache(const at::Tensor& cache, int64_t B, int64_t H) {
  check_cuda(cache, "cache", BF16);
  TORCH_CHECK(cache.dim() == 5 && cache.size(0) == 2 && cache.size(1) == B && cache.size(2) == H && cache.size(4) == 64,
              "cache layer must be [2, B, H, Tmax, 64]");
  check_al16(cache, "cache");
}

void decode_attention(const at::Tensor& qkv, const at::Tensor& cache, const at::Tensor& state, const at::Tensor& part,
                      const at::Tensor& out, int64_t H, double scale) {
  TORCH_CHECK(qkv.dim() == 2 && H >= 1 && qkv.size(1) == 3 * H * 64, "decode_attention: qkv must be [B, 3 * H * 64]");
  const int64_t B = qkv.size(0);
  TORCH_CHECK(B >= 1 && B <= PDE_DS_MAX_ROWS, "decode_attention: 1 <= B <= ", PDE_DS_MAX_ROWS, ", got ", B);
  check_cuda(qkv, "qkv", BF16);
  check_al16(qkv, "qkv");
  check_cache(cache, B, H);
  const int64_t Tmax = cache.size(3), nch = (Tmax + pde_decode_attn_chunk() - 1) / pde_decode_attn_chunk();
  check_state(state);
  check_cuda(part, "part", F32, B * H * nch * 66);
  check_cuda(out, "out", BF16, B * H * 64);
  hip_check(pde_decode_attention(qkv.data_ptr(), cache.data_ptr(), ptr<int>(state), ptr<float>(part), out.data_ptr(),
                                 (int)B, (int)H, (int)Tmax, (float)scale, cur_stream()),
            "decode_attention");
}

void cache_fill(const at::Tensor& qkv, const at::Tensor& cache, int64_t T0, int64_t H) {
  TORCH_CHECK(qkv.dim() == 3 && H >= 1 && qkv.size(2) == 3 * H * 64, "cache_fill: qkv must be [B, Tpad, 3 * H * 64]");
  const int64_t B = qkv.size(0), Tpad = qkv.size(1);
  check_cuda(qkv, "qkv", BF16);
  check_al16(qkv, "qkv");
  check_cache(cache, B, H);
  TORCH_CHECK(T0 >= 1 && T0 <= Tpad && T0 <= cache.size(3), "cache_fill: 1 <= T0 <= min(Tpad, Tmax), got ", T0);
  hip_check(pde_cache_fill(qkv.data_ptr(), cache.data_ptr(), (int)B, (int)H, (int)Tpad, (int)T0, (int)cache.size(3),
                           cur_stream()),
            "cache_fill");
}

void decode_embed(const at::Tensor& tok, const at::Tensor& wte, const at::Tensor& wpe, const at::Tensor& state,
                  const at::Tensor& out) {
  check_cuda(tok, "tok", I64);
  check_cuda(wte, "wte", BF16);
  check_cuda(wpe, "wpe", BF16);
  TORCH_CHECK(wte.dim() == 2 && wpe.dim() == 2 && wte.size(1) == wpe.size(1) && wte.size(1) % 8 == 0,
              "decode_embed: wte [Vp, C], wpe [n_pos, C], C % 8 == 0");
  const int64_t B = tok.numel(), C = wte.size(1);
  TORCH_CHECK(B >= 1 && B <= PDE_DS_MAX_ROWS, "decode_embed: 1 <= B <= ", PDE_DS_MAX_ROWS, ", got ", B);
  check_cuda(out, "out", BF16, B * C);
  check_al16(wte, "wte");
  check_al16(wpe, "wpe");
  check_al16(out, "out");
  check_state(state);
  hip_check(pde_decode_embed(ptr<int64_t>(tok), wte.data_ptr(), wpe.data_ptr(), ptr<int>(state), out.data_ptr(), (int)B,
                             (int)C, (int)wte.size(0), (int)wpe.size(0), cur_stream()),
            "decode_embed");
}

bool given(const OptT& t) { return t.has_value() && t->defined(); }

// the checked core arguments of the sampler entry
PdeSample sample_args(const at::Tensor& logits, int64_t V, const at::Tensor& state, const at::Tensor& next,
                      const at::Tensor& out, const OptT& logits_out, int64_t T0, double inv_temp, bool greedy,
                      int64_t top_k, int64_t eos, const OptT& thr_out, double top_p) {
  check_cuda(logits, "logits", BF16);
  TORCH_CHECK(logits.dim() == 2 && logits.size(1) % 8 == 0, "sample: logits must be [B, Vp] with Vp % 8 == 0");
  const int64_t B = logits.size(0), Vp = logits.size(1);
  TORCH_CHECK(B >= 1 && B <= PDE_DS_MAX_ROWS, "sample: 1 <= B <= ", PDE_DS_MAX_ROWS, ", got ", B);
  TORCH_CHECK(V >= 1 && V <= Vp, "sample: 1 <= V <= Vp");
  TORCH_CHECK(top_k >= 0 && eos >= -1 && eos < V, "sample: top_k >= 0 and eos in [-1, V)");
  TORCH_CHECK(top_p >= 0.0 && top_p <= 1.0, "sample: top_p in [0, 1] (0 and 1: off), got ", top_p);
  check_al16(logits, "logits");
  check_state(state);
  check_cuda(next, "next", I64, B);
  check_cuda(out, "out", I64);
  TORCH_CHECK(out.dim() == 2 && out.size(0) == B && T0 >= 0 && T0 <= out.size(1), "sample: out must be [B, >= T0]");
  PdeSample a{};
  a.logits = logits.data_ptr();
  a.state = ptr<int>(state);
  a.next = ptr<int64_t>(next);
  a.out = ptr<int64_t>(out);
  a.logits_out = nullptr;
  a.max_new = 0;
  if (given(logits_out)) {
    check_cuda(*logits_out, "logits_out", BF16);
    TORCH_CHECK(logits_out->dim() == 3 && logits_out->size(0) == B && logits_out->size(2) == V,
                "sample: logits_out must be [B, max_new, V]");
    a.logits_out = logits_out->data_ptr();
    a.max_new = (int)logits_out->size(1);
  }
  a.thr_out = optr<int>(thr_out, "thr_out", I32, B);
  a.B = (int)B;
  a.V = (int)V;
  a.Vp = (int)Vp;
  a.T0 = (int)T0;
  a.out_stride = (int)out.size(1);
  a.inv_temp = (float)inv_temp;
  a.greedy = greedy ? 1 : 0;
  a.top_k = (int)top_k;
  a.eos = (int)eos;
  a.top_p = top_p;
  return a;
}

// The sampler with the logit processors (PdeSampleProc in pde_decode.h).  counts: int32 [B, Vp]; bias: fp32
// [1 or B, Vp] or None; work: bf16 [B, Vp], receives the processed logits; rep / inv_rep: fp32(r), fp32(1 / r).
PdeSampleProc proc_args(const PdeSample& a, const at::Tensor& logits, const at::Tensor& counts, const OptT& bias,
                        const at::Tensor& work, double rep, double inv_rep, double freq, double pres, int64_t min_new) {
  const int64_t B = a.B, Vp = a.Vp, eos = a.eos;
  check_cuda(counts, "counts", I32, B * Vp);
  TORCH_CHECK(counts.dim() == 2 && counts.size(0) == B && counts.size(1) == Vp, "sample: counts must be [B, Vp]");
  check_al16(counts, "counts");
  check_cuda(work, "processed_out", BF16, B * Vp);
  TORCH_CHECK(work.dim() == 2 && work.size(0) == B && work.size(1) == Vp, "sample: processed_out must be [B, Vp]");
  check_al16(work, "processed_out");
  TORCH_CHECK(work.data_ptr() != logits.data_ptr(), "sample: processed_out must not be the logits");
  PdeSampleProc p{};
  p.counts = ptr<int>(counts);
  p.work = work.data_ptr();
  p.bias = nullptr;
  p.bias_stride = 0;
  if (given(bias)) {
    check_cuda(*bias, "bias", F32);
    TORCH_CHECK(bias->dim() == 2 && (bias->size(0) == 1 || bias->size(0) == B) && bias->size(1) == Vp,
                "sample: the padded bias must be [1 or B, Vp]");
    check_al16(*bias, "bias");
    p.bias = ptr<float>(*bias);
    p.bias_stride = bias->size(0) == 1 ? 0 : (int)Vp;
  }
  TORCH_CHECK(rep > 0.0 && inv_rep > 0.0, "sample: repetition penalty must be > 0");
  TORCH_CHECK(min_new >= 0 && (min_new == 0 || eos >= 0), "sample: min_new_tokens >= 0, and > 0 needs eos");
  p.min_new = (int)std::min<int64_t>(min_new, INT32_MAX);
  p.rep = (float)rep;
  p.inv_rep = (float)inv_rep;
  p.freq = (float)freq;
  p.pres = (float)pres;
  return p;
}

// a packed sequence table (PdeSampleHist in pde_decode.h): int32 [count + 1 offsets][tokens], or None with count 0
const int* seq_table(const OptT& t, int64_t count, const char* name) {
  TORCH_CHECK(count >= 0 && count <= PDE_HIST_MAX_SEQS, "sample: ", name, " holds 0 .. ", PDE_HIST_MAX_SEQS,
              " sequences, got ", count);
  if (count == 0) return nullptr;
  TORCH_CHECK(given(t), "sample: ", name, " is missing");
  check_cuda(*t, name, I32);
  TORCH_CHECK(t->dim() == 1 && t->numel() >= 2 * count + 1, "sample: ", name, " must be [count + 1 offsets][tokens]");
  return ptr<int>(*t);
}

// The one sampler entry.  The processor group (counts, bias, work, rep, inv_rep, freq, pres, min_new) is on when counts
// and work are given and launches pde_sample_proc; the history group (ngram, ban, n_ban, stop, n_stop, stop_hit) is on
// when any of its arguments is set, needs the processor group (the history kernel sits on the processors' prologue)
// and launches pde_sample_hist.  ban / stop: packed int32 sequence tables or None; stop_hit: int32 [B], needed with
// stop sequences.  A group given in part is an error.
void sample(const at::Tensor& logits, int64_t V, const at::Tensor& state, const at::Tensor& next, const at::Tensor& out,
            const OptT& logits_out, int64_t T0, double inv_temp, bool greedy, int64_t top_k, int64_t eos,
            const OptT& thr_out, double top_p, const OptT& counts, const OptT& bias, const OptT& work, double rep,
            double inv_rep, double freq, double pres, int64_t min_new, int64_t ngram, const OptT& ban, int64_t n_ban,
            const OptT& stop, int64_t n_stop, const OptT& stop_hit) {
  const PdeSample a = sample_args(logits, V, state, next, out, logits_out, T0, inv_temp, greedy, top_k, eos, thr_out,
                                  top_p);
  const bool proc = given(counts) && given(work);
  const bool hist = ngram != 0 || n_ban != 0 || n_stop != 0 || given(ban) || given(stop) || given(stop_hit);
  TORCH_CHECK(given(counts) == given(work), "sample: the processors take counts and work together");
  TORCH_CHECK(proc || (!given(bias) && rep == 1.0 && inv_rep == 1.0 && freq == 0.0 && pres == 0.0 && min_new == 0),
              "sample: processor arguments need counts and work");
  TORCH_CHECK(proc || !hist, "sample: the history constraints need the processors' counts and work");
  if (!proc) {
    hip_check(pde_sample(a, cur_stream()), "sample");
    return;
  }
  const PdeSampleProc p = proc_args(a, logits, *counts, bias, *work, rep, inv_rep, freq, pres, min_new);
  if (!hist) {
    hip_check(pde_sample_proc(a, p, cur_stream()), "sample");
    return;
  }
  TORCH_CHECK(out.is_contiguous(), "sample: out must be contiguous");
  TORCH_CHECK(ngram >= 0 && ngram <= PDE_HIST_MAX_NGRAM, "sample: no_repeat_ngram_size in 0 .. ", PDE_HIST_MAX_NGRAM,
              ", got ", ngram);
  PdeSampleHist h{};
  h.n = (int)ngram;
  h.ban = seq_table(ban, n_ban, "the banned sequences");
  h.stop = seq_table(stop, n_stop, "the stop sequences");
  h.n_ban = (int)n_ban;
  h.n_stop = (int)n_stop;
  h.stop_hit = optr<int>(stop_hit, "stop_hit", I32, a.B);
  TORCH_CHECK(n_stop == 0 || (h.stop_hit != nullptr && eos >= 0), "sample: stop sequences need stop_hit and eos");
  hip_check(pde_sample_hist(a, p, h, cur_stream()), "sample");
}

// counts[b, idx[b, t]] = prompt flag for t < T0 + the state's offset of row b; idx: int64 [B, width]
void count_prompt(const at::Tensor& idx, const at::Tensor& state, const at::Tensor& counts, int64_t T0) {
  check_cuda(idx, "idx", I64);
  TORCH_CHECK(idx.dim() == 2 && idx.size(1) >= 1, "count_prompt: idx must be [B, width >= 1]");
  const int64_t B = idx.size(0), Vp = counts.dim() == 2 ? counts.size(1) : 0;
  TORCH_CHECK(B >= 1 && B <= PDE_DS_MAX_ROWS, "count_prompt: 1 <= B <= ", PDE_DS_MAX_ROWS, ", got ", B);
  check_cuda(counts, "counts", I32, B * Vp);
  TORCH_CHECK(counts.dim() == 2 && counts.size(0) == B && Vp >= 1, "count_prompt: counts must be [B, Vp]");
  TORCH_CHECK(T0 >= 0 && T0 <= idx.size(1), "count_prompt: 0 <= T0 <= width");
  check_state(state);
  hip_check(pde_count_prompt(ptr<int64_t>(idx), ptr<int>(state), ptr<int>(counts), (int)B, (int)idx.size(1),
                             (int)idx.size(1), (int)T0, (int)Vp, cur_stream()),
            "count_prompt");
}

// ------------------------------------------------------------------------------------------ beam search
// table: uint8 [2, PDE_DS_MAX_ROWS, stride], stride % 4 == 0
int table_stride(const at::Tensor& table, int64_t Tmax) {
  check_cuda(table, "beam table", at::kByte);
  TORCH_CHECK(table.dim() == 3 && table.size(0) == 2 && table.size(1) == PDE_DS_MAX_ROWS && table.size(2) >= Tmax &&
                  table.size(2) % 4 == 0,
              "beam table must be uint8 [2, ", PDE_DS_MAX_ROWS, ", stride >= Tmax = ", Tmax, "], stride % 4 == 0");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(table.data_ptr()) % 4 == 0, "beam table must be 4-byte aligned");
  return (int)table.size(2);
}

void decode_attention_beam(const at::Tensor& qkv, const at::Tensor& cache, const at::Tensor& state,
                           const at::Tensor& part, const at::Tensor& out, int64_t H, double scale,
                           const at::Tensor& table) {
  TORCH_CHECK(qkv.dim() == 2 && H >= 1 && qkv.size(1) == 3 * H * 64, "decode_attention: qkv must be [B, 3 * H * 64]");
  const int64_t B = qkv.size(0);
  TORCH_CHECK(B >= 1 && B <= PDE_DS_MAX_ROWS, "decode_attention: 1 <= B <= ", PDE_DS_MAX_ROWS, ", got ", B);
  check_cuda(qkv, "qkv", BF16);
  check_al16(qkv, "qkv");
  check_cache(cache, B, H);
  const int64_t Tmax = cache.size(3), nch = (Tmax + pde_decode_attn_chunk() - 1) / pde_decode_attn_chunk();
  check_state(state);
  check_cuda(part, "part", F32, B * H * nch * 66);
  check_cuda(out, "out", BF16, B * H * 64);
  PdeBeamTable t{};
  t.stride = table_stride(table, Tmax);
  t.anc = static_cast<const unsigned char*>(table.data_ptr());
  hip_check(pde_decode_attention_beam(qkv.data_ptr(), cache.data_ptr(), ptr<int>(state), ptr<float>(part),
                                      out.data_ptr(), (int)B, (int)H, (int)Tmax, (float)scale, t, cur_stream()),
            "decode_attention");
}

// One beam step (PdeBeam in pde_decode.h).  logits: bf16 [R = B * K, Vp]; score fp32 [R]; len int32 [R]; cand_score /
// cand_tok: fp32 / int32 [R, K] workspaces; the traces [max_new, R]; logits_out: bf16 [R, max_new, V] or None.
void beam_step(const at::Tensor& logits, int64_t V, int64_t K, const at::Tensor& state, const at::Tensor& next,
               const at::Tensor& score, const at::Tensor& len, const at::Tensor& cand_score,
               const at::Tensor& cand_tok, const at::Tensor& table, int64_t Tmax, const at::Tensor& tok_trace,
               const at::Tensor& parent_trace, const at::Tensor& score_trace, const OptT& logits_out, int64_t eos) {
  check_cuda(logits, "logits", BF16);
  TORCH_CHECK(logits.dim() == 2 && logits.size(1) % 8 == 0, "beam_step: logits must be [R, Vp] with Vp % 8 == 0");
  const int64_t R = logits.size(0), Vp = logits.size(1);
  TORCH_CHECK(K >= 1 && R >= 1 && R <= PDE_DS_MAX_ROWS && R % K == 0, "beam_step: R = B * K <= ", PDE_DS_MAX_ROWS,
              " rows, got R ", R, ", K ", K);
  TORCH_CHECK(V >= K && V <= Vp && eos >= -1 && eos < V, "beam_step: K <= V <= Vp and eos in [-1, V)");
  check_al16(logits, "logits");
  check_state(state);
  check_cuda(next, "next", I64, R);
  check_cuda(score, "score", F32, R);
  check_cuda(len, "len", I32, R);
  check_cuda(cand_score, "cand_score", F32, R * K);
  check_cuda(cand_tok, "cand_tok", I32, R * K);
  TORCH_CHECK(Tmax >= 1 && tok_trace.dim() == 2 && tok_trace.size(1) == R, "beam_step: traces must be [max_new, R]");
  const int64_t max_new = tok_trace.size(0);
  check_cuda(tok_trace, "tok_trace", I32, max_new * R);
  check_cuda(parent_trace, "parent_trace", I32, max_new * R);
  check_cuda(score_trace, "score_trace", F32, max_new * R);
  PdeBeam a{};
  a.logits = logits.data_ptr();
  a.state = ptr<int>(state);
  a.next = ptr<int64_t>(next);
  a.score = ptr<float>(score);
  a.len = ptr<int>(len);
  a.cand_score = ptr<float>(cand_score);
  a.cand_tok = ptr<int>(cand_tok);
  a.stride = table_stride(table, Tmax);
  a.anc = static_cast<unsigned char*>(table.data_ptr());
  a.tok_trace = ptr<int>(tok_trace);
  a.parent_trace = ptr<int>(parent_trace);
  a.score_trace = ptr<float>(score_trace);
  a.logits_out = nullptr;
  if (given(logits_out)) {
    check_cuda(*logits_out, "logits_out", BF16, R * max_new * V);
    TORCH_CHECK(logits_out->dim() == 3 && logits_out->size(0) == R && logits_out->size(1) == max_new &&
                    logits_out->size(2) == V,
                "beam_step: logits_out must be [R, max_new, V]");
    a.logits_out = logits_out->data_ptr();
  }
  a.B = (int)(R / K);
  a.K = (int)K;
  a.V = (int)V;
  a.Vp = (int)Vp;
  a.Tmax = (int)Tmax;
  a.max_new = (int)max_new;
  a.eos = (int)eos;
  hip_check(pde_beam_step(a, cur_stream()), "beam_step");
}

// out: int64 [B, K, width] with the prompts in place; scores: fp32 [B, K]
void beam_finalize(const at::Tensor& state, const at::Tensor& score, const at::Tensor& len,
                   const at::Tensor& tok_trace, const at::Tensor& parent_trace, const at::Tensor& out,
                   const at::Tensor& scores, int64_t T0, int64_t n_steps, double length_penalty) {
  check_cuda(out, "out", I64);
  TORCH_CHECK(out.dim() == 3, "beam_finalize: out must be [B, K, width]");
  const int64_t B = out.size(0), K = out.size(1), R = B * K;
  TORCH_CHECK(B >= 1 && K >= 1 && R <= PDE_DS_MAX_ROWS, "beam_finalize: B * K <= ", PDE_DS_MAX_ROWS);
  check_state(state);
  check_cuda(score, "score", F32, R);
  check_cuda(len, "len", I32, R);
  TORCH_CHECK(tok_trace.dim() == 2 && tok_trace.size(1) == R && n_steps >= 1 && n_steps <= tok_trace.size(0) &&
                  T0 >= 0 && T0 + n_steps <= out.size(2),
              "beam_finalize: traces [>= n_steps, R] and out wide enough for T0 + n_steps");
  check_cuda(tok_trace, "tok_trace", I32, tok_trace.size(0) * R);
  check_cuda(parent_trace, "parent_trace", I32, tok_trace.size(0) * R);
  check_cuda(scores, "scores", F32, R);
  PdeBeamFinal a{};
  a.state = ptr<int>(state);
  a.score = ptr<float>(score);
  a.len = ptr<int>(len);
  a.tok_trace = ptr<int>(tok_trace);
  a.parent_trace = ptr<int>(parent_trace);
  a.out = ptr<int64_t>(out);
  a.scores = ptr<float>(scores);
  a.B = (int)B;
  a.K = (int)K;
  a.T0 = (int)T0;
  a.out_stride = (int)out.size(2);
  a.n_steps = (int)n_steps;
  a.length_penalty = length_penalty;
  hip_check(pde_beam_finalize(a, cur_stream()), "beam_finalize");
}

// cache_fill of the B prompts into rows b * K of a cache layer of B * K rows
void cache_fill_beam(const at::Tensor& qkv, const at::Tensor& cache, int64_t T0, int64_t H, int64_t K) {
  TORCH_CHECK(qkv.dim() == 3 && H >= 1 && qkv.size(2) == 3 * H * 64, "cache_fill: qkv must be [B, Tpad, 3 * H * 64]");
  const int64_t B = qkv.size(0), Tpad = qkv.size(1);
  TORCH_CHECK(K >= 1 && B * K <= PDE_DS_MAX_ROWS, "cache_fill: B * K <= ", PDE_DS_MAX_ROWS);
  check_cuda(qkv, "qkv", BF16);
  check_al16(qkv, "qkv");
  check_cache(cache, B * K, H);
  TORCH_CHECK(T0 >= 1 && T0 <= Tpad && T0 <= cache.size(3), "cache_fill: 1 <= T0 <= min(Tpad, Tmax), got ", T0);
  hip_check(pde_cache_fill_beam(qkv.data_ptr(), cache.data_ptr(), (int)B, (int)K, (int)H, (int)Tpad, (int)T0,
                                (int)cache.size(3), cur_stream()),
            "cache_fill");
}

}  // namespace

void register_decode(pybind11::module& m) {
  namespace py = pybind11;
  m.def("skinny_splits", &skinny_splits);
  m.def("skinny_linear", &skinny_linear, py::arg("x"), py::arg("w"), py::arg("bias"), py::arg("y"),
        py::arg("part") = py::none(), py::arg("gelu") = false);
  m.def("decode_attn_chunk", &decode_attn_chunk);
  m.def("decode_attention", &decode_attention);
  m.def("cache_fill", &cache_fill);
  m.def("decode_embed", &decode_embed);
  m.def("decode_sample", &sample, py::arg("logits"), py::arg("V"), py::arg("state"), py::arg("next"), py::arg("out"),
        py::arg("logits_out"), py::arg("T0"), py::arg("inv_temp"), py::arg("greedy"), py::arg("top_k"), py::arg("eos"),
        py::arg("thr_out") = py::none(), py::arg("top_p") = 0.0, py::kw_only(), py::arg("counts") = py::none(),
        py::arg("bias") = py::none(), py::arg("work") = py::none(), py::arg("rep") = 1.0, py::arg("inv_rep") = 1.0,
        py::arg("freq") = 0.0, py::arg("pres") = 0.0, py::arg("min_new") = 0, py::arg("ngram") = 0,
        py::arg("ban") = py::none(), py::arg("n_ban") = 0, py::arg("stop") = py::none(), py::arg("n_stop") = 0,
        py::arg("stop_hit") = py::none());
  m.def("decode_count_prompt", &count_prompt);
  m.def("decode_attention_beam", &decode_attention_beam);
  m.def("beam_step", &beam_step, py::arg("logits"), py::arg("V"), py::arg("K"), py::arg("state"), py::arg("next"),
        py::arg("score"), py::arg("len"), py::arg("cand_score"), py::arg("cand_tok"), py::arg("table"),
        py::arg("Tmax"), py::arg("tok_trace"), py::arg("parent_trace"), py::arg("score_trace"),
        py::arg("logits_out"), py::arg("eos"));
  m.def("beam_finalize", &beam_finalize);
  m.def("cache_fill_beam", &cache_fill_beam);
  m.attr("DECODE_STATE_WORDS") = PDE_DS_WORDS;
}

}  // namespace pde
