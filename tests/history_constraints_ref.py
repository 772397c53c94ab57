"""The history constraints' definition as plain loops over ``b``, ``j`` and the sequences, the inputs shared by
``test_history_constraints_cpu.py`` and ``test_history_constraints_gpu.py`` -- so that what the CPU tests establish
about a case holds for the very tensors the GPU tests feed to the kernel -- and a host replay of a finished
generation from its ``out`` and raw logits, in the manner of ``logit_processors_ref.replay_generation``."""
import functools
import math

import torch

from pytorch_distributed_example_amd.ops import (DeviceRNG, HistoryConstraints, LogitProcessors, TokenCounts,
                                                 process_logits_reference, sample_reference)
from pytorch_distributed_example_amd.ops import decode as D

import logit_processors_ref as LR

B, V, VP = 3, 1000, 1008                  # the kernel tests' shape: Vp is no multiple of 64
EOS = 990
MAX_N, MAX_LEN, MAX_SEQS = HistoryConstraints.MAX_NGRAM, HistoryConstraints.MAX_SEQ_LEN, HistoryConstraints.MAX_SEQS
GAP = LR.GAP


# --------------------------------------------------------------------------------------- the definition
def bans_loops(hists, n, bad_words, V):
    """``hists``: one list of tokens per row (``h[0 .. L-1]``).  Returns one set of banned tokens per row."""
    res = []
    for h in hists:
        L, ban = len(h), set()
        if n >= 1 and L >= n - 1:
            for j in range(n - 1, L):
                same = True
                for i in range(1, n):
                    if h[j - i] != h[L - i]:
                        same = False
                if same and 0 <= h[j] < V:
                    ban.add(h[j])
        for seq in bad_words:
            m = len(seq)
            if m > 1 and L >= m - 1:
                same = True
                for i in range(m - 1):
                    if h[L - m + 1 + i] != seq[i]:
                        same = False
                if same and 0 <= seq[m - 1] < V:
                    ban.add(seq[m - 1])
        res.append(ban)
    return res


def stop_loops(generated, stops):
    """``generated``: a row's generated tokens, the one emitted now included.  The lowest index of a stop
    sequence they end in, or -1."""
    for q, seq in enumerate(stops):
        m = len(seq)
        if len(generated) >= m:
            same = True
            for i in range(m):
                if generated[len(generated) - m + i] != seq[i]:
                    same = False
            if same:
                return q
    return -1


def has_repeated_ngram(tokens, n):
    grams = [tuple(tokens[i:i + n]) for i in range(len(tokens) - n + 1)]
    return len(grams) != len(set(grams))


def contains(tokens, seq):
    return any(tokens[i:i + len(seq)] == list(seq) for i in range(len(tokens) - len(seq) + 1))


# --------------------------------------------------------------------------------------- kernel cases
class Case:
    """One ``ops.sample`` call at ``B, V, VP``: per row a prompt and the tokens generated so far (all rows the same
    number: the state's step), planted logits, constraints, processors and sampling settings.  ``poison`` fills
    the columns of ``out`` at and past each row's history; the kernel must not read them."""

    def __init__(self, rows, history, plant=(), procs=None, fin=(0, 0, 0), sampling=(0.0, None, None), seed=1,
                 poison=None, width=None, counts=False, eos=EOS):
        assert len(rows) == B and len({len(g) for _, g in rows}) == 1
        self.rows, self.history, self.plant, self.procs_kw = rows, history, plant, procs or {}
        self.fin, self.sampling, self.seed, self.poison, self.counts, self.eos = fin, sampling, seed, poison, counts, eos
        self.lens = [len(p) for p, _ in rows]
        self.step = len(rows[0][1])
        self.T0 = max(self.lens)
        self.width = self.T0 + self.step + 1 if width is None else width

    def hists(self):
        return [list(p) + list(g) for p, g in self.rows]

    def logits(self):
        g = torch.Generator().manual_seed(7000 + self.seed)
        lg = (torch.randn(B, VP, generator=g) * 3).to(torch.bfloat16)
        for b, v, x in self.plant:
            lg[b, v] = x
        return lg

    def out(self):
        out = torch.full((B, self.width), -7, dtype=torch.int64)
        for b, h in enumerate(self.hists()):
            out[b, :len(h)] = torch.tensor(h, dtype=torch.int64)
            if self.poison is not None:
                tail = self.poison(b)
                k = min(len(tail), self.width - len(h))
                out[b, len(h):len(h) + k] = torch.tensor(tail[:k], dtype=torch.int64)
        return out

    def constraints(self):
        return HistoryConstraints(eos_token_id=self.eos, **self.history)

    def processors(self, device="cpu"):
        kw = dict(self.procs_kw)
        if kw.get("logit_bias") is not None:
            kw["logit_bias"] = kw["logit_bias"].to(device)
        return LogitProcessors(eos_token_id=self.eos, **kw) if kw else None

    def run(self, device="cpu"):
        """The call on ``device``; every result as a CPU tensor."""
        t, k, p = self.sampling
        hist, procs = self.constraints(), self.processors(device)
        state = D.DecodeState(device, DeviceRNG(self.seed).next().to(device), pos=self.T0 + self.step - 1,
                              step=self.step, row_offsets=[n - self.T0 for n in self.lens])
        state.finished[:B] = torch.tensor(self.fin, dtype=torch.int32)
        out = self.out().to(device)
        tc = TokenCounts(B, VP, device)
        if self.counts:                              # the counts of this very history
            for b, (pr, gen) in enumerate(self.rows):
                for v in pr:
                    if 0 <= v < VP:
                        tc.buf[b, v] |= TokenCounts.PROMPT
                for v in gen:
                    if 0 <= v < VP:
                        tc.buf[b, v] += 1
        work = torch.full((B, VP), 7.0, device=device, dtype=torch.bfloat16)
        stop_hit = torch.full((B,), -1, device=device, dtype=torch.int32)
        nxt = torch.full((B,), -1, device=device, dtype=torch.int64)
        D.sample(self.logits().to(device), V, state, t, k, self.eos, next=nxt, out=out, T0=self.T0, top_p=p,
                 processors=procs, counts=tc, processed_out=work, history=hist, stop_hit=stop_hit)
        return dict(next=nxt.cpu(), out=out.cpu(), finished=state.finished.cpu().clone(), stop_hit=stop_hit.cpu(),
                    counts=tc.buf.cpu(), work=work.cpu().view(torch.int16), state=state.buf.cpu().clone())


def _rand_tokens(n, seed, lo=0, hi=900):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi, (n,), generator=g).tolist()


def _cases():
    c = {}
    # 1. L < n-1, L = n-1, L = n (n = 3): only the last row has a window to match
    c["short"] = Case([([5], []), ([5, 5], []), ([5, 5, 5], [])], dict(no_repeat_ngram_size=3),
                      plant=[(b, 5, 30.0) for b in range(B)])
    # 2. the overlapping window: n = 2 and a history `.. a a` bans a; `a b .. a` bans b; row 2: nothing repeats
    c["overlap"] = Case([([1, 2], [7, 7]), ([8, 9, 3], [4, 8]), ([1], [2, 3])], dict(no_repeat_ngram_size=2),
                        plant=[(0, 7, 30.0), (1, 9, 30.0), (2, 3, 30.0)])
    # 3. matches that span the boundary between prompt and generated tokens.  Row 0: the trigram (11, 12 | 13)
    # begins in the prompt and bans 13.  Row 1: the banned sequence's head (21 | 22) does.  Row 2: the stop sequence
    # [31, 32, 33] would match with 31 the prompt's last token and must not fire; [32, 33] fires.
    c["boundary"] = Case([([10, 11, 12], [13, 14, 11, 12]), ([20, 21], [22, 23, 24, 25]), ([30, 31], [32, 1, 31, 32])],
                         dict(no_repeat_ngram_size=3, bad_words_ids=[[21, 22, 23, 24, 25, 26]],
                              stop_sequences=[[40, 41], [31, 32, 1, 31, 32, 33], [32, 33]]),
                         plant=[(0, 13, 30.0), (0, 50, 20.0), (1, 26, 30.0), (1, 51, 20.0), (2, 33, 30.0)])
    # 4. ragged, three different len_b; what lies at and past len_b + step would ban the favourites and stop the
    # rows if it were read (the stop sequences end in each row's favourite)
    rows = [(_rand_tokens(n, 40 + n), _rand_tokens(3, 50 + n)) for n in (2, 9, 5)]
    c["poison"] = Case(rows, dict(no_repeat_ngram_size=2, bad_words_ids=[[600, 601, 602 + b] for b in range(B)],
                                  stop_sequences=[[950, 951, 602 + b] for b in range(B)]),
                       plant=[(b, 602 + b, 30.0) for b in range(B)], width=24,
                       poison=lambda b: [602 + b, rows[b][1][-1], 602 + b, 600, 601, 950, 951, 602 + b] * 2)
    # 5. L = 1500 with out_stride = 1501: the strided loop past the block's 1024 threads.  The matches sit at
    # j = 3 (first round) and j = 1400 (second round)
    long_rows = []
    for b in range(B):
        h = _rand_tokens(1500, 60 + b, 0, 400)
        h[-2:] = [900 + b, 901 + b]
        h[1:4] = [900 + b, 901 + b, 700 + b]
        h[1398:1401] = [900 + b, 901 + b, 710 + b]
        long_rows.append((h[:700], h[700:]))
    c["long"] = Case(long_rows, dict(no_repeat_ngram_size=3), width=1501,
                     plant=[(b, 700 + b, 30.0) for b in range(B)] + [(b, 710 + b, 29.0) for b in range(B)]
                     + [(b, 720 + b, 28.0) for b in range(B)])
    # 6. every n: the history ends in the n - 1 tokens that preceded 800 earlier
    for n in range(1, MAX_N + 1):
        rows_n = []
        for b in range(B):
            pat = [810 + i for i in range(n - 1)]
            rows_n.append((_rand_tokens(3 + b, 70 + b) + pat + [800 + b] + _rand_tokens(2, 80 + b), pat))
        c[f"n{n}"] = Case(rows_n, dict(no_repeat_ngram_size=n),
                          plant=[(b, 800 + b, 30.0) for b in range(B)] + [(b, 830 + b, 20.0) for b in range(B)])
    # 7. the longest banned and stop sequences, in the last slot of full tables
    head = [400 + i for i in range(MAX_LEN - 1)]
    filler = [[500 + (q % 100), 300 + (q // 100), 299] for q in range(MAX_SEQS - 1)]
    c["tables"] = Case([(_rand_tokens(2 + b, 90 + b), head) for b in range(B)],
                       dict(bad_words_ids=filler + [head + [777]],
                            stop_sequences=filler + [head + [778]]),
                       plant=[(0, 777, 30.0), (0, 778, 20.0), (1, 778, 30.0), (2, 777, 30.0), (2, 779, 20.0)])
    # 8. history tokens >= V (and below 0) in out: skipped, nothing is stored out of range
    c["range"] = Case([([V, 5, V, 6], [1 << 40, 5]), ([VP + 3, 2], [-1, VP + 3]), ([7, 8], [V + 1, V + 2])],
                      dict(no_repeat_ngram_size=1), plant=[(0, 5, 30.0), (0, 6, 29.0), (1, 2, 30.0), (2, 8, 30.0)])
    # 9. a finished row ignores bans, emits eos and leaves stop_hit alone (row 1); rows 0 and 2 as in "overlap"
    c["finished"] = Case([([1, 2], [7, 7]), ([8, 9, 3], [4, 8]), ([1], [2, 3])],
                         dict(no_repeat_ngram_size=2, stop_sequences=[[8, 9], [3, 4]]), fin=(0, 1, 0),
                         plant=[(0, 7, 30.0), (1, 9, 30.0), (2, 4, 30.0)])
    # 10. with every penalty, the bias and min_new_tokens: the order of the processor steps.  Row 0's favourite gets
    # a large bias and is banned by the n-gram all the same (ban after bias); eos is banned by min_new_tokens
    bias = LR.make_bias(B, V, True)
    bias[0, 7] = 50.0
    c["all"] = Case([([1, 2], [7, 7]), ([8, 9, 3], [4, 8]), ([1], [2, 3])],
                    dict(no_repeat_ngram_size=2, bad_words_ids=[[4, 8, 100], [55]], stop_sequences=[[3, 60]]),
                    procs=dict(repetition_penalty=1.3, frequency_penalty=0.3, presence_penalty=0.5, logit_bias=bias,
                               suppress_tokens=LR.SUPPRESS, min_new_tokens=5),
                    plant=[(0, 7, 30.0), (1, 100, 30.0), (1, 55, 29.0), (2, EOS, 30.0), (2, 60, 29.0)], counts=True)
    # 11. sampled: the settings of the processor tests, the seeds below
    for i, st in enumerate(LR.SETTINGS[1:]):
        c[f"sampled{i}"] = Case([([1, 2], [7, 7]), ([8, 9, 3], [4, 8]), ([1], [2, 3])],
                                dict(no_repeat_ngram_size=2, bad_words_ids=[[4, 8, 100]], stop_sequences=[[3, 60]]),
                                procs=dict(repetition_penalty=1.3, frequency_penalty=0.3), sampling=st,
                                seed=SAMPLED_SEEDS[i], counts=True,
                                plant=[(0, 7, 9.0), (1, 9, 9.0), (1, 100, 9.0), (2, 60, 9.0)])
    return c


# seeds of the sampled cases: with them every row's best-minus-runner-up gap is >= GAP and, under top-p, every row's
# target mass is >= P_SLACK away from a threshold boundary (test_history_constraints_cpu.py checks it)
SAMPLED_SEEDS = [11, 12, 13]
CASES = _cases()


@functools.lru_cache(maxsize=None)
def twin(name):
    """The CPU twin's results of a case, computed once; treat as read-only."""
    return CASES[name].run("cpu")


# --------------------------------------------------------------------------------------- the model test's inputs
N_NEW, NGRAM, ALLOWED, MODEL_EOS = 40, 3, 12, 999
MODEL_LENS = [7, 2, 12]
MODEL_SEED = 5
MODEL_SAMPLING = dict(temperature=0.7, top_k=8)
MIN_BLOCKED = 10
# the second is the trigram that row 0 of the CPU fp32 model emits at steps 33 .. 35 (no trigram occurs twice, so it
# fires there and nowhere else); the tokens of rows 1 and 2 are their own, and nobody may emit 900: they never stop
MODEL_STOPS = [[900, 901], [12, 11, 11]]


def model_bias():
    """fp32 ``[3, V]``: every row keeps 12 tokens of its own (row b: 100 b + 10 .. 100 b + 21), the preference
    among them falling by 1 per token, so that a row keeps wanting the tokens it has just used."""
    bias = torch.full((B, V), -math.inf)
    for b in range(B):
        bias[b, 100 * b + 10:100 * b + 10 + ALLOWED] = -1.0 * torch.arange(ALLOWED, dtype=torch.float32)
    return bias


def replay_generation(out, raw, idx, lens, V, Vp, procs, history, seed, temperature, top_k, top_p, eos):
    """Check a finished generation from its own outputs: for every step the counts and the histories are rebuilt
    on the host from the prompt and the tokens returned so far, the raw logits are processed with the twin, the bans
    of ``bans_loops`` applied and the step's snapshot sampled.  Returns a dict: ``mismatches`` (the ``(b, s)`` where
    the returned token differs from the twin's although the twin's gap is at least ``GAP``), ``close`` (rows and steps
    closer than that), ``blocked`` (per row: steps at which the token chosen without the bans is a banned one),
    ``fin_step`` (per row: the step at which it finished, or -1) and ``stop_hit`` (per row)."""
    out, raw, idx = out.cpu(), raw.cpu(), idx.cpu()
    nB, n_new = raw.shape[:2]
    lens = [idx.shape[1]] * nB if lens is None else list(lens)
    counts = torch.zeros(nB, Vp, dtype=torch.int32)
    for b, n in enumerate(lens):
        for t in range(n):
            counts[b, int(idx[b, t])] = LR.PROMPT
    bias = history.merge_bias(procs.bias(nB, V, Vp), V, Vp)
    rng = DeviceRNG(seed)
    fin = torch.zeros(nB, dtype=torch.bool)
    rows = torch.arange(nB)
    res = dict(mismatches=[], close=0, blocked=[0] * nB, fin_step=[-1] * nB, stop_hit=[-1] * nB)
    for s in range(n_new):
        lg = torch.zeros(nB, Vp, dtype=raw.dtype)
        lg[:, :V] = raw[:, s]
        free = process_logits_reference(lg, V, counts, procs, s, _bias=bias)
        hists = [out[b, :lens[b] + s].tolist() for b in range(nB)]
        bans = bans_loops(hists, history.no_repeat_ngram_size, history.bad_words, V)
        y = free.clone()
        for b in range(nB):
            if not fin[b] and bans[b]:
                y[b, sorted(bans[b])] = -math.inf
        snap = rng.next()
        ref, info = sample_reference(y, V, snap, temperature, top_k, top_p=top_p, return_info=True)
        unbanned = sample_reference(free, V, snap, temperature, top_k, top_p=top_p)
        got = out[rows, torch.tensor(lens) + s]
        if eos is not None:
            ref = torch.where(fin, torch.full_like(ref, eos), ref)
        near = torch.from_numpy(info["gap"] < GAP) & ~fin
        res["close"] += int(near.sum())
        for b in range(nB):
            if got[b] != ref[b] and not near[b]:
                res["mismatches"].append((b, s, int(got[b]), int(ref[b])))
            if fin[b]:
                continue
            if int(unbanned[b]) in bans[b]:
                res["blocked"][b] += 1
            q = stop_loops(out[b, lens[b]:lens[b] + s + 1].tolist(), history.stop_sequences)
            if q >= 0:
                res["stop_hit"][b] = q
            if q >= 0 or (eos is not None and got[b] == eos):
                fin[b] = True
                res["fin_step"][b] = s
        counts[rows, got] += 1                    # the history is what the generation returned
    return res
