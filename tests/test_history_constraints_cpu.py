"""History constraints on the CPU: ``ops.history_bans_reference`` against the plain loops, the host-side errors,
the CPU twin of the kernel cases (the very inputs ``test_history_constraints_gpu.py`` feeds to the kernel) against
what each case is built to show, and ``GPT.generate`` on the tiny CPU model checked from its own outputs."""
import math

import pytest
import torch

from pytorch_distributed_example_amd.models import build_gpt2
from pytorch_distributed_example_amd.ops import (DeviceRNG, HistoryConstraints, LogitProcessors, history_bans_reference,
                                                 sample_reference)
from pytorch_distributed_example_amd.ops import decode as D

import generate_cases as GC
import history_constraints_ref as HR
import logit_processors_ref as LR

V, VP, EOS = HR.V, HR.VP, HR.EOS


# --------------------------------------------------------------------------------------- definition and errors
@pytest.mark.parametrize("name", list(HR.CASES))
def test_bans_reference_matches_the_loops(name):
    c = HR.CASES[name]
    hist = c.constraints()
    got = history_bans_reference(c.out(), [len(h) for h in c.hists()], V, hist)
    want = HR.bans_loops(c.hists(), hist.no_repeat_ngram_size, hist.bad_words, V)
    assert [set(torch.nonzero(r).flatten().tolist()) for r in got] == want


def test_bans_reference_on_random_histories():
    g = torch.Generator().manual_seed(3)
    for n in range(0, HR.MAX_N + 1):
        out = torch.randint(0, 4, (4, 60), generator=g)          # 4 tokens: every n-gram repeats
        lens = [0, 1, 33, 60]
        hist = HistoryConstraints(n, [[1, 2, 3], [0, 0], [3] * 16, [2]])
        got = history_bans_reference(out, lens, V, hist)
        want = HR.bans_loops([out[b, :L].tolist() for b, L in enumerate(lens)], n, hist.bad_words, V)
        assert [set(torch.nonzero(r).flatten().tolist()) for r in got] == want
        assert hist.bad_tokens == [2] and [2] not in hist.bad_words


def test_errors():
    H = HistoryConstraints
    for kw in (dict(no_repeat_ngram_size=-1), dict(no_repeat_ngram_size=2.0), dict(no_repeat_ngram_size=HR.MAX_N + 1),
               dict(no_repeat_ngram_size=True), dict(bad_words_ids=[[1, 2.5]]), dict(bad_words_ids=[[1, -2]]),
               dict(bad_words_ids=[[]]), dict(bad_words_ids=[3]), dict(bad_words_ids=[[1] * (HR.MAX_LEN + 1)]),
               dict(bad_words_ids=[[1, 2]] * (HR.MAX_SEQS + 1)), dict(stop_sequences=[[1, 2]]),
               dict(stop_sequences=[[]], eos_token_id=5), dict(stop_sequences=[[1, "a"]], eos_token_id=5),
               dict(stop_sequences=[[-1]], eos_token_id=5), dict(stop_sequences=[[1]] * (HR.MAX_SEQS + 1), eos_token_id=5),
               dict(stop_sequences=[[1] * (HR.MAX_LEN + 1)], eos_token_id=5), dict(eos_token_id=-1)):
        with pytest.raises(ValueError):
            H(**kw)
    for kw in (dict(bad_words_ids=[[1, V]]), dict(bad_words_ids=[[V]]), dict(stop_sequences=[[V]], eos_token_id=5),
               dict(stop_sequences=[[1]], eos_token_id=V)):
        with pytest.raises(ValueError):
            H(**kw).check(V)
    full = H(HR.MAX_N, [[1, 2]] * HR.MAX_SEQS + [[7]], [[1] * HR.MAX_LEN] * HR.MAX_SEQS, 5).check(V)
    assert full.active and not H().active and not H(eos_token_id=5).active
    ban, stop = full.tables()
    assert ban.dtype == torch.int32 and ban[:HR.MAX_SEQS + 1].tolist() == list(range(0, 2 * HR.MAX_SEQS + 1, 2))
    assert stop.numel() == HR.MAX_SEQS + 1 + HR.MAX_SEQS * HR.MAX_LEN and full.tables()[0] is ban
    lg = torch.zeros(1, 8)
    with pytest.raises(ValueError):                              # the history is read from `out`
        D.sample(lg, 8, DeviceRNG(1).next(), 0.0, history=H(2))
    with pytest.raises(ValueError):                              # stop sequences need stop_hit
        D.sample(lg, 8, DeviceRNG(1).next(), 0.0, history=H(0, None, [[1]], 3), out=torch.zeros(1, 4, dtype=torch.int64))
    model = build_gpt2(GC.tiny_cfg(), seed=0, dtype=torch.float32)
    idx = GC.ragged_prompt((4,))
    for kw in (dict(stop_sequences=[[1, 2]]), dict(no_repeat_ngram_size=9), dict(bad_words_ids=[[1000, 1]]),
               dict(bad_words_ids=[[]])):
        with pytest.raises(ValueError):
            model.generate(idx, 2, **kw)


def test_ngram_1_bans_exactly_the_seen_tokens():
    c = HR.CASES["n1"]
    ban = history_bans_reference(c.out(), [len(h) for h in c.hists()], V, c.constraints())
    for b, h in enumerate(c.hists()):
        assert set(torch.nonzero(ban[b]).flatten().tolist()) == set(h)
    y = HR.twin("n1")["work"].view(torch.bfloat16)
    for b, h in enumerate(c.hists()):
        seen = torch.zeros(VP, dtype=torch.bool)
        seen[h] = True
        assert (y[b][seen] == -math.inf).all() and torch.equal(y[b][~seen], c.logits()[b][~seen])


def test_single_token_bad_words_equal_suppress_tokens():
    lg = LR.make_logits(3, V, VP)
    res = []
    for kw in (dict(processors=LogitProcessors(suppress_tokens=[5, 17, 998]), _force_proc=True),
               dict(history=HistoryConstraints(bad_words_ids=[[17], [998], [5]]))):
        for t, k, p in LR.SETTINGS:
            work = torch.zeros(3, VP, dtype=torch.bfloat16)
            out = torch.zeros(3, 2, dtype=torch.int64)
            tok = D.sample(lg, V, DeviceRNG(4).next(), t, k, top_p=p, out=out, processed_out=work,
                           counts=D.TokenCounts(3, VP), **kw)
            res.append((tok.clone(), work.view(torch.int16), out))
    half = len(res) // 2
    for a, b in zip(res[:half], res[half:]):
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert (res[0][1].view(torch.bfloat16)[:, [5, 17, 998]] == -math.inf).all()


# --------------------------------------------------------------------------------------- the kernel cases' twin
def test_cases_show_what_they_are_built_for():
    """Every kernel case on the CPU twin: the planted favourite is banned exactly where the definition bans it."""
    t = HR.twin
    assert t("short")["next"][:2].tolist() == [5, 5] and t("short")["next"][2] != 5
    assert t("overlap")["next"][0] != 7 and t("overlap")["next"][1] != 9 and t("overlap")["next"][2] == 3
    assert t("boundary")["next"].tolist() == [50, 51, 33] and t("boundary")["stop_hit"].tolist() == [-1, -1, 2]
    assert t("boundary")["finished"][:3].tolist() == [0, 0, 1]
    assert t("poison")["next"].tolist() == [602, 603, 604] and t("poison")["stop_hit"].tolist() == [-1] * 3
    assert t("poison")["finished"].sum() == 0
    assert t("long")["next"].tolist() == [720, 721, 722]         # both matches found: j = 3 and j = 1400
    for n in range(1, HR.MAX_N + 1):
        assert t(f"n{n}")["next"].tolist() == [830, 831, 832]
    assert t("tables")["next"].tolist() == [778, 778, 779]
    assert t("tables")["stop_hit"].tolist() == [HR.MAX_SEQS - 1, HR.MAX_SEQS - 1, -1]
    assert t("range")["next"][0] not in (5, 6) and t("range")["next"][1] != 2 and t("range")["next"][2] != 8
    fin = t("finished")
    assert fin["next"][1] == EOS and fin["stop_hit"].tolist() == [-1, -1, 1] and fin["finished"][:3].tolist() == [0, 1, 1]
    c = HR.CASES["finished"]                                     # the finished row's y carries no ban
    assert torch.equal(fin["work"][1], c.logits()[1].view(torch.int16)) and fin["next"][0] != 7
    al = t("all")                                                # ban after bias (row 0), min_new bans eos, a stop fires
    y = al["work"].view(torch.bfloat16)
    assert y[0, 7] == -math.inf and y[1, 100] == -math.inf and y[1, 55] == -math.inf and y[2, EOS] == -math.inf
    assert al["next"][2] == 60 and al["stop_hit"].tolist() == [-1, -1, 0] and al["finished"][:3].tolist() == [0, 0, 1]
    for name, c in HR.CASES.items():                             # bookkeeping of every case
        r = t(name)
        for b in range(HR.B):
            assert r["out"][b, c.lens[b] + c.step] == r["next"][b]
        assert int(r["state"][D._STEP]) == c.step + 1


def test_sampled_seeds_keep_every_row_away_from_a_tie():
    for i, (tmp, k, p) in enumerate(LR.SETTINGS[1:]):
        c = HR.CASES[f"sampled{i}"]
        y = HR.twin(f"sampled{i}")["work"].view(torch.bfloat16)
        tok, info = sample_reference(y, V, DeviceRNG(c.seed).next(), tmp, k, top_p=p, return_info=True)
        assert torch.equal(tok, HR.twin(f"sampled{i}")["next"])
        assert (info["gap"] >= HR.GAP).all() and (p is None or (info["p_slack"] >= LR.P_SLACK).all())


# --------------------------------------------------------------------------------------- the tiny CPU model
@pytest.fixture(scope="module")
def model():
    return build_gpt2(GC.tiny_cfg(), seed=0, dtype=torch.float32)


@pytest.mark.parametrize("lens", [None, [7, 2, 12]], ids=["equal", "ragged"])
@pytest.mark.parametrize("sampling", [dict(temperature=0.0), dict(temperature=0.8, top_k=40)], ids=["greedy", "sampled"])
def test_generation_replayed_from_its_own_outputs(model, lens, sampling):
    n_new, seed = 24, 21
    idx = GC.ragged_prompt(lens or (9, 9, 9), width=14 if lens else None)
    bad = [[int(idx[0, 0]), 7], [3, 4, 5], [6]]
    kw = dict(no_repeat_ngram_size=2, bad_words_ids=bad, frequency_penalty=0.1)
    out, raw = model.generate(idx, n_new, seed=seed, prompt_lens=lens, return_logits=True, **kw, **sampling)
    hist = HistoryConstraints(2, bad)
    r = HR.replay_generation(out, raw, idx, lens, V, raw.shape[2], LogitProcessors(frequency_penalty=0.1), hist, seed,
                             sampling["temperature"], sampling.get("top_k"), None, None)
    assert not r["mismatches"] and r["close"] <= 1, r
    for b, n in enumerate(lens or [9] * 3):
        row = out[b, :n + n_new].tolist()
        assert not HR.has_repeated_ngram(row, 2) and 6 not in row[n:]
        assert not any(HR.contains(row[max(n - len(s) + 1, 0):], s) for s in hist.bad_words)
    if sampling["temperature"] == 0:                             # the constraint did something
        free = model.generate(idx, n_new, prompt_lens=lens, frequency_penalty=0.1, **sampling)
        assert not torch.equal(free, out)


def test_model_case_meets_the_condition_against_a_vacuous_test(model):
    """The inputs of the GPU model test on the CPU fp32 model: every row is blocked at 10 steps or more, one row
    finishes by a stop sequence before the last step and one never finishes."""
    out, r = run_model_case(model, "cpu")
    print(r, [out[b, n:n + HR.N_NEW].tolist() for b, n in enumerate(HR.MODEL_LENS)])
    check_model_case(out, r)


def run_model_case(model, device):
    idx = GC.ragged_prompt(HR.MODEL_LENS).to(device)
    bias = HR.model_bias().to(device)
    kw = dict(no_repeat_ngram_size=HR.NGRAM, stop_sequences=HR.MODEL_STOPS, logit_bias=bias, eos_token_id=HR.MODEL_EOS)
    out, raw = model.generate(idx, HR.N_NEW, seed=HR.MODEL_SEED, prompt_lens=HR.MODEL_LENS, return_logits=True, **kw,
                              **HR.MODEL_SAMPLING)
    hist = HistoryConstraints(HR.NGRAM, None, HR.MODEL_STOPS, HR.MODEL_EOS)
    Vp = model.transformer.wte.weight.shape[0] if raw.is_cuda else raw.shape[2]      # the sampler's row width
    r = HR.replay_generation(out, raw, idx, HR.MODEL_LENS, V, Vp, LogitProcessors(logit_bias=bias.cpu()), hist,
                             HR.MODEL_SEED, HR.MODEL_SAMPLING["temperature"], HR.MODEL_SAMPLING.get("top_k"), None,
                             HR.MODEL_EOS)
    return out.cpu(), r


def check_model_case(out, r):
    assert not r["mismatches"] and r["close"] <= 1, r
    assert min(r["blocked"]) >= HR.MIN_BLOCKED, r
    assert any(0 <= s < HR.N_NEW - 1 and q >= 0 for s, q in zip(r["fin_step"], r["stop_hit"])), r
    assert any(s < 0 for s in r["fin_step"]), r
    for b, n in enumerate(HR.MODEL_LENS):
        s = r["fin_step"][b]
        live = out[b, n:n + (HR.N_NEW if s < 0 else s + 1)].tolist()
        assert not HR.has_repeated_ngram(out[b, :n].tolist() + live, HR.NGRAM)
        assert set(live) <= set(range(100 * b + 10, 100 * b + 10 + HR.ALLOWED))
        if s >= 0:
            assert HR.stop_loops(live, HR.MODEL_STOPS) == r["stop_hit"][b]
            assert out[b, n + s + 1:n + HR.N_NEW].tolist() == [HR.MODEL_EOS] * (HR.N_NEW - s - 1)


# --------------------------------------------------------------------------------------- stop sequences
def _stop_run(model, idx, n_new, stops, eos, lens=None, **kw):
    out, raw = model.generate(idx, n_new, temperature=0.0, prompt_lens=lens, return_logits=True, stop_sequences=stops,
                              eos_token_id=eos, **kw)
    hist = HistoryConstraints(kw.get("no_repeat_ngram_size", 0), None, stops, eos)
    procs = LogitProcessors(min_new_tokens=kw.get("min_new_tokens", 0), eos_token_id=eos)
    r = HR.replay_generation(out, raw, idx, lens, V, raw.shape[2], procs, hist, 0, 0.0, None, None, eos)
    assert not r["mismatches"]
    return out, r


def test_stop_sequences(model):
    lens, n_new, eos = [7, 2, 12], 12, 999
    idx = GC.ragged_prompt(lens)
    free = model.generate(idx, n_new, temperature=0.0, prompt_lens=lens, no_repeat_ngram_size=2)
    gen = [free[b, n:n + n_new].tolist() for b, n in enumerate(lens)]
    # row 0 stops on its tokens 3..5, row 1 on its tokens 0..1 (a stop at the first possible step); row 2 never
    stops = [gen[0][3:6], [1, 2, 3], gen[1][0:2]]
    out, r = _stop_run(model, idx, n_new, stops, eos, lens, no_repeat_ngram_size=2, min_new_tokens=8)
    assert r["fin_step"] == [5, 1, -1] and r["stop_hit"] == [0, 2, -1]       # min_new_tokens does not delay a stop
    assert out[0, 7:7 + n_new].tolist() == gen[0][:6] + [eos] * 6            # the sequence stays, then eos
    assert out[1, 2:2 + n_new].tolist() == gen[1][:2] + [eos] * 10
    assert out[2, 12:12 + n_new].tolist() == gen[2]
    # a stop sequence that begins in the prompt does not fire: the prompt's last token, then the first two tokens
    part = [[int(idx[0, 6])] + gen[0][:2]]
    out, r = _stop_run(model, idx, n_new, part, eos, lens, no_repeat_ngram_size=2)
    assert r["fin_step"] == [-1, -1, -1] and torch.equal(out, free)
    # of two sequences of which one is a suffix of the other, the lower index is reported
    long, short = gen[0][3:6], gen[0][4:6]
    for stops, want in (([long, short], 0), ([short, long], 0), ([[998, 997], short, long], 1)):
        out, r = _stop_run(model, idx, n_new, stops, eos, lens, no_repeat_ngram_size=2)
        assert r["fin_step"][0] == 5 and r["stop_hit"][0] == want


def test_stop_hit_of_the_cpu_sampler(model):
    """``stop_hit`` as the CPU generation keeps it, against the replay's."""
    lens, eos = [3, 5, 4], 999
    idx = GC.ragged_prompt(lens)
    lg = torch.full((3, V), -5.0)
    hist = HistoryConstraints(0, None, [[40, 41], [41], [7, 40, 41]], eos)
    smp = D.SampleBuffers(D.SamplerConfig(0.0, eos_token_id=eos, history=hist), idx, lens, 4, V, V, "cpu",
                          DeviceRNG(1).state, dtype=torch.float32)
    want = [[7, 40, 41, eos], [41, eos, eos, eos], [7, 7, 40, 7]]
    hits = []
    for s in range(4):
        x = lg.clone()
        for b in range(3):
            x[b, want[b][s]] = 5.0
        tok = smp.sample(x)
        assert tok.tolist() == [want[b][s] for b in range(3)]
        hits.append(smp.stop_hit.tolist())
    assert hits == [[-1, 1, -1], [-1, 1, -1], [0, 1, -1], [0, 1, -1]]
    assert smp.state.finished[:3].tolist() == [1, 1, 0]
    for b, n in enumerate(lens):
        assert smp.out[b, n:n + 4].tolist() == want[b]


def test_defaults_are_the_call_as_it_was(model):
    idx = GC.ragged_prompt((7, 7, 7))
    for kw in (dict(temperature=0.8, top_k=40, seed=11), dict(temperature=0.0, frequency_penalty=0.3),
               dict(temperature=0.8, top_p=0.9, seed=11, prompt_lens=[7, 3, 5])):
        a, la = model.generate(idx, 8, return_logits=True, **kw)
        b, lb = model.generate(idx, 8, return_logits=True, no_repeat_ngram_size=0, bad_words_ids=None,
                               stop_sequences=None, **kw)
        assert torch.equal(a, b) and torch.equal(la, lb), kw
