"""History constraints on the GPU: the ``HIST`` instantiations of the sampler kernel against the CPU twin, bit for
bit, on the cases of ``history_constraints_ref.py`` (what each case shows is established on the CPU by
``test_history_constraints_cpu.py``), and ``GPT.generate`` / ``DecodeSession`` with n-gram blocking and stop sequences
under graph replay, checked from their own outputs."""
import pytest
import torch

from pytorch_distributed_example_amd.models import build_gpt2
from pytorch_distributed_example_amd.models.gpt2 import DecodeSession
from pytorch_distributed_example_amd.ops import DeviceRNG, HistoryConstraints, LogitProcessors
from pytorch_distributed_example_amd.ops import decode as D

import generate_cases as GC
import history_constraints_ref as HR
from test_history_constraints_cpu import check_model_case, run_model_case

pytestmark = pytest.mark.gpu

dev = "cuda"


# --------------------------------------------------------------------------------------- kernel against twin
@pytest.mark.parametrize("name", list(HR.CASES))
def test_kernel_matches_twin(name):
    """``processed_out`` over all ``Vp`` columns, ``next``, ``out`` (its poisoned columns included: nothing but the
    token's slot is written), the finished flags, ``stop_hit``, the counts and the advanced state, bit for bit."""
    want, got = HR.twin(name), HR.CASES[name].run(dev)
    for key in want:
        assert torch.equal(got[key], want[key]), (name, key, got[key], want[key])


def test_launcher_rejects_invalid_arguments():
    c = HR.CASES["overlap"]
    lg, out = c.logits().to(dev), c.out().to(dev)
    state = D.DecodeState(dev, DeviceRNG(1).next().to(dev))
    tc, work = D.TokenCounts(HR.B, HR.VP, dev), torch.empty_like(lg)
    nxt = torch.zeros(HR.B, device=dev, dtype=torch.int64)
    hit = torch.zeros(HR.B, device=dev, dtype=torch.int32)
    tab = torch.tensor([0, 2, 5, 6], device=dev, dtype=torch.int32)

    def call(ngram=2, ban=None, n_ban=0, stop=None, n_stop=0, stop_hit=None, eos=5, counts=tc.buf, work=work):
        D.kernels().decode_sample(lg, HR.V, state.buf, nxt, out, None, c.T0, 0.0, True, 0, eos, counts=counts, work=work,
                                  ngram=ngram, ban=ban, n_ban=n_ban, stop=stop, n_stop=n_stop, stop_hit=stop_hit)

    call(stop=tab, n_stop=1, stop_hit=hit)                       # a valid call
    for kw in (dict(ngram=HR.MAX_N + 1), dict(ngram=-1), dict(n_ban=1), dict(ban=tab, n_ban=HR.MAX_SEQS + 1),
               dict(stop=tab, n_stop=1), dict(stop=tab, n_stop=1, stop_hit=hit, eos=-1),
               dict(stop=tab.long(), n_stop=1, stop_hit=hit), dict(ban=tab, n_ban=2),
               dict(counts=None), dict(ngram=0, counts=None),    # a group given in part: work without counts ...
               dict(counts=None, work=None)):                    # ... and history arguments without the processors'
        with pytest.raises(RuntimeError):
            call(**kw)
    with pytest.raises(ValueError):                              # stop sequences need stop_hit on the device
        D.sample(lg, HR.V, state, 0.0, out=out, T0=c.T0, history=HistoryConstraints(0, None, [[1]], 5),
                 stop_hit=hit.cpu())


# --------------------------------------------------------------------------------------- whole model
@pytest.fixture(scope="module")
def model():
    return build_gpt2(GC.tiny_cfg(), seed=0, device=dev)


def _session(model, use_graph, **kw):
    """A generation through ``DecodeSession`` as ``GPT.generate`` runs it; returns the session."""
    idx = GC.ragged_prompt(HR.MODEL_LENS).to(dev)
    model.eval()
    with torch.no_grad():
        ses = DecodeSession(model, idx, HR.N_NEW, rng_state=DeviceRNG(HR.MODEL_SEED, device=dev).state,
                            return_logits=True, prompt_lens=HR.MODEL_LENS, eos=HR.MODEL_EOS,
                            logit_bias=HR.model_bias().to(dev), **HR.MODEL_SAMPLING, **kw)
        if use_graph:
            hit = ses.stop_hit.clone()
            graph = ses.capture()
            assert torch.equal(ses.stop_hit, hit)                # capture() undoes its warm-up step
            for _ in range(HR.N_NEW - 1):
                graph.replay()
        else:
            for _ in range(HR.N_NEW - 1):
                ses.step()
    return ses


def test_model_case_replayed_from_its_own_outputs(model):
    """Graph replay against eager launches, bit for bit; the host replay from the returned raw logits reproduces
    every token, the finished steps and ``stop_hit``; and the condition against a vacuous test holds for this run:
    every row blocked at 10 steps or more, one row stopped by a sequence before the last step, one never."""
    out, r = run_model_case(model, dev)
    print(r, [out[b, n:n + HR.N_NEW].tolist() for b, n in enumerate(HR.MODEL_LENS)])
    check_model_case(out, r)
    kw = dict(no_repeat_ngram_size=HR.NGRAM, stop_sequences=HR.MODEL_STOPS)
    g, e = _session(model, True, **kw), _session(model, False, **kw)
    assert torch.equal(g.out.cpu(), out)                         # the session is what generate runs
    for a, b in ((g.out, e.out), (g.logits_out, e.logits_out), (g.stop_hit, e.stop_hit), (g.state.buf, e.state.buf),
                 (g.counts.buf, e.counts.buf)):
        assert torch.equal(a, b)
    assert g.stop_hit.dtype == torch.int32 and g.stop_hit.tolist() == r["stop_hit"]
    assert g.state.finished[:3].tolist() == [int(s >= 0) for s in r["fin_step"]]


def test_banned_sequences_under_graph_replay(model):
    lens, n_new = [7, 2, 12], 24
    idx = GC.ragged_prompt(lens).to(dev)
    free = model.generate(idx, n_new, temperature=0.0, prompt_lens=lens)
    gen = [free[b, n:n + n_new].tolist() for b, n in enumerate(lens)]
    bad = [gen[0][2:5], [int(idx[1, 1]), gen[1][0]], [gen[2][0]]]     # inside the output, across the boundary, one token
    kw = dict(temperature=0.0, prompt_lens=lens, bad_words_ids=bad, return_logits=True)
    out, raw = model.generate(idx, n_new, **kw)
    eager, raw_e = model.generate(idx, n_new, use_graph=False, **kw)
    assert torch.equal(out, eager) and torch.equal(raw, raw_e)
    hist = HistoryConstraints(0, bad)
    r = HR.replay_generation(out, raw, idx, lens, 1000, 1024, LogitProcessors(), hist, 0, 0.0, None, None, None)
    assert not r["mismatches"] and min(r["blocked"][:2]) >= 1, r
    for b, n in enumerate(lens):
        row = out[b, :n + n_new].tolist()
        assert gen[2][0] not in row[n:]
        assert not any(HR.contains(row[max(n - len(s) + 1, 0):], s) for s in hist.bad_words)


def test_defaults_allocate_nothing_and_change_nothing(model):
    idx = GC.ragged_prompt((7, 7, 7)).to(dev)
    for kw in (dict(temperature=0.8, top_k=40, seed=11), dict(temperature=0.0, frequency_penalty=0.3),
               dict(temperature=0.8, top_p=0.9, seed=11, prompt_lens=[7, 3, 5])):
        a, la = model.generate(idx, 12, return_logits=True, **kw)
        b, lb = model.generate(idx, 12, return_logits=True, no_repeat_ngram_size=0, bad_words_ids=None,
                               stop_sequences=None, **kw)
        assert torch.equal(a, b) and torch.equal(la, lb), kw
    model.eval()
    with torch.no_grad():
        ses = DecodeSession(model, idx, 4, 0.8, 40, DeviceRNG(3, device=dev).state, no_repeat_ngram_size=0,
                            bad_words_ids=None, stop_sequences=None)
        assert ses.history is None and ses.stop_hit is None and ses.processors is None and ses.counts is None
        ses = DecodeSession(model, idx, 4, 0.8, 40, DeviceRNG(3, device=dev).state, no_repeat_ngram_size=2)
        assert ses.history is not None and ses.stop_hit is None and ses.counts is not None and ses.bias is None
        ses = DecodeSession(model, idx, 4, 0.8, 40, DeviceRNG(3, device=dev).state, eos=5, stop_sequences=[[1, 2]])
        assert ses.stop_hit.tolist() == [-1, -1, -1] and ses.stop_hit.device.type == "cuda"
    with pytest.raises(ValueError):
        model.generate(idx, 2, stop_sequences=[[1, 2]])          # no eos
