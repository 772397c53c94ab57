"""Logit processors on the GPU: the ``PROC`` instantiations of the sampler kernel against the numpy twin, bit for
bit; their side effects on the token counts and the decode state; ``k_count_prompt`` against the CPU path; and
``GPT.generate`` with penalties, bias and ``min_new_tokens`` checked from its own outputs, under graph replay."""

import pytest
import torch

from pytorch_distributed_example_amd.models import build_gpt2
from pytorch_distributed_example_amd.models.gpt2 import DecodeSession
from pytorch_distributed_example_amd.ops import (DeviceRNG, LogitProcessors, TokenCounts, process_logits_reference,
                                                 sample_reference)
from pytorch_distributed_example_amd.ops import decode as D

import generate_cases as GC
import logit_processors_ref as LR
from test_logit_processors_cpu import twin_reference

pytestmark = pytest.mark.gpu

dev = "cuda"
BF16 = torch.bfloat16


def _bits(t):
    return t.cpu().view(torch.int16)


# --------------------------------------------------------------------------------------- kernel against twin
@pytest.mark.parametrize("B,V,Vp", LR.SHAPES)
def test_kernel_matches_twin(B, V, Vp):
    """``processed_out`` equals ``process_logits_reference`` bit for bit, the threshold is the reference's on ``y``
    exactly, and the token is ``sample_reference(y)``'s.  The tie rule is the existing sampler tests': the seeds
    keep every row's gap >= 1e-4 and every row's top-p slack >= 1e-4 (checked on the CPU by
    ``test_twin_seeds_keep_every_row_away_from_a_tie``), so every comparison is exact."""
    lg, counts, _, y, refs = twin_reference(B, V, Vp)
    procs = LR.make_case("all", B, V, dev)[0]               # the twin's processors, their bias on the device
    lgd = lg.to(dev)
    for (t, k, p), (snap, ref, info) in zip(LR.SETTINGS, refs):
        assert (info["gap"] >= LR.GAP).all() and (p is None or t == 0 or (info["p_slack"] >= LR.P_SLACK).all())
        tc = LR.token_counts(B, V, Vp, dev)
        state = D.DecodeState(dev, snap.to(dev), pos=7, step=LR.STEP)
        work = torch.full((B, Vp), 7.0, device=dev, dtype=BF16)
        thr = torch.full((B,), -1, device=dev, dtype=torch.int32)
        tok = D.sample(lgd, V, state, t, k, top_p=p, processors=procs, counts=tc, processed_out=work,
                       threshold_out=thr).cpu()
        assert torch.equal(_bits(work[:, :V]), _bits(y[:, :V])), (t, k, p)
        if t > 0:
            assert (D.key16_to_float(thr) == info["threshold"]).all(), (t, k, p)
        assert torch.equal(tok, ref), (t, k, p, tok, ref)
        expect = counts.clone()
        expect[torch.arange(B), ref] += 1
        assert torch.equal(tc.buf.cpu(), expect)
    assert torch.equal(lgd.cpu().view(torch.int16), lg.view(torch.int16))       # the raw logits are read only


@pytest.mark.parametrize("case", [c for c in LR.CASES if c != "all"])
def test_kernel_matches_twin_each_processor_alone(case):
    """Every processor alone at the largest shape, the processed row bit for bit.  "frequency+presence" is the case
    a kernel that contracts ``x - f * n`` into a fused multiply-add fails (see the CPU test)."""
    B, V, Vp = LR.SHAPES[-1]
    lg, counts = LR.make_logits(B, V, Vp), LR.make_counts(B, V, Vp)
    y = process_logits_reference(lg, V, counts, LR.make_case(case, B, V)[0], LR.STEP)
    procs = LR.make_case(case, B, V, dev)[0]
    tc = LR.token_counts(B, V, Vp, dev)
    state = D.DecodeState(dev, DeviceRNG(3).next().to(dev), pos=7, step=LR.STEP)
    work = torch.empty(B, Vp, device=dev, dtype=BF16)
    tok = D.sample(lg.to(dev), V, state, 0.0, processors=procs, counts=tc, processed_out=work).cpu()
    assert torch.equal(_bits(work[:, :V]), _bits(y[:, :V])), case
    assert torch.equal(tok, sample_reference(y, V, state, 0.0)), case


def test_neutral_processors_forced_through_the_kernel_change_nothing():
    B, V, Vp, T0, n_new = 5, 997, 1000, 4, 2
    lg = LR.make_logits(B, V, Vp).to(dev)
    snap = DeviceRNG(17).next().to(dev)
    for t, k, p in LR.SETTINGS:
        res = []
        for force in (False, True):
            state = D.DecodeState(dev, snap, pos=9, step=1)
            thr = torch.full((B,), -1, device=dev, dtype=torch.int32)
            out = torch.full((B, T0 + n_new), -1, device=dev, dtype=torch.int64)
            lout = torch.zeros(B, n_new, V, device=dev, dtype=BF16)
            tc = TokenCounts(B, Vp, dev)
            tok = D.sample(lg, V, state, t, k, top_p=p, out=out, logits_out=lout, T0=T0, threshold_out=thr,
                           processors=LogitProcessors(), counts=tc, _force_proc=force)
            assert int(tc.buf.sum()) == (B if force else 0)  # inactive processors: the plain kernel, no counting
            res.append((tok, thr, out, _bits(lout), state.buf.clone()))
        for a, b in zip(*res):
            assert torch.equal(a, b), (t, k, p)


def test_side_effects_two_calls():
    B, V, Vp, T0, n_new = 5, 1000, 1024, 4, 3
    offs = (0, -3, -1, 0, -2)
    g = torch.Generator().manual_seed(5)
    lgs = [(torch.randn(B, Vp, generator=g) * 3).to(BF16) for _ in range(2)]
    rng = DeviceRNG(31)
    for _ in range(6):
        rng.next()                                       # a draw number other than 0
    procs = LogitProcessors(1.3, 0.3, 0.5, suppress_tokens=[5])
    prompt = torch.randint(0, V, (B, 6), generator=g)
    tc = TokenCounts(B, Vp, dev).add_prompt(prompt.to(dev))
    flags = tc.buf.cpu().clone()
    assert torch.equal(flags, TokenCounts(B, Vp).add_prompt(prompt).buf)
    state = D.DecodeState(dev, rng.state.to(dev), pos=9, step=0, row_offsets=offs)
    nxt = torch.zeros(B, device=dev, dtype=torch.int64)
    out = torch.full((B, T0 + n_new), -1, device=dev, dtype=torch.int64)
    lout = torch.zeros(B, n_new, V, device=dev, dtype=BF16)
    # the reference, call by call: the second call sees the first call's tokens in the counts
    host = TokenCounts(B, Vp)
    host.buf.copy_(flags)
    y0 = process_logits_reference(lgs[0], V, host, procs, 0)
    ref0, i0 = sample_reference(y0, V, rng.next(), 0.9, 40, return_info=True)
    eos = int(ref0[0])                                   # row 0 finishes at the first call
    host.add_(ref0)
    y1 = process_logits_reference(lgs[1], V, host, procs, 1)
    ref1, i1 = sample_reference(y1, V, rng.next(), 0.9, 40, return_info=True)
    assert (i0["gap"] >= LR.GAP).all() and (i1["gap"] >= LR.GAP).all()
    assert eos not in ref0[1:].tolist() and eos not in ref1[1:].tolist()
    ref1[0] = eos                                        # forced on the finished row, and counted
    host.add_(ref1)
    for lg in lgs:
        D.sample(lg.to(dev), V, state, 0.9, 40, eos, next=nxt, out=out, logits_out=lout, T0=T0, processors=procs,
                 counts=tc)
    expect = torch.full((B, T0 + n_new), -1, dtype=torch.int64)
    for b, off in enumerate(offs):
        expect[b, T0 + off], expect[b, T0 + off + 1] = ref0[b], ref1[b]
    assert torch.equal(out.cpu(), expect) and torch.equal(nxt.cpu(), ref1)
    # the counts grew by one at exactly the emitted tokens; the prompt flags are untouched
    assert torch.equal(tc.buf.cpu(), host.buf)
    assert torch.equal(tc.buf.cpu() & LR.PROMPT, flags) and int(tc.generated().sum()) == 2 * B
    assert int(tc.generated()[0, eos]) == 2 and state.finished.cpu().tolist() == [1] + [0] * 15
    assert torch.equal(_bits(lout[:, 0]), _bits(lgs[0][:, :V])) and torch.equal(_bits(lout[:, 1]), _bits(lgs[1][:, :V]))
    assert (lout.cpu()[:, 2] == 0).all()                 # logits_out holds the raw rows
    assert state.pos() == 11 and state.step() == 2 and state.row_pos(B) == [11 + o for o in offs]
    assert torch.equal(state.rng.cpu(), rng.state)


def test_count_prompt_matches_the_cpu_path():
    lens = [7, 1, 130, 64, 130]
    idx = GC.ragged_prompt(lens, width=132, seed=3)          # the pad columns hold real-looking tokens
    idx[2, 5:40] = idx[2, 4]                                 # duplicates
    idx[0, :7] = torch.tensor([9, 9, 9, 2, 9, 2, 999])
    ref = TokenCounts(5, 1024).add_prompt(idx, lens).buf
    assert torch.equal(TokenCounts(5, 1024, dev).add_prompt(idx.to(dev), lens).buf.cpu(), ref)
    state = D.DecodeState(dev, row_offsets=[n - 130 for n in lens])
    assert torch.equal(TokenCounts(5, 1024, dev).add_prompt(idx.to(dev), state, T0=130).buf.cpu(), ref)
    full = TokenCounts(5, 1024, dev).add_prompt(idx.to(dev))
    assert torch.equal(full.buf.cpu(), TokenCounts(5, 1024).add_prompt(idx).buf)
    assert torch.equal(full.seen().cpu(), full.buf.cpu() != 0) and not full.generated().any()


# --------------------------------------------------------------------------------------- whole model
@pytest.fixture(scope="module")
def model():
    return build_gpt2(GC.tiny_cfg(), seed=0, device=dev)


def _kw(eos):
    return dict(repetition_penalty=1.3, frequency_penalty=0.3, presence_penalty=0.5,
                logit_bias=LR.make_bias(3, 1000, True).to(dev), suppress_tokens=LR.SUPPRESS, min_new_tokens=6,
                eos_token_id=eos)


@pytest.mark.parametrize("lens", [None, [7, 2, 12]], ids=["equal", "ragged"])
def test_generation_replayed_from_its_own_outputs(model, lens):
    """The whole chain under graph replay: for every step the counts are rebuilt on the host from the prompt and
    the returned tokens, the returned raw logits go through the twin and the step's snapshot, and the device's
    token is required wherever the twin's own gap is at least 1e-4 (at most one of the 72 (row, step) pairs may
    be closer).  Covers the counts across replays, ``min_new_tokens`` against the device step, and eos."""
    V, n_new, seed = 1000, 24, 21
    idx = GC.ragged_prompt(lens or (9, 9, 9), width=14 if lens else None)
    first = (lens or [9])[0]
    free = model.generate(idx.to(dev), 3, temperature=0.8, top_k=40, seed=seed, prompt_lens=lens)
    eos = int(free[0, first])                                # the token row 0 of the free run emits first
    kw = _kw(eos)
    out, raw = model.generate(idx.to(dev), n_new, temperature=0.8, top_k=40, seed=seed, prompt_lens=lens,
                              return_logits=True, **kw)
    assert raw.dtype == BF16 and tuple(raw.shape) == (3, n_new, V)
    procs = LogitProcessors(**{**kw, "logit_bias": kw["logit_bias"].cpu()})
    bad, close = LR.replay_generation(out, raw, idx, lens, V, 1024, procs, seed, 0.8, 40, None, eos)
    print(f"lens {lens}: {len(bad)} mismatches, {close} of {3 * n_new} (row, step) pairs within the gap")
    assert not bad and close <= 1, (bad, close)
    gen = out.cpu()
    for b, n in enumerate(lens or [9] * 3):
        row = gen[b, n:n + n_new].tolist()
        assert eos not in row[:6] and not set(row) & set(LR.SUPPRESS) and 11 not in row
    wrong = out.clone()                                      # the check notices a history that is off by one token
    wrong[0, first + 2] = (wrong[0, first + 2] + 1) % V
    assert LR.replay_generation(wrong, raw, idx, lens, V, 1024, procs, seed, 0.8, 40, None, eos)[0]


def test_graph_replay_equals_eager(model):
    lens = [7, 2, 12]
    idx = GC.ragged_prompt(lens).to(dev)
    kw = _kw(5)
    for extra in (dict(temperature=0.0), dict(temperature=0.8, top_k=40, seed=11),
                  dict(temperature=0.8, top_k=40, top_p=0.9, seed=11, prompt_lens=lens)):
        a, la = model.generate(idx, 12, return_logits=True, **kw, **extra)
        b, lb = model.generate(idx, 12, return_logits=True, use_graph=False, **kw, **extra)
        assert torch.equal(a, b) and torch.equal(la, lb), extra
    greedy = model.generate(idx, 20, temperature=0.0, frequency_penalty=1e4)
    assert all(len(set(r.tolist())) == 20 for r in greedy[:, 12:])


def test_defaults_allocate_nothing_and_change_nothing(model):
    idx = GC.ragged_prompt((7, 7, 7)).to(dev)
    for kw in (dict(temperature=0.8, top_k=40, seed=11), dict(temperature=0.0),
               dict(temperature=0.8, top_p=0.9, seed=11, prompt_lens=[7, 3, 5])):
        a, la = model.generate(idx, 12, return_logits=True, **kw)
        b, lb = model.generate(idx, 12, return_logits=True, repetition_penalty=1.0, frequency_penalty=0.0,
                               presence_penalty=0.0, logit_bias=None, suppress_tokens=None, min_new_tokens=0, **kw)
        assert torch.equal(a, b) and torch.equal(la, lb), kw
    model.eval()
    with torch.no_grad():
        ses = DecodeSession(model, idx, 4, 0.8, 40, DeviceRNG(3, device=dev).state)
        assert ses.processors is None and ses.counts is None and ses.work is None and ses.bias is None
        ses = DecodeSession(model, idx, 4, 0.8, 40, DeviceRNG(3, device=dev).state, frequency_penalty=0.5)
        assert ses.counts is not None and int(ses.counts.generated().sum()) == 3
        ses.step()
        assert int(ses.counts.generated().sum()) == 6
    with pytest.raises(ValueError):
        model.generate(idx, 2, logit_bias=torch.zeros(1000))           # a bias on the wrong device
    with pytest.raises(ValueError):
        model.generate(idx, 2, min_new_tokens=2)
