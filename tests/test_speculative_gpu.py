"""Speculative decoding on the GPU: the decode attention over sibling rows against the plain kernel driven one row at
a time (bit for bit) and against the fp64 reference, the verify / draft kernels against their CPU twins on hand-made
steps, and ``GPT.generate(num_draft_tokens=)`` against the plain greedy call: same tokens, same logits bits, and the
step and acceptance counts that ``spec_trace_reference`` derives from the plain output."""
import pytest
import torch

from pytorch_distributed_example_amd.models import build_gpt2
from pytorch_distributed_example_amd.models.gpt2 import DecodeSession
from pytorch_distributed_example_amd.ops import decode as D

import attention_ref as A
import spec_cases as SC

pytestmark = pytest.mark.gpu

dev = "cuda"
BF16 = torch.bfloat16
H, TMAX, Q = 2, 256, 4


class _Cfg:
    n_layer, n_head, n_embd = 1, H, 64 * H


def _state(positions):
    state = D.DecodeState(dev, pos=0)
    state.row_offsets[:len(positions)] = torch.tensor(positions, dtype=torch.int32, device=dev)
    return state


# --------------------------------------------------------------------------------------- attention over sibling rows
@pytest.mark.parametrize("bases", [(0, 130), (1, 128), (126, 127), (127, 1), (128, 126), (130, 0)])
def test_sibling_attention_is_the_plain_kernel_row_by_row(bases):
    B, C = len(bases), 64 * H
    R = B * Q
    g = torch.Generator().manual_seed(sum(bases))
    before = torch.randn(1, 2, B, H, TMAX, 64, generator=g).to(dev, BF16)
    qkv = torch.randn(R, 3 * C, generator=g).to(dev, BF16)
    shared, plain = D.KVCache(_Cfg, B, TMAX, dev, rows=R), D.KVCache(_Cfg, B, TMAX, dev)
    shared.data.copy_(before)
    plain.data.copy_(before)
    pos = [P + i for P in bases for i in range(Q)]
    y = D.decode_attention(qkv, shared, 0, _state(pos), spec=Q)
    ref = torch.empty_like(y)
    for i in range(Q):                           # sibling i of every group, after siblings < i were appended
        ref[i::Q] = D.decode_attention(qkv[i::Q].contiguous(), plain, 0, _state(pos[i::Q]))
    assert torch.equal(y, ref)
    assert torch.equal(shared.data, plain.data)
    worst = 0.0
    for r, p in enumerate(pos):
        b = r // Q
        k_new, v_new = (qkv[r, s * C:(s + 1) * C].view(H, 64) for s in (1, 2))
        assert torch.equal(shared.data[0, 0, b, :, p], k_new) and torch.equal(shared.data[0, 1, b, :, p], v_new)
        Ks, Vs = (shared.data[0, s, b, :, :p + 1].cpu()[None] for s in (0, 1))
        want, den = A.decode_reference(qkv[r, :C].view(1, H, 64).cpu(), Ks, Vs)
        worst = max(worst, A.row_error(y[r].view(1, H, 64).cpu(), want, den))
    print(f"bases {bases}: worst row error {worst:.3e} (bound {A.DECODE_BOUND:.3e})")
    assert worst <= A.DECODE_BOUND


# --------------------------------------------------------------------------------------- verify and draft kernels
def _logits(greedy):
    """Rows whose maximum over the first V columns is at ``greedy[r]``, attained again at a higher index where one
    fits (the lowest wins), with larger values in the pad columns (ignored)."""
    lg = torch.rand(len(greedy), SC.VP, generator=torch.Generator().manual_seed(1)) - 1.0
    for r, t in enumerate(greedy):
        lg[r, t] = 5.0
        if t + 1234 < SC.V:
            lg[r, t + 1234] = 5.0
    lg[:, SC.V:] = 9.0
    return lg.to(dev, BF16)


@pytest.mark.parametrize("names", SC.BATCHES, ids="+".join)
def test_verify_and_draft_kernels_match_the_twins(names):
    cases = [SC.HAND[n] for n in names]
    B, K, q, n_pos = len(cases), SC.K, SC.K + 1, 4096
    lens = [len(c[0]) for c in cases]
    idx = torch.zeros(B, max(lens), dtype=torch.int64)
    for b, c in enumerate(cases):
        idx[b, :lens[b]] = torch.tensor(c[0])
    sb = D.SpecBuffers(D.SpecConfig(K, SC.NGRAM, SC.EOS), idx.to(dev), lens, SC.MAX_NEW, SC.V, SC.VP, dev, n_pos,
                       return_logits=True)
    for b, (_, gen, _, drafts, *_) in enumerate(cases):      # in the middle of a generation
        sb.out[b, lens[b]:lens[b] + len(gen)] = torch.tensor(gen, device=dev)
        sb.n[b] = len(gen)
        sb.next[b * q:(b + 1) * q] = torch.tensor([gen[-1]] + drafts, device=dev)
    logits = _logits([t for c in cases for t in c[2]])
    want_out, want_lg = sb.out.clone(), torch.zeros_like(sb.logits_out)
    D.spec_step(logits, sb)
    all_fin = True
    for b, (prompt, gen, greedy, drafts, *_) in enumerate(cases):
        emit, fin = D.spec_accept_reference(greedy, drafts, len(gen), SC.MAX_NEW, SC.EOS)
        h = prompt + gen + emit
        want_out[b, len(h) - len(emit):len(h)] = torch.tensor(emit, device=dev)
        if SC.EOS in emit:
            want_out[b, len(h):lens[b] + SC.MAX_NEW] = SC.EOS
        want_lg[b, len(gen):len(gen) + len(emit)] = logits[b * q:b * q + len(emit), :SC.V]
        n2 = len(gen) + len(emit)
        got = (int(sb.n[b]), int(sb.steps[b]), int(sb.accepted[b]), bool(sb.state.finished[b]))
        assert got == (n2, 1, len(emit) - 1, fin), (names[b], got)
        d = [h[-1]] * K if fin else D.draft_reference(h, K, SC.NGRAM)
        live = [0] + [i if not fin and i < SC.MAX_NEW - n2 else 0 for i in range(1, q)]     # idle rows sit on row 0
        assert sb.next[b * q:(b + 1) * q].tolist() == [h[-1]] + [d[i - 1] if live[i] else h[-1] for i in range(1, q)]
        assert sb.state.row_offsets[b * q:(b + 1) * q].tolist() == [len(h) - 1 + i for i in live], names[b]
        all_fin = all_fin and fin
    assert torch.equal(sb.out, want_out) and torch.equal(sb.logits_out, want_lg)
    assert bool(sb.done.item()) == all_fin


# --------------------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def model():
    return build_gpt2(SC.tiny_cfg(), seed=1, device=dev, dtype=BF16)


@pytest.mark.parametrize("lens", [None, [12, 7]], ids=["equal", "ragged"])
@pytest.mark.parametrize("K", [1, 3, 7])
def test_generate_equals_plain_greedy(model, K, lens):
    n_new = 24
    idx = torch.randint(0, 1000, (2, 12), generator=torch.Generator().manual_seed(4)).to(dev)
    ln = lens or [12, 12]
    first = model.generate(idx, n_new, temperature=0.0, prompt_lens=lens)
    for eos in (None, int(first[0, ln[0] + 5])):          # without, and one that stops row 0 early
        plain, lp = model.generate(idx, n_new, temperature=0.0, prompt_lens=lens, eos_token_id=eos, return_logits=True)
        steps, acc = D.spec_trace_reference(plain.cpu(), ln, n_new, K, 3, eos)
        for use_graph in (True, False):
            stats = {}
            out, lg = model.generate(idx, n_new, temperature=0.0, prompt_lens=lens, eos_token_id=eos, return_logits=True,
                                     num_draft_tokens=K, spec_stats=stats, use_graph=use_graph)
            assert torch.equal(out, plain), (eos, use_graph)
            for b in range(2):                   # the same bits up to and including the finishing eos, zeros after
                gen = plain[b, ln[b]:ln[b] + n_new].tolist()
                cut = gen.index(eos) + 1 if eos in gen else n_new
                assert torch.equal(lg[b, :cut], lp[b, :cut]) and not lg[b, cut:].any(), (eos, use_graph, b)
            assert stats["model_steps"] == steps and torch.equal(stats["accepted"], acc.sum(0)), (eos, use_graph)


@pytest.mark.parametrize("K", [1, 3, 7])
def test_full_acceptance_on_the_repeating_model(K):
    g = SC.repeating_model(dev, BF16)
    idx, n_new = SC.REPEAT_PROMPT.to(dev), SC.REPEAT_NEW
    plain = g.generate(idx, n_new, temperature=0.0)
    steps, acc = D.spec_trace_reference(plain.cpu(), [idx.shape[1]], n_new, K)
    assert steps == -(-(n_new - 1) // (K + 1)) and (acc == K).all()      # every step accepts all K drafts
    stats = {}
    assert torch.equal(g.generate(idx, n_new, temperature=0.0, num_draft_tokens=K, spec_stats=stats), plain)
    assert stats["model_steps"] == steps < n_new - 1 and stats["accepted"].tolist() == [steps * K]


def test_errors_and_the_default(model):
    idx = torch.randint(0, 1000, (3, 6), generator=torch.Generator().manual_seed(6)).to(dev)
    with pytest.raises(ValueError, match="temperature"):
        model.generate(idx, 4, num_draft_tokens=2)
    with pytest.raises(ValueError, match="top_k"):
        model.generate(idx, 4, temperature=0.0, top_k=5, num_draft_tokens=2)
    with pytest.raises(NotImplementedError):
        model.generate(idx, 4, temperature=0.0, num_draft_tokens=5)          # 3 * 6 rows
    for kw in (dict(temperature=0.8, top_k=40, seed=11), dict(temperature=0.0)):
        a, la = model.generate(idx, 6, return_logits=True, **kw)
        b, lb = model.generate(idx, 6, return_logits=True, num_draft_tokens=0, draft_ngram=2, **kw)
        assert torch.equal(a, b) and torch.equal(la, lb)
    with torch.no_grad():
        ses = DecodeSession(model, idx, 3, spec=D.SpecConfig(0))
    assert ses.spec is None and isinstance(ses.buffers, D.SampleBuffers) and ses.cache.rows == ses.cache.batch == 3
