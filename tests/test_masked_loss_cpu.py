"""Masked loss on the CPU: ``ops.loss_targets`` against the definition written as loops
(``tests/masked_loss_ref.py``), the CPU path of ``ops.transformer.lm_head_loss`` against ``F.cross_entropy`` in
fp32 and against the definition, and the tiny CPU GPT: ``loss_mask`` / ``mask_doc_ends`` against hand-made
``-100`` targets, a shared ``denom`` over two micro-batches, the error cases and the untouched default."""
import pytest
import torch
import torch.nn.functional as F

from pytorch_distributed_example_amd import ops
from pytorch_distributed_example_amd.models import GPTConfig, build_gpt2
from pytorch_distributed_example_amd.ops import transformer as TR

import masked_loss_ref as M

V = 50


def _check(got, tg, kw, doc_end=None, reduction="mean", denom=None):
    eff, count, inv, oor = M.loop_targets(tg, V, doc_end=doc_end, reduction=reduction, denom=denom, **kw)
    assert got.targets.dtype == torch.int64 and got.targets.shape == tg.shape
    assert torch.equal(got.targets, eff)
    assert got.count.dtype == torch.int32 and got.count.item() == count
    assert got.out_of_range.dtype == torch.int32 and got.out_of_range.item() == oor
    assert got.inv.dtype == torch.float32 and torch.equal(got.inv, inv), (got.inv, inv)
    return count


# --------------------------------------------------------------------------------------- loss_targets
@pytest.mark.parametrize("name", M.CASES)
def test_loss_targets_against_the_loops(name):
    tg, kw = M.make_case(name, 3, 17, V, seed=1)
    count = _check(ops.loss_targets(tg, vocab_size=V, **kw), tg, kw)
    if name.startswith("all_"):
        assert count == 0
    _check(ops.loss_targets(tg, vocab_size=V, reduction="sum", **kw), tg, kw, reduction="sum")
    for d in (3.0, 0.0, -2.0):
        _check(ops.loss_targets(tg, vocab_size=V, denom=torch.tensor(d), **kw), tg, kw, denom=d)


@pytest.mark.parametrize("layout", ["len1", "mid200", "span"])
def test_loss_targets_document_ends(layout):
    """``span`` row 1 has a document that begins (and ends) at ``T - 1``: its target is kept."""
    B, T = 2, 256
    ids, de = M.doc_end_of(layout, B, T)
    tg, kw = M.make_case("everything", B, T, V, seed=2)
    bounds = ops.doc_bounds(ids)
    got = ops.loss_targets(tg, vocab_size=V, doc_bounds=bounds, mask_doc_ends=True, **kw)
    _check(got, tg, kw, doc_end=de)
    plain, _ = M.make_case("plain", B, T, V, seed=3)
    got = ops.loss_targets(plain, vocab_size=V, doc_bounds=bounds, mask_doc_ends=True)
    n_docs = sum(len(r) for r in M.P.LAYOUTS[layout](T)[:B])
    ends_at_last = B                                    # every row's last document ends at T - 1
    assert got.count.item() == B * T - (n_docs - ends_at_last)
    assert (got.targets[:, T - 1] >= 0).all()
    # bounds given but not asked for: nothing is masked
    assert ops.loss_targets(plain, vocab_size=V, doc_bounds=bounds).count.item() == B * T


def test_loss_targets_errors():
    tg = torch.zeros(2, 8, dtype=torch.int64)
    with pytest.raises(ValueError):
        ops.loss_targets(tg, vocab_size=V, mask_doc_ends=True)
    with pytest.raises(ValueError):
        ops.loss_targets(tg, vocab_size=V, reduction="sum", denom=torch.tensor(2.0))
    with pytest.raises(ValueError):
        ops.loss_targets(tg, vocab_size=V, reduction="median")
    with pytest.raises(ValueError):
        ops.loss_targets(tg, vocab_size=V, loss_mask=torch.ones(2, 7, dtype=torch.bool))
    with pytest.raises(ValueError):
        ops.loss_targets(tg.float(), vocab_size=V)


# --------------------------------------------------------------------------------------- lm_head_loss
def _hw(N, C=16, Vp=56, seed=4):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(N, C, generator=g).requires_grad_(), (0.5 * torch.randn(Vp, C, generator=g)).requires_grad_())


def _rel(a, b):
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def test_cpu_lm_head_loss_against_torch():
    N = 40
    h, w = _hw(N)
    tg, _ = M.make_case("ignore_neg", 1, N, V, seed=5)
    tg = tg[0]
    loss = TR.lm_head_loss(h, w, tg, V, ignore_index=-100)
    loss.backward()
    hr, wr = h.detach().clone().requires_grad_(), w.detach().clone().requires_grad_()
    ref = F.cross_entropy((hr @ wr.t())[:, :V], tg, ignore_index=-100)
    ref.backward()
    assert abs(loss.item() - ref.item()) < 1e-6 * abs(ref.item())
    assert _rel(h.grad, hr.grad) < 1e-6 and _rel(w.grad, wr.grad) < 1e-6
    assert h.grad[tg == -100].abs().max().item() == 0.0


def test_cpu_lm_head_loss_zero_count_is_zero_not_nan():
    N = 12
    h, w = _hw(N)
    tg = torch.full((N,), -100)
    loss = TR.lm_head_loss(h, w, tg, V, ignore_index=-100)
    loss.backward()
    assert loss.item() == 0.0
    assert h.grad.abs().max().item() == 0.0 and w.grad.abs().max().item() == 0.0
    loss = TR.lm_head_loss(h, w, torch.zeros(N, dtype=torch.int64), V, loss_mask=torch.zeros(N, dtype=torch.bool))
    assert loss.item() == 0.0


def test_cpu_lm_head_loss_sum_none_and_denom():
    B, T = 2, 20
    h, w = _hw(B * T)
    h3 = h.detach().view(B, T, -1)
    tg, kw = M.make_case("everything", B, T, V, seed=6)
    eff, count, _, _ = M.loop_targets(tg, V, **kw)
    logits = (h3 @ w.detach().t())[..., :V]
    rows = torch.zeros(B, T)
    for b in range(B):
        for t in range(T):
            if eff[b, t] >= 0:
                rows[b, t] = torch.logsumexp(logits[b, t], 0) - logits[b, t, eff[b, t]]
    with torch.no_grad():
        none = TR.lm_head_loss(h3, w, tg, V, reduction="none", **kw)
        assert none.shape == (B, T) and none.dtype == torch.float32
        assert _rel(none, rows) < 1e-5 and (none[eff < 0] == 0).all()
        assert abs(TR.lm_head_loss(h3, w, tg, V, reduction="sum", **kw).item() - rows.sum().item()) < 1e-5 * rows.sum()
        assert abs(TR.lm_head_loss(h3, w, tg, V, **kw).item() - rows.sum().item() / count) < 1e-5 * rows.mean()
        got = TR.lm_head_loss(h3, w, tg, V, denom=torch.tensor(7.0), **kw).item()
        assert abs(got - rows.sum().item() / 7.0) < 1e-5 * rows.sum().item() / 7.0
        assert TR.lm_head_loss(h3, w, tg, V, denom=torch.tensor(0.0), **kw).item() == 0.0
    with pytest.raises(NotImplementedError):
        TR.lm_head_loss(h.view(B, T, -1), w, tg, V, reduction="none", **kw)
    with pytest.raises(ValueError):
        TR.lm_head_loss(h3, w, tg, V, reduction="sum", denom=torch.tensor(2.0))


def test_cpu_lm_head_loss_ignores_nan_rows():
    N = 10
    h, w = _hw(N)
    tg = torch.randint(0, V, (N,), generator=torch.Generator().manual_seed(7))
    tg[0] = tg[N - 1] = -100
    clean = TR.lm_head_loss(h.detach(), w.detach(), tg, V, ignore_index=-100)
    hn = h.detach().clone()
    hn[0] = float("nan")
    hn[N - 1] = float("inf")
    assert torch.equal(TR.lm_head_loss(hn, w.detach(), tg, V, ignore_index=-100), clean)


# --------------------------------------------------------------------------------------- the tiny GPT
CFG = dict(block_size=64, vocab_size=V, padded_vocab=56, n_layer=2, n_head=2, n_embd=128)
B, T = 4, 64


@pytest.fixture(scope="module")
def gpt():
    torch.manual_seed(8)
    return (build_gpt2(GPTConfig(**CFG), seed=0, dtype=torch.float32), torch.randint(0, V, (B, T)),
            torch.randint(0, V, (B, T)))


def _grads(model, loss):
    model.zero_grad(set_to_none=True)
    loss.backward()
    return [p.grad.clone() for p in model.parameters()]


def test_gpt_loss_mask_equals_ignored_targets(gpt):
    model, idx, tgt = gpt
    m = torch.rand(B, T, generator=torch.Generator().manual_seed(9)) < 0.5
    a = model(idx, tgt, loss_mask=m)
    b = model(idx, tgt.masked_fill(~m, -100), ignore_index=-100)
    ref = F.cross_entropy(model(idx).reshape(-1, V).float(), tgt.masked_fill(~m, -100).reshape(-1), ignore_index=-100)
    assert torch.equal(a, b)
    assert abs(a.item() - ref.item()) < 1e-6 * abs(ref.item())
    assert torch.equal(model(idx, tgt, loss_mask=m.to(torch.uint8)), a)


def test_gpt_mask_doc_ends_equals_the_hand_made_mask(gpt):
    model, idx, tgt = gpt
    ids = M.P.doc_ids(T, [[0, 10, 11], [0, 32], [0], [0, 5, T - 1]])
    de = M.P.loop_bounds(ids)[1]
    keep = torch.ones(B, T, dtype=torch.bool)
    for b in range(B):
        for t in range(T - 1):
            if int(de[b, t]) == t:
                keep[b, t] = False
    assert keep.sum().item() == B * T - 5 and keep[:, T - 1].all()
    a = model(idx, tgt, doc_ids=ids, mask_doc_ends=True)
    assert torch.equal(a, model(idx, tgt, doc_ids=ids, loss_mask=keep))
    assert not torch.equal(a, model(idx, tgt, doc_ids=ids))


def test_gpt_micro_batches_with_a_shared_denom(gpt):
    model, idx, tgt = gpt
    m = torch.rand(B, T, generator=torch.Generator().manual_seed(10)) < 0.6
    m[:2, 10:] = False                                   # very different counts in the two halves
    full = model(idx, tgt, loss_mask=m)
    gfull = _grads(model, full)
    total = ops.loss_targets(tgt, vocab_size=V, loss_mask=m).count.float()
    model.zero_grad(set_to_none=True)
    parts = []
    for s in (slice(0, 2), slice(2, 4)):
        part = model(idx[s], tgt[s], loss_mask=m[s], denom=total)
        part.backward()
        parts.append(part.item())
    assert abs(sum(parts) - full.item()) < 1e-5 * abs(full.item())
    for p, gf in zip(model.parameters(), gfull):
        assert _rel(p.grad, gf) < 1e-5


def test_gpt_errors(gpt):
    model, idx, tgt = gpt
    with pytest.raises(ValueError):
        model(idx, tgt, mask_doc_ends=True)
    with pytest.raises(ValueError):
        model(idx, tgt, reduction="sum", denom=torch.tensor(3.0))
    with pytest.raises(NotImplementedError):
        model(idx, tgt, ignore_index=-100, reduction="none")
    with torch.no_grad():
        assert model(idx, tgt, ignore_index=-100, reduction="none").shape == (B, T)


def test_gpt_defaults_are_the_call_as_it_was(gpt):
    model, idx, tgt = gpt
    a = model(idx, tgt)
    ga = _grads(model, a)
    b = model(idx, tgt, ignore_index=None, loss_mask=None)
    gb = _grads(model, b)
    assert torch.equal(a, b) and all(torch.equal(x, y) for x, y in zip(ga, gb))
    assert torch.equal(TR.lm_head_loss(*_hw(8), torch.arange(8), V),
                       TR.lm_head_loss(*_hw(8), torch.arange(8), V, ignore_index=None, loss_mask=None,
                                       doc_bounds=None, mask_doc_ends=False, reduction="mean", denom=None))
