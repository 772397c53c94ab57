"""Smoothed and weighted loss on the CPU: ``ops.transformer.lm_head_loss(label_smoothing=, z_loss=, loss_weights=)``
against the definition written as fp64 loops (``tests/loss_smoothing_ref.py``) and against
``F.cross_entropy(label_smoothing=)``, its gradients by autograd, the weighted-mean recipe, accumulation with a
shared ``denom``, NaN safety, the errors, the model's keywords and the untouched defaults."""
import pytest
import torch
import torch.nn.functional as F

from pytorch_distributed_example_amd import ops
from pytorch_distributed_example_amd.models import GPTConfig, build_gpt2
from pytorch_distributed_example_amd.models import gpt2 as gpt2_module
from pytorch_distributed_example_amd.ops import transformer as TR

import loss_smoothing_ref as S
import masked_loss_ref as M

F64 = torch.float64
V, Vp, C = 11, 16, 8
B, T = 2, 6
EPS, ZC = 0.1, 1e-3
KNOBS = {"eps": dict(eps=EPS), "zc": dict(zc=ZC), "weights": dict(weights=True),
         "all": dict(eps=EPS, zc=ZC, weights=True)}


def _hw(seed=40, b=B, t=T, v=V, vp=Vp, dtype=F64):
    g = torch.Generator().manual_seed(seed)
    h = torch.randn(b, t, C, generator=g, dtype=dtype).requires_grad_()
    w = (0.7 * torch.randn(vp, C, generator=g, dtype=dtype)).requires_grad_()
    return h, w


def _weights(shape, seed=41):
    """fp32 weights in [0, 2] with an exact 0 and an exact 1"""
    wt = 2 * torch.rand(shape, generator=torch.Generator().manual_seed(seed))
    wt.view(-1)[1], wt.view(-1)[2] = 0.0, 1.0
    return wt


def _op_kw(knob, wt):
    return dict(label_smoothing=knob.get("eps", 0.0), z_loss=knob.get("zc", 0.0),
                loss_weights=wt if knob.get("weights") else None)


def _ref(h, w, tg, knob, wt, **kw):
    logits = (h.detach() @ w.detach().t())[..., :V]
    return S.loop_loss(logits, tg, V, knob.get("eps", 0.0), knob.get("zc", 0.0), wt if knob.get("weights") else None,
                       **kw)


def _close(a, b, tol=1e-10):
    a, b = torch.as_tensor(a, dtype=F64), torch.as_tensor(b, dtype=F64)
    assert ((a - b).abs().max() <= tol * b.abs().max().clamp_min(1.0)).item(), (a, b)


MASKS = ("plain", "ignore_neg", "mask_bool", "everything", "doc_ends")


@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("knob", sorted(KNOBS))
def test_cpu_loss_and_gradients_against_the_loops(knob, mask):
    """mean, a given ``denom``, sum and none; ``dh`` and ``dw`` by autograd against ``dlogits`` of the loops."""
    knob = KNOBS[knob]
    h, w = _hw()
    wt = _weights((B, T))
    if mask == "doc_ends":
        tg, kw = M.make_case("ignore_neg", B, T, V, seed=42)
        ids = M.P.doc_ids(T, [[0, 2, 3], [0, 4]])
        de = M.P.loop_bounds(ids)[1]
        op_kw = dict(kw, doc_bounds=ops.doc_bounds(ids), mask_doc_ends=True)
        ref_kw = dict(kw, doc_end=de)
    else:
        tg, kw = M.make_case(mask, B, T, V, seed=42)
        op_kw, ref_kw = dict(kw), dict(kw)
    for extra_op, extra_ref in ((dict(), dict()), (dict(denom=torch.tensor(5.0)), dict(denom=5.0)),
                                (dict(reduction="sum"), dict(reduction="sum"))):
        want = _ref(h, w, tg, knob, wt, **ref_kw, **extra_ref)
        h.grad = w.grad = None
        loss = TR.lm_head_loss(h, w, tg, V, **op_kw, **extra_op, **_op_kw(knob, wt))
        assert loss.dtype == F64
        loss.backward()
        _close(loss.item(), want.loss)
        d = want.dlogits.reshape(-1, V)
        _close(h.grad.reshape(-1, C), d @ w.detach()[:V])
        _close(w.grad[:V], d.t() @ h.detach().reshape(-1, C))
        assert w.grad[V:].abs().max().item() == 0.0
        assert h.grad.reshape(-1, C)[want.eff.reshape(-1) < 0].abs().sum().item() == 0.0
    with torch.no_grad():
        none = TR.lm_head_loss(h, w, tg, V, reduction="none", **op_kw, **_op_kw(knob, wt))
    want = _ref(h, w, tg, knob, wt, **ref_kw, reduction="none")
    assert none.shape == (B, T)
    _close(none, want.rows)
    assert (none[want.eff < 0] == 0).all()
    with pytest.raises(NotImplementedError):
        TR.lm_head_loss(h, w, tg, V, reduction="none", **op_kw, **_op_kw(knob, wt))


@pytest.mark.parametrize("eps", [0.1, 0.5])
def test_cpu_label_smoothing_is_torchs(eps):
    h, w = _hw(seed=43)
    tg, _ = M.make_case("ignore_neg", B, T, V, seed=44)
    loss = TR.lm_head_loss(h, w, tg, V, ignore_index=-100, label_smoothing=eps)
    loss.backward()
    hr, wr = h.detach().clone().requires_grad_(), w.detach().clone().requires_grad_()
    ref = F.cross_entropy((hr @ wr.t())[..., :V].reshape(-1, V), tg.reshape(-1), ignore_index=-100,
                          label_smoothing=eps)
    ref.backward()
    # inv is an fp32 value (1 / count), torch divides in fp64
    _close(loss.item(), ref.item(), 1e-7)
    _close(h.grad, hr.grad, 1e-7)
    _close(w.grad, wr.grad, 1e-7)
    # without ignore_index, through the new path alone
    tg2 = tg.clamp(min=0)
    _close(TR.lm_head_loss(h.detach(), w.detach(), tg2, V, label_smoothing=eps).item(),
           F.cross_entropy((hr @ wr.t())[..., :V].reshape(-1, V), tg2.reshape(-1), label_smoothing=eps).item(), 1e-7)


def test_cpu_gradcheck():
    g = torch.Generator().manual_seed(45)
    h = torch.randn(3, C, generator=g, dtype=F64).requires_grad_()
    w = torch.randn(8, C, generator=g, dtype=F64).requires_grad_()
    tg = torch.tensor([2, -100, 6])
    wt = torch.tensor([0.5, float("nan"), 1.75])

    def f(h_, w_):
        return TR.lm_head_loss(h_, w_, tg, 7, ignore_index=-100, label_smoothing=EPS, z_loss=ZC, loss_weights=wt)

    assert torch.autograd.gradcheck(f, (h, w))


def test_cpu_weighted_mean_recipe():
    h, w = _hw(seed=46)
    tg, kw = M.make_case("everything", B, T, V, seed=47)
    wt = _weights((B, T), seed=48)
    lt = ops.loss_targets(tg, vocab_size=V, **kw)
    denom = (wt * (lt.targets >= 0)).sum()
    got = TR.lm_head_loss(h, w, tg, V, denom=denom, loss_weights=wt, label_smoothing=EPS, z_loss=ZC, **kw)
    want = _ref(h, w, tg, KNOBS["all"], wt, reduction="sum", **kw)
    wsum = sum(float(wt[b, t]) for b in range(B) for t in range(T) if want.eff[b, t] >= 0)
    _close(got.item(), want.loss / wsum, 1e-6)       # 1 / denom is an fp32 value
    # the plain mean does not change with the weights' scale: it divides by the count
    a = TR.lm_head_loss(h, w, tg, V, loss_weights=wt, **kw)
    b = TR.lm_head_loss(h, w, tg, V, loss_weights=2 * wt, **kw)
    _close(b.item(), 2 * a.item())


def test_cpu_micro_batches_with_a_shared_denom():
    h, w = _hw(seed=49, b=4)
    tg, kw = M.make_case("mask_bool", 4, T, V, seed=50)
    m = kw["loss_mask"]
    m[:2, 2:] = False
    wt = _weights((4, T), seed=51)
    sm = dict(label_smoothing=EPS, z_loss=ZC)
    full = TR.lm_head_loss(h, w, tg, V, loss_mask=m, loss_weights=wt, **sm)
    gfull = torch.autograd.grad(full, (h, w))
    total = (wt * (ops.loss_targets(tg, vocab_size=V, loss_mask=m).targets >= 0)).sum()
    fullw = TR.lm_head_loss(h, w, tg, V, loss_mask=m, loss_weights=wt, denom=total, **sm)
    gfullw = torch.autograd.grad(fullw, (h, w))
    count = ops.loss_targets(tg, vocab_size=V, loss_mask=m).count.float()
    for denom, whole, gwhole in ((count, full, gfull), (total, fullw, gfullw)):
        parts, gh, gw = 0.0, torch.zeros_like(h), torch.zeros_like(w)
        for s in (slice(0, 2), slice(2, 4)):
            part = TR.lm_head_loss(h[s], w, tg[s], V, loss_mask=m[s], loss_weights=wt[s], denom=denom, **sm)
            a, b = torch.autograd.grad(part, (h, w))
            gh += a
            gw += b
            parts += part.item()
        _close(parts, whole.item())
        _close(gh, gwhole[0])
        _close(gw, gwhole[1])


def test_cpu_no_valid_target_is_zero_not_nan():
    h, w = _hw(seed=52)
    wt = _weights((B, T))
    sm = dict(label_smoothing=EPS, z_loss=ZC, loss_weights=wt)
    for kw, tg in ((dict(ignore_index=-100), torch.full((B, T), -100)),
                   (dict(loss_mask=torch.zeros(B, T, dtype=torch.bool)), torch.zeros(B, T, dtype=torch.int64))):
        h.grad = w.grad = None
        loss = TR.lm_head_loss(h, w, tg, V, **kw, **sm)
        loss.backward()
        assert loss.item() == 0.0
        assert h.grad.abs().max().item() == 0.0 and w.grad.abs().max().item() == 0.0


def test_cpu_nan_in_invalid_rows_does_not_leak():
    h, w = _hw(seed=53)
    tg = torch.randint(0, V, (B, T), generator=torch.Generator().manual_seed(54))
    tg[0, 0] = tg[1, T - 1] = -100
    tg[1, 1] = V + 3                                    # out of range: not valid either
    wt = _weights((B, T))
    sm = dict(ignore_index=-100, label_smoothing=EPS, z_loss=ZC)
    clean = TR.lm_head_loss(h, w, tg, V, loss_weights=wt, **sm)
    gclean = torch.autograd.grad(clean, (h, w))
    wn = wt.clone()
    wn[0, 0] = wn[1, 1] = float("nan")
    wn[1, T - 1] = float("inf")
    dirty = TR.lm_head_loss(h, w, tg, V, loss_weights=wn, **sm)
    assert torch.equal(dirty, clean)
    assert all(torch.equal(a, b) for a, b in zip(torch.autograd.grad(dirty, (h, w)), gclean))
    # NaN / inf logits too (made by hidden states: dw = dlogits^T h then meets 0 * NaN in the matmul's own backward,
    # which is no business of the loss, so dw is left out)
    hn = h.detach().clone()
    hn[0, 0] = float("nan")
    hn[1, T - 1] = float("inf")
    hn.requires_grad_()
    dirty = TR.lm_head_loss(hn, w, tg, V, loss_weights=wn, **sm)
    assert torch.equal(dirty, clean)
    dh, = torch.autograd.grad(dirty, (hn,))
    keep = torch.ones(B, T, dtype=torch.bool)
    keep[0, 0] = keep[1, T - 1] = False
    assert torch.equal(dh[keep], gclean[0][keep])
    assert dh[~keep].abs().max().item() == 0.0
    with torch.no_grad():
        rows = TR.lm_head_loss(hn, w, tg, V, loss_weights=wn, reduction="none", **sm)
    assert torch.isfinite(rows).all() and rows[0, 0] == 0 and rows[1, 1] == 0 and rows[1, T - 1] == 0


# --------------------------------------------------------------------------------------- the tiny GPT
CFG = dict(block_size=16, vocab_size=V, padded_vocab=Vp, n_layer=1, n_head=2, n_embd=32)


def test_gpt_forwards_the_keywords(monkeypatch):
    """The model's loss with the three keywords is the op called on its final hidden states."""
    torch.manual_seed(55)
    model = build_gpt2(GPTConfig(**CFG), seed=0, dtype=torch.float32)
    idx, tgt = torch.randint(0, V, (2, 16)), torch.randint(0, V, (2, 16))
    tgt[0, :3] = -100
    wt = _weights((2, 16))
    seen = {}
    real = TR.lm_head_loss

    def spy(x, w, *a, **kw):
        seen["x"], seen["w"] = x.detach(), w.detach()
        return real(x, w, *a, **kw)

    monkeypatch.setattr(gpt2_module.T, "lm_head_loss", spy)
    kw = dict(ignore_index=-100, label_smoothing=EPS, z_loss=ZC, loss_weights=wt)
    got = model(idx, tgt, **kw)
    assert torch.equal(got.detach(), real(seen["x"], seen["w"], tgt, V, **kw))
    want = S.loop_loss((seen["x"] @ seen["w"].t())[..., :V], tgt, V, EPS, ZC, wt, ignore_index=-100)
    _close(got.item(), want.loss, 1e-5)
    plain = model(idx, tgt, ignore_index=-100)
    for one in (dict(label_smoothing=EPS), dict(z_loss=ZC), dict(loss_weights=wt)):
        assert not torch.equal(model(idx, tgt, ignore_index=-100, **one), plain), one
    with torch.no_grad():
        assert model(idx, tgt, reduction="none", **kw).shape == (2, 16)


def test_errors():
    h, w = _hw(seed=56)
    tg = torch.zeros(B, T, dtype=torch.int64)
    ok = torch.ones(B, T)
    for bad in (dict(label_smoothing=-0.1), dict(label_smoothing=1.0), dict(label_smoothing=1.5),
                dict(label_smoothing=float("nan")), dict(label_smoothing=float("inf")),
                dict(z_loss=-1e-4), dict(z_loss=float("nan")), dict(z_loss=float("inf")),
                dict(loss_weights=ok.long()), dict(loss_weights=ok.bool()), dict(loss_weights=torch.ones(B, T + 1)),
                dict(loss_weights=torch.ones(B * T)), dict(loss_weights=ok.to("meta"))):
        with pytest.raises(ValueError):
            TR.lm_head_loss(h, w, tg, V, **bad)
    assert TR.lm_head_loss(h, w, tg, V, loss_weights=ok.double()).dtype == F64       # any floating dtype
    assert TR.lm_head_loss(h, w, tg, V, loss_weights=ok.to(torch.bfloat16)).dtype == F64


def test_defaults_are_the_call_as_it_was():
    h, w = _hw(seed=57, dtype=torch.float32)
    tg = torch.randint(0, V, (B, T), generator=torch.Generator().manual_seed(58))
    outs = []
    for kw in (dict(), dict(label_smoothing=0.0, z_loss=0.0, loss_weights=None)):
        loss = TR.lm_head_loss(h, w, tg, V, **kw)
        outs.append((loss.detach(),) + torch.autograd.grad(loss, (h, w)))
    assert all(torch.equal(a, b) for a, b in zip(*outs))
    tg[0, 0] = -100
    outs = []
    for kw in (dict(), dict(label_smoothing=0.0, z_loss=0.0, loss_weights=None)):
        loss = TR.lm_head_loss(h, w, tg, V, ignore_index=-100, **kw)
        outs.append((loss.detach(),) + torch.autograd.grad(loss, (h, w)))
    assert all(torch.equal(a, b) for a, b in zip(*outs))
