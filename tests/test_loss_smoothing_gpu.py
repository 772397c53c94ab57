"""Smoothed and weighted loss on the GPU: the ``SMOOTH`` instantiations of the three softmax-CE kernels against the
definition written as fp64 loops (``tests/loss_smoothing_ref.py``) on the same bf16 logits, element by element;
their bits against the ``MASK`` instantiations' when nothing is smoothed; ``lm_head_loss`` against its CPU fp32
path; graph replay with new weights, targets and masks; the model against its CPU fp32 twin; accumulation with a
shared weighted ``denom``; the untouched default.

``eps = 0.1`` and ``zc = 1e-3`` (ten times the usual value, so that its term stands clear of rounding); weights
from ``[0, 2]`` with an exact 0 and an exact 1.  Gradient bound, per element of every valid row::

    |got - want| <= 2^-7 * w * inv * ((1 + 2 zc lse) p[v] + (1 - eps) [v == t] + eps / V)

one fp16 round-toward-zero of ``p`` on the ``reg2`` route (2^-10) plus one bf16 rounding of the result (2^-9),
applied to the sum of the terms' magnitudes, is under 2^-8; the bound doubles it.  A norm would not do: at
V = 50257 the whole ``eps / V`` term has a norm of about 5e-4 of the row's.  Per-row loss: 4e-3 absolute, the 2e-3
of ``test_masked_loss_gpu.py`` times the largest weight.  The op and the model keep the bounds of that file for
the same quantities.  Each test prints its figures (``-s`` shows them)."""
import functools

import pytest
import torch
import torch.nn.functional as F

from pytorch_distributed_example_amd import ops
from pytorch_distributed_example_amd._ext import kernels
from pytorch_distributed_example_amd.ops import transformer as TR

import loss_smoothing_ref as S
import test_masked_loss_gpu as MG

pytestmark = pytest.mark.gpu

dev = "cuda"
BF16 = torch.bfloat16
EPS, ZC = 0.1, 1e-3
rel_err = MG.rel_err

# route, PDE_XENT_V, N, V, Vp
ROUTES = [("reg", "1", 24, 50257, 50304),              # the two-exp register-resident kernel
          ("reg2", "2", 24, 50257, 50304),             # the last vocabulary chunk is partly padding
          ("reg2_whole_chunk", "2", 24, 32760, 32768),  # the padding is exactly one chunk; the smallest wide row
          ("reg_narrow_pad", "2", 24, 32765, 32768),   # Vp - V < 8 forces the old wide kernel
          ("twopass", "2", 8, 1000, 1024)]
IDS = [r[0] for r in ROUTES]


def _weights(n, g):
    wt = 2 * torch.rand(n, generator=g)
    return wt


@functools.lru_cache(maxsize=None)
def _case(N, V, Vp):
    """bf16 logits (NaN in ignored row 0, +inf in the ignored last row, random padding columns), targets (-1 =
    ignored; row 3 ignored by a target past V), weights (NaN on ignored row 0; an exact 0 and an exact 1 on valid
    rows) and the fp64 loops over the valid rows, computed once per shape."""
    g = torch.Generator().manual_seed(31)
    logits = (3 * torch.randn(N, Vp, generator=g)).to(BF16)
    tg = torch.randint(0, V, (N,), generator=g)
    # 0, V - 1, and the first column of the last 8-wide chunk that holds vocabulary
    tg[1], tg[2], tg[4] = 0, V - 1, V - (V % 8 or 8)
    ign = torch.zeros(N, dtype=torch.bool)
    ign[0] = ign[N - 1] = ign[3] = True
    if N > 8:
        ign[torch.randperm(N, generator=g)[:N // 3]] = True
        ign[[1, 2, 4, 5]] = False
    tg[ign] = -1
    tg[3] = V + 1
    logits[0] = float("nan")
    logits[N - 1] = float("inf")
    wt = _weights(N, g)
    wt[5], wt[2] = 0.0, 1.0
    wt[0] = float("nan")
    want = S.loop_loss(logits[None], tg[None], V, EPS, ZC, wt[None])
    assert torch.equal(want.eff[0] >= 0, ~ign) and want.count == int((~ign).sum())
    return logits, tg, ~ign, wt, want


def _run(logits, tg, V, inv, wt, write_grad=True, eps=EPS, zc=ZC):
    L = logits.to(dev)
    rows = torch.full((L.shape[0],), float("nan"), device=dev)
    kernels().xent_bf16(L, tg.to(dev), V, 1.0, rows, write_grad,
                        scale_dev=torch.tensor([inv], dtype=torch.float32, device=dev), label_smoothing=eps,
                        z_loss=zc, loss_weights=None if wt is None else wt.to(dev))
    return L.cpu(), rows.cpu()


@pytest.mark.parametrize("route,variant,N,V,Vp", ROUTES, ids=IDS)
def test_smooth_xent_kernels_against_the_loops(route, variant, N, V, Vp, monkeypatch):
    monkeypatch.setenv("PDE_XENT_V", variant)
    logits, tg, valid, wt, want = _case(N, V, Vp)
    nign = int((~valid).sum())
    L, rows = _run(logits, tg, V, want.inv, wt)
    got = L.double()
    err = (got[valid][:, :V] - want.dlogits[0][valid]).abs()
    mag = want.mag[0][valid]
    ratio = torch.where(mag > 0, err / mag.clamp_min(1e-300), torch.where(err > 0, float("inf"), 0.0).double())
    e_loss = (rows.double() - want.rows[0]).abs().max().item()
    print(f"SMOOTH xent {route}: largest |got - want| / magnitude = {ratio.max().item():.3e} (bound {2.0 ** -7:.3e}), "
          f"loss err {e_loss:.2e}")
    assert (err <= 2.0 ** -7 * mag).all(), ratio.max().item()
    assert e_loss <= 4e-3
    assert torch.equal(L[:, V:], torch.zeros(N, Vp - V, dtype=BF16))
    assert torch.equal(L[~valid], torch.zeros(nign, Vp, dtype=BF16))
    assert torch.equal(rows[~valid], torch.zeros(nign))
    assert torch.equal(L[5].float(), torch.zeros(Vp)) and rows[5].item() == 0.0        # the valid row of weight 0
    # loss only: the logits' bits stay, the rows are the same
    L0, rows0 = _run(logits, tg, V, want.inv, wt, write_grad=False)
    assert torch.equal(MG._bits(L0), MG._bits(logits))
    if route.startswith("reg2"):      # loss-only calls take the two-exp kernel: same value, other rounding
        assert (rows0.double() - want.rows[0]).abs().max().item() <= 4e-3
        assert torch.equal(rows0[~valid], torch.zeros(nign))
    else:
        assert torch.equal(rows0, rows)
    # nothing valid
    L1, rows1 = _run(logits, torch.full((N,), -1), V, want.inv, wt)
    assert torch.equal(L1, torch.zeros(N, Vp, dtype=BF16)) and torch.equal(rows1, torch.zeros(N))


@pytest.mark.parametrize("route,variant,N,V,Vp", ROUTES, ids=IDS)
def test_nothing_smoothed_has_the_mask_bits(route, variant, N, V, Vp, monkeypatch):
    """``eps = 0``, ``zc = 0`` and weights all 1.0 through the ``SMOOTH`` instantiation: ``1 + 0``, ``x - 0`` and
    ``1 * x`` are exact, so rows and gradient have the ``MASK`` instantiation's bits."""
    monkeypatch.setenv("PDE_XENT_V", variant)
    logits, tg, valid, _, want = _case(N, V, Vp)
    for write_grad in (True, False):
        a = logits.to(dev)
        ra = torch.full((N,), float("nan"), device=dev)
        kernels().xent_bf16(a, tg.to(dev), V, 1.0, ra, write_grad,
                            scale_dev=torch.tensor([want.inv], dtype=torch.float32, device=dev))
        b, rb = _run(logits, tg, V, want.inv, torch.ones(N), write_grad=write_grad, eps=0.0, zc=0.0)
        assert torch.equal(MG._bits(a.cpu()), MG._bits(b)), write_grad
        assert torch.equal(ra.cpu(), rb), write_grad
    assert int(valid.sum()) > 0 and ra.cpu()[valid].abs().min().item() > 0.0


def test_kernel_binding_errors():
    L = torch.zeros(4, 1024, device=dev, dtype=BF16)
    tg = torch.zeros(4, dtype=torch.int64, device=dev)
    rows = torch.empty(4, device=dev)
    one = torch.ones(1, device=dev)
    K = kernels()
    with pytest.raises(RuntimeError):
        K.xent_bf16(L, tg, 1000, 1.0, rows, True, label_smoothing=0.1)                       # needs scale_dev
    with pytest.raises(RuntimeError):
        K.xent_bf16(L, tg, 1000, 1.0, rows, True, scale_dev=one, label_smoothing=1.0)
    with pytest.raises(RuntimeError):
        K.xent_bf16(L, tg, 1000, 1.0, rows, True, scale_dev=one, z_loss=-1.0)
    with pytest.raises(RuntimeError):
        K.xent_bf16(L, tg, 1000, 1.0, rows, True, scale_dev=one, loss_weights=torch.ones(3, device=dev))
    with pytest.raises(RuntimeError):
        K.xent_bf16(L, tg, 1000, 1.0, rows, True, scale_dev=one, loss_weights=torch.ones(4))  # on the CPU


# --------------------------------------------------------------------------------------- the op
def _knobs(N, seed=32):
    g = torch.Generator().manual_seed(seed)
    wt = _weights(N, g)
    wt[1], wt[2] = 0.0, 1.0
    drop = torch.arange(N) % 3 == 0
    mask = torch.rand(N, generator=g) < 0.7
    return {
        "eps": (dict(label_smoothing=EPS), None, None),
        "zc": (dict(z_loss=ZC), None, None),
        "weights": (dict(loss_weights=wt), None, None),
        "all": (dict(label_smoothing=EPS, z_loss=ZC, loss_weights=wt), None, None),
        "all+masks": (dict(label_smoothing=EPS, z_loss=ZC, loss_weights=wt, ignore_index=-100), drop, mask),
    }


def _to(kw, device):
    return {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in kw.items()}


@pytest.mark.parametrize("N,V,Vp,C", MG.OP_SHAPES)
def test_smooth_lm_head_loss_matches_the_cpu_fp32_path(N, V, Vp, C):
    h, w, tg = MG._op_inputs(N, V, Vp, C, seed=33)
    hc, wc = h.detach().cpu().float(), w.detach().cpu().float()
    for name, (kw, drop, mask) in _knobs(N).items():
        given = tg if drop is None else tg.masked_fill(drop, -100)
        kw = dict(kw) if mask is None else dict(kw, loss_mask=mask)
        h.grad = w.grad = None
        loss = TR.lm_head_loss(h, w, given.to(dev), V, **_to(kw, dev))
        loss.backward()
        hr, wr = hc.clone().requires_grad_(), wc.clone().requires_grad_()
        lr = TR.lm_head_loss(hr, wr, given, V, **kw)
        lr.backward()
        print(f"smooth lm_head_loss {name} N={N}: {loss.item():.5f} vs {lr.item():.5f}, "
              f"dh {rel_err(h.grad, hr.grad):.2e}, dw {rel_err(w.grad, wr.grad):.2e}")
        assert abs(loss.item() - lr.item()) < 2e-2 * max(1.0, abs(lr.item())), name
        assert rel_err(h.grad, hr.grad) < 3e-2, name
        assert rel_err(w.grad, wr.grad) < 3e-2, name
        assert w.grad[V:].abs().max().item() == 0.0
        if drop is not None:
            ign = (drop | ~mask).to(dev)
            assert ign.any() and torch.equal(h.grad[ign], torch.zeros_like(h.grad[ign])), name
        with torch.no_grad():
            s = TR.lm_head_loss(h, w, given.to(dev), V, reduction="sum", **_to(kw, dev))
            sr = TR.lm_head_loss(hc, wc, given, V, reduction="sum", **kw)
            assert abs(s.item() - sr.item()) < 2e-2 * max(1.0, abs(sr.item())), name
            per = TR.lm_head_loss(h, w, given.to(dev), V, reduction="none", **_to(kw, dev))
            pr = TR.lm_head_loss(hc, wc, given, V, reduction="none", **kw)
            assert per.dtype == torch.float32 and per.shape == (N,)
            assert (per.cpu() - pr).abs().max().item() < 2e-2 * max(1.0, pr.abs().max().item()), name
            if drop is not None:
                assert torch.equal(per[ign], torch.zeros_like(per[ign]))
    with pytest.raises(NotImplementedError):
        TR.lm_head_loss(h, w, tg.to(dev), V, label_smoothing=EPS, reduction="none")
    with pytest.raises(ValueError):
        TR.lm_head_loss(h, w, tg.to(dev), V, loss_weights=torch.ones(N))                     # on the CPU
    with pytest.raises(ValueError):
        TR.lm_head_loss(h, w, tg.to(dev), V, loss_weights=torch.ones(N, device=dev, dtype=torch.int32))


@pytest.mark.parametrize("N,V,Vp,C", MG.OP_SHAPES)
def test_smooth_lm_head_loss_zero_count(N, V, Vp, C):
    h, w, tg = MG._op_inputs(N, V, Vp, C, seed=34)
    wt = torch.full((N,), float("nan"), device=dev)        # never read
    sm = dict(label_smoothing=EPS, z_loss=ZC, loss_weights=wt)
    for kw, given in ((dict(ignore_index=-100), torch.full((N,), -100)),
                      (dict(loss_mask=torch.zeros(N, dtype=torch.bool, device=dev)), tg)):
        h.grad = w.grad = None
        loss = TR.lm_head_loss(h, w, given.to(dev), V, **kw, **sm)
        loss.backward()
        assert loss.item() == 0.0
        assert torch.equal(h.grad, torch.zeros_like(h)) and torch.equal(w.grad, torch.zeros_like(w))


# --------------------------------------------------------------------------------------- replay
def test_replay_with_new_weights_targets_and_masks():
    """Forward + backward captured once with static ``targets``, ``loss_mask`` and ``loss_weights`` buffers; new
    data is copied in and replayed.  Loss and ``dh`` have the bits of an eager call on the same data; ``dw`` (the
    split-K wgrad GEMM) too where two eager runs of it agree bit for bit, as ``test_replay_with_new_masks`` does."""
    N, V, Vp, C = 37, 1000, 1024, 64
    h, w, tg = MG._op_inputs(N, V, Vp, C, seed=35)
    g = torch.Generator().manual_seed(36)
    masks = [torch.rand(N, generator=g) < 0.5, torch.zeros(N, dtype=torch.bool), torch.rand(N, generator=g) < 0.8]
    tgs = [torch.randint(0, V, (N,), generator=g).masked_fill(torch.rand(N, generator=g) < 0.2, -100)
           for _ in masks]
    wts = [_weights(N, g) for _ in masks]
    s_tg, s_m, s_w = tgs[0].to(dev), masks[0].to(dev), wts[0].to(dev)

    def step(t, m, wt):
        loss = TR.lm_head_loss(h, w, t, V, ignore_index=-100, loss_mask=m, label_smoothing=EPS, z_loss=ZC,
                               loss_weights=wt)
        dh, dw = torch.autograd.grad(loss, (h, w))
        return loss.detach(), dh, dw

    cur = torch.cuda.current_stream()
    side = torch.cuda.Stream()
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        step(s_tg, s_m, s_w)                               # warm-up outside the capture
    cur.wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step(s_tg, s_m, s_w)
    data = list(zip(tgs, masks, wts)) + [(tgs[0], masks[0], wts[2])]      # the weights alone change
    eager = [step(*(x.to(dev) for x in d)) for d in data]
    again = [step(*(x.to(dev) for x in d)) for d in data]
    dw_exact = all(torch.equal(a[2], b[2]) for a, b in zip(eager, again))
    losses = [e[0].item() for e in eager]
    print(f"replay: eager dw bit-stable = {dw_exact}, losses {losses}")
    assert len(set(losses)) == 4 and losses[1] == 0.0
    for i in (0, 1, 2, 3, 0):
        for buf, new in zip((s_tg, s_m, s_w), data[i]):
            buf.copy_(new)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out[0], eager[i][0]) and torch.equal(out[1], eager[i][1]), i
        if dw_exact:
            assert torch.equal(out[2], eager[i][2]), i
        else:
            assert rel_err(out[2], eager[i][2]) < 3e-2 or eager[i][2].abs().max().item() == 0.0, i


# --------------------------------------------------------------------------------------- defaults, model
def test_default_keywords_are_the_call_without_them():
    N, V, Vp, C = 37, 1000, 1024, 64
    h, w, tg = MG._op_inputs(N, V, Vp, C, seed=37)
    tg[5] = -1
    for base in (dict(), dict(ignore_index=-1)):
        outs = []
        for kw in (dict(), dict(label_smoothing=0.0, z_loss=0.0, loss_weights=None)):
            h.grad = w.grad = None
            loss = TR.lm_head_loss(h, w, tg.to(dev), V, **base, **kw)
            loss.backward()
            outs.append((loss.detach(), h.grad, w.grad))
        assert all(torch.equal(a, b) for a, b in zip(*outs)), base
    g, _, idx, tgt, _, _ = MG._models()
    outs = []
    for kw in (dict(), dict(label_smoothing=0.0, z_loss=0.0, loss_weights=None)):
        g.zero_grad(set_to_none=True)
        loss = g(idx.to(dev), tgt.to(dev), **kw)
        loss.backward()
        outs.append([loss.detach()] + [p.grad.clone() for p in g.parameters()])
    assert all(torch.equal(a, b) for a, b in zip(*outs))
    g.zero_grad(set_to_none=True)


def _model_weights():
    wt = _weights(MG.B * MG.T, torch.Generator().manual_seed(38)).view(MG.B, MG.T)
    wt[0, 50], wt[0, 51] = 0.0, 1.0
    return wt


def test_smooth_gpt2_gpu_matches_cpu_fp32():
    g, c, idx, tgt, ids, m = MG._models()
    wt = _model_weights()
    g.zero_grad(set_to_none=True)
    c.zero_grad(set_to_none=True)
    sm = dict(mask_doc_ends=True, label_smoothing=EPS, z_loss=ZC)
    lg = g(idx.to(dev), tgt.to(dev), doc_ids=ids.to(dev), loss_mask=m.to(dev), loss_weights=wt.to(dev), **sm)
    lc = c(idx, tgt, doc_ids=ids, loss_mask=m, loss_weights=wt, **sm)
    with torch.no_grad():
        plain = c(idx, tgt, doc_ids=ids, loss_mask=m, mask_doc_ends=True)
    lg.backward()
    lc.backward()
    fails = []
    if not abs(lg.item() - lc.item()) < 1e-2:
        fails.append(f"loss {lg.item():.5f} vs {lc.item():.5f}")
    for (n, pg), pc in zip(g.named_parameters(), c.parameters()):
        cos = F.cosine_similarity(pg.grad.float().flatten().cpu(), pc.grad.flatten(), dim=0).item()
        if not cos >= 0.99:
            fails.append(f"grad {n}: cos {cos:.4f}")
    print(f"SMOOTH model parity: loss {lg.item():.5f} vs {lc.item():.5f} (unsmoothed {plain.item():.5f})")
    assert not fails, fails
    g.zero_grad(set_to_none=True)
    c.zero_grad(set_to_none=True)


def test_accumulation_with_a_shared_weighted_denom():
    """Two micro-batches, each given the whole batch's weight sum as ``denom``, against the one full batch."""
    g, _, idx, tgt, _, m = MG._models()
    idx, tgt, m, wt = idx.to(dev), tgt.to(dev), m.clone().to(dev), _model_weights().to(dev)
    m[:2, 100:] = False                                    # very different counts in the two halves
    sm = dict(label_smoothing=EPS, z_loss=ZC)
    lt = ops.loss_targets(tgt, vocab_size=MG.CFG["vocab_size"], loss_mask=m)
    total = (wt * (lt.targets >= 0)).sum()
    g.zero_grad(set_to_none=True)
    full = g(idx, tgt, loss_mask=m, loss_weights=wt, denom=total, **sm)
    full.backward()
    want = [p.grad.clone() for p in g.parameters()]
    g.zero_grad(set_to_none=True)
    parts = []
    for s in (slice(0, 2), slice(2, 4)):
        part = g(idx[s], tgt[s], loss_mask=m[s], loss_weights=wt[s], denom=total, **sm)
        part.backward()
        parts.append(part.item())
    worst = max(rel_err(p.grad, gw) for p, gw in zip(g.parameters(), want))
    print(f"weighted accumulation: {sum(parts):.5f} vs {full.item():.5f}, worst grad rel_err {worst:.2e}")
    assert abs(sum(parts) - full.item()) < 2e-2 * abs(full.item())
    assert worst < 3e-2
    g.zero_grad(set_to_none=True)
