"""Masked loss on the GPU: ``k_loss_targets`` against the definition written as loops
(``tests/masked_loss_ref.py``), the ``MASK`` instantiations of the three softmax-CE kernels against fp32 torch on
the bf16 logits, the ``lm_head_loss`` op against ``F.cross_entropy(ignore_index=)``, graph replay with new masks,
the model against its CPU fp32 twin, accumulation with a shared ``denom``, and the untouched default.

Tolerances are those of the tests of the same kernels: ``test_xent_kernel_matches_torch`` (per-row loss 2e-3
absolute, gradient ``rel_err`` 1e-2), ``test_lm_head_loss`` (loss ``2e-2 * max(1, |ref|)``, gradients 3e-2) and
``test_packed_gpt2_gpu_matches_cpu_fp32`` (loss 1e-2, per-parameter cosine 0.99).  Each test prints its figures
(``-s`` shows them)."""
import functools

import pytest
import torch
import torch.nn.functional as F

from pytorch_distributed_example_amd import ops
from pytorch_distributed_example_amd._ext import kernels
from pytorch_distributed_example_amd.models import GPTConfig, build_gpt2
from pytorch_distributed_example_amd.ops import gemm as G
from pytorch_distributed_example_amd.ops import transformer as TR

import masked_loss_ref as M

pytestmark = pytest.mark.gpu

dev = "cuda"
BF16 = torch.bfloat16


def rel_err(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-12)).item()


def _bits(t):
    return t.view(torch.int16) if t.dtype == BF16 else t.view(torch.int32)


# --------------------------------------------------------------------------------------- k_loss_targets
V0 = 50
SHAPE_OF = {1: (1, 1), 63: (1, 63), 1024: (4, 256), 1025: (5, 205), 5000: (5, 1000)}


def _random_docs(B, T, seed):
    """Document starts of every row: about one per 20 positions, with a document of length 1 and, in odd rows, one
    that begins at ``T - 1``."""
    g = torch.Generator().manual_seed(seed)
    rows = []
    for b in range(B):
        s = {0} | {int(x) for x in torch.randint(0, T, (T // 20,), generator=g)}
        if T > 8:
            s |= {5, 6}
        if b % 2 and T > 1:
            s.add(T - 1)
        rows.append(sorted(s))
    return M.P.doc_ids(T, rows)


def _same(got, want, what):
    eff, count, inv, oor = want
    assert torch.equal(got.targets.cpu(), eff), what
    assert got.count.item() == count and got.out_of_range.item() == oor, (what, got.count.item(), count)
    assert torch.equal(got.inv.cpu(), inv), (what, got.inv.item(), inv.item())


@pytest.mark.parametrize("N", sorted(SHAPE_OF))
def test_loss_targets_kernel_against_the_loops(N):
    """One block's first pass covers 1024 positions: below, at and past it.  ``count`` and ``out_of_range`` are
    exact and ``inv`` has the bits of torch's fp32 ``1 / max(count, 1)`` (or ``1 / denom``)."""
    B, T = SHAPE_OF[N]
    ids = _random_docs(B, T, seed=N)
    de = M.P.loop_bounds(ids)[1]
    bounds = ops.doc_bounds(ids.to(dev))
    for name in M.CASES:
        tg, kw = M.make_case(name, B, T, V0, seed=N)
        gkw = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in kw.items()}
        for cast in (torch.int64, torch.int32):
            _same(ops.loss_targets(tg.to(dev, cast), vocab_size=V0, **gkw), M.loop_targets(tg, V0, **kw), name)
        _same(ops.loss_targets(tg.to(dev), vocab_size=V0, doc_bounds=bounds, mask_doc_ends=True, **gkw),
              M.loop_targets(tg, V0, doc_end=de, **kw), name + "+doc_ends")
        _same(ops.loss_targets(tg.to(dev), vocab_size=V0, reduction="sum", **gkw),
              M.loop_targets(tg, V0, reduction="sum", **kw), name + "+sum")
        if name in ("everything", "all_ignored"):
            for d in (3.0, 0.0, -1.5):
                _same(ops.loss_targets(tg.to(dev), vocab_size=V0, denom=torch.tensor(d, device=dev), **gkw),
                      M.loop_targets(tg, V0, denom=d, **kw), f"{name}+denom{d}")
    cpu = ops.loss_targets(tg, vocab_size=V0, doc_bounds=ops.doc_bounds(ids), mask_doc_ends=True, **kw)
    _same(ops.loss_targets(tg.to(dev), vocab_size=V0, doc_bounds=bounds, mask_doc_ends=True, **gkw),
          (cpu.targets, cpu.count.item(), cpu.inv, cpu.out_of_range.item()), "GPU against CPU op")


def test_loss_targets_gpu_errors():
    tg = torch.zeros(2, 8, dtype=torch.int64, device=dev)
    with pytest.raises(ValueError):
        ops.loss_targets(tg, vocab_size=V0, mask_doc_ends=True)
    with pytest.raises(ValueError):
        ops.loss_targets(tg, vocab_size=V0, reduction="sum", denom=torch.ones(1, device=dev))
    with pytest.raises(ValueError):
        ops.loss_targets(tg, vocab_size=V0, loss_mask=torch.ones(2, 8, dtype=torch.bool))        # on the CPU
    with pytest.raises(RuntimeError):
        kernels().loss_targets(tg.view(-1), torch.empty(16, dtype=torch.int64, device=dev),
                               torch.empty(4, dtype=torch.float32, device=dev), V0)              # info dtype


# --------------------------------------------------------------------------------------- MASK CE kernels
ROUTES = [("reg", "1", 64, 50257, 50304), ("reg2", "2", 64, 50257, 50304), ("twopass", "2", 8, 1000, 1024)]


@functools.lru_cache(maxsize=None)
def _xent_case(N, V, Vp):
    """bf16 logits (NaN in ignored row 0, +inf in the ignored last row), targets (-1 = ignored; one ignored row
    by a target past V), and the fp32 reference of the valid rows, computed once."""
    g = torch.Generator().manual_seed(21)
    logits = (3 * torch.randn(N, Vp, generator=g)).to(BF16)
    tg = torch.randint(0, V, (N,), generator=g)
    # 0, V - 1, and the first column of the last 8-wide chunk that holds vocabulary (partly padding at 50257)
    tg[1], tg[2], tg[4] = 0, V - 1, V - (V % 8 or 8)
    ign = torch.zeros(N, dtype=torch.bool)
    ign[0] = ign[N - 1] = ign[3] = True
    if N > 8:
        ign[torch.randperm(N, generator=g)[:N // 3]] = True
        ign[[1, 2, 4]] = False
    tg[ign] = -1
    tg[3] = V + 1
    logits[0] = float("nan")
    logits[N - 1] = float("inf")
    valid = ~ign
    ref = logits.float()[:, :V]
    lse = torch.logsumexp(ref[valid], 1)
    loss = torch.zeros(N)
    loss[valid] = lse - ref[valid].gather(1, tg[valid][:, None])[:, 0]
    inv = 1.0 / torch.tensor(float(valid.sum()))
    grad = torch.zeros(N, V)
    p = torch.softmax(ref[valid], 1)
    p[torch.arange(p.shape[0]), tg[valid]] -= 1
    grad[valid] = p * inv
    return logits, tg, valid, loss, grad, inv


@pytest.mark.parametrize("route,variant,N,V,Vp", ROUTES, ids=[r[0] for r in ROUTES])
def test_mask_xent_kernels_match_torch(route, variant, N, V, Vp, monkeypatch):
    """Per-row loss and in-place gradient with ``inv = 1 / count`` from device memory; padding columns and every
    column of an ignored row are exactly zero, NaN / +inf rows included; ``write_grad = 0`` leaves the logits'
    bits alone; with every row ignored everything is zero."""
    monkeypatch.setenv("PDE_XENT_V", variant)
    logits, tg, valid, want_loss, want_grad, inv = _xent_case(N, V, Vp)
    K = kernels()
    L, tgd, invd = logits.to(dev), tg.to(dev), inv.reshape(1).to(dev)
    rows = torch.full((N,), float("nan"), device=dev)
    K.xent_bf16(L, tgd, V, 1.0, rows, True, scale_dev=invd)
    got = L.float().cpu()
    e_loss = (rows.cpu() - want_loss).abs().max().item()
    e_grad = rel_err(got[valid][:, :V], want_grad[valid])
    print(f"MASK xent {route}: loss err {e_loss:.2e}, grad rel_err {e_grad:.2e}")
    assert e_loss < 2e-3
    assert e_grad < 1e-2
    assert torch.equal(got[:, V:], torch.zeros(N, Vp - V))
    assert torch.equal(got[~valid], torch.zeros(int((~valid).sum()), Vp))
    assert torch.equal(rows.cpu()[~valid], torch.zeros(int((~valid).sum())))
    # loss only
    L0 = logits.to(dev)
    rows0 = torch.full((N,), float("nan"), device=dev)
    K.xent_bf16(L0, tgd, V, 1.0, rows0, False, scale_dev=invd)
    assert (rows0.cpu() - want_loss).abs().max().item() < 2e-3
    assert torch.equal(_bits(L0.cpu()), _bits(logits))
    # nothing valid
    L1 = logits.to(dev)
    K.xent_bf16(L1, torch.full((N,), -1, device=dev), V, 1.0, rows, True, scale_dev=invd)
    assert torch.equal(L1.cpu(), torch.zeros(N, Vp, dtype=BF16)) and torch.equal(rows.cpu(), torch.zeros(N))


@pytest.mark.parametrize("route,variant,N,V,Vp", [(r[0], r[1], 64, r[3], r[4]) for r in ROUTES],
                         ids=[r[0] for r in ROUTES])
def test_mask_xent_with_nothing_ignored_has_the_unmasked_bits(route, variant, N, V, Vp, monkeypatch):
    """``N = 64``: the host's ``1 / N`` and the device's ``inv`` are the same exact fp32 value."""
    monkeypatch.setenv("PDE_XENT_V", variant)
    g = torch.Generator().manual_seed(22)
    logits = (3 * torch.randn(N, Vp, generator=g)).to(dev, BF16)
    tg = torch.randint(0, V, (N,), generator=g).to(dev)
    lt = ops.loss_targets(tg, vocab_size=V)
    assert lt.count.item() == N and torch.equal(lt.targets, tg)
    K = kernels()
    a, b = logits.clone(), logits.clone()
    ra, rb = torch.empty(N, device=dev), torch.empty(N, device=dev)
    K.xent_bf16(a, tg, V, 1.0 / N, ra, True)
    K.xent_bf16(b, lt.targets, V, 1.0, rb, True, scale_dev=lt.inv)
    assert torch.equal(a, b) and torch.equal(ra, rb)
    ta, tb = torch.empty(1, device=dev), torch.empty(1, device=dev)
    K.sum_f32(ra, ta, 1.0 / N)
    K.sum_f32(rb, tb, 1.0, scale_dev=lt.inv)
    assert torch.equal(ta, tb)


# --------------------------------------------------------------------------------------- the op
OP_SHAPES = [(37, 1000, 1024, 64), (8, 50257, 50304, 64)]


def _op_inputs(N, V, Vp, C, seed=23):
    g = torch.Generator().manual_seed(seed)
    h = torch.randn(N, C, generator=g).to(dev, BF16).requires_grad_()
    w = (0.5 * torch.randn(Vp, C, generator=g)).to(dev, BF16).requires_grad_()
    return h, w, torch.randint(0, V, (N,), generator=g)


def _mechanisms(tg, N):
    """name -> (kwargs of the op, targets given to the op, the same selection as -100 targets), each ignoring
    about half the rows, rows 0-or-1 and the neighbourhood of the last row included."""
    drop = torch.arange(N) % 2 == 0
    ids = M.P.doc_ids(N, [list(range(0, N, 2))])                   # documents of two positions
    ends = torch.zeros(N, dtype=torch.bool)
    ends[1:N - 1:2] = True                                         # every odd t but T - 1
    return {
        "ignore_index": (dict(ignore_index=-100), tg.masked_fill(drop, -100), tg.masked_fill(drop, -100)),
        "loss_mask": (dict(loss_mask=(~drop).to(dev)), tg, tg.masked_fill(drop, -100)),
        "doc_ends": (dict(doc_bounds=ops.doc_bounds(ids.to(dev)), mask_doc_ends=True), tg,
                     tg.masked_fill(ends, -100)),
    }


@pytest.mark.parametrize("N,V,Vp,C", OP_SHAPES)
def test_masked_lm_head_loss_matches_torch(N, V, Vp, C):
    h, w, tg = _op_inputs(N, V, Vp, C)
    for name, (kw, given, masked) in _mechanisms(tg, N).items():
        h.grad = w.grad = None
        loss = TR.lm_head_loss(h, w, given.to(dev), V, **kw)
        loss.backward()
        hr, wr = h.detach().float().requires_grad_(), w.detach().float().requires_grad_()
        lr = F.cross_entropy((hr @ wr.t())[:, :V], masked.to(dev), ignore_index=-100)
        lr.backward()
        print(f"masked lm_head_loss {name} N={N}: {loss.item():.5f} vs {lr.item():.5f}, "
              f"dh {rel_err(h.grad, hr.grad):.2e}, dw {rel_err(w.grad, wr.grad):.2e}")
        assert abs(loss.item() - lr.item()) < 2e-2 * max(1.0, abs(lr.item())), name
        assert rel_err(h.grad, hr.grad) < 3e-2, name
        assert rel_err(w.grad, wr.grad) < 3e-2, name
        assert w.grad[V:].abs().max().item() == 0.0
        ign = (masked == -100).to(dev)
        assert ign.any() and torch.equal(h.grad[ign], torch.zeros_like(h.grad[ign])), name
        with torch.no_grad():
            s = TR.lm_head_loss(h, w, given.to(dev), V, reduction="sum", **kw)
            sr = F.cross_entropy((hr @ wr.t())[:, :V], masked.to(dev), ignore_index=-100, reduction="sum")
            assert abs(s.item() - sr.item()) < 2e-2 * max(1.0, abs(sr.item())), name
            per = TR.lm_head_loss(h, w, given.to(dev), V, reduction="none", **kw)
            pr = F.cross_entropy((hr @ wr.t())[:, :V], masked.to(dev), ignore_index=-100, reduction="none")
            assert per.dtype == torch.float32 and per.shape == (N,)
            assert (per - pr).abs().max().item() < 2e-2 * max(1.0, pr.abs().max().item()), name
            assert torch.equal(per[ign], torch.zeros_like(per[ign]))
    with pytest.raises(NotImplementedError):
        TR.lm_head_loss(h, w, tg.to(dev), V, ignore_index=-100, reduction="none")


@pytest.mark.parametrize("N,V,Vp,C", OP_SHAPES)
def test_masked_lm_head_loss_zero_count(N, V, Vp, C):
    """No valid target: loss 0 and exactly zero gradients (``F.cross_entropy`` gives NaN)."""
    h, w, tg = _op_inputs(N, V, Vp, C)
    for kw, given in ((dict(ignore_index=-100), torch.full((N,), -100)),
                      (dict(loss_mask=torch.zeros(N, dtype=torch.bool, device=dev)), tg)):
        h.grad = w.grad = None
        loss = TR.lm_head_loss(h, w, given.to(dev), V, **kw)
        loss.backward()
        assert loss.item() == 0.0
        assert torch.equal(h.grad, torch.zeros_like(h)) and torch.equal(w.grad, torch.zeros_like(w))


@pytest.mark.parametrize("N,V,Vp,C", OP_SHAPES)
def test_every_flavour_is_its_launches_written_out(N, V, Vp, C):
    """Plain, masked and smoothed, ``mean`` and ``none``: the op's result has the bits of ``G.fprop`` +
    ``xent_bf16`` + ``sum_f32`` called here with the arguments the host path is documented to pass (plain: the
    host's ``1 / N``; otherwise ``scale = 1`` with ``loss_targets``' ``inv`` as ``scale_dev``, and the three
    smoothing keywords only when something is smoothed).  ``dh`` of the ``mean`` calls is compared with the dgrad
    GEMM of the ``dlogits`` written here, which pins the scale inside the CE kernel too.  One target is ``-1``:
    with default keywords its row is zero and still counts in ``N``: ``loss * N`` is the sum of the rows to 1e-5
    (an fp32 sum of ``N <= 37`` positive terms is off by at most ``N * 2^-24 = 2.2e-6``; dividing by the count
    ``N - 1`` instead would be off by ``1 / N >= 2.7e-2``)."""
    h, w, tg = _op_inputs(N, V, Vp, C, seed=29)
    tg[N // 2] = -1
    tg = tg.to(dev)
    mask = (torch.arange(N) % 3 != 0).to(dev)
    wt = (2 * torch.rand(N, generator=torch.Generator().manual_seed(30))).to(dev)
    sm = dict(label_smoothing=0.1, z_loss=1e-3, loss_weights=wt)
    K = kernels()
    one = torch.ones(1, device=dev)

    def written_out(targets, write_grad, scale, **smooth):
        logits = G.fprop(h.detach(), w.detach(), nt_out=True)
        rows, tot = torch.empty(N, device=dev), torch.empty(1, device=dev)
        K.xent_bf16(logits, targets, V, loss_rows=rows, write_grad=write_grad, **scale, **smooth)
        K.sum_f32(rows, tot, **scale)
        return rows, tot.reshape(()), (G.dgrad(logits, w.detach(), scale=one) if write_grad else None)

    for name, kw, smooth in (("plain", {}, {}), ("masked", dict(loss_mask=mask), {}), ("smoothed", sm, sm)):
        if name == "plain":
            targets, scale = tg, dict(scale=1.0 / N)
        else:
            lt = ops.loss_targets(tg, vocab_size=V, loss_mask=kw.get("loss_mask"))
            targets, scale = lt.targets, dict(scale=1.0, scale_dev=lt.inv)
        loss = TR.lm_head_loss(h, w, tg, V, **kw)
        dh, = torch.autograd.grad(loss, h)
        rows, tot, dh_ref = written_out(targets, True, scale, **smooth)
        assert torch.equal(loss.detach(), tot) and torch.equal(dh, dh_ref), name
        assert rows[N // 2].item() == 0.0 and not dh[N // 2].any(), name
        if name == "plain":     # the -1 row counts in the mean's denominator: sum / N, not sum / (N - 1)
            total = rows.double().sum().item()
            assert rows.count_nonzero().item() == N - 1 and abs(loss.item() * N - total) <= 1e-5 * total
        # reduction="none" is not a default: without other keywords it is the masked flavour with every row selected
        with torch.no_grad():
            per = TR.lm_head_loss(h, w, tg, V, reduction="none", **kw)
        lt = ops.loss_targets(tg, vocab_size=V, loss_mask=kw.get("loss_mask"), reduction="none")
        rows = written_out(lt.targets, False, dict(scale=1.0, scale_dev=lt.inv), **smooth)[0]
        assert per.shape == (N,) and torch.equal(per, rows), name


# --------------------------------------------------------------------------------------- replay
def test_replay_with_new_masks():
    """Forward + backward of the op captured once with static ``targets`` and ``loss_mask`` buffers; three masks
    (one with everything ignored) are copied in and replayed.  The loss and ``dh`` have the bits of an eager call
    on the same inputs.  ``dw`` comes from the split-K wgrad GEMM: it is compared bit for bit if two eager runs of
    it agree bit for bit (they do on the MI355X: the slabs are summed in slab order), else at ``rel_err < 3e-2``."""
    N, V, Vp, C = 37, 1000, 1024, 64
    h, w, tg = _op_inputs(N, V, Vp, C, seed=24)
    g = torch.Generator().manual_seed(25)
    masks = [torch.rand(N, generator=g) < 0.5, torch.zeros(N, dtype=torch.bool), torch.rand(N, generator=g) < 0.8]
    tgs = [torch.randint(0, V, (N,), generator=g).masked_fill(torch.rand(N, generator=g) < 0.2, -100)
           for _ in masks]
    s_tg, s_m = tgs[0].to(dev), masks[0].to(dev)

    def step(t, m):
        loss = TR.lm_head_loss(h, w, t, V, ignore_index=-100, loss_mask=m)
        dh, dw = torch.autograd.grad(loss, (h, w))
        return loss.detach(), dh, dw

    cur = torch.cuda.current_stream()
    side = torch.cuda.Stream()
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        step(s_tg, s_m)                                    # warm-up outside the capture
    cur.wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step(s_tg, s_m)
    eager = [step(t.to(dev), m.to(dev)) for t, m in zip(tgs, masks)]
    again = [step(t.to(dev), m.to(dev)) for t, m in zip(tgs, masks)]
    dw_exact = all(torch.equal(a[2], b[2]) for a, b in zip(eager, again))
    print(f"replay: eager dw bit-stable = {dw_exact}, losses {[e[0].item() for e in eager]}")
    losses = [e[0].item() for e in eager]
    assert len(set(losses)) == 3 and losses[1] == 0.0
    for i in (0, 1, 2, 0):
        s_tg.copy_(tgs[i])
        s_m.copy_(masks[i])
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out[0], eager[i][0]) and torch.equal(out[1], eager[i][1]), i
        if dw_exact:
            assert torch.equal(out[2], eager[i][2]), i
        else:
            assert rel_err(out[2], eager[i][2]) < 3e-2 or eager[i][2].abs().max().item() == 0.0, i


# --------------------------------------------------------------------------------------- model
CFG = dict(block_size=256, vocab_size=1000, padded_vocab=1024, n_layer=2, n_head=2, n_embd=128)
B, T = 4, 256


@functools.lru_cache(maxsize=None)
def _models():
    cfg = GPTConfig(**CFG)
    g = build_gpt2(cfg, seed=0, device=dev)
    c = build_gpt2(cfg, seed=0, dtype=torch.float32)
    with torch.no_grad():
        g.transformer.wpe.weight.normal_(0.0, 0.1)
        for pc, pg in zip(c.parameters(), g.parameters()):
            pc.copy_(pg.float())
    gen = torch.Generator().manual_seed(26)
    idx = torch.randint(0, cfg.vocab_size, (B, T), generator=gen)
    tgt = torch.randint(0, cfg.vocab_size, (B, T), generator=gen)
    ids = torch.cat([M.P.layout("mid200", 2, T), M.P.layout("len1", 2, T)])
    m = torch.ones(B, T, dtype=torch.bool)
    m[:, :40] = False                                      # the "prompt" of every row
    return g, c, idx, tgt, ids, m


def test_masked_gpt2_gpu_matches_cpu_fp32():
    g, c, idx, tgt, ids, m = _models()
    g.zero_grad(set_to_none=True)
    c.zero_grad(set_to_none=True)
    lg = g(idx.to(dev), tgt.to(dev), doc_ids=ids.to(dev), mask_doc_ends=True, loss_mask=m.to(dev))
    lc = c(idx, tgt, doc_ids=ids, mask_doc_ends=True, loss_mask=m)
    lg.backward()
    lc.backward()
    n_ends = sum(len(r) - 1 for n in ("mid200", "len1") for r in M.P.LAYOUTS[n](T)[:2])
    count = ops.loss_targets(tgt.to(dev), vocab_size=CFG["vocab_size"], loss_mask=m.to(dev),
                             doc_bounds=ops.doc_bounds(ids.to(dev)), mask_doc_ends=True).count.item()
    assert count == B * (T - 40) - n_ends                  # every masked end lies past position 40
    fails = []
    if not abs(lg.item() - lc.item()) < 1e-2:
        fails.append(f"loss {lg.item():.5f} vs {lc.item():.5f}")
    for (n, pg), pc in zip(g.named_parameters(), c.parameters()):
        cos = F.cosine_similarity(pg.grad.float().flatten().cpu(), pc.grad.flatten(), dim=0).item()
        if not cos >= 0.99:
            fails.append(f"grad {n}: cos {cos:.4f}")
    print(f"MASKED model parity: loss {lg.item():.5f} vs {lc.item():.5f}, count {count}")
    assert not fails, fails


def test_accumulation_with_a_shared_denom():
    """Two micro-batches, each given the total count as ``denom``, against the one full batch."""
    g, _, idx, tgt, ids, m = _models()
    idx, tgt, m = idx.to(dev), tgt.to(dev), m.clone().to(dev)
    m[:2, 100:] = False                                    # very different counts in the two halves
    g.zero_grad(set_to_none=True)
    full = g(idx, tgt, loss_mask=m)
    full.backward()
    want = [p.grad.clone() for p in g.parameters()]
    total = ops.loss_targets(tgt, vocab_size=CFG["vocab_size"], loss_mask=m).count.float()
    g.zero_grad(set_to_none=True)
    parts = []
    for s in (slice(0, 2), slice(2, 4)):
        part = g(idx[s], tgt[s], loss_mask=m[s], denom=total)
        part.backward()
        parts.append(part.item())
    worst = max(rel_err(p.grad, gw) for p, gw in zip(g.parameters(), want))
    print(f"accumulation: {sum(parts):.5f} vs {full.item():.5f}, worst grad rel_err {worst:.2e}")
    assert abs(sum(parts) - full.item()) < 2e-2 * abs(full.item())
    assert worst < 3e-2
    g.zero_grad(set_to_none=True)


def test_defaults_are_unchanged_bit_for_bit():
    """All-default keywords against the bare calls, a batch with a ``-1`` target included (loss 0 for that row,
    still divided by ``N``)."""
    N, V, Vp, C = 37, 1000, 1024, 64
    h, w, tg = _op_inputs(N, V, Vp, C, seed=27)
    tg[5] = -1
    outs = []
    for kw in ({}, dict(ignore_index=None, loss_mask=None, doc_bounds=None, mask_doc_ends=False, reduction="mean",
                        denom=None)):
        h.grad = w.grad = None
        loss = TR.lm_head_loss(h, w, tg.to(dev), V, **kw)
        loss.backward()
        outs.append((loss.detach(), h.grad, w.grad))
    assert all(torch.equal(a, b) for a, b in zip(*outs))
    g, _, idx, tgt, ids, _ = _models()
    tgt = tgt.clone()
    tgt[0, 3] = -1
    outs = []
    for kw in ({}, dict(ignore_index=None, loss_mask=None, mask_doc_ends=False, reduction="mean", denom=None)):
        g.zero_grad(set_to_none=True)
        loss = g(idx.to(dev), tgt.to(dev), **kw)
        loss.backward()
        outs.append([loss.detach()] + [p.grad.clone() for p in g.parameters()])
    assert all(torch.equal(a, b) for a, b in zip(*outs))
    g.zero_grad(set_to_none=True)
