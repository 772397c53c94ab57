"""Packed sequences on the GPU: the document-masked (``DOC``) instantiations of the flash-attention kernels
against the fp64 reference of ``tests/attention_ref.py`` with an ``allowed`` mask, under its per-row metric and
``A.BOUND`` unchanged (a document-masked row is a causal row of a shorter sequence, so the floor measured for
causal rows up to T = 1024 covers it); isolation, dropout and graph replay of the op; the embedding with
positions that restart per document; and the model against its CPU fp32 twin.  Layouts and the "needle outside"
family are in ``tests/packed_ref.py``.  Each test prints its worst errors (``-s`` shows them)."""
import functools
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

from pytorch_distributed_example_amd import ops
from pytorch_distributed_example_amd._ext import kernels
from pytorch_distributed_example_amd.models import GPTConfig, build_gpt2
from pytorch_distributed_example_amd.ops import DeviceRNG
from pytorch_distributed_example_amd.ops import rng as R
from pytorch_distributed_example_amd.ops import transformer as TR

import attention_ref as A
import packed_ref as P

pytestmark = pytest.mark.gpu

dev = "cuda"
BF16 = torch.bfloat16
NAN = float("nan")
OUTS = ("y", "dq", "dk", "dv")
ALL = OUTS + ("lse2", "D")

SHAPES = [(2, 256, 3), (1, 384, 2)]
FAMILIES = ("gauss1", "needle_outside")
CASES = [(f, l, s) for s in SHAPES for l in P.LAYOUTS for f in FAMILIES]


def _id(case):
    f, l, (B, T, H) = case
    return f"{f}-{l}-{B}x{T}x{H}"


@functools.lru_cache(maxsize=None)
def _bounds(name, B, T):
    """(ids, doc_start, doc_end) on the CPU, by the loops of packed_ref (never by the code under test)."""
    ids = P.layout(name, B, T)
    return (ids,) + P.loop_bounds(ids)


@functools.lru_cache(maxsize=4)
def _inputs(family, name, B, T, H):
    return P.make(family, _bounds(name, B, T)[1], B, H, T)


def _btc(t):
    B, H, T, _ = t.shape
    return t.transpose(1, 2).reshape(B, T, H * 64)


def _bhtd(t, H):
    B, T, _ = t.shape
    return t.reshape(B, T, H, 64).transpose(1, 2)


def _run(q, k, v, dO, bounds=None, drop=None):
    """``attn_fwd`` + ``attn_bwd`` called directly on the fused [B, T, 3C] layout, which makes ``lse`` and ``Dd``
    visible.  ``bounds`` = CPU ``(doc_start, doc_end)`` or ``None`` for the plain kernels; ``drop`` = ``(snapshot,
    site, thr, 1 / keep)``.  Every output buffer starts as NaN.  Returns CPU tensors, [B, H, T, ...]."""
    B, H, T, _ = q.shape
    C = 64 * H
    K = kernels()
    qkv = torch.cat([_btc(q), _btc(k), _btc(v)], 2).to(dev)
    dqkv = torch.full_like(qkv, NAN)
    qs, ks, vs = (qkv[:, :, i * C:(i + 1) * C] for i in range(3))
    dqs, dks, dvs = (dqkv[:, :, i * C:(i + 1) * C] for i in range(3))
    o = torch.full((B, T, C), NAN, device=dev, dtype=BF16)
    g = _btc(dO).contiguous().to(dev)
    lse = torch.full((B * H * T,), NAN, device=dev, dtype=torch.float32)
    Dd = torch.full((B * H * T,), NAN, device=dev, dtype=torch.float32)
    extra = (None, 0, 0, 1.0) if drop is None else tuple(drop)
    if bounds is None:
        K.attn_fwd(qs, ks, vs, o, lse, H, A.SCALE, *extra)
        K.attn_bwd(qs, ks, vs, o, g, lse, Dd, dqs, dks, dvs, H, A.SCALE, *extra)
    else:
        ds, de = (t.to(dev) for t in bounds)
        K.attn_fwd(qs, ks, vs, o, lse, H, A.SCALE, *extra, ds)
        K.attn_bwd(qs, ks, vs, o, g, lse, Dd, dqs, dks, dvs, H, A.SCALE, *extra, ds, de)
    torch.cuda.synchronize()
    return SimpleNamespace(y=_bhtd(o.cpu(), H), dq=_bhtd(dqs.cpu(), H), dk=_bhtd(dks.cpu(), H), dv=_bhtd(dvs.cpu(), H),
                           lse2=lse.cpu().view(B, H, T), D=Dd.cpu().view(B, H, T))


def _check(got, q, k, v, dO, tag, **kw):
    """Every output against the reference, as ``test_attention_gpu._check`` does for the plain kernels (same
    metric, same bounds): ``A.BOUND`` for y, dq, dk, dv, 1e-4 relative for the LSE, 2^-8 for ``D``.  The
    reference backward takes the kernels' own bf16 ``y`` for ``D = rowsum(dO * y)``."""
    for n in ALL:
        assert torch.isfinite(getattr(got, n)).all(), (tag, n, "not finite")
    ref = A.reference(q, k, v, dO, y_for_D=got.y, **kw)
    fails, line = [], []
    for n in OUTS:
        e, idx = A.worst_row(getattr(got, n), getattr(ref, n), getattr(ref, "den_" + n))
        line.append(f"{n} {e:.5f}")
        if not e <= A.BOUND:
            fails.append(f"{n}: {e:.5f} > {A.BOUND:.5f} at (b, h, row) {idx}")
    lse_e = ((got.lse2.double() - ref.lse2).abs() / ref.lse2.abs().clamp_min(1.0)).max().item()
    d_e = A.row_error(got.D.unsqueeze(-1), ref.D.unsqueeze(-1), ref.den_D.unsqueeze(-1))
    line += [f"lse2 {lse_e:.2e}", f"D {d_e:.2e}"]
    print(f"PACKED {tag}: " + " ".join(line))
    if not lse_e <= 1e-4:
        fails.append(f"lse2: {lse_e:.3e} > 1e-4")
    if not d_e <= 2.0 ** -8:
        fails.append(f"D: {d_e:.3e} > 2^-8")
    assert not fails, (tag, fails)
    return ref


def _same_bits(a, b, sel=None):
    """Names of the outputs that differ, over all rows or the rows ``sel`` (bool [B, T])."""
    def rows(t):
        return t if sel is None else t.transpose(0, 1)[:, sel]      # [H, n, ...]
    return [n for n in ALL if not torch.equal(rows(getattr(a, n)), rows(getattr(b, n)))]


# --------------------------------------------------------------------------------------- kernel accuracy
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_packed_attention_against_fp64_reference(case):
    family, name, (B, T, H) = case
    _, ds, de = _bounds(name, B, T)
    q, k, v, dO = _inputs(family, name, B, T, H)
    allowed = P.allowed_mask(ds)
    if family == "needle_outside" and name != "one":
        # the construction is potent: admitting the previous document moves every row that has one by more than
        # half its magnitude
        masked = A.reference(q, k, v, dO, allowed=allowed)
        leaky = A.reference(q, k, v, dO)
        moved = A.row_errors(leaky.y, masked.y, masked.den_y)[(ds > 0)[:, None, :].expand(B, H, T)]
        assert moved.min().item() > 0.5, moved.min().item()
    got = _run(q, k, v, dO, bounds=(ds, de))
    ref = _check(got, q, k, v, dO, _id(case), allowed=allowed)
    if name == "one":
        # a single document: the DOC instantiations against the plain kernels, under the same metric and bound
        plain = _run(q, k, v, dO)
        for n in OUTS:
            e = A.row_error(getattr(got, n), getattr(plain, n), getattr(ref, "den_" + n))
            assert e <= A.BOUND, (n, e)
        assert (got.lse2 - plain.lse2).abs().max().item() <= 1e-4
        _check(plain, q, k, v, dO, "plain-" + _id(case))


def test_fully_masked_tile_has_the_true_lse():
    """Layout ``mid200``: queries 200 .. 255 meet the key tile 128 .. 191 wholly masked before their first visible
    key.  With q = 0 every visible key weighs the same, so lse2[t] = log2(t - doc_start[t] + 1) exactly."""
    B, T, H = 2, 256, 3
    _, ds, de = _bounds("mid200", B, T)
    q, k, v, dO = _inputs("gauss1", "mid200", B, T, H)
    got = _run(torch.zeros_like(q), k, v, dO, bounds=(ds, de))
    want = torch.log2((torch.arange(T)[None, :] - ds + 1).double())[:, None, :].expand(B, H, T)
    assert torch.isfinite(got.y).all() and torch.isfinite(got.lse2).all()
    assert (got.lse2.double() - want).abs().max().item() <= 2e-5


# --------------------------------------------------------------------------------------- isolation
def test_isolation_bit_for_bit():
    """q, k, v and dO inside document B replaced by other finite values: every output row of the documents
    before and after B keeps its bits (masked probabilities are exact zeros and the values are finite).  Row 0:
    A = 0 .. 149, B = 150 .. 219, A' = 220 .. 255, so A ends and A' begins inside a 64-tile that B shares.  Row 1:
    B = 30 .. 99 inside the first two tiles."""
    B, T, H = 2, 256, 3
    rows = [[0, 150, 220], [0, 30, 100]]
    ids = P.doc_ids(T, rows)
    ds, de = P.loop_bounds(ids)
    inside = torch.zeros(B, T, dtype=torch.bool)
    inside[0, 150:220] = True
    inside[1, 30:100] = True
    q, k, v, dO = A.make("gauss1", B, H, T, seed=3)
    other = A.make("gauss4", B, H, T, seed=4)
    sel = inside[:, None, :, None]
    q2, k2, v2, dO2 = (torch.where(sel, o, t) for t, o in zip((q, k, v, dO), other))
    assert not torch.equal(q2, q) and torch.isfinite(q2.float()).all()
    base = _run(q, k, v, dO, bounds=(ds, de))
    swap = _run(q2, k2, v2, dO2, bounds=(ds, de))
    assert not _same_bits(base, swap, ~inside), _same_bits(base, swap, ~inside)
    assert set(_same_bits(base, swap, inside)) == set(ALL)          # and B itself did change, in every output
    _check(swap, q2, k2, v2, dO2, "isolation-swapped", allowed=P.allowed_mask(ds))


# --------------------------------------------------------------------------------------- dropout
def test_dropout_composes_with_documents():
    B, T, H, p, site = 2, 256, 3, 0.1, 3
    _, ds, de = _bounds("mid200", B, T)
    q, k, v, dO = _inputs("gauss1", "mid200", B, T, H)
    snap_gpu, snap_cpu = DeviceRNG(101, device=dev).next(), DeviceRNG(101).next()
    mask = R.dropout_mask(snap_cpu, site, p, bht=(B, H, T))
    keep = 1.0 - R.effective_p(p, "attention")
    got = _run(q, k, v, dO, bounds=(ds, de), drop=(snap_gpu, site, R.threshold(p, "attention"), 1.0 / keep))
    _check(got, q, k, v, dO, "drop0.1-mid200", mask=mask, inv_keep=1.0 / keep, allowed=P.allowed_mask(ds))
    # the LSE is undropped: the p = 0 run's, bit for bit
    assert torch.equal(got.lse2, _run(q, k, v, dO, bounds=(ds, de)).lse2)


# --------------------------------------------------------------------------------------- replay
def test_replay_with_new_boundaries():
    """Forward + backward of the op captured with layout ``mid200`` in static bounds buffers; ``tiles`` (other
    boundaries, so other trip counts) copied in and replayed gives the bits of an eager call with ``tiles``."""
    B, T, H = 2, 256, 3
    C = 64 * H
    q, k, v, dO = _inputs("gauss1", "mid200", B, T, H)
    qkv = torch.cat([_btc(q), _btc(k), _btc(v)], 2).to(dev).requires_grad_()
    g = _btc(dO).contiguous().to(dev)
    lay = {n: tuple(t.to(dev) for t in _bounds(n, B, T)[1:]) for n in ("mid200", "tiles")}
    static = tuple(t.clone() for t in lay["mid200"])

    def step(bounds):
        y = TR.causal_attention(qkv, H, doc_bounds=bounds)
        (dx,) = torch.autograd.grad(y, qkv, g)
        return y.detach(), dx

    cur = torch.cuda.current_stream()
    side = torch.cuda.Stream()
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        step(static)                                       # warm-up outside the capture
    cur.wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ys, dxs = step(static)
    eager = {n: step(lay[n]) for n in lay}
    assert not torch.equal(eager["mid200"][0], eager["tiles"][0])
    for n in ("mid200", "tiles", "mid200"):
        for s, t in zip(static, lay[n]):
            s.copy_(t)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(ys, eager[n][0]) and torch.equal(dxs, eager[n][1]), n


# --------------------------------------------------------------------------------------- doc_bounds, embedding
def test_doc_bounds_gpu_matches_the_loops():
    T = 256
    ids = torch.cat([P.layout(n, 2, T) for n in P.LAYOUTS] + [torch.arange(T)[None], torch.zeros(1, T, dtype=torch.int64)])
    want = P.loop_bounds(ids)
    for cast in (torch.int64, torch.int32):
        got = ops.doc_bounds(ids.to(dev, cast))
        assert got[0].dtype == torch.int32 and got[0].is_cuda
        assert torch.equal(got[0].cpu(), want[0]) and torch.equal(got[1].cpu(), want[1])
    cpu = ops.doc_bounds(ids)
    assert torch.equal(cpu[0], want[0]) and torch.equal(cpu[1], want[1])
    # row lengths that are no multiple of 64 (a partial last bitmap word), longer than one pass of the block's
    # 256 threads, documents that span several words, a boundary on a word's last bit, and T = 1
    g = torch.Generator().manual_seed(2)
    for T, every in ((1000, 37), (1000, 400), (70, 5), (64, 63), (1, 1)):
        ids = (torch.rand(3, T, generator=g) < 1.0 / every).cumsum(1)
        ids[1, T - 1:] += 1
        want = P.loop_bounds(ids)
        got = ops.doc_bounds(ids.to(dev))
        assert torch.equal(got[0].cpu(), want[0]) and torch.equal(got[1].cpu(), want[1]), (T, every)


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_embedding_positions_restart_per_document(p):
    """Forward and dwpe against torch indexing (``wpe[t - doc_start]`` / ``index_add_``), with and without
    embedding dropout; two runs give dwpe bit for bit."""
    torch.manual_seed(3)
    B, Tn, C, Vp = 4, 256, 128, 512
    ids = torch.cat([P.layout("len1", 2, Tn), P.layout("span", 2, Tn)])
    ds, de = P.loop_bounds(ids)
    bounds = ops.doc_bounds(ids.to(dev))
    pos = (torch.arange(Tn)[None, :] - ds).long().to(dev)
    idx = torch.randint(0, 40, (B, Tn), device=dev)
    wte = torch.randn(Vp, C).to(dev, BF16).requires_grad_()
    wpe = torch.randn(Tn + 64, C).to(dev, BF16).requires_grad_()         # rows past T, too
    g = torch.randn(B, Tn, C).to(dev, BF16)
    snap = DeviceRNG(7, device=dev).next() if p else None
    x = TR.embedding(idx, wte, wpe, p, snap, 0, doc_bounds=bounds)
    x.backward(g)
    scale = torch.ones(B, Tn, C, device=dev)
    if p:
        m = R.elementwise_mask(DeviceRNG(7).next(), 0, B * Tn * C, p).view(B, Tn, C).to(dev)
        scale = m.float() * R.inv_keep(p, "elementwise")
    xr = (wte.detach().float()[idx] + wpe.detach().float()[pos]) * scale
    err = ((x.detach().float() - xr).abs().max() / xr.abs().max()).item()
    assert err < 1e-2, err
    want = torch.zeros(Tn + 64, C, device=dev).index_add_(0, pos.flatten(), (g.float() * scale).view(-1, C))
    got = wpe.grad.float()
    err = ((got - want).abs().max() / want.abs().max()).item()
    assert err < 2e-2, err
    reached = torch.zeros(Tn + 64, dtype=torch.bool, device=dev)
    reached[pos.flatten()] = True
    assert not reached.all() and got[~reached].abs().max().item() == 0.0      # rows no position reaches: zero
    first = wpe.grad.clone()
    wpe.grad = None
    TR.embedding(idx, wte, wpe, p, snap, 0, doc_bounds=bounds).backward(g)
    assert torch.equal(wpe.grad, first)


# --------------------------------------------------------------------------------------- model
CFG = dict(block_size=256, vocab_size=1000, padded_vocab=1024, n_layer=2, n_head=2, n_embd=128)


def test_packed_gpt2_gpu_matches_cpu_fp32():
    """The small GPT on the GPU in bf16 against its CPU fp32 twin with the same ``doc_ids``: loss within 1e-2
    and every parameter gradient at cosine >= 0.99, the tolerances of
    ``test_transformer_gpu.test_gpt2_gpu_matches_cpu_fp32``."""
    cfg = GPTConfig(**CFG)
    g = build_gpt2(cfg, seed=0, device=dev)
    c = build_gpt2(cfg, seed=0, dtype=torch.float32)
    with torch.no_grad():
        g.transformer.wpe.weight.normal_(0.0, 0.1)          # the initial std of 0.01 would hide a wrong position
        for pc, pg in zip(c.parameters(), g.parameters()):
            pc.copy_(pg.float())
    torch.manual_seed(5)
    B, T = 4, 256
    idx = torch.randint(0, cfg.vocab_size, (B, T))
    tgt = torch.randint(0, cfg.vocab_size, (B, T))
    ids = torch.cat([P.layout("mid200", 2, T), P.layout("len1", 2, T)])
    lg = g(idx.to(dev), tgt.to(dev), doc_ids=ids.to(dev))
    lc = c(idx, tgt, doc_ids=ids)
    lg.backward()
    lc.backward()
    fails = []
    if not abs(lg.item() - lc.item()) < 1e-2:
        fails.append(f"loss {lg.item():.5f} vs {lc.item():.5f}")
    for (n, pg), pc in zip(g.named_parameters(), c.parameters()):
        cos = F.cosine_similarity(pg.grad.float().flatten().cpu(), pc.grad.flatten(), dim=0).item()
        if not cos >= 0.99:
            fails.append(f"grad {n}: cos {cos:.4f}")
    print(f"PACKED model parity: loss {lg.item():.5f} vs {lc.item():.5f}")
    assert not fails, fails


def test_default_is_unchanged_bit_for_bit():
    """``doc_bounds=None`` / ``doc_ids=None`` against calls that omit the argument."""
    B, T, H = 2, 256, 2
    torch.manual_seed(6)
    qkv = torch.randn(B, T, 3 * 64 * H).to(dev, BF16)
    g = torch.randn(B, T, 64 * H).to(dev, BF16)
    outs = []
    for kw in ({}, {"doc_bounds": None}):
        x = qkv.clone().requires_grad_()
        y = TR.causal_attention(x, H, **kw)
        y.backward(g)
        outs.append((y.detach(), x.grad))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    idx = torch.randint(0, 40, (B, T), device=dev)
    wte = torch.randn(512, 128).to(dev, BF16)
    wpe = torch.randn(T, 128).to(dev, BF16).requires_grad_()
    ge = torch.randn(B, T, 128).to(dev, BF16)
    emb = []
    for kw in ({}, {"doc_bounds": None}):
        wpe.grad = None
        e = TR.embedding(idx, wte, wpe, **kw)
        e.backward(ge)
        emb.append((e.detach(), wpe.grad.clone()))
    assert torch.equal(emb[0][0], emb[1][0]) and torch.equal(emb[0][1], emb[1][1])
    m = build_gpt2(GPTConfig(**CFG), seed=1, device=dev)
    tok = torch.randint(0, CFG["vocab_size"], (B, T), device=dev)
    with torch.no_grad():
        assert torch.equal(m(tok), m(tok, doc_ids=None))
        assert torch.equal(m(tok, tok), m(tok, tok, doc_ids=None))
        assert torch.equal(m(tok, tok), m(tok, tok, None))
